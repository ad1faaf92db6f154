"""Fused RoPE + KV-cache write (ops.rope_and_cache) on the GPU.

The fused kernel must reproduce apply_rope followed by reshape_and_cache
bit for bit (torch.equal on q, k and the whole cache), and agree with the
fp32 PyTorch reference within the tolerance test_kernels_gpu.py uses
(2e-2; 6e-2 through an fp8 cache). Runs only on an MI355X (-m gpu).
"""

import pytest
import torch

from vllm_amd.ops import _torch_ref as ref

pytestmark = pytest.mark.gpu

MAX_POS = 2048


def _hip():
    from vllm_amd.ops import hip_ops

    return hip_ops


@pytest.fixture(autouse=True)
def _seed():
    torch.manual_seed(0)


def _cos_sin(rot):
    inv = 1.0 / (10000.0 ** (torch.arange(0, rot, 2).float() / rot))
    freqs = torch.outer(torch.arange(MAX_POS).float(), inv)
    return torch.cat([freqs.cos(), freqs.sin()], dim=-1).cuda()


def _qkv(T, Hq, Hkv, D, dtype):
    """q, k, v as head slices of one [T, (Hq+2*Hkv)*D] buffer."""
    buf = torch.randn(T, (Hq + 2 * Hkv) * D, dtype=dtype, device="cuda")
    q = buf[:, :Hq * D].view(T, Hq, D)
    k = buf[:, Hq * D:(Hq + Hkv) * D].view(T, Hkv, D)
    v = buf[:, (Hq + Hkv) * D:].view(T, Hkv, D)
    return buf, q, k, v


def _cache(NB, Hkv, BS, D, dtype, fp8):
    c = torch.randn(2, NB, Hkv, BS, D, dtype=dtype, device="cuda")
    return c.to(torch.float8_e4m3fn) if fp8 else c


def _bits(t):
    return t.view(torch.uint8) if t.dtype == torch.float8_e4m3fn else t


def _check(T, Hq, Hkv, D, rot, dtype, fp8, slots, NB=8, BS=64):
    hip = _hip()
    cs = _cos_sin(rot)
    pos = torch.randint(0, MAX_POS, (T,), device="cuda")
    buf, q, k, v = _qkv(T, Hq, Hkv, D, dtype)
    cache = _cache(NB, Hkv, BS, D, dtype, fp8)

    # Two-kernel path on a copy.
    buf2 = buf.clone()
    q2 = buf2[:, :Hq * D].view(T, Hq, D)
    k2 = buf2[:, Hq * D:(Hq + Hkv) * D].view(T, Hkv, D)
    v2 = buf2[:, (Hq + Hkv) * D:].view(T, Hkv, D)
    cache2 = cache.clone()

    # fp32 reference on the un-rotated inputs; padding rows write no slot.
    rq, rk = ref.apply_rope(pos, q.float(), k.float(), cs, rot)
    ref_cache = cache.float()
    keep = slots >= 0
    ref.reshape_and_cache(rk[keep], v.float()[keep], ref_cache, slots[keep])

    hip.rope_and_cache(pos, q, k, v, cs, rot, cache, slots)
    hip.apply_rope(pos, q2, k2, cs, rot)
    hip.reshape_and_cache(k2, v2, cache2, slots)

    assert torch.equal(q, q2)
    assert torch.equal(k, k2)
    assert torch.equal(buf, buf2)          # v and everything else untouched
    assert torch.equal(_bits(cache), _bits(cache2))

    torch.testing.assert_close(q.float(), rq, atol=2e-2, rtol=2e-2)
    torch.testing.assert_close(k.float(), rk, atol=2e-2, rtol=2e-2)
    tol = 6e-2 if fp8 else 2e-2
    torch.testing.assert_close(cache.float(), ref_cache, atol=tol, rtol=tol)
    return q, k, cache


@pytest.mark.parametrize("fp8", [False, True], ids=["c16", "cfp8"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16],
                         ids=["bf16", "fp16"])
@pytest.mark.parametrize("half_rot", [False, True], ids=["full", "half"])
@pytest.mark.parametrize("D", [64, 128, 256])
def test_matches_two_kernels(D, half_rot, dtype, fp8):
    T, NB, BS = 33, 8, 64
    slots = torch.randperm(NB * BS, device="cuda")[:T]
    _check(T, 8, 2, D, D // 2 if half_rot else D, dtype, fp8, slots)


def test_padding_rows_rotate_but_skip_cache():
    T, NB, BS, D = 33, 8, 64, 128
    slots = torch.randperm(NB * BS, device="cuda")[:T]
    pad = [0, 5, 17, 32]
    slots[pad] = -1
    hip = _hip()
    cs = _cos_sin(D)
    pos = torch.randint(0, MAX_POS, (T,), device="cuda")
    buf, q, k, v = _qkv(T, 8, 2, D, torch.bfloat16)
    cache = _cache(NB, 2, BS, D, torch.bfloat16, False)
    before = cache.clone()
    q0, k0 = q.clone(), k.clone()
    hip.rope_and_cache(pos, q, k, v, cs, D, cache, slots)
    # Slots no token maps to keep their old contents.
    written = torch.zeros(NB * BS, dtype=torch.bool, device="cuda")
    written[slots[slots >= 0]] = True
    flat = cache.permute(0, 1, 3, 2, 4).reshape(2, NB * BS, 2, D)
    flat0 = before.permute(0, 1, 3, 2, 4).reshape(2, NB * BS, 2, D)
    assert torch.equal(flat[:, ~written], flat0[:, ~written])
    # Padding rows are still rotated, exactly as rope alone does it.
    hip.apply_rope(pos, q0, k0, cs, D)
    assert torch.equal(q, q0) and torch.equal(k, k0)
    assert not torch.equal(flat[:, written], flat0[:, written])
    # And the full equality / reference check with the same padding.
    _check(T, 8, 2, D, D, torch.bfloat16, False, slots)


@pytest.mark.parametrize("T", [1, 0])
def test_tiny_token_counts(T):
    slots = torch.randperm(8 * 64, device="cuda")[:T]
    _check(T, 8, 2, 128, 128, torch.bfloat16, False, slots)


def test_many_tokens_permuted_slots():
    T, NB, BS = 300, 8, 64
    slots = torch.randperm(NB * BS, device="cuda")[:T]
    _check(T, 8, 2, 128, 128, torch.bfloat16, False, slots)


def test_graph_capture_replays():
    """Captured once, replayed with new positions / slot_mapping contents:
    every replay equals the eager result on the same inputs."""
    hip = _hip()
    T, Hq, Hkv, D, NB, BS = 33, 8, 2, 128, 8, 64
    cs = _cos_sin(D)
    src, _, _, _ = _qkv(T, Hq, Hkv, D, torch.bfloat16)
    cache0 = _cache(NB, Hkv, BS, D, torch.bfloat16, False)

    buf = src.clone()
    q = buf[:, :Hq * D].view(T, Hq, D)
    k = buf[:, Hq * D:(Hq + Hkv) * D].view(T, Hkv, D)
    v = buf[:, (Hq + Hkv) * D:].view(T, Hkv, D)
    cache = cache0.clone()
    pos = torch.zeros(T, dtype=torch.int64, device="cuda")
    slots = torch.arange(T, dtype=torch.int64, device="cuda")

    # Warm up on a side stream, then capture.
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        hip.rope_and_cache(pos, q, k, v, cs, D, cache, slots)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        hip.rope_and_cache(pos, q, k, v, cs, D, cache, slots)

    for _ in range(2):
        new_pos = torch.randint(0, MAX_POS, (T,), device="cuda")
        new_slots = torch.randperm(NB * BS, device="cuda")[:T]
        # Eager result on fresh copies of the same inputs.
        ebuf = src.clone()
        eq = ebuf[:, :Hq * D].view(T, Hq, D)
        ek = ebuf[:, Hq * D:(Hq + Hkv) * D].view(T, Hkv, D)
        ev = ebuf[:, (Hq + Hkv) * D:].view(T, Hkv, D)
        ecache = cache0.clone()
        hip.rope_and_cache(new_pos, eq, ek, ev, cs, D, ecache, new_slots)
        # Replay on the captured buffers.
        buf.copy_(src)
        cache.copy_(cache0)
        pos.copy_(new_pos)
        slots.copy_(new_slots)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(buf, ebuf)
        assert torch.equal(cache, ecache)
