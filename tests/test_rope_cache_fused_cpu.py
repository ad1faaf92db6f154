"""ops.rope_and_cache on CPU tensors equals apply_rope followed by
reshape_and_cache, on the strided head slices of a fused QKV buffer."""

import pytest
import torch

from vllm_amd import ops


@pytest.mark.parametrize("rot", [64, 32])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_rope_and_cache_equals_composition(rot, dtype):
    torch.manual_seed(0)
    T, Hq, Hkv, D, NB, BS = 9, 4, 2, 64, 4, 16
    inv = 1.0 / (10000.0 ** (torch.arange(0, rot, 2).float() / rot))
    freqs = torch.outer(torch.arange(128).float(), inv)
    cs = torch.cat([freqs.cos(), freqs.sin()], dim=-1)
    pos = torch.randint(0, 128, (T,))
    slots = torch.randperm(NB * BS)[:T]

    def split(buf):
        return (buf[:, :Hq * D].view(T, Hq, D),
                buf[:, Hq * D:(Hq + Hkv) * D].view(T, Hkv, D),
                buf[:, (Hq + Hkv) * D:].view(T, Hkv, D))

    buf_a = torch.randn(T, (Hq + 2 * Hkv) * D, dtype=dtype)
    buf_b = buf_a.clone()
    cache_a = torch.randn(2, NB, Hkv, BS, D, dtype=dtype)
    cache_b = cache_a.clone()

    qa, ka, va = split(buf_a)
    out_q, out_k = ops.rope_and_cache(pos, qa, ka, va, cs, rot, cache_a,
                                      slots)
    qb, kb, vb = split(buf_b)
    ops.apply_rope(pos, qb, kb, cs, rot)
    ops.reshape_and_cache(kb, vb, cache_b, slots)

    assert out_q is qa and out_k is ka
    assert torch.equal(buf_a, buf_b)
    assert torch.equal(cache_a, cache_b)
    assert not torch.equal(cache_a[0], cache_a[1])
