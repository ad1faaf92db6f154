"""Paged decode attention with the one-trip K/V prefetch and the merged
prologue loads: values against the fp32 PyTorch reference at every context
length where the prefetch changes shape (fewer tokens than one trip, exactly
one trip, cache-block and partition edges), with the tolerance
test_kernels_gpu.py uses (2e-2; 6e-2 through an fp8 cache).
Runs only on an MI355X (-m gpu).
"""

import pytest
import torch

from vllm_amd.ops import _torch_ref as ref

pytestmark = pytest.mark.gpu

BS = 64


def _hip():
    from vllm_amd.ops import hip_ops

    return hip_ops


@pytest.fixture(autouse=True)
def _seed():
    torch.manual_seed(0)


def _make_paged(ctx_lens, Hq, Hkv, D=128, fp8=False):
    """q + populated paged cache + metadata for decode rows. Blocks are
    handed out densely from 1, so the last request's last block is the last
    block of the allocation, and the block table has exactly
    ceil(max ctx / 64) columns."""
    n = len(ctx_lens)
    max_blocks = max((c + BS - 1) // BS for c in ctx_lens)
    num_blocks = sum((c + BS - 1) // BS for c in ctx_lens) + 1
    q = torch.randn(n, Hq, D, dtype=torch.bfloat16, device="cuda")
    cache = torch.randn(2, num_blocks, Hkv, BS, D, dtype=torch.bfloat16,
                        device="cuda")
    if fp8:
        cache = cache.to(torch.float8_e4m3fn)
    block_table = torch.zeros(n, max_blocks, dtype=torch.int32,
                              device="cuda")
    nxt = 1
    for i, c in enumerate(ctx_lens):
        nb = (c + BS - 1) // BS
        block_table[i, :nb] = torch.arange(nxt, nxt + nb)
        nxt += nb
    assert nxt == num_blocks
    qsl = torch.arange(n + 1, dtype=torch.int32, device="cuda")
    seq_lens = torch.tensor(ctx_lens, dtype=torch.int32, device="cuda")
    return q, cache, block_table, qsl, seq_lens


def _check(ctx_lens, group, D=128, fp8=False, window=0, tol=2e-2):
    hip = _hip()
    Hkv = 2
    n = len(ctx_lens)
    q, cache, bt, qsl, sl = _make_paged(ctx_lens, Hkv * group, Hkv, D, fp8)
    scale = 1.0 / D**0.5
    out = hip.attention_unified(q, cache, bt, qsl, sl, scale, num_decodes=n,
                                sliding_window=window,
                                max_seq_len=max(ctx_lens), max_query_len=1)
    expect = ref.attention_unified(q, cache, bt, qsl, sl, scale,
                                   num_decodes=n, sliding_window=window)
    torch.testing.assert_close(out.float(), expect.float(), atol=tol,
                               rtol=tol,
                               msg=lambda m: f"ctx={ctx_lens} group={group} "
                                             f"D={D}: {m}")


@pytest.mark.parametrize("group", [1, 4, 8])
@pytest.mark.parametrize(
    "ctx", [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 150, 511, 512, 513, 1025])
def test_prefetch_edges(group, ctx):
    _check([ctx] * 4, group)


@pytest.mark.parametrize("group", [1, 4, 8])
def test_mixed_contexts(group):
    _check([1, 33, 150, 513], group)


def test_sliding_window_shorter_than_one_trip():
    _check([200] * 4, 4, window=8)


def test_fp8_cache():
    _check([150] * 4, 4, fp8=True, tol=6e-2)


@pytest.mark.parametrize("ctx", [33, 150])
@pytest.mark.parametrize("D", [64, 256])
def test_other_head_dims(D, ctx):
    _check([ctx] * 4, 4, D=D)


@pytest.mark.parametrize("ctx", [33, 150, 513])
def test_prefetch_stays_inside_last_block(ctx):
    """The last request's last block is the last block of the cache and the
    block table has exactly ceil(ctx/64) columns, so the clamped prefetch of
    the final trip has nowhere else valid to point. Values only."""
    Hkv, group, n = 2, 4, 4
    q, cache, bt, qsl, sl = _make_paged([ctx] * n, Hkv * group, Hkv)
    assert bt.shape[1] == (ctx + BS - 1) // BS
    assert int(bt[-1, -1]) == cache.shape[1] - 1
    scale = 1.0 / 128**0.5
    out = _hip().attention_unified(q, cache, bt, qsl, sl, scale,
                                   num_decodes=n, max_seq_len=ctx,
                                   max_query_len=1)
    expect = ref.attention_unified(q, cache, bt, qsl, sl, scale,
                                   num_decodes=n)
    torch.testing.assert_close(out.float(), expect.float(), atol=2e-2,
                               rtol=2e-2)
