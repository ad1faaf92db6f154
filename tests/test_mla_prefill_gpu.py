"""MFMA MLA prefill kernel (csrc/mla_prefill.hip) and its dispatch through
ops.mla_attention, against the fp32 torch composition over the latent
cache (DeepSeek geometry: lora 512 + rope 64). Inputs, scaling and the
4e-2 tolerance are those of test_mla_decode_kernel: the same arithmetic
and the same rounding of P to the input dtype."""

import pytest
import torch

import vllm_amd.ops as ops
from vllm_amd.ops import _torch_ref as ref

pytestmark = pytest.mark.gpu

TOL = dict(atol=4e-2, rtol=4e-2)
SCALE = (128 + 64) ** -0.5


def _inputs(Hq, q_lens, ctx_lens, bs, dtype=torch.bfloat16):
    """Requests in the given order over a permuted block table."""
    torch.manual_seed(0)
    R, T = len(q_lens), sum(q_lens)
    nb = max(-(-c // bs) for c in ctx_lens)
    kv = torch.randn(R * nb + 1, bs, 576, dtype=dtype, device="cuda") * 0.5
    bt = (torch.randperm(R * nb, device="cuda").int() + 1).view(R, nb)
    q_nope = torch.randn(T, Hq, 512, dtype=dtype, device="cuda") * 0.3
    q_pe = torch.randn(T, Hq, 64, dtype=dtype, device="cuda") * 0.3
    qsl = torch.tensor([0] + q_lens, device="cuda").cumsum(0).int()
    seq_lens = torch.tensor(ctx_lens, dtype=torch.int32, device="cuda")
    return q_nope, q_pe, kv, bt.contiguous(), qsl, seq_lens


def _expect(q_nope, q_pe, kv, bt, qsl, seq_lens):
    return ref.mla_attention(q_nope.float(), q_pe.float(), kv.float(), bt,
                             qsl, seq_lens, SCALE)


@pytest.mark.parametrize("Hq,q_lens,ctx_lens,bs,dtype", [
    # from scratch: 4 tokens per tile, partial last tile, mask in subtile 0
    (16, [5], [5], 16, torch.bfloat16),
    # diagonal crosses the 32-token subtile edge; second request exits early
    (16, [33, 7], [33, 40], 16, torch.bfloat16),
    # two tiles per token, q_len 1 as a prefill row, engine block size
    (128, [3, 1], [67, 130], 64, torch.bfloat16),
    # Hq neither divides 64 nor is a multiple of 16; long unmasked run
    (24, [17, 70], [100, 300], 16, torch.bfloat16),
    # smallest: most of the tile is padding rows
    (8, [2], [2], 16, torch.bfloat16),
    (16, [33, 7], [33, 40], 16, torch.float16),
])
def test_mla_prefill_kernel(Hq, q_lens, ctx_lens, bs, dtype):
    from vllm_amd.ops import hip_ops

    args = _inputs(Hq, q_lens, ctx_lens, bs, dtype)
    out = torch.full_like(args[0], float("nan"))
    hip_ops.mla_prefill(out, *args, SCALE, 0, max(q_lens))
    torch.testing.assert_close(out.float(), _expect(*args), **TOL)


# 3 decode rows, then a continuation and a from-scratch prefill.
MIXED = dict(Hq=32, q_lens=[1, 1, 1, 5, 40], ctx_lens=[77, 50, 77, 40, 40],
             bs=16)
MIXED_HINTS = dict(num_decodes=3, max_seq_len=77, max_query_len=40)


def test_mla_attention_dispatch_never_reaches_torch(monkeypatch):
    args = _inputs(**MIXED)
    expect = _expect(*args)

    def boom(*a, **k):
        raise AssertionError("MLA row reached the torch path")

    monkeypatch.setattr(ref, "mla_attention", boom)
    out = ops.mla_attention(*args, SCALE, **MIXED_HINTS)
    torch.testing.assert_close(out.float(), expect, **TOL)


def test_mla_attention_graph_capturable():
    """With both hints given the call has no host sync: it captures on
    one stream and replays correctly with new query values."""
    q_nope, q_pe, *rest = _inputs(**MIXED)
    s_nope, s_pe = q_nope.clone(), q_pe.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.mla_attention(s_nope, s_pe, *rest, SCALE, **MIXED_HINTS)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = ops.mla_attention(s_nope, s_pe, *rest, SCALE, **MIXED_HINTS)
    for mul in (1.0, -0.5, 2.0):
        s_nope.copy_(q_nope * mul)
        s_pe.copy_(q_pe * mul)
        g.replay()
        torch.cuda.synchronize()
        torch.testing.assert_close(
            out.float(), _expect(s_nope, s_pe, *rest), **TOL)
