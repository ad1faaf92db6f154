"""fp8 (e4m3) latent KV cache for MLA: the HIP cache write, the decode
and prefill kernels over an fp8 cache through ops.mla_attention, and the
engine. Attention reference: the fp32 torch composition over the
dequantised cache; e4m3 -> bf16/fp16 is exact, so the 16-bit tests' 4e-2
holds. The write is held to the project's fp8-cache tolerance (6e-2: e4m3
keeps 3 mantissa bits, half an ulp is 2^-4 relative)."""

import pytest
import torch

import vllm_amd.ops as ops
from tests.test_mla_prefill_gpu import MIXED, MIXED_HINTS
from vllm_amd.ops import _torch_ref as ref

pytestmark = pytest.mark.gpu

FP8 = torch.float8_e4m3fn
TOL = dict(atol=4e-2, rtol=4e-2)
FP8_TOL = dict(atol=6e-2, rtol=6e-2)
SCALE = (128 + 64) ** -0.5


@pytest.mark.parametrize("lora,rope", [(512, 64), (64, 16)])
@pytest.mark.parametrize("fp8_cache", [True, False])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_concat_and_cache_mla(dtype, fp8_cache, lora, rope):
    torch.manual_seed(0)
    T, NB, BS = 33, 8, 16
    wide = torch.randn(T, lora + 24, dtype=dtype, device="cuda")
    c_kv = wide[:, 8:8 + lora]  # row-strided, 16 B-aligned column slice
    k_pe = torch.randn(T, rope, dtype=dtype, device="cuda")
    c_kv[0, 0], c_kv[5, lora - 1], k_pe[7, 3], k_pe[32, rope - 1] = (
        1000.0, -1000.0, 1000.0, -1000.0)
    slots = torch.randperm(NB * BS, device="cuda")[:T]
    slots[[2, 11, 20, 32]] = -1
    cdt = FP8 if fp8_cache else dtype
    cache = torch.randn(NB, BS, lora + rope, device="cuda").to(cdt)
    before = cache.clone()

    ops.concat_and_cache_mla(c_kv, k_pe, cache, slots)

    valid = slots >= 0
    untouched = torch.ones(NB * BS, dtype=torch.bool, device="cuda")
    untouched[slots[valid]] = False
    raw, raw_before = (c.view(NB * BS, -1).view(torch.uint8)
                       for c in (cache, before))
    assert torch.equal(raw[untouched], raw_before[untouched])
    x = torch.cat([c_kv, k_pe], dim=1)[valid]
    got = cache.view(NB * BS, -1).float()[slots[valid]]
    if fp8_cache:
        assert not got.isnan().any()
        torch.testing.assert_close(got, x.float().clamp(-448, 448),
                                   **FP8_TOL)
    else:
        assert torch.equal(got, x.float())


def _expect(q_nope, q_pe, kv, bt, qsl, seq_lens):
    return ref.mla_attention(q_nope.float(), q_pe.float(), kv.float(), bt,
                             qsl, seq_lens, SCALE)


def _inputs(Hq, q_lens, ctx_lens, bs, dtype=torch.bfloat16):
    """Requests in order over a permuted block table and an fp8 cache."""
    torch.manual_seed(0)
    R, T = len(q_lens), sum(q_lens)
    nb = max(-(-c // bs) for c in ctx_lens)
    kv = (torch.randn(R * nb + 1, bs, 576, device="cuda") * 0.5).to(FP8)
    bt = (torch.randperm(R * nb, device="cuda").int() + 1).view(R, nb)
    q_nope = torch.randn(T, Hq, 512, dtype=dtype, device="cuda") * 0.3
    q_pe = torch.randn(T, Hq, 64, dtype=dtype, device="cuda") * 0.3
    qsl = torch.tensor([0] + q_lens, device="cuda").cumsum(0).int()
    seq_lens = torch.tensor(ctx_lens, dtype=torch.int32, device="cuda")
    return q_nope, q_pe, kv, bt.contiguous(), qsl, seq_lens


@pytest.mark.parametrize("T,Hq,ctx,bs", [
    (1, 128, 33, 16),    # partial subtile
    (2, 32, 1024, 64),   # exact partition edge, engine block size
    (3, 16, 2500, 16),   # multi-partition + reduce
])
def test_mla_decode_fp8_cache(T, Hq, ctx, bs):
    ctx_lens = [max(1, ctx - 7)] + [ctx] * (T - 1)  # ragged
    args = _inputs(Hq, [1] * T, ctx_lens, bs)
    out = ops.mla_attention(*args, SCALE, num_decodes=T, max_seq_len=ctx,
                            max_query_len=1)
    torch.testing.assert_close(out.float(), _expect(*args), **TOL)


@pytest.mark.parametrize("Hq,q_lens,ctx_lens,bs,dtype", [
    (16, [5], [5], 16, torch.bfloat16),
    (16, [33, 7], [33, 40], 16, torch.bfloat16),
    (128, [3, 1], [67, 130], 64, torch.bfloat16),
    (24, [17, 70], [100, 300], 16, torch.bfloat16),
    (8, [2], [2], 16, torch.bfloat16),
    (16, [33, 7], [33, 40], 16, torch.float16),
])
def test_mla_prefill_fp8_cache(Hq, q_lens, ctx_lens, bs, dtype):
    args = _inputs(Hq, q_lens, ctx_lens, bs, dtype)
    out = ops.mla_attention(*args, SCALE, num_decodes=0,
                            max_seq_len=max(ctx_lens),
                            max_query_len=max(q_lens))
    torch.testing.assert_close(out.float(), _expect(*args), **TOL)


def test_mla_attention_fp8_cache_never_reaches_torch(monkeypatch):
    q_nope, q_pe, *rest = _inputs(**MIXED)
    expect = _expect(q_nope, q_pe, *rest)

    def boom(*a, **k):
        raise AssertionError("MLA row reached the torch path")

    monkeypatch.setattr(ref, "mla_attention", boom)
    out = ops.mla_attention(q_nope, q_pe, *rest, SCALE, **MIXED_HINTS)
    torch.testing.assert_close(out.float(), expect, **TOL)

    # One capture; replays with new query values against the eager result.
    s_nope, s_pe = q_nope.clone(), q_pe.clone()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        g_out = ops.mla_attention(s_nope, s_pe, *rest, SCALE, **MIXED_HINTS)
    for mul in (1.0, -0.5):
        s_nope.copy_(q_nope * mul)
        s_pe.copy_(q_pe * mul)
        g.replay()
        torch.cuda.synchronize()
        eager = ops.mla_attention(s_nope, s_pe, *rest, SCALE, **MIXED_HINTS)
        torch.testing.assert_close(g_out.float(), eager.float(), **TOL)


def test_deepseek_fp8_kv_cache_e2e():
    from vllm_amd.entrypoints.llm import LLM
    from vllm_amd.sampling_params import SamplingParams

    llm = LLM(model="tiny-deepseek", dtype="bf16", load_format="dummy",
              block_size=16, num_gpu_blocks=128, max_model_len=2048,
              device="cuda", max_num_batched_tokens=2048, max_num_seqs=16,
              kv_cache_dtype="fp8")
    caches = llm.engine.engine_core.worker.runner.kv_caches
    assert caches and all(c.dtype == FP8 for c in caches)
    prompts = [[(i * 11 + j) % 900 + 3 for j in range(50)] for i in range(2)]
    p = SamplingParams(temperature=0.0, max_tokens=6, ignore_eos=True)
    outs = llm.generate(prompts, p)
    llm.shutdown()
    assert all(len(o.outputs[0].token_ids) == 6 for o in outs)
