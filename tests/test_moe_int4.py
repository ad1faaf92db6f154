"""--quantization int4 on MoE experts: the stacked quantizer and CPU path,
the gfx950 grouped W4A16 GEMM against an fp64 reference, the fused
expert MLP and the engine wiring."""

import pytest
import torch

from vllm_amd.ops import _torch_ref as ref


def _moe_layers(llm):
    from vllm_amd.layers.fused_moe import FusedMoE

    model = llm.engine.engine_core.worker.runner.model
    return [m for m in model.modules() if isinstance(m, FusedMoE)]


def _assert_quantized_and_repeatable(llm, prompts, n_tokens):
    from vllm_amd.sampling_params import SamplingParams

    p = SamplingParams(temperature=0.0, max_tokens=n_tokens, ignore_eos=True)
    outs = llm.generate(prompts, p)
    outs2 = llm.generate(prompts, p)
    moe = _moe_layers(llm)
    state = [(getattr(m, "w13_int4", None), getattr(m, "w2_int4", None),
              m.w13.numel(), m.w2.numel()) for m in moe]
    llm.shutdown()
    assert all(len(o.outputs[0].token_ids) == n_tokens for o in outs)
    for a, b in zip(outs, outs2):
        assert a.outputs[0].token_ids == b.outputs[0].token_ids
    assert state
    for q13, q2, n13, n2 in state:
        assert q13 is not None and q2 is not None and n13 == 0 and n2 == 0


def test_engine_moe_int4_cpu_e2e():
    from vllm_amd.entrypoints.llm import LLM

    llm = LLM(model="tiny-mixtral", dtype="fp32", device="cpu",
              quantization="int4", block_size=16, num_gpu_blocks=128,
              max_model_len=256, max_num_batched_tokens=64, max_num_seqs=4)
    prompts = [[(i * 7 + j) % 900 + 3 for j in range(24)] for i in range(2)]
    _assert_quantized_and_repeatable(llm, prompts, 6)


def test_ref_fused_moe_int4_is_dequant_then_fused_moe():
    torch.manual_seed(0)
    T, H, I, E, k = 9, 128, 128, 4, 2
    w13 = torch.randn(E, 2 * I, H) * 0.2
    w2 = torch.randn(E, H, I) * 0.2
    w2[1] *= 30.0  # per-expert ranges differ
    q13, q2 = ref.quantize_experts_int4(w13), ref.quantize_experts_int4(w2)
    assert q13[0].shape == (E, 2 * I // 16, H // 128, 64, 4)
    hidden = torch.randn(T, H)
    tw, ti = ref.topk_softmax(torch.randn(T, E), k)
    d13 = torch.stack([ref.dequantize_weight_int4(*(t[e] for t in q13))
                       for e in range(E)])
    d2 = torch.stack([ref.dequantize_weight_int4(*(t[e] for t in q2))
                      for e in range(E)])
    got = ref.fused_moe_int4(hidden, *q13, *q2, tw, ti)
    assert torch.equal(got, ref.fused_moe(hidden, d13, d2, tw, ti))


# ------------------------------------------------------------------ GPU

E_, K_TOP, T_ = 4, 2, 65


def _gemm_case(K, N, seed):
    """Per-expert weights built directly (no min/max quantizer), drawn
    independently per expert: random codes, integer zeros differing per
    (expert, row, group), scales spread ~4x between neighbours. Routing
    is forced: every token picks expert 0, tokens 0..63 also expert 2,
    token 64 also expert 1, expert 3 gets nothing."""
    g = torch.Generator().manual_seed(seed)
    G = K // 128
    packed = []
    for e in range(E_):
        q = torch.randint(0, 16, (N, K), generator=g)
        z = torch.randint(0, 16, (N, G), generator=g)
        n_i = torch.arange(N).view(N, 1)
        g_i = torch.arange(G).view(1, G)
        s = (0.01 * 4.0 ** ((n_i + 2 * g_i + e) % 3)
             * (1 + torch.rand(N, G, generator=g))).to(torch.bfloat16)
        packed.append(ref.pack_weight_int4(q, s, z))
    qw, s, z = (torch.stack(t) for t in zip(*packed))
    ids = torch.zeros(T_, K_TOP, dtype=torch.int32)
    ids[:64, 1] = 2
    ids[64, 1] = 1
    return qw, s, z, ids, g


@pytest.mark.gpu
@pytest.mark.parametrize("use_topk_div", [True, False])
@pytest.mark.parametrize("K,N", [(128, 16), (384, 48), (256, 272)])
def test_hip_moe_gemm_w4a16(K, N, use_topk_div):
    from vllm_amd.ops import hip_ops as hip

    qw, s, z, ids, g = _gemm_case(K, N, seed=K + N)
    total = T_ * K_TOP
    em, sorted_ids, tiles, _ = hip._moe_align(ids.cuda(), E_, "cuda")
    sorted_c, tiles_c = sorted_ids.cpu(), tiles.cpu()
    valid = sorted_c < total
    # Tiles of 65 rows (64 + 1), 1 row and 64 rows; expert 3 has none.
    assert valid.view(-1, 64).sum(1).tolist() == [64, 1, 1, 64, 0, 0]
    assert tiles_c.tolist() == [0, 0, 1, 2, -1, -1]
    x = torch.randn(T_ if use_topk_div else em, K,
                    generator=g).to(torch.bfloat16)
    pos = valid.nonzero().flatten()
    rows = sorted_c[pos].long() // K_TOP if use_topk_div else pos
    experts = tiles_c[pos // 64].long()
    wd = torch.stack([ref.dequantize_weight_int4(qw[e], s[e], z[e])
                      for e in range(E_)]).double()
    xa = x.double()[rows]
    want = torch.einsum("pk,pnk->pn", xa, wd[experts])
    mag = torch.einsum("pk,pnk->pn", xa.abs(), wd[experts].abs())
    # bf16 rounding of each dequantized weight + bf16 rounding of the
    # output + fp32 accumulation (the bound test_hip_w4a16_gemm derives).
    tol = (2.0 ** -9 + 2.0 ** -9 + K * 2.0 ** -24) * mag

    sentinel = 12352.0  # exact in bf16
    args = [t.cuda() for t in (x, qw, s, z)]
    outs = []
    for _ in range(2):
        c = torch.full((em, N), sentinel, dtype=torch.bfloat16, device="cuda")
        torch.ops.vllm_amd.moe_gemm_w4a16(
            *args, c, sorted_ids, tiles, K_TOP if use_topk_div else 0, total)
        outs.append(c.cpu())
    err = (outs[0][pos].double() - want).abs()
    print(f"max err/tol = {(err / tol).max().item():.4f}")
    assert (err <= tol).all()
    assert torch.equal(outs[0], outs[1])
    assert (outs[0][~valid] == sentinel).all()


@pytest.mark.gpu
@pytest.mark.parametrize("T,H,I,E,k", [(1, 128, 128, 4, 2),
                                       (37, 256, 128, 16, 4)])
def test_hip_fused_moe_int4(T, H, I, E, k):
    from vllm_amd.ops import hip_ops as hip

    torch.manual_seed(0)
    hidden = torch.randn(T, H).to(torch.bfloat16) * 0.3
    q13 = ref.quantize_experts_int4(torch.randn(E, 2 * I, H) * 0.2)
    q2 = ref.quantize_experts_int4(torch.randn(E, H, I) * 0.2)
    tw, ti = ref.topk_softmax(torch.randn(T, E), k)
    expect = ref.fused_moe_int4(hidden.float(), *q13, *q2, tw, ti)
    out = hip.fused_moe_int4(hidden.cuda(), *(t.cuda() for t in q13 + q2),
                             tw.cuda(), ti.cuda())
    torch.testing.assert_close(out.float().cpu(), expect, atol=8e-2,
                               rtol=8e-2)


@pytest.mark.gpu
def test_engine_moe_int4_gpu_e2e():
    """tiny-mixtral-128 with quantization=int4 decodes on the GPU through
    the grouped W4A16 kernel, decode graphs enabled."""
    from vllm_amd.entrypoints.llm import LLM

    llm = LLM(model="tiny-mixtral-128", dtype="bf16", device="cuda",
              quantization="int4", block_size=64, num_gpu_blocks=256,
              max_model_len=512, max_num_batched_tokens=512,
              max_num_seqs=8)
    prompts = [[(i * 11 + j) % 900 + 3 for j in range(48)]
               for i in range(4)]
    _assert_quantized_and_repeatable(llm, prompts, 8)
