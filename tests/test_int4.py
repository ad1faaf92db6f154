"""W4A16 (--quantization int4): quantizer contract, packed layout, the
gfx950 dequant-GEMM against an fp64 reference, and the engine wiring."""

import pytest
import torch

from vllm_amd import ops
from vllm_amd.ops import _torch_ref as ref


def test_int4_round_trip_and_footprint():
    torch.manual_seed(0)
    N, K = 96, 384
    w = torch.randn(N, K)
    w[5] *= 100.0
    qw, s, z = ops.quantize_weight_int4(w)
    # Half a step from rounding q, up to half a step where the rounded z
    # pushes a range end into the clamp, 15*2^-9 of a step from storing
    # s in bf16.
    s_full = (s.float().view(N // 16, K // 128, 16).permute(0, 2, 1)
              .reshape(N, K // 128).repeat_interleave(128, dim=1))
    err = (ref.dequantize_weight_int4(qw, s, z) - w).abs()
    assert (err <= (1 + 2.0 ** -4) * s_full).all()
    nbytes = sum(t.numel() * t.element_size() for t in (qw, s, z))
    assert nbytes <= N * K * (0.5 + 4 / 128)


def test_engine_int4_cpu_e2e():
    from vllm_amd.entrypoints.llm import LLM
    from vllm_amd.sampling_params import SamplingParams

    llm = LLM(model="tiny-llama", dtype="fp32", device="cpu",
              quantization="int4", block_size=16, num_gpu_blocks=128,
              max_model_len=256, max_num_batched_tokens=64, max_num_seqs=4)
    prompts = [[(i * 7 + j) % 900 + 3 for j in range(24)] for i in range(2)]
    p = SamplingParams(temperature=0.0, max_tokens=6, ignore_eos=True)
    outs = llm.generate(prompts, p)
    outs2 = llm.generate(prompts, p)
    model = llm.engine.engine_core.worker.runner.model
    quantized = [m for m in model.modules()
                 if getattr(m, "weight_int4", None) is not None]
    llm.shutdown()
    assert all(len(o.outputs[0].token_ids) == 6 for o in outs)
    for a, b in zip(outs, outs2):
        assert a.outputs[0].token_ids == b.outputs[0].token_ids
    assert quantized and all(m.weight.numel() == 0 for m in quantized)


# ------------------------------------------------------------------ GPU

def _direct_case(M, N, K, seed):
    """Inputs built directly (no min/max quantizer): random codes, integer
    zeros differing per (row, group), scales spread ~4x between
    neighbouring groups and rows."""
    g = torch.Generator().manual_seed(seed)
    G = K // 128
    q = torch.randint(0, 16, (N, K), generator=g)
    z = torch.randint(0, 16, (N, G), generator=g)
    n_i = torch.arange(N).view(N, 1)
    g_i = torch.arange(G).view(1, G)
    s = (0.01 * 4.0 ** ((n_i + 2 * g_i) % 3)
         * (1 + torch.rand(N, G, generator=g))).to(torch.bfloat16)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16)
    bias = torch.randn(N, generator=g).to(torch.bfloat16)
    return x, ref.pack_weight_int4(q, s, z), bias


@pytest.mark.gpu
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("M,N,K", [
    (1, 16, 128), (16, 80, 384), (17, 80, 384), (33, 32, 128),
    (65, 48, 256), (130, 1024, 512)])
def test_hip_w4a16_gemm(M, N, K, with_bias):
    x, (qw, s, z), bias = _direct_case(M, N, K, seed=M + N + K)
    wd = ref.dequantize_weight_int4(qw, s, z).double()
    want = x.double() @ wd.T
    mag = x.double().abs() @ wd.abs().T
    if with_bias:
        want = want + bias.double()
        mag = mag + bias.double().abs()
    # bf16 rounding of each dequantized weight + bf16 rounding of the
    # output + fp32 accumulation.
    tol = (2.0 ** -9 + 2.0 ** -9 + K * 2.0 ** -24) * mag
    args = [t.cuda() for t in (x, qw, s, z)]
    b = bias.cuda() if with_bias else None
    y = ops.linear_int4(*args, b)
    y2 = ops.linear_int4(*args, b)
    assert y.dtype == torch.bfloat16 and y.shape == (M, N)
    err = (y.cpu().double() - want).abs()
    print(f"max err/tol = {(err / tol).max().item():.4f}")
    assert (err <= tol).all()
    assert torch.equal(y, y2)


@pytest.mark.gpu
def test_engine_int4_gpu_e2e():
    """tiny-llama-128 with quantization=int4 decodes on the GPU through
    the W4A16 kernel, decode graphs enabled."""
    from vllm_amd.entrypoints.llm import LLM
    from vllm_amd.sampling_params import SamplingParams

    llm = LLM(model="tiny-llama-128", dtype="bf16", device="cuda",
              quantization="int4", block_size=64, num_gpu_blocks=256,
              max_model_len=512, max_num_batched_tokens=512,
              max_num_seqs=8)
    prompts = [[(i * 11 + j) % 900 + 3 for j in range(48)]
               for i in range(4)]
    p = SamplingParams(temperature=0.0, max_tokens=8, ignore_eos=True)
    outs = llm.generate(prompts, p)
    outs2 = llm.generate(prompts, p)
    model = llm.engine.engine_core.worker.runner.model
    n_q = sum(1 for m in model.modules()
              if getattr(m, "weight_int4", None) is not None)
    llm.shutdown()
    assert all(len(o.outputs[0].token_ids) == 8 for o in outs)
    for a, b in zip(outs, outs2):
        assert a.outputs[0].token_ids == b.outputs[0].token_ids
    assert n_q > 0
