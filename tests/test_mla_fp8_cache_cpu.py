"""fp8 (e4m3) latent KV cache for MLA: the reference write saturates,
attention over the cache equals attention over its values, and the engine
allocates what kv_cache_dtype="fp8" asks for."""

import torch

from vllm_amd.ops import _torch_ref as ref

FP8 = torch.float8_e4m3fn


def test_ref_write_then_attention_over_fp8_cache():
    torch.manual_seed(0)
    lora, rope, bs, T, Hq = 64, 16, 16, 20, 4
    c_kv, k_pe = torch.randn(T, lora), torch.randn(T, rope)
    c_kv[3, 5], k_pe[9, 0] = 500.0, -1000.0
    slots = torch.randperm(2 * bs)[:T] + bs  # blocks 1 and 2
    cache = torch.zeros(3, bs, lora + rope, dtype=FP8)
    ref.concat_and_cache_mla(c_kv, k_pe, cache, slots)

    quant = torch.cat([c_kv, k_pe], 1).clamp(-448, 448).to(FP8).float()
    assert not quant.isnan().any() and quant.abs().max() == 448
    dense = torch.zeros(3 * bs, lora + rope)
    dense[slots] = quant
    assert torch.equal(cache.float().view(3 * bs, -1), dense)

    q_nope, q_pe = torch.randn(1, Hq, lora), torch.randn(1, Hq, rope)
    args = (torch.tensor([[1, 2]], dtype=torch.int32),
            torch.tensor([0, 1], dtype=torch.int32),
            torch.tensor([2 * bs], dtype=torch.int32), 0.1)
    assert torch.equal(ref.mla_attention(q_nope, q_pe, cache, *args),
                       ref.mla_attention(q_nope, q_pe, dense.view(3, bs, -1),
                                         *args))


def test_cpu_engine_allocates_fp8_mla_cache():
    from vllm_amd.entrypoints.llm import LLM
    from vllm_amd.sampling_params import SamplingParams

    llm = LLM(model="tiny-deepseek", dtype="fp32", device="cpu",
              block_size=16, num_gpu_blocks=32, max_model_len=128,
              max_num_batched_tokens=32, max_num_seqs=2,
              kv_cache_dtype="fp8")
    runner = llm.engine.engine_core.worker.runner
    assert runner.kv_caches
    assert all(c.dtype == FP8 for c in runner.kv_caches)
    assert runner.kv_cache_page_bytes() == sum(
        c[0].numel() * c.element_size() for c in runner.kv_caches)
    outs = llm.generate(
        [[3, 4, 5, 6, 7]],
        SamplingParams(temperature=0.0, max_tokens=3, ignore_eos=True))
    llm.shutdown()
    assert len(outs[0].outputs[0].token_ids) == 3
