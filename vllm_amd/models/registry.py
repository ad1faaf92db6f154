"""Architecture registry (role of vllm/model_executor/models/registry.py:72)."""

from __future__ import annotations


import torch

from vllm_amd.config import ModelConfig


def get_model_class(architecture: str):
    if architecture in ("llama", "qwen2", "qwen3", "phi3"):
        # Qwen2/Qwen3/Phi-3 are llama-structured (reference qwen2.py /
        # qwen3.py / phi3.py); they differ only by spec knobs
        # (qkv_bias, qk_norm) and checkpoint fusion (phi3 loader).
        from vllm_amd.models.llama import LlamaForCausalLM

        return LlamaForCausalLM
    if architecture == "opt":
        from vllm_amd.models.opt import OPTForCausalLM

        return OPTForCausalLM
    if architecture in ("mixtral", "qwen3_moe"):
        # Qwen3-MoE is mixtral-structured + per-head qk-norm (spec knob).
        from vllm_amd.models.mixtral import MixtralForCausalLM

        return MixtralForCausalLM
    if architecture == "gemma3":
        from vllm_amd.models.gemma import GemmaForCausalLM

        return GemmaForCausalLM
    if architecture == "bart":
        from vllm_amd.models.bart import BartForConditionalGeneration

        return BartForConditionalGeneration
    if architecture == "whisper":
        from vllm_amd.models.whisper import WhisperForConditionalGeneration

        return WhisperForConditionalGeneration
    if architecture == "bert":
        from vllm_amd.models.bert_embed import BertEmbeddingModel

        return BertEmbeddingModel
    if architecture == "jamba":
        from vllm_amd.models.jamba import JambaForCausalLM

        return JambaForCausalLM
    if architecture == "mamba":
        from vllm_amd.models.mamba import MambaForCausalLM

        return MambaForCausalLM
    if architecture == "deepseek":
        from vllm_amd.models.deepseek import DeepseekForCausalLM

        return DeepseekForCausalLM
    raise ValueError(f"Unknown architecture: {architecture}")


def initialize_dummy_weights(model: torch.nn.Module, seed: int = 0) -> None:
    """Random-init all weights (reference dummy_loader.py:22 pattern) —
    the offline benchmark path; no checkpoints are available.

    PARTITION-INVARIANT across both parallel axes:
    - Seeded PER PARAMETER NAME (stable crc32), not by iteration order,
      so a pipeline-parallel stage holding layers [lo, hi) materializes
      exactly the weights a single-process model would.
    - TP-sharded layers expose dummy_shard_shapes()/dummy_shard(): the
      FULL-shape tensor is generated and each rank copies its slice
      through the same mapping the checkpoint loaders use — so tp=N
      dummy weights are exact slices of the tp=1 weights and tp2==tp1
      greedy outputs are bit-comparable (fp reduction order aside).
    """
    import math
    import zlib

    def gen_full(name: str, shape: tuple) -> torch.Tensor:
        gen = torch.Generator()
        gen.manual_seed(seed ^ zlib.crc32(name.encode()))
        cpu_val = torch.rand(shape, generator=gen,
                             dtype=torch.float32).mul_(2.0).sub_(1.0)
        # Scales chosen so the network is a FUNCTIONING transformer, not
        # a constant map: norm gains at ~1 and matrices at 1/sqrt(fan_in)
        # keep activations O(1) through deep stacks (RMSNorm re-centers
        # every layer), so outputs genuinely depend on inputs — an
        # all-tiny init drives fp32 logits to exactly-uniform and lets
        # equality-style e2e tests pass vacuously.
        if len(shape) == 1 and "norm" in name.lower():
            return 1.0 + 0.05 * cpu_val
        if len(shape) == 1:  # biases
            return 1e-3 * cpu_val
        fan_in = shape[-1] if len(shape) >= 2 else 1
        if len(shape) > 2 and "patch" in name.lower():
            fan_in = int(torch.tensor(shape[1:]).prod())
        return cpu_val.div_(math.sqrt(fan_in))

    # (numel, name, full shape, param, shard fn) per distinct parameter.
    # The CPU generator is serial, and every parameter has its own, so
    # the parameters are filled on a thread pool (largest first): the
    # values do not depend on the order or the number of threads.
    jobs = []
    handled: set[int] = set()
    for mod_name, mod in model.named_modules():
        shapes_fn = getattr(mod, "dummy_shard_shapes", None)
        if shapes_fn is None:
            continue
        for pname, full_shape in shapes_fn().items():
            param = getattr(mod, pname, None)
            if param is None or id(param) in handled:
                continue
            gname = f"{mod_name}.{pname}" if mod_name else pname
            shard = (lambda full, mod=mod, pname=pname:
                     mod.dummy_shard(pname, full))
            jobs.append((math.prod(full_shape), gname, tuple(full_shape),
                         param, shard))
            handled.add(id(param))
    for name, param in model.named_parameters():
        if id(param) in handled:
            continue
        handled.add(id(param))
        jobs.append((param.numel(), name, tuple(param.shape), param, None))

    def fill(job) -> None:
        _, name, shape, param, shard = job
        val = gen_full(name, shape)
        if shard is not None:
            val = shard(val)
        param.data.copy_(val.to(param.dtype))

    jobs.sort(key=lambda j: -j[0])
    from concurrent.futures import ThreadPoolExecutor

    with ThreadPoolExecutor(max_workers=max(1, torch.get_num_threads())) \
            as pool:
        list(pool.map(fill, jobs))


def load_model(config: ModelConfig, device: torch.device) -> torch.nn.Module:
    cls = get_model_class(config.spec.architecture)
    model = cls(config)
    if config.load_format == "dummy":
        initialize_dummy_weights(model, seed=config.seed)
    elif config.load_format == "safetensors":
        from vllm_amd.models.weight_loader import load_safetensors_weights

        load_safetensors_weights(model, config)
    elif config.load_format == "sharded":
        from vllm_amd.models.weight_loader import load_sharded_state

        load_sharded_state(model, config.model_path or config.model)
    else:
        raise ValueError(f"Unknown load_format {config.load_format}")
    model = model.to(device).eval()
    if config.quantization == "fp8":
        quantize_model_fp8(model)
    elif config.quantization == "int4":
        quantize_model_int4(model)
    return model


def quantize_model_fp8(model: torch.nn.Module) -> None:
    """Quantize every dense linear to W8A8 fp8 after load (per-channel
    weight scales; activations get per-token scales at run time). The
    lm_head stays in model dtype (logit sensitivity — same choice as the
    reference's fp8 config), as do MoE expert weights (grouped-GEMM path
    is bf16 this round) and the embedding."""
    from vllm_amd.layers.linear import (
        ColumnParallelLinear,
        ReplicatedLinear,
        RowParallelLinear,
    )

    for module in model.modules():
        if isinstance(module, (ColumnParallelLinear, RowParallelLinear,
                               ReplicatedLinear)):
            module.quantize_fp8()


def quantize_model_int4(model: torch.nn.Module) -> None:
    """Quantize every dense linear and every FusedMoE's expert weights to
    W4A16 after load and after TP/EP sharding (4-bit codes, bf16 scale +
    zero-point per 128-wide K group). lm_head and embedding stay in model
    dtype. A layer whose local shape the kernels cannot tile (linear:
    K % 128, N % 16; experts: H % 128, I % 128), a non-silu expert MLP
    and an EPLB layer are left in model dtype."""
    from vllm_amd.layers.fused_moe import FusedMoE
    from vllm_amd.layers.linear import (
        ColumnParallelLinear,
        ReplicatedLinear,
        RowParallelLinear,
    )

    for module in model.modules():
        if isinstance(module, (ColumnParallelLinear, RowParallelLinear,
                               ReplicatedLinear, FusedMoE)):
            module.quantize_int4()
