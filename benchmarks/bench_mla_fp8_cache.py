"""fp8 (e4m3) latent KV cache for MLA against the bf16 cache: one layer's
ops.mla_attention over an fp8 cache and over the same values held in
bf16, plus the HIP cache write against the torch index_put composition it
replaced.

Decode: batch 128 at context 4096 and 16384, Hq 16 (TP=8 shard) and 128
(TP=1). Prefill: a 2048-token chunk from scratch and a 512-token chunk
continuing an 8192-token context. Cache block size 64 over a permuted
block table. The bf16 cache is the fp8 cache dequantised, so both kernels
do the same arithmetic and the last column (largest absolute difference
of the two outputs) is expected to be 0. Write: T = 128 and 2048 rows of
512 + 64 bf16 values into a bf16 and into an fp8 cache.

Device events, both paths warmed up, the two paths alternated inside one
process, several repeats (median, min..max printed). GB/s counts the
cache bytes a decode step has to stream (context x 576 x element size per
request, once) over the median time. Needs a GPU.

    python benchmarks/bench_mla_fp8_cache.py [--repeats 7] [--iters 20]
"""

from __future__ import annotations

import argparse
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from vllm_amd.ops import _torch_ref, hip_ops  # noqa: E402

BS = 64
FP8 = torch.float8_e4m3fn
DECODE = [(128, 4096), (128, 16384)]  # batch, context
PREFILL = [  # name, q_lens, ctx_lens
    ("scratch 2048", [2048], [2048]),
    ("512 after 8192", [512], [8192 + 512]),
]
HEADS = [16, 128]
WRITE_T = [128, 2048]


def time_ms(fn, iters):
    """Mean ms per call over `iters` back-to-back calls."""
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def compare(paths, repeats, iters):
    """Alternate the two callables; [(median, min, max)] per path."""
    for fn in paths:  # warm-up: code objects, allocator
        fn()
        time_ms(fn, 2)
    t = [[] for _ in paths]
    for _ in range(repeats):
        for i, fn in enumerate(paths):
            t[i].append(time_ms(fn, iters))
    return [(statistics.median(x), min(x), max(x)) for x in t]


def cell(s):
    return f"{s[0]:.3f} ({s[1]:.3f}..{s[2]:.3f})"


def caches(num_blocks, dev):
    """The same latent values as an fp8 cache and as a bf16 cache."""
    kv8 = torch.empty(num_blocks, BS, 576, dtype=FP8, device=dev)
    step = 4096  # quantise in slices: the fp32 staging stays small
    for b in range(0, num_blocks, step):
        n = min(step, num_blocks - b)
        kv8[b:b + n] = (torch.randn(n, BS, 576, device=dev) * 0.5).to(FP8)
    return kv8, kv8.to(torch.bfloat16)


def bench_attention(args, dev, scale):
    print("| shape | Hq | bf16 cache ms (min..max) | fp8 cache ms (min..max) "
          "| bf16/fp8 | fp8 GB/s | fp8 faster (max < bf16 min) "
          "| max abs diff |")
    print("|---|---|---|---|---|---|---|---|")
    shapes = [(f"decode {b} x {c}", [1] * b, [c] * b, b)
              for b, c in DECODE]
    shapes += [(name, ql, cl, 0) for name, ql, cl in PREFILL]
    for name, q_lens, ctx_lens, num_decodes in shapes:
        R, T = len(q_lens), sum(q_lens)
        nb = max(-(-c // BS) for c in ctx_lens)
        kv8, kv16 = caches(R * nb + 1, dev)
        bt = (torch.randperm(R * nb, device=dev).int() + 1).view(R, nb)
        qsl = torch.tensor([0] + q_lens, device=dev).cumsum(0).int()
        seq_lens = torch.tensor(ctx_lens, dtype=torch.int32, device=dev)
        hints = dict(num_decodes=num_decodes, max_seq_len=max(ctx_lens),
                     max_query_len=max(q_lens))
        for Hq in HEADS:
            q_nope = (torch.randn(T, Hq, 512, device=dev) * 0.3).to(
                torch.bfloat16)
            q_pe = (torch.randn(T, Hq, 64, device=dev) * 0.3).to(
                torch.bfloat16)

            def run(kv):
                return hip_ops.mla_attention(q_nope, q_pe, kv, bt, qsl,
                                             seq_lens, scale, **hints)

            diff = (run(kv16).float() - run(kv8).float()).abs().max().item()
            s16, s8 = compare([lambda: run(kv16), lambda: run(kv8)],
                              args.repeats, args.iters)
            gbs = (f"{sum(ctx_lens) * 576 / (s8[0] * 1e-3) / 1e9:.0f}"
                   if num_decodes else "-")
            faster = "yes" if s8[2] < s16[1] else "no"
            print(f"| {name} | {Hq} | {cell(s16)} | {cell(s8)} | "
                  f"{s16[0] / s8[0]:.2f} | {gbs} | {faster} | {diff:.4f} |",
                  flush=True)
        del kv8, kv16
        torch.cuda.empty_cache()


def bench_write(args, dev):
    print()
    print("| T | cache | torch index_put ms (min..max) | kernel ms "
          "(min..max) | torch/kernel | kernel faster (max < torch min) |")
    print("|---|---|---|---|---|---|")
    for T in WRITE_T:
        c_kv = torch.randn(T, 512, device=dev).to(torch.bfloat16)
        k_pe = torch.randn(T, 64, device=dev).to(torch.bfloat16)
        nb = -(-T // BS) * 2
        slots = torch.randperm(nb * BS, device=dev)[:T]
        for cdt, label in ((torch.bfloat16, "bf16"), (FP8, "fp8")):
            cache = torch.zeros(nb, BS, 576, dtype=cdt, device=dev)
            a = (c_kv, k_pe, cache, slots)
            st, sk = compare(
                [lambda: _torch_ref.concat_and_cache_mla(*a),
                 lambda: hip_ops.concat_and_cache_mla(*a)],
                args.repeats, args.iters)
            faster = "yes" if sk[2] < st[1] else "no"
            print(f"| {T} | {label} | {cell(st)} | {cell(sk)} | "
                  f"{st[0] / sk[0]:.1f} | {faster} |", flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_mla_fp8_cache needs a GPU")
    dev = torch.device("cuda")
    torch.manual_seed(0)
    bench_attention(args, dev, (128 + 64) ** -0.5)
    bench_write(args, dev)


if __name__ == "__main__":
    main()
