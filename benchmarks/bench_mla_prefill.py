"""MLA prefill attention: hip_ops.mla_attention (MFMA flash kernel,
csrc/mla_prefill.hip) against _torch_ref.mla_attention on the same GPU
tensors — the per-request torch composition that served these rows
before the kernel existed.

Pure-prefill batches at Hq 16 (TP=8 shard) and 128 (TP=1), bf16, cache
block size 64 over a permuted block table: from-scratch chunks of 512 and
2048 tokens, a 512-token chunk continuing an 8192-token context, and 64
speculative-verification requests of 4 tokens at context 4096.

Device events, both paths warmed up, the two paths alternated inside one
process, several repeats (median, min..max printed). FLOP/s counts
2 * rows * keys_seen * (576 + 512) over the kernel path's median time.
The last column is the largest absolute difference between the two
paths' outputs at that shape. Needs a GPU.

    python benchmarks/bench_mla_prefill.py [--repeats 5] [--iters 5]
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
SHAPES = [  # name, q_lens, ctx_lens
    ("scratch 512", [512], [512]),
    ("scratch 2048", [2048], [2048]),
    ("512 after 8192", [512], [8192 + 512]),
    ("verify 64 x 4 @ 4096", [4] * 64, [4096] * 64),
]
HEADS = [16, 128]


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


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_mla_prefill needs a GPU")
    dev = torch.device("cuda")
    torch.manual_seed(0)
    scale = (128 + 64) ** -0.5
    print("| shape | Hq | torch ms (min..max) | kernel ms (min..max) | "
          "torch/kernel | kernel TFLOP/s | kernel faster (max < torch min) "
          "| max abs diff |")
    print("|---|---|---|---|---|---|---|---|")
    for name, q_lens, ctx_lens in SHAPES:
        R, T = len(q_lens), sum(q_lens)
        nb = max(-(-c // BS) for c in ctx_lens)
        kv = (torch.randn(R * nb + 1, BS, 576, device=dev) * 0.5).to(
            torch.bfloat16)
        bt = (torch.randperm(R * nb, device=dev).int() + 1).view(R, nb)
        qsl = torch.tensor([0] + q_lens, device=dev).cumsum(0).int()
        seq_lens = torch.tensor(ctx_lens, dtype=torch.int32, device=dev)
        keys_seen = sum(ql * (c - ql) + ql * (ql + 1) // 2
                        for ql, c in zip(q_lens, ctx_lens))
        for Hq in HEADS:
            q_nope = (torch.randn(T, Hq, 512, device=dev) * 0.3).to(
                torch.bfloat16)
            q_pe = (torch.randn(T, Hq, 64, device=dev) * 0.3).to(
                torch.bfloat16)
            a = (q_nope, q_pe, kv, bt, qsl, seq_lens, scale)
            paths = [
                lambda: _torch_ref.mla_attention(*a),
                lambda: hip_ops.mla_attention(
                    *a, num_decodes=0, max_seq_len=max(ctx_lens),
                    max_query_len=max(q_lens)),
            ]
            # The torch path holds fp32 scores, probabilities and the
            # einsum operands of one request at a time.
            need = 3 * Hq * max(q * c for q, c in zip(q_lens, ctx_lens)) * 4
            fits = need < torch.cuda.mem_get_info()[0]
            live = paths if fits else paths[1:]
            outs = [fn() for fn in live]  # warm-up: code objects, GEMM algos
            for fn in live:
                time_ms(fn, 2)
            diff = ((outs[0].float() - outs[1].float()).abs().max().item()
                    if fits else float("nan"))
            t = [[], []]
            for _ in range(args.repeats):
                for i, fn in enumerate(paths):
                    if fits or i == 1:
                        t[i].append(time_ms(fn, args.iters))
            k_med = statistics.median(t[1])
            k_cell = f"{k_med:.3f} ({min(t[1]):.3f}..{max(t[1]):.3f})"
            tflops = 2 * Hq * keys_seen * (576 + 512) / (k_med * 1e-3) / 1e12
            if fits:
                t_med = statistics.median(t[0])
                t_cell = f"{t_med:.3f} ({min(t[0]):.3f}..{max(t[0]):.3f})"
                ratio = f"{t_med / k_med:.1f}"
                faster = "yes" if max(t[1]) < min(t[0]) else "no"
            else:
                t_cell = f"does not fit ({need / 2**30:.0f} GiB of scores)"
                ratio = faster = "-"
            print(f"| {name} | {Hq} | {t_cell} | {k_cell} | {ratio} | "
                  f"{tflops:.1f} | {faster} | {diff:.4f} |", flush=True)
            del outs
        del kv
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
