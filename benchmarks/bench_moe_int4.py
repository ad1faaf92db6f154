"""Int4 MoE expert MLP (ops.fused_moe_int4, grouped W4A16 dequant-GEMM)
against the bf16 grouped GEMM (ops.fused_moe, default staged-LDS path) on
the Mixtral-8x7B expert shapes: E=8, k=2, H=4096, I=14336 and the TP=8
shard I=1792.

Device events, both paths warmed up, the two paths alternated inside one
process, several repeats (median, min..max printed). Routing is uniform
random. One call at I=14336 streams more than the last-level cache
holds; at I=1792 each path rotates over enough weight copies (>= 1 GB of
bf16) that a call does not find its weights cached. Needs a GPU.

    python benchmarks/bench_moe_int4.py [--repeats 7] [--iters 48]
"""

from __future__ import annotations

import argparse
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from vllm_amd import ops  # noqa: E402

E, TOPK, H = 8, 2, 4096
INTERMEDIATE = [14336, 1792]
TS = [1, 16, 64, 256, 1024]


def time_ms(fn, iters):
    """Mean ms per call over `iters` back-to-back calls."""
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    start.record()
    for i in range(iters):
        fn(i)
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=48)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_moe_int4 needs a GPU")
    dev = torch.device("cuda")
    torch.manual_seed(0)
    print("| I | T | rows/expert | bf16 ms (min..max) | int4 ms (min..max) | "
          "bf16/int4 | int4 faster (max < bf16 min) |")
    print("|---|---|---|---|---|---|---|")
    for inter in INTERMEDIATE:
        w13 = (torch.randn(E, 2 * inter, H, device=dev) * 0.02).to(
            torch.bfloat16)
        w2 = (torch.randn(E, H, inter, device=dev) * 0.02).to(torch.bfloat16)
        w_bytes = (w13.numel() + w2.numel()) * 2
        copies = max(1, -(-(1 << 30) // w_bytes))
        q = ops.quantize_experts_int4(w13) + ops.quantize_experts_int4(w2)
        ws = [(w13.clone(), w2.clone()) for _ in range(copies)]
        qs = [[t.clone() for t in q] for _ in range(copies)]
        q_bytes = sum(t.numel() * t.element_size() for t in q)
        print(f"<!-- I={inter}: bf16 {w_bytes / 2**20:.0f} MiB, int4 "
              f"{q_bytes / 2**20:.0f} MiB per copy, {copies} copies -->")
        for T in TS:
            x = torch.randn(T, H, device=dev).to(torch.bfloat16)
            ids = torch.rand(T, E, device=dev).topk(TOPK, dim=1).indices.to(
                torch.int32)
            tw = torch.rand(T, TOPK, device=dev).softmax(dim=1)
            paths = [lambda i: ops.fused_moe(x, *ws[i % copies], tw, ids),
                     lambda i: ops.fused_moe_int4(x, *qs[i % copies], tw, ids)]
            iters = max(4, args.iters // max(1, T // 256))
            for fn in paths:  # warm-up: code objects
                time_ms(fn, max(3, copies))
            t = [[], []]
            for _ in range(args.repeats):
                for i, fn in enumerate(paths):
                    t[i].append(time_ms(fn, iters))
            med = [statistics.median(v) for v in t]
            cells = [f"{med[i]:.4f} ({min(t[i]):.4f}..{max(t[i]):.4f})"
                     for i in range(2)]
            faster = "yes" if max(t[1]) < min(t[0]) else "no"
            print(f"| {inter} | {T} | {T * TOPK / E:g} | {cells[0]} | "
                  f"{cells[1]} | {med[0] / med[1]:.2f} | {faster} |",
                  flush=True)
        del ws, qs, q, w13, w2
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
