"""W4A16 dequant-GEMM (ops.linear_int4) against the bf16 hipBLASLt GEMM
(ops.linear) on the Llama-3-8B layer shapes.

Device events, both paths warmed up, the two paths alternated inside one
process, several repeats (median, min..max printed). Each path rotates
over enough weight copies (>= 512 MB of bf16) that a call does not find
its weights in the last-level cache, as in a decode step that walks the
layers. Needs a GPU.

    python benchmarks/bench_w4a16.py [--repeats 7] [--iters 96]
"""

from __future__ import annotations

import argparse
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from vllm_amd import ops  # noqa: E402

SHAPES = [(6144, 4096), (4096, 4096), (28672, 4096), (4096, 14336)]  # N, K
MS = [1, 16, 64, 256, 1024, 4096]


def time_ms(fn, iters):
    """Mean ms per call over `iters` back-to-back launches."""
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
    ap.add_argument("--iters", type=int, default=96)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_w4a16 needs a GPU")
    dev = torch.device("cuda")
    torch.manual_seed(0)
    print("| N | K | M | bf16 ms (min..max) | int4 ms (min..max) | "
          "bf16 weight GB/s | int4 weight GB/s | bf16/int4 |")
    print("|---|---|---|---|---|---|---|---|")
    for N, K in SHAPES:
        w = (torch.randn(N, K, device=dev) * 0.02).to(torch.bfloat16)
        copies = -(-(512 << 20) // (w.numel() * 2))
        ws = [w.clone() for _ in range(copies)]
        qs = [[t.clone() for t in ops.quantize_weight_int4(w)]
              for _ in range(copies)]
        qw, s, z = qs[0]
        w_bytes = w.numel() * 2
        q_bytes = sum(t.numel() * t.element_size() for t in (qw, s, z))
        for M in MS:
            x = torch.randn(M, K, device=dev).to(torch.bfloat16)
            paths = [lambda i: ops.linear(x, ws[i % copies]),
                     lambda i: ops.linear_int4(x, *qs[i % copies])]
            iters = max(2, args.iters // max(1, M // 256))
            for fn in paths:  # warm-up: code objects, hipBLASLt algo search
                time_ms(fn, 3)
            t = [[], []]
            for _ in range(args.repeats):
                for i, fn in enumerate(paths):
                    t[i].append(time_ms(fn, iters))
            med = [statistics.median(v) for v in t]
            cells = [f"{med[i]:.4f} ({min(t[i]):.4f}..{max(t[i]):.4f})"
                     for i in range(2)]
            print(f"| {N} | {K} | {M} | {cells[0]} | {cells[1]} | "
                  f"{w_bytes / med[0] / 1e6:.0f} | "
                  f"{q_bytes / med[1] / 1e6:.0f} | "
                  f"{med[0] / med[1]:.2f} |", flush=True)


if __name__ == "__main__":
    main()
