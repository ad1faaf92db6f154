"""GPU microbenchmark of the hand-written kernels between qkv_proj and
o_proj at the flagship decode shapes (not a pytest file). Run on the GPU box:

    python benchmarks/bench_decode_path.py [--repeats 3] [--decode-only]

Times, at n in {256, 1024} decode rows, Hq=32, Hkv=8, D=128, block 64:
  * apply_rope + reshape_and_cache (two launches) against rope_and_cache;
  * decode attention at ctx in {144, 176, 1024, 4096}, as KV TB/s next to
    the device copy bandwidth measured in the same run.
Every figure is printed once per repeat so the spread is visible.
"""

import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HQ, HKV, D, BS = 32, 8, 128, 64


def timed(fn, iters=50, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def fmt(vals, unit, scale=1.0):
    return "  ".join(f"{v * scale:8.2f}" for v in vals) + f"  {unit}"


def bench_copy(repeats):
    n = 512 * 1024 * 1024 // 2
    a = torch.empty(n, dtype=torch.bfloat16, device="cuda")
    b = torch.empty_like(a)
    bw = [2 * n * 2 / timed(lambda: b.copy_(a)) / 1e12 for _ in range(repeats)]
    print(f"copy 512 MiB:                      {fmt(bw, 'TB/s')}")


def bench_rope_cache(hip_ops, n, repeats):
    rot, max_pos = D, 4096
    inv = 1.0 / (500000.0 ** (torch.arange(0, rot, 2).float() / rot))
    freqs = torch.outer(torch.arange(max_pos).float(), inv)
    cs = torch.cat([freqs.cos(), freqs.sin()], dim=-1).cuda()
    qkv = torch.randn(n, (HQ + 2 * HKV) * D, dtype=torch.bfloat16,
                      device="cuda")
    q = qkv[:, :HQ * D].view(n, HQ, D)
    k = qkv[:, HQ * D:(HQ + HKV) * D].view(n, HKV, D)
    v = qkv[:, (HQ + HKV) * D:].view(n, HKV, D)
    nb = n * 3 + 1
    cache = torch.zeros(2, nb, HKV, BS, D, dtype=torch.bfloat16,
                        device="cuda")
    pos = torch.randint(136, 176, (n,), device="cuda")
    # One slot per row, each in a block of its own, as in decode.
    slots = (torch.arange(n, device="cuda") * 3 + 3) * BS + pos % BS

    def pair():
        hip_ops.apply_rope(pos, q, k, cs, rot)
        hip_ops.reshape_and_cache(k, v, cache, slots)

    def fused():
        hip_ops.rope_and_cache(pos, q, k, v, cs, rot, cache, slots)

    tp = [timed(pair) for _ in range(repeats)]
    tf = [timed(fused) for _ in range(repeats)]
    print(f"n={n:5d} rope + reshape_and_cache:   {fmt(tp, 'us', 1e6)}")
    print(f"n={n:5d} rope_and_cache (fused):     {fmt(tf, 'us', 1e6)}")


def bench_decode(hip_ops, n, ctx, repeats):
    nb_per = (ctx + BS - 1) // BS
    cache = torch.randn(2, n * nb_per + 1, HKV, BS, D, dtype=torch.bfloat16,
                        device="cuda")
    q = torch.randn(n, HQ, D, dtype=torch.bfloat16, device="cuda")
    bt = torch.arange(1, n * nb_per + 1, dtype=torch.int32,
                      device="cuda").reshape(n, nb_per)
    qsl = torch.arange(n + 1, dtype=torch.int32, device="cuda")
    sl = torch.full((n,), ctx, dtype=torch.int32, device="cuda")

    def run():
        hip_ops.attention_unified(q, cache, bt, qsl, sl, D**-0.5,
                                  num_decodes=n, max_seq_len=ctx,
                                  max_query_len=1)

    iters = 50 if n * ctx <= 1024 * 1024 else 20
    ts = [timed(run, iters=iters) for _ in range(repeats)]
    kv_bytes = n * ctx * HKV * D * 2 * 2
    print(f"n={n:5d} decode_attn ctx={ctx:5d}:       {fmt(ts, 'us', 1e6)}"
          f"   KV {fmt([kv_bytes / t / 1e12 for t in ts], 'TB/s')}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--decode-only", action="store_true",
                    help="skip the rope/cache part (trees without the op)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    from vllm_amd.ops import hip_ops

    print(torch.cuda.get_device_name(0))
    bench_copy(args.repeats)
    for n in (256, 1024):
        if not args.decode_only:
            bench_rope_cache(hip_ops, n, args.repeats)
        for ctx in (144, 176, 1024, 4096):
            bench_decode(hip_ops, n, ctx, args.repeats)


if __name__ == "__main__":
    main()
