// Grouped W4A16 dequant-GEMM for MoE experts on CDNA4 (gfx950):
//   C[p, n] = sum_k A[row(p), k] * W~[expert(p)][n, k]
// bf16 A and C, fp32 accumulation, expert weights as 4-bit codes with one
// bf16 scale and one integer zero-point per (row, 128-wide K group):
// W~[n,k] = (q[n,k] - z[n,g]) * s[n,g]. Rows p are the sorted, BM=64
// aligned positions moe_align (moe.hip) produces; sorted / expert_tiles /
// topk_div / total_flat mean exactly what they mean for moe_gemm.
//
// Weight layout: the dense W4A16 consumer layout (gemm_w4a16.hip,
// ops/_torch_ref.pack_weight_int4) with a leading expert dimension:
//   qweight int32 [E][N/16][K/128][64 lanes][4]
//   scales  bf16  [E][N/16][K/128][16]
//   zeros   uint8 [E][N/16][K/128][16]
// One 16 B load per lane is the 4 MFMA K-steps of one quantization group
// of one 16-column n-tile.
//
// Work split: a block owns one 64-row m-tile and a strip of NW*NT
// n-tiles. Wave w owns n-tiles strip*NW*NT + w*NT + t over the whole K
// range: no cross-wave reduction, no atomics, no workspace, so the
// result is bit-identical run to run and the layer stays capturable.
//
// A goes through LDS, one K group (64 rows x 128 K = 16 KB) at a time,
// gathered through sorted/topk_div with zero rows for padding, XOR
// swizzled so the 16-row fragment reads are conflict-free, and double
// buffered: group g+1 is loaded from global into registers before group
// g is consumed and written to the other buffer after it, with one
// barrier per group. Every wave of the block shares the stage.
//
// Weight codes go from HBM straight into registers, PF groups ahead of
// use. Each slot of the prefetch ring is refilled right after the A
// loads of the iteration are issued, so the wait in front of the LDS
// write (the oldest loads) leaves the weight stream in flight.
//
// Dequant stays on exact integers: ((w >> 4p) & 0x000F000F) | 0x43004300
// is the bf16 pair (128+q, 128+q'). The zero-point is not a second MFMA
// per n-tile: once per (group, m-frag) one MFMA against an all-ones B
// fragment leaves the group's row sums r[m] in every column of a C
// fragment, and per lane tot += s[n] * (acc - (128 + z[n]) * r[m]).
// That is 1 + 1/NT MFMAs per (K-step, n-tile, m-frag). No weight is
// rounded to bf16; the scale is folded into fp32 once per group.
//
// Valid rows of a tile are a prefix (moe_align fills each expert's range
// from the front), so m-frags past the last valid row are skipped
// block-wide: not staged, not multiplied, not stored.

#include <torch/all.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime.h>

#include "common.h"

namespace vllm_amd {

namespace moe_w4a16 {

constexpr int BM = 64;       // rows per m-tile == moe::BM
constexpr int GROUP = 128;   // K values per (scale, zero) pair
constexpr int NW = 4;        // waves per block
constexpr int NT = 2;        // n-tiles per wave
constexpr int PF = 3;        // weight groups in flight ahead of use
constexpr int THREADS = NW * WAVE_SIZE;
constexpr int TILE_BYTES = BM * GROUP * 2;         // 16 KB
// One stage buffer: the tile plus a 256 B sink. A thread that owns a
// chunk of a padding row stores into the sink, so the row keeps the
// zeros written before the loop.
constexpr int STAGE_BYTES = TILE_BYTES + 256;
constexpr int ROWS_PER_IT = THREADS / 16;          // rows staged per pass
static_assert(ROWS_PER_IT == 16, "one staging pass per m-frag");

// A stage rows are 256 B = 16 chunks of 16 B; chunk ^= row & 15 spreads
// the 16 rows of a fragment read over 16 distinct chunks.
DEVINL int swz16(int row, int chunk) {
  return row * 256 + ((chunk ^ (row & 15)) << 4);
}

struct WSlot {
  i32x4 w[NT];
  short s[NT];
  uint8_t z[NT];
};

// One K group for the first NMF m-frags of the tile.
template <int NMF>
DEVINL void consume_group(const char* __restrict__ stage, const WSlot& cur,
                          int l16, int l4, f32x4 (&tot)[NMF][NT]) {
  const s16x8 ones = {0x3F80, 0x3F80, 0x3F80, 0x3F80,
                      0x3F80, 0x3F80, 0x3F80, 0x3F80};
  f32x4 acc[NMF][NT];
  f32x4 rs[NMF];
#pragma unroll
  for (int mf = 0; mf < NMF; ++mf) {
    rs[mf] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[mf][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    s16x8 bfrag[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      i32x4 bw;
#pragma unroll
      for (int p = 0; p < 4; ++p)
        bw[p] = (int)((((uint32_t)cur.w[t][j] >> (4 * p)) & 0x000F000Fu) |
                      0x43004300u);
      bfrag[t] = __builtin_bit_cast(s16x8, bw);
    }
#pragma unroll
    for (int mf = 0; mf < NMF; ++mf) {
      // A-frag: lane&15 = row, k = j*32 + l4*8 + e -> chunk j*4 + l4.
      const s16x8 a = *reinterpret_cast<const s16x8*>(
          stage + swz16(mf * 16 + l16, j * 4 + l4));
      rs[mf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, ones, rs[mf], 0, 0,
                                                       0);
#pragma unroll
      for (int t = 0; t < NT; ++t)
        acc[mf][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            a, bfrag[t], acc[mf][t], 0, 0, 0);
    }
  }
  // C-frag col = lane&15 (the column whose s, z this lane loaded),
  // row = l4*4 + r; rs holds the row sum in every column.
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const float s = bf16_to_f32(cur.s[t]);
    const float zc = 128.f + (float)cur.z[t];
#pragma unroll
    for (int mf = 0; mf < NMF; ++mf)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        tot[mf][t][r] += s * __builtin_fmaf(-zc, rs[mf][r], acc[mf][t][r]);
  }
}

// The K loop for a tile whose first NMF m-frags hold its valid rows.
// Branch-free apart from the block-uniform loop exit: a conditional load
// or store inside the loop makes the compiler drain every outstanding
// load (vmcnt(0)) where the branches join, which empties the weight
// stream, and a select on the loaded value is scheduled right behind the
// load with the same effect. So padding rows load row 0 and store it to
// the sink, a group index past the end is clamped, and an n-tile past
// N/16 re-reads the last one (in bounds) and is masked at the store.
template <int NMF>
DEVINL void run_tile(const short* __restrict__ A, long lda,
                     const i32x4* __restrict__ QW,
                     const short* __restrict__ S,
                     const uint8_t* __restrict__ Z, short* __restrict__ C,
                     long ldc, char* a_lds, const int* rows_sh, int tile_m,
                     int expert, int ntiles, int G) {
  const int tid = threadIdx.x;
  const int wave = tid / WAVE_SIZE;
  const int lane = tid % WAVE_SIZE;
  const int l16 = lane & 15;
  const int l4 = lane >> 4;

  // A staging: per staged m-frag the thread owns 16 B chunk tid & 15 of
  // row mf*16 + (tid >> 4); 16 lanes read one row's 256 contiguous bytes.
  const short* a_src[NMF];
  int a_dst[NMF];
#pragma unroll
  for (int mf = 0; mf < NMF; ++mf) {
    const int row = mf * ROWS_PER_IT + (tid >> 4);
    const int chunk = tid & 15;
    const int arow = rows_sh[row];
    a_src[mf] = A + (long)(arow >= 0 ? arow : 0) * lda + chunk * 8;
    a_dst[mf] = arow >= 0 ? swz16(row, chunk) : TILE_BYTES + chunk * 16;
    if (arow < 0) {
      const s16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
      *reinterpret_cast<s16x8*>(a_lds + swz16(row, chunk)) = zero;
      *reinterpret_cast<s16x8*>(a_lds + STAGE_BYTES + swz16(row, chunk)) =
          zero;
    }
  }
  auto load_a = [&](int g, s16x8 (&v)[NMF]) {
#pragma unroll
    for (int mf = 0; mf < NMF; ++mf)
      v[mf] = *reinterpret_cast<const s16x8*>(a_src[mf] + (long)g * GROUP);
  };
  auto store_a = [&](int buf, const s16x8 (&v)[NMF]) {
#pragma unroll
    for (int mf = 0; mf < NMF; ++mf)
      *reinterpret_cast<s16x8*>(a_lds + buf * STAGE_BYTES + a_dst[mf]) =
          v[mf];
  };

  const int nt0 = (blockIdx.x * NW + wave) * NT;
  const i32x4* qp[NT];
  const short* sp[NT];
  const uint8_t* zp[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int nt = nt0 + t < ntiles ? nt0 + t : ntiles - 1;
    const long base = ((long)expert * ntiles + nt) * G;
    qp[t] = QW + base * WAVE_SIZE + lane;
    sp[t] = S + base * 16 + l16;
    zp[t] = Z + base * 16 + l16;
  }
  auto load_w = [&](int g, WSlot& slot) {
    const int gc = g < G ? g : G - 1;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      slot.w[t] = qp[t][(long)gc * WAVE_SIZE];
      slot.s[t] = sp[t][gc * 16];
      slot.z[t] = zp[t][gc * 16];
    }
  };

  f32x4 tot[NMF][NT];
#pragma unroll
  for (int mf = 0; mf < NMF; ++mf)
#pragma unroll
    for (int t = 0; t < NT; ++t) tot[mf][t] = f32x4{0.f, 0.f, 0.f, 0.f};

  WSlot ring[PF];
  {
    s16x8 a0[NMF];
    load_a(0, a0);
#pragma unroll
    for (int u = 0; u < PF; ++u) load_w(u, ring[u]);
    store_a(0, a0);
  }
  __syncthreads();

  for (int g0 = 0; g0 < G; g0 += PF) {
#pragma unroll
    for (int u = 0; u < PF; ++u) {
      const int g = g0 + u;
      if (g >= G) break;  // block-uniform
      // Oldest first: A of the next group, then the ring refill. The
      // wait in front of store_a then leaves the refill in flight. The
      // last group re-stages itself into the idle buffer.
      s16x8 an[NMF];
      load_a(g + 1 < G ? g + 1 : g, an);
      const WSlot cur = ring[u];
      load_w(g + PF, ring[u]);
      consume_group<NMF>(a_lds + (g & 1) * STAGE_BYTES, cur, l16, l4, tot);
      store_a((g + 1) & 1, an);
      __syncthreads();
    }
  }

  // Epilogue: C rows are sorted positions; padding rows are not written.
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    if (nt0 + t >= ntiles) continue;
    const int n = (nt0 + t) * 16 + l16;
#pragma unroll
    for (int mf = 0; mf < NMF; ++mf) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = mf * 16 + l4 * 4 + r;
        if (rows_sh[row] >= 0)
          C[(long)(tile_m * BM + row) * ldc + n] = f32_to_bf16(tot[mf][t][r]);
      }
    }
  }
}

__launch_bounds__(THREADS) __global__
void moe_gemm_w4a16_kernel(const short* __restrict__ A, long lda,
                           const i32x4* __restrict__ QW,
                           const short* __restrict__ S,
                           const uint8_t* __restrict__ Z,
                           short* __restrict__ C, long ldc,
                           const int* __restrict__ sorted,
                           const int* __restrict__ expert_tiles, int E,
                           int ntiles, int G, int topk_div, int total_flat) {
  const int tile_m = blockIdx.y;
  const int expert = expert_tiles[tile_m];
  if (expert < 0 || expert >= E) return;  // padding tile

  __shared__ __attribute__((aligned(16))) char a_lds[2 * STAGE_BYTES];
  __shared__ int rows_sh[BM];  // A source row per tile row, -1 = padding
  __shared__ int nmf_sh;       // m-frags up to the last valid row

  const int tid = threadIdx.x;
  if (tid < BM) {  // exactly wave 0
    const int sid = sorted[tile_m * BM + tid];
    const bool valid = sid >= 0 && sid < total_flat;
    rows_sh[tid] =
        valid ? (topk_div > 0 ? sid / topk_div : tile_m * BM + tid) : -1;
    const unsigned long long mask = __ballot(valid);
    if (tid == 0) nmf_sh = mask ? (64 - __clzll(mask) + 15) / 16 : 0;
  }
  __syncthreads();
  switch (nmf_sh) {  // block-uniform
    case 0: break;
    case 1:
      run_tile<1>(A, lda, QW, S, Z, C, ldc, a_lds, rows_sh, tile_m, expert,
                  ntiles, G);
      break;
    case 2:
      run_tile<2>(A, lda, QW, S, Z, C, ldc, a_lds, rows_sh, tile_m, expert,
                  ntiles, G);
      break;
    case 3:
      run_tile<3>(A, lda, QW, S, Z, C, ldc, a_lds, rows_sh, tile_m, expert,
                  ntiles, G);
      break;
    default:
      run_tile<4>(A, lda, QW, S, Z, C, ldc, a_lds, rows_sh, tile_m, expert,
                  ntiles, G);
      break;
  }
}

}  // namespace moe_w4a16

// a: [T, K] (topk_div > 0: row = sorted id / topk_div) or [EM, K]
// (topk_div == 0: row = sorted position); c: [EM, N] bf16, EM % 64 == 0.
void moe_gemm_w4a16(torch::Tensor a, torch::Tensor qweight,
                    torch::Tensor scales, torch::Tensor zeros,
                    torch::Tensor c, torch::Tensor sorted,
                    torch::Tensor expert_tiles, int64_t topk_div,
                    int64_t total_flat) {
  using namespace moe_w4a16;
  TORCH_CHECK(a.dim() == 2 && c.dim() == 2);
  TORCH_CHECK(a.is_contiguous() && c.is_contiguous());
  TORCH_CHECK(a.scalar_type() == torch::kBFloat16 &&
              c.scalar_type() == torch::kBFloat16,
              "moe_gemm_w4a16: bf16 activations only");
  TORCH_CHECK(qweight.dim() == 5 && qweight.is_contiguous() &&
              qweight.scalar_type() == torch::kInt32 &&
              qweight.size(3) == WAVE_SIZE && qweight.size(4) == 4,
              "moe_gemm_w4a16: qweight must be int32 [E, N/16, K/128, 64, 4]");
  const int E = (int)qweight.size(0);
  const int ntiles = (int)qweight.size(1);
  const int G = (int)qweight.size(2);
  const int N = ntiles * 16;
  TORCH_CHECK(E > 0 && ntiles > 0 && G > 0);
  TORCH_CHECK(a.size(1) == (int64_t)G * GROUP, "moe_gemm_w4a16: K mismatch");
  const int64_t nsz = (int64_t)E * ntiles * G * 16;
  TORCH_CHECK(scales.scalar_type() == torch::kBFloat16 &&
              scales.is_contiguous() && scales.numel() == nsz);
  TORCH_CHECK(zeros.scalar_type() == torch::kByte && zeros.is_contiguous() &&
              zeros.numel() == nsz);
  const int em = (int)c.size(0);
  TORCH_CHECK(c.size(1) == N);
  TORCH_CHECK(em % BM == 0 && em / BM <= (int)expert_tiles.numel());
  TORCH_CHECK(sorted.scalar_type() == torch::kInt32 &&
              expert_tiles.scalar_type() == torch::kInt32 &&
              sorted.is_contiguous() && expert_tiles.is_contiguous() &&
              sorted.numel() >= em);
  // Every row the gather can name lies inside a.
  TORCH_CHECK(topk_div >= 0 && total_flat >= 0);
  TORCH_CHECK(topk_div > 0 ? a.size(0) * topk_div >= total_flat
                           : a.size(0) >= em,
              "moe_gemm_w4a16: a has too few rows");
  if (em == 0) return;
  auto stream = c10::hip::getCurrentHIPStream().stream();
  dim3 grid(ceil_div(ntiles, NW * NT), em / BM);
  hipLaunchKernelGGL(
      moe_gemm_w4a16_kernel, grid, dim3(THREADS), 0, stream,
      (const short*)a.data_ptr(), a.size(1),
      (const i32x4*)qweight.data_ptr(), (const short*)scales.data_ptr(),
      (const uint8_t*)zeros.data_ptr(), (short*)c.data_ptr(), c.size(1),
      sorted.data_ptr<int>(), expert_tiles.data_ptr<int>(), E, ntiles, G,
      (int)topk_div, (int)total_flat);
  HIP_CHECK_KERNEL();
}

}  // namespace vllm_amd
