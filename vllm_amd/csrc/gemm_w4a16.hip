// W4A16 dequant-GEMM for CDNA4 (gfx950): y[M,N] = x[M,K] * W~^T (+bias),
// bf16 activations/output, fp32 accumulate, weights stored as 4-bit codes
// with one bf16 scale and one integer zero-point per (row, 128-wide K
// group):  W~[n,k] = (q[n,k] - z[n,g]) * s[n,g]   (AWQ's arithmetic).
//
// Decode is weight-streaming; this kernel reads 0.52 B per weight instead
// of bf16's 2 B. hipBLASLt has no packed-uint4 + group-scale input, so
// the GEMM is hand-written, in the style of moe_gemm_shuf_kernel
// (moe.hip): weights live in consumer order and are streamed straight
// from HBM into the MFMA B operand with no LDS staging and no barrier in
// the K loop.
//
// Weight layout (written once at load, ops/_torch_ref.pack_weight_int4):
//   qweight int32 [N/16][K/128][64 lanes][4]
//   scales  bf16  [N/16][K/128][16]
//   zeros   uint8 [N/16][K/128][16]
// For v_mfma_f32_16x16x32_bf16 a B-fragment lane (col = lane&15,
// l4 = lane>>4) holds the 8 K-values k = l4*8 + e of one column: one
// int32 of nibbles. Word j of a lane's int4 is MFMA K-step j of the
// group, so ONE 16 B load per lane is 4 K-steps = 128 K-values = exactly
// one quantization group (one (s, z) pair per lane per load), and a wave
// walks linear 1 KB lines. Inside a word element e sits at nibble
// (e>>1) + 4*(e&1): then ((w >> 4p) & 0x000F000F) | 0x43004300 is the
// bf16 pair (128+q[2p], 128+q[2p+1]) — two VALU ops per two weights.
//
// Dequant without per-weight float math: the MFMAs run on the exact
// integers. Per group the accumulator gets x*(128+q) and then
// x*(-(128+z)) (a constant B fragment 0xC300|z), i.e. sum x*(q-z) with
// every product exact in fp32, and the bf16 scale is folded into the
// fp32 running total once per group. No weight is ever rounded to bf16.
//
// Work split: a block is NWN x NWK waves. Wave (wn, wk) owns the 16-col
// tile blockIdx.x*NWN + wn and the K groups g = wk, wk+NWK, ...; the NWK
// partial tiles are summed through LDS once, in a fixed order (no
// atomics — results are bit-identical run to run). blockIdx.y walks
// MF*16-row M tiles; weights are re-streamed per M tile.
//   M <= 16 : MF=1, 1x8 waves   (N/16 blocks, 8-way K split)
//   M <= 32 : MF=2, 1x8 waves
//   else    : MF=4, 2x4 waves   (64 rows x 32 cols per block)

#include <torch/all.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime.h>

#include "common.h"

namespace vllm_amd {

namespace w4a16 {

constexpr int GROUP = 128;

template <int MF, int NWN, int NWK>
__launch_bounds__(NWN * NWK * WAVE_SIZE) __global__
void w4a16_gemm_kernel(const short* __restrict__ A, long lda,
                       const i32x4* __restrict__ QW,
                       const short* __restrict__ S,
                       const uint8_t* __restrict__ Z,
                       const short* __restrict__ bias,
                       short* __restrict__ C, long ldc, int M, int ntiles,
                       int G) {
  const int wave = threadIdx.x / WAVE_SIZE;
  const int lane = threadIdx.x % WAVE_SIZE;
  const int l16 = lane & 15;
  const int l4 = lane >> 4;
  const int wn = wave % NWN;
  const int wk = wave / NWN;
  const int ntile = blockIdx.x * NWN + wn;
  const int m0 = blockIdx.y * (MF * 16);
  const bool active = ntile < ntiles;  // wave-uniform

  f32x4 tot[MF];
#pragma unroll
  for (int mf = 0; mf < MF; ++mf) tot[mf] = f32x4{0.f, 0.f, 0.f, 0.f};

  if (active) {
    // A-frag: lane&15 = row, k = l4*8 + e. Tail rows re-read row M-1
    // (real memory); MFMA rows are independent and the epilogue masks.
    const short* a_ptr[MF];
#pragma unroll
    for (int mf = 0; mf < MF; ++mf) {
      int r = m0 + mf * 16 + l16;
      r = r < M ? r : M - 1;
      a_ptr[mf] = A + (long)r * lda + l4 * 8;
    }
    const i32x4* qp = QW + (long)ntile * G * WAVE_SIZE + lane;
    const short* sp = S + (long)ntile * G * 16 + l16;
    const uint8_t* zp = Z + (long)ntile * G * 16 + l16;

    // U groups per iteration, all of their loads issued before the first
    // MFMA, so each wave keeps U KB of codes (plus its A fragments) in
    // flight: at M <= 16 a K=4096 wave has its whole K slice requested
    // up front. A group index past the end is clamped to G-1 (in bounds)
    // and its scale forced to 0, which keeps the body branch-free.
    constexpr int U = 4 / MF;
    for (int g0 = wk; g0 < G; g0 += U * NWK) {
      i32x4 w[U];
      float s[U];
      int z[U];
      s16x8 a[U][MF][4];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int gu = g0 + u * NWK;
        const int g = gu < G ? gu : G - 1;
        w[u] = qp[(long)g * WAVE_SIZE];
        s[u] = gu < G ? bf16_to_f32(sp[g * 16]) : 0.f;
        z[u] = zp[g * 16];
#pragma unroll
        for (int mf = 0; mf < MF; ++mf)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            a[u][mf][j] = *reinterpret_cast<const s16x8*>(
                a_ptr[mf] + (long)g * GROUP + j * 32);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int zw = (int)0xC300C300u | z[u] | (z[u] << 16);  // -(128+z)
        const s16x8 zfrag =
            __builtin_bit_cast(s16x8, i32x4{zw, zw, zw, zw});
        f32x4 acc[MF];
#pragma unroll
        for (int mf = 0; mf < MF; ++mf) acc[mf] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          i32x4 bw;
#pragma unroll
          for (int p = 0; p < 4; ++p)
            bw[p] = (int)((((uint32_t)w[u][j] >> (4 * p)) & 0x000F000Fu) |
                          0x43004300u);
          const s16x8 bfrag = __builtin_bit_cast(s16x8, bw);
#pragma unroll
          for (int mf = 0; mf < MF; ++mf) {
            acc[mf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                a[u][mf][j], bfrag, acc[mf], 0, 0, 0);
            acc[mf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                a[u][mf][j], zfrag, acc[mf], 0, 0, 0);
          }
        }
        // C-frag col = lane&15 — the column whose scale this lane loaded.
#pragma unroll
        for (int mf = 0; mf < MF; ++mf) tot[mf] += s[u] * acc[mf];
      }
    }
  }

  // Split-K reduce: waves wk>0 park their tiles in LDS, wave wk==0 of
  // each column tile adds them in wk order. Every slot read was written
  // by its owner before the barrier (inactive waves write zeros).
  if constexpr (NWK > 1) {
    __shared__ float red[(NWK - 1) * NWN * MF * 4 * WAVE_SIZE];
    if (wk > 0) {
#pragma unroll
      for (int mf = 0; mf < MF; ++mf)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          red[((((wk - 1) * NWN + wn) * MF + mf) * 4 + r) * WAVE_SIZE +
              lane] = tot[mf][r];
    }
    __syncthreads();
    if (wk > 0) return;
#pragma unroll
    for (int k = 1; k < NWK; ++k)
#pragma unroll
      for (int mf = 0; mf < MF; ++mf)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          tot[mf][r] +=
              red[((((k - 1) * NWN + wn) * MF + mf) * 4 + r) * WAVE_SIZE +
                  lane];
  }
  if (!active) return;

  // Epilogue: C-frag col = lane&15, row = l4*4 + r.
  const int n = ntile * 16 + l16;
  const float b = bias != nullptr ? bf16_to_f32(bias[n]) : 0.f;
#pragma unroll
  for (int mf = 0; mf < MF; ++mf) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = m0 + mf * 16 + l4 * 4 + r;
      if (row < M) C[(long)row * ldc + n] = f32_to_bf16(tot[mf][r] + b);
    }
  }
}

template <int MF, int NWN, int NWK>
void launch(const torch::Tensor& x, const torch::Tensor& qweight,
            const torch::Tensor& scales, const torch::Tensor& zeros,
            const short* bias, torch::Tensor& y, int M, int ntiles, int G,
            hipStream_t stream) {
  dim3 grid(ceil_div(ntiles, NWN), ceil_div(M, MF * 16));
  hipLaunchKernelGGL(
      (w4a16_gemm_kernel<MF, NWN, NWK>), grid, dim3(NWN * NWK * WAVE_SIZE),
      0, stream, (const short*)x.data_ptr(), x.size(1),
      (const i32x4*)qweight.data_ptr(), (const short*)scales.data_ptr(),
      (const uint8_t*)zeros.data_ptr(), bias, (short*)y.data_ptr(),
      y.size(1), M, ntiles, G);
}

}  // namespace w4a16

// x: [M, K] bf16; qweight/scales/zeros as laid out above -> y [M, N] bf16.
torch::Tensor w4a16_gemm(torch::Tensor x, torch::Tensor qweight,
                         torch::Tensor scales, torch::Tensor zeros,
                         c10::optional<torch::Tensor> bias) {
  using namespace w4a16;
  TORCH_CHECK(x.dim() == 2 && x.is_contiguous());
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16,
              "w4a16_gemm: bf16 activations only");
  TORCH_CHECK(qweight.dim() == 4 && qweight.is_contiguous() &&
              qweight.scalar_type() == torch::kInt32 &&
              qweight.size(2) == WAVE_SIZE && qweight.size(3) == 4,
              "w4a16_gemm: qweight must be int32 [N/16, K/128, 64, 4]");
  const int ntiles = (int)qweight.size(0);
  const int G = (int)qweight.size(1);
  const int M = (int)x.size(0);
  const int N = ntiles * 16;
  TORCH_CHECK(x.size(1) == (int64_t)G * GROUP, "w4a16_gemm: K mismatch");
  TORCH_CHECK(scales.scalar_type() == torch::kBFloat16 &&
              scales.is_contiguous() &&
              scales.numel() == (int64_t)ntiles * G * 16);
  TORCH_CHECK(zeros.scalar_type() == torch::kByte && zeros.is_contiguous() &&
              zeros.numel() == (int64_t)ntiles * G * 16);
  const short* bptr = nullptr;
  if (bias.has_value()) {
    TORCH_CHECK(bias->scalar_type() == torch::kBFloat16 &&
                bias->is_contiguous() && bias->numel() == N);
    bptr = (const short*)bias->data_ptr();
  }
  auto y = torch::empty({M, N}, x.options());
  if (M == 0) return y;
  auto stream = c10::hip::getCurrentHIPStream().stream();
  if (M <= 16)
    launch<1, 1, 8>(x, qweight, scales, zeros, bptr, y, M, ntiles, G, stream);
  else if (M <= 32)
    launch<2, 1, 8>(x, qweight, scales, zeros, bptr, y, M, ntiles, G, stream);
  else
    launch<4, 2, 4>(x, qweight, scales, zeros, bptr, y, M, ntiles, G, stream);
  HIP_CHECK_KERNEL();
  return y;
}

}  // namespace vllm_amd
