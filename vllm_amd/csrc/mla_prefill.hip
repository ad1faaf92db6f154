// MLA prefill attention for CDNA4 (gfx950): MFMA flash kernel over the
// compressed latent KV cache.
//
// Serves every MLA row that is not a plain decode row: prefill chunks,
// chunked-prefill continuations and speculative-verification rows. Same
// absorbed-MQA geometry as mla.hip (kv_lora 512 + rope 64 = 576, the
// value is the first 512 dims of the same latent row), so all Hq heads
// of all query tokens of a request attend to ONE shared latent stream.
//
// Work split: a request's queries are flattened to rows i = t*Hq + h
// (q_nope / q_pe / out are contiguous [T, Hq, .], so row i is global row
// query_start_loc[r]*Hq + i). A block owns 64 consecutive rows; grid
// (ceil(max_query_len*Hq/64), num_prefill_reqs). Row i sees keys
// [0, lim_i), lim_i = ctx - q_len + i/Hq + 1; the block streams keys
// [0, lim of its last valid row) in 32-token subtiles and applies the
// per-element mask only in subtiles that reach past its smallest lim.
// Nothing assumes Hq % 16 == 0: a tile may straddle tokens unevenly.
//
// Block = 4 waves; wave w owns rows [16w, 16w+16) for the whole kernel:
//   QK:  18 Q fragments in registers; S for both 16-token n-tiles
//        (36 MFMA 16x16x32).
//   softmax: online, log2 domain; a row lives in one wave, so max/sum
//        are 16-lane shuffles — no cross-wave exchange, no softmax
//        barriers. P is rounded to the input dtype through a
//        wave-private LDS patch (C layout -> A layout).
//   PV:  all 512 output columns per wave (32 f32x4 accumulators,
//        32 MFMA).
// The KV subtile is staged once per block: [tok][576] swizzled (QK) plus
// a [dim][tok] copy of the first 512 dims (PV). Staging maps lanes to
// tokens, so the transposed copy is built from lane-pair exchanges (DPP)
// and written as packed dwords (a lane-per-feature mapping would put a
// whole wave's 2-byte writes on one LDS bank). The next subtile's global
// loads are issued before the MFMA phase and land in registers while it
// runs. The only block barriers are the two around staging.
// 256 VGPRs + 216 AGPRs, no scratch, 73 KB LDS: one block per CU.
// Measurements: profiles/mla_prefill.md. With an e4m3 latent cache
// (CTag = FP8CacheTag; 198 AGPRs) the prefetch holds raw fp8 and staging
// dequantises: profiles/mla_fp8_cache.md.

#include <torch/all.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime.h>

#include "common.h"

namespace vllm_amd {

namespace mla_pf {

constexpr int LORA = 512;
constexpr int ROPE = 64;
constexpr int DK = LORA + ROPE;  // 576
constexpr int ROWS = 64;         // flattened (token, head) rows per block
constexpr int SUB = 32;          // KV tokens per subtile
constexpr int THREADS = 256;
constexpr int KF = DK / 32;      // 18 k-fragments over the 576 dim
constexpr int NF = LORA / 16;    // 32 output column fragments
constexpr int PSTR = 40;         // P patch row stride (shorts), 16B-aligned
// Staging: thread -> token tid&31, 8-elem feature chunks (tid>>5) + 8*it.
constexpr int STAGE_IT = SUB * (DK / 8) / THREADS;  // 9; it==8 is rope-only
constexpr float NEG_INF = -1e30f;

static_assert(THREADS % SUB == 0 && SUB * (DK / 8) % THREADS == 0);

DEVINL int swz(int row, int byte_off) { return byte_off ^ ((row & 7) << 4); }

typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));

template <typename Tag> DEVINL f32x4 mma(s16x8 a, s16x8 b, f32x4 c);
template <> DEVINL f32x4 mma<BF16Tag>(s16x8 a, s16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
template <> DEVINL f32x4 mma<FP16Tag>(s16x8 a, s16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(
      __builtin_bit_cast(h16x8, a), __builtin_bit_cast(h16x8, b), c, 0, 0, 0);
}

// CTag is the cache element: the compute dtype, or FP8CacheTag for an
// e4m3 latent cache, whose prefetched subtile waits in registers as raw
// fp8 (18 dwords, not 36) and is dequantised (exactly) on its way into LDS.
template <typename Tag, typename CTag>
__launch_bounds__(THREADS) __global__
void mla_prefill_kernel(short* __restrict__ out,           // [T, Hq, LORA]
                        const short* __restrict__ q_nope,  // [T, Hq, LORA]
                        const short* __restrict__ q_pe,    // [T, Hq, ROPE]
                        const typename CacheTraits<CTag>::elem* __restrict__
                            kv,                            // [NB, BS, DK]
                        const int* __restrict__ block_table, int bt_stride,
                        const int* __restrict__ query_start_loc,
                        const int* __restrict__ seq_lens, float scale,
                        int num_heads, int block_size, int num_decodes) {
  const int req = num_decodes + blockIdx.y;
  const int q_start = query_start_loc[req];
  const int ql = query_start_loc[req + 1] - q_start;
  const int nrows = ql * num_heads;
  const int row0 = blockIdx.x * ROWS;
  if (row0 >= nrows) return;
  const int ctx = seq_lens[req];
  const int pos0 = ctx - ql;  // position of the request's query token 0
  const int last_row = min(row0 + ROWS, nrows) - 1;
  const int kv_end = pos0 + last_row / num_heads + 1;  // largest lim
  const int min_lim = pos0 + row0 / num_heads + 1;     // smallest lim

  __shared__ __attribute__((aligned(16))) short k_lds[SUB * DK];
  __shared__ __attribute__((aligned(16))) short vt_lds[LORA * SUB];
  __shared__ __attribute__((aligned(16))) short p_lds[4][16 * PSTR];

  const int tid = threadIdx.x;
  const int wave = tid / WAVE_SIZE;
  const int lane = tid % WAVE_SIZE;
  const int l16 = lane & 15;
  const int l4 = lane >> 4;
  // A wave whose 16 rows are all padding still stages and hits the
  // barriers, but skips the MFMA phase.
  const bool wave_active = row0 + wave * 16 < nrows;
  const long g_row0 = (long)q_start * num_heads;

  // Q fragments (A layout: row l16, k = l4*8 + j). Padding rows read the
  // last valid row and are never stored.
  s16x8 qfrag[KF];
  {
    const long g = g_row0 + min(row0 + wave * 16 + l16, nrows - 1);
#pragma unroll
    for (int kf = 0; kf < KF; ++kf) {
      const int f = kf * 32 + l4 * 8;
      qfrag[kf] = (f < LORA)
          ? *reinterpret_cast<const s16x8*>(q_nope + g * LORA + f)
          : *reinterpret_cast<const s16x8*>(q_pe + g * ROPE + (f - LORA));
    }
  }

  // Per-row state in the C layout: this lane's rows are l4*4 + r.
  int lim[4];
  float m_st[4], l_st[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = min(row0 + wave * 16 + l4 * 4 + r, nrows - 1);
    lim[r] = pos0 + row / num_heads + 1;
    m_st[r] = NEG_INF;
    l_st[r] = 0.f;
  }
  f32x4 o_acc[NF];
#pragma unroll
  for (int nf = 0; nf < NF; ++nf) o_acc[nf] = f32x4{0.f, 0.f, 0.f, 0.f};

  const float sc2 = scale * 1.4426950408889634f;  // log2(e)

  // ---- staging helpers.
  const int s_tok = tid & (SUB - 1);
  const int s_f8 = tid / SUB;  // 0..7; chunk it covers features (s_f8+8it)*8
  using cvec = typename CacheTraits<CTag>::vec8;
  cvec pre[STAGE_IT];
  auto load_subtile = [&](int sub0) {
    const int t_glob = sub0 + s_tok;
    if (t_glob < kv_end) {
      const int blk =
          block_table[(long)req * bt_stride + t_glob / block_size];
      const typename CacheTraits<CTag>::elem* src =
          kv + ((long)blk * block_size + t_glob % block_size) * DK + s_f8 * 8;
#pragma unroll
      for (int it = 0; it < STAGE_IT; ++it)
        pre[it] = *reinterpret_cast<const cvec*>(src + it * 64);
    } else {
#pragma unroll
      for (int it = 0; it < STAGE_IT; ++it)
        pre[it] = cvec{0, 0, 0, 0, 0, 0, 0, 0};
    }
  };
  // Transposed copy through the lane pair (tok, tok^1): each lane gets
  // its partner's dword (dims 2jj, 2jj+1) by DPP and byte-permutes the two
  // into vt[dim][tok&~1 .. +1] — the even lane keeps the low halves (dim
  // 2jj), the odd lane the high halves (dim 2jj+1).
  const bool s_odd = s_tok & 1;
  const unsigned s_sel = s_odd ? 0x03020706u : 0x05040100u;
  auto store_subtile = [&]() {
    unsigned* vt32 = reinterpret_cast<unsigned*>(vt_lds);
#pragma unroll
    for (int it = 0; it < STAGE_IT; ++it) {
      const int f8 = s_f8 + it * 8;
      const s16x8 v = cache_vec8_to_16<Tag, CTag>(pre[it]);
      *reinterpret_cast<s16x8*>(reinterpret_cast<char*>(k_lds) +
                                s_tok * (DK * 2) + swz(s_tok, f8 * 16)) = v;
      if (it < LORA / 64) {
        const i32x4 w = __builtin_bit_cast(i32x4, v);
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          // quad_perm(1,0,3,2): lane ^ 1.
          const int pw = __builtin_amdgcn_update_dpp(0, w[jj], 0xB1, 0xF, 0xF,
                                                     false);
          const int dim = f8 * 8 + jj * 2 + (s_odd ? 1 : 0);
          vt32[dim * (SUB / 2) + (s_tok >> 1)] = __builtin_amdgcn_perm(
              (unsigned)pw, (unsigned)w[jj], s_sel);
        }
      }
    }
  };

  load_subtile(0);
  for (int sub0 = 0; sub0 < kv_end; sub0 += SUB) {
    store_subtile();
    __syncthreads();
    if (sub0 + SUB < kv_end) load_subtile(sub0 + SUB);

    if (wave_active) {
      // ---- QK: S[16 rows x 32 tok], two independent n-tile chains.
      // Four independent accumulation chains (n-tile x kf parity).
      f32x4 s_frag[2][2];
#pragma unroll
      for (int i = 0; i < 4; ++i)
        s_frag[i >> 1][i & 1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kf = 0; kf < KF; ++kf) {
#pragma unroll
        for (int n = 0; n < 2; ++n) {
          const int tok = n * 16 + l16;  // B-frag col
          const s16x8 bfrag = *reinterpret_cast<const s16x8*>(
              reinterpret_cast<const char*>(k_lds) + tok * (DK * 2) +
              swz(tok, kf * 64 + l4 * 16));
          s_frag[n][kf & 1] = mma<Tag>(qfrag[kf], bfrag, s_frag[n][kf & 1]);
        }
      }

      // ---- mask + online softmax. C layout: col l16 = token, row
      // l4*4 + r. Key 0 is visible to every valid row, so m is finite
      // after the first subtile and fully masked later subtiles give p=0.
      float sv[2][4];
#pragma unroll
      for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          sv[n][r] = (s_frag[n][0][r] + s_frag[n][1][r]) * sc2;
      if (sub0 + SUB > min_lim) {
#pragma unroll
        for (int n = 0; n < 2; ++n) {
          const int kpos = sub0 + n * 16 + l16;
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (kpos >= lim[r]) sv[n][r] = NEG_INF;
        }
      }
      float factor[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float m_new = fmaxf(
            m_st[r], group16_reduce_max(fmaxf(sv[0][r], sv[1][r])));
        factor[r] = exp2f(m_st[r] - m_new);
        m_st[r] = m_new;
        float psum = 0.f;
#pragma unroll
        for (int n = 0; n < 2; ++n) {
          const float p = exp2f(sv[n][r] - m_new);
          psum += p;
          p_lds[wave][(l4 * 4 + r) * PSTR + n * 16 + l16] = from_f32<Tag>(p);
        }
        l_st[r] = l_st[r] * factor[r] + group16_reduce_sum(psum);
      }
      // The patch is wave-private: LDS serves one wave's accesses in
      // order, so only the compiler has to be kept from moving the
      // A-fragment read above the writes.
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      const s16x8 pfrag = *reinterpret_cast<const s16x8*>(
          &p_lds[wave][l16 * PSTR + l4 * 8]);

      // ---- PV: O[16 rows x 512] = O*factor + P[16 x 32] V[32 x 512].
      // Once the running maxima have settled every factor is 1 and the
      // 128-register rescale is skipped (wave-uniform branch).
      if (__any(factor[0] != 1.f || factor[1] != 1.f || factor[2] != 1.f ||
                factor[3] != 1.f)) {
#pragma unroll
        for (int nf = 0; nf < NF; ++nf)
#pragma unroll
          for (int r = 0; r < 4; ++r) o_acc[nf][r] *= factor[r];
      }
#pragma unroll
      for (int nf = 0; nf < NF; ++nf) {
        const int col = nf * 16 + l16;
        const s16x8 bfrag = *reinterpret_cast<const s16x8*>(
            vt_lds + col * SUB + l4 * 8);
        o_acc[nf] = mma<Tag>(pfrag, bfrag, o_acc[nf]);
      }
    }
    __syncthreads();
  }

  // ---- write out: row l4*4 + r, col nf*16 + l16.
  if (wave_active) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = row0 + wave * 16 + l4 * 4 + r;
      if (row >= nrows) continue;
      const float inv_l = 1.f / l_st[r];
      short* o = out + (g_row0 + row) * LORA + l16;
#pragma unroll
      for (int nf = 0; nf < NF; ++nf)
        o[nf * 16] = from_f32<Tag>(o_acc[nf][r] * inv_l);
    }
  }
}

}  // namespace mla_pf

void mla_prefill(torch::Tensor out, torch::Tensor q_nope, torch::Tensor q_pe,
                 torch::Tensor kv_cache, torch::Tensor block_table,
                 torch::Tensor query_start_loc, torch::Tensor seq_lens,
                 double scale, int64_t num_decodes, int64_t max_query_len) {
  using namespace mla_pf;
  TORCH_CHECK(q_nope.dim() == 3 && q_nope.size(2) == LORA,
              "mla_prefill expects kv_lora_rank=512");
  TORCH_CHECK(q_pe.dim() == 3 && q_pe.size(2) == ROPE,
              "mla_prefill expects rope dim 64");
  TORCH_CHECK(q_pe.size(0) == q_nope.size(0) &&
              q_pe.size(1) == q_nope.size(1));
  TORCH_CHECK(kv_cache.dim() == 3 && kv_cache.size(2) == DK);
  TORCH_CHECK(q_nope.is_contiguous() && q_pe.is_contiguous() &&
              out.is_contiguous() && kv_cache.is_contiguous() &&
              block_table.is_contiguous());
  TORCH_CHECK(out.sizes() == q_nope.sizes());
  TORCH_CHECK(out.scalar_type() == q_nope.scalar_type() &&
              q_pe.scalar_type() == q_nope.scalar_type());
  const bool fp8c = kv_cache.scalar_type() == torch::kFloat8_e4m3fn;
  TORCH_CHECK(fp8c || kv_cache.scalar_type() == q_nope.scalar_type(),
              "mla_prefill: kv_cache must be fp8 or the q dtype");
  const int num_reqs = (int)seq_lens.size(0);
  TORCH_CHECK(query_start_loc.numel() == num_reqs + 1 &&
              block_table.size(0) >= num_reqs);
  TORCH_CHECK(num_decodes >= 0 && num_decodes <= num_reqs);
  const int num_prefills = num_reqs - (int)num_decodes;
  if (num_prefills == 0 || max_query_len <= 0) return;
  const int Hq = (int)q_nope.size(1);
  const int bs = (int)kv_cache.size(1);
  auto stream = c10::hip::getCurrentHIPStream().stream();
  dim3 grid(ceil_div((int)max_query_len * Hq, ROWS), num_prefills);
  auto launch = [&](auto tag, auto ctag) {
    using Tag = decltype(tag);
    using CTag = decltype(ctag);
    hipLaunchKernelGGL(
        (mla_prefill_kernel<Tag, CTag>), grid, dim3(THREADS), 0, stream,
        (short*)out.data_ptr(), (const short*)q_nope.data_ptr(),
        (const short*)q_pe.data_ptr(),
        (const typename CacheTraits<CTag>::elem*)kv_cache.data_ptr(),
        block_table.data_ptr<int>(), (int)block_table.size(1),
        query_start_loc.data_ptr<int>(), seq_lens.data_ptr<int>(),
        (float)scale, Hq, bs, (int)num_decodes);
  };
  if (q_nope.scalar_type() == torch::kBFloat16) {
    if (fp8c) launch(BF16Tag{}, FP8CacheTag{});
    else      launch(BF16Tag{}, BF16Tag{});
  } else if (q_nope.scalar_type() == torch::kHalf) {
    if (fp8c) launch(FP16Tag{}, FP8CacheTag{});
    else      launch(FP16Tag{}, FP16Tag{});
  } else {
    TORCH_CHECK(false, "mla_prefill: bf16/fp16 only");
  }
  HIP_CHECK_KERNEL();
}

}  // namespace vllm_amd
