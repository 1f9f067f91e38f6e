// Row-wise fused kernels (HBM-bound), float4 / 8-byte bf16 vector accesses, wave-shuffle reductions.  D % 4 == 0.  Two forms:
//   - one WORKGROUP per token row (combine_norm_row_kernel, embed_tokens_row_kernel, head_ddim_row_kernel, head_ddim_guided_row_kernel): a thread
//     owns 4 columns per 1024 and keeps them in registers, every load is unconditional and requested before the one cross-wave reduction.  This is
//     the form every sampler call takes (D <= 4096, k <= 2, y_splits <= 8, "combine_row_max" not 0).
//   - the fallbacks, one WAVE64 per token row, four rows per workgroup, the row cached in LDS between the reduce and the normalise pass
//     (rmsnorm_cond_kernel, combine_norm_kernel, embed_tokens_kernel, head_ddim_kernel): any D, k <= 8, any slab count.  rmsnorm_cond has this form only.
//   rmsnorm_cond      : ln_1(x)+c / ln_2 / final ln                        (modedit.py:72-80, 532, 539, 818)
//   combine_norm      : MoE weighted combine + residual + next block's ln_1+c   (modedit.py:566, 595, 532)
//   embed_tokens      : sequence assembly + first ln_1+c                    (modedit.py:760-790, 847-860)
//   head_ddim         : last combine + final ln + Linear(D,A) + EDM/DDIM update  (modedit.py:807-808; score_wrappers.py:79-80;
//                                                                             gc_sampling.py:948-950)
#include <type_traits>

#include "mode_common.h"

namespace mode {

constexpr int ROWS_PER_BLOCK = 4;   // 4 waves
// The one-wave-per-row kernels cache ROWS_PER_BLOCK rows in dynamic LDS and are launched without the large-LDS attribute: their launchers refuse
// what does not fit in 64 KiB (D > 4096) with MODE_ERR_UNSUPPORTED, as rmsnorm_bwd_launch does, instead of returning the launch's hipError_t.
constexpr size_t kWaveRowLdsMax = 64 * 1024;

// Visit the float4 chunks of one row owned by this lane: d = lane*4 + c*256.  NCH > 0 (D == 256*NCH) fully unrolls, so every
// global load of the row is in flight before the first use; NCH == 0 is the generic (any D % 4 == 0) loop.
template <int NCH, typename F>
__device__ __forceinline__ void for_chunks(int D, int lane, F&& f) {
  if constexpr (NCH > 0) {
#pragma unroll
    for (int c = 0; c < NCH; ++c) f(lane * 4 + c * 256);
  } else {
    for (int d = lane * 4; d < D; d += 256) f(d);
  }
}

// store 4 consecutive elements at element offset `off` of a bf16 (8-byte store) or fp32 tensor; POL: the store's cache policy (mode_common.h)
template <bool LP_BF16, int POL = ST_PLAIN>
__device__ __forceinline__ void store_lp4(void* base, long off, float4 o) {
  if constexpr (LP_BF16) store_out8<POL>(reinterpret_cast<uint16_t*>(base) + off, out_u2{pack_bf16x2(o.x, o.y), pack_bf16x2(o.z, o.w)});
  else store_out16<POL>(reinterpret_cast<float*>(base) + off, as_out_u4(o));
}

__device__ __forceinline__ float4 scale4(float4 v, float s, float4 g) {   // v * s * g, in this order (s: the row's one reciprocal norm)
  return make_float4(v.x * s * g.x, v.y * s * g.y, v.z * s * g.z, v.w * s * g.w);
}

// normalise the cached row: y = v / max(sqrt(ssq) * D^-1/2, eps) * g (+ cond); write fp32 and/or low-precision copies
template <bool LP_BF16, int NCH>
__device__ __forceinline__ void norm_store(const float* row, int D, float ssq, const float* g, const float* cond, float eps,
                                           float* y_f32, void* y_lp, int lane) {
  const float nrm = fmaxf(sqrtf(ssq) * rsqrtf((float)D), eps);
  const float rnrm = __frcp_rn(nrm);                       // one reciprocal per row: a per-element fp32 division is a ~10-instruction VCC-serialised sequence
  for_chunks<NCH>(D, lane, [&](int d) {
    const float4 v = *reinterpret_cast<const float4*>(row + d);
    const float4 gg = *reinterpret_cast<const float4*>(g + d);
    float4 o = scale4(v, rnrm, gg);
    if (cond) {
      const float4 c = *reinterpret_cast<const float4*>(cond + d);
      o.x += c.x; o.y += c.y; o.z += c.z; o.w += c.w;
    }
    if (y_f32) *reinterpret_cast<float4*>(y_f32 + d) = o;
    if (y_lp) store_lp4<LP_BF16>(y_lp, d, o);
  });
}

// Fused ln_2: the residual operand u arrives un-normalised together with per-64-column sums of squares (MODE_EPI_RESIDUAL_NORM); the
// normalised row is u / max(sqrt(sum) * D^-1/2, eps) * gain, the expression of norm_store, evaluated on the fly.
__device__ __forceinline__ float row_norm_from_partials(const float* ss, int n, int D, float eps, int lane) {
  return fmaxf(sqrtf(sum_row_partials_wave(ss, n, lane)) * rsqrtf((float)D), eps);   // same order as the GEMM-side consumers (gemm_bf16*.hip)
}

template <bool YBF>   // one float4 of an expert output row: 4 bf16 (8 bytes) widened, or 4 fp32
__device__ __forceinline__ float4 load_y4(const void* Y, long off) {
  if constexpr (YBF) {
    const uint2 r = *reinterpret_cast<const uint2*>(reinterpret_cast<const uint16_t*>(Y) + off);
    return make_float4(bf16_bits_to_f32(r.x & 0xffff), bf16_bits_to_f32(r.x >> 16), bf16_bits_to_f32(r.y & 0xffff),
                       bf16_bits_to_f32(r.y >> 16));
  } else {
    return *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(Y) + off);
  }
}
__device__ __forceinline__ float4 load_y4(const void* Y, bool y_bf16, long off) {   // dtype at run time: the one-wave-per-row kernels
  return y_bf16 ? load_y4<true>(Y, off) : load_y4<false>(Y, off);
}

// ------------------------------------------------------------------------------------------------------------ rmsnorm
template <bool LP_BF16, int NCH>
__global__ __launch_bounds__(256) void rmsnorm_cond_kernel(const float* x, const float* __restrict__ g,
                                                           const float* __restrict__ cond, int rows, int D, int rpc, float eps,
                                                           float* y_f32, void* y_lp) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row = blockIdx.x * ROWS_PER_BLOCK + wave;
  if (row >= rows) return;
  float* cache = reinterpret_cast<float*>(smem) + (size_t)wave * D;
  const float* xr = x + (long)row * D;
  float ssq = 0.f;
  for_chunks<NCH>(D, lane, [&](int d) {
    const float4 v = *reinterpret_cast<const float4*>(xr + d);
    *reinterpret_cast<float4*>(cache + d) = v;
    ssq += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
  });
  ssq = wave_sum(ssq);
  norm_store<LP_BF16, NCH>(cache, D, ssq, g, cond ? cond + (long)(row / rpc) * D : nullptr, eps,
                      y_f32 ? y_f32 + (long)row * D : nullptr,
                      y_lp ? (void*)((char*)y_lp + (long)row * D * (LP_BF16 ? 2 : 4)) : nullptr, lane);
}

// ------------------------------------------------------------------------------------------------------- combine + norm
// YS = split-K slab count of the down-projection when known at compile time (1, 2, 4), else 0.  With a run-time slab loop every slab's load
// waited for the previous one's add (four dependent round trips per row at four slabs: 12 -> 16 us at B=128); unrolled, all the row's loads
// are in flight together.
template <bool LP_BF16, int NCH, int KK, bool FUSED, int YS>   // KK = top_k when known at compile time (1, 2), else 0; FUSED = ln_2 applied to u here
__global__ __launch_bounds__(256) void combine_norm_kernel(const float* u, const void* __restrict__ Y, int y_bf16, int y_splits,
                                                           long y_split_stride, const int* __restrict__ pos,
                                                           const float* __restrict__ posw, int N, int D, int k,
                                                           const float* __restrict__ g,
                                                           const float* __restrict__ cond, int rpc, float eps, float* x_next,
                                                           void* h, const float* __restrict__ u_ss, int u_ss_n,
                                                           const float* __restrict__ u_gain) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row = blockIdx.x * ROWS_PER_BLOCK + wave;
  if (row >= N) return;
  float* cache = reinterpret_cast<float*>(smem) + (size_t)wave * D;
  const float* ur = u + (long)row * D;
  float u_nrm = 1.0f;
  if constexpr (FUSED) u_nrm = row_norm_from_partials(u_ss + (long)row * u_ss_n, u_ss_n, D, eps, lane);
  [[maybe_unused]] const float ru_nrm = __frcp_rn(u_nrm);
  const int kk = KK ? KK : k;
  long prow[KK ? KK : 8]; float pw[KK ? KK : 8];
#pragma unroll
  for (int j = 0; j < (KK ? KK : 8); ++j) {
    if (j < kk) { prow[j] = (long)pos[(long)row * kk + j] * D; pw[j] = posw[(long)row * kk + j]; }
  }
  float ssq = 0.f;
  for_chunks<NCH>(D, lane, [&](int d) {
    float4 uu = *reinterpret_cast<const float4*>(ur + d);
    if constexpr (FUSED) {                                // ln_2 applied here instead of in a kernel of its own
      const float4 gg = *reinterpret_cast<const float4*>(u_gain + d);
      uu = make_float4(uu.x * ru_nrm * gg.x, uu.y * ru_nrm * gg.y, uu.z * ru_nrm * gg.z, uu.w * ru_nrm * gg.w);
    }
    float4 nx = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int j = 0; j < (KK ? KK : 8); ++j) {           // ascending expert id: next += w * expert(x)   (modedit.py:566)
      if (j < kk) {
        float4 y;
        if constexpr (YS > 0) {                           // split-K slabs of the down-projection, added in slice order
          float4 ys[YS];
#pragma unroll
          for (int z = 0; z < YS; ++z) ys[z] = load_y4(Y, y_bf16 != 0, (long)z * y_split_stride + prow[j] + d);
          y = ys[0];
#pragma unroll
          for (int z = 1; z < YS; ++z) { y.x += ys[z].x; y.y += ys[z].y; y.z += ys[z].z; y.w += ys[z].w; }
        } else {
          y = load_y4(Y, y_bf16 != 0, prow[j] + d);
          for (int z = 1; z < y_splits; ++z) {
            const float4 t = load_y4(Y, y_bf16 != 0, (long)z * y_split_stride + prow[j] + d);
            y.x += t.x; y.y += t.y; y.z += t.z; y.w += t.w;
          }
        }
        const float w = pw[j];
        nx.x = __fadd_rn(nx.x, __fmul_rn(w, y.x)); nx.y = __fadd_rn(nx.y, __fmul_rn(w, y.y));
        nx.z = __fadd_rn(nx.z, __fmul_rn(w, y.z)); nx.w = __fadd_rn(nx.w, __fmul_rn(w, y.w));
      }
    }
    const float4 v = make_float4(uu.x + nx.x, uu.y + nx.y, uu.z + nx.z, uu.w + nx.w);   // x + next_states (:595)
    *reinterpret_cast<float4*>(cache + d) = v;
    if (x_next) *reinterpret_cast<float4*>(x_next + (long)row * D + d) = v;
    ssq += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
  });
  if (!h) return;
  if constexpr (NCH > 0) {
    // the gain / conditioning rows do not depend on the reduction: fetch them before it so that their round trip overlaps the wave reduction
    // instead of following it (one dependent L2 round trip less per row)
    const float* cr = cond ? cond + (long)(row / rpc) * D : nullptr;
    float4 gq[NCH], cq[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      gq[c] = *reinterpret_cast<const float4*>(g + lane * 4 + c * 256);
      cq[c] = cr ? *reinterpret_cast<const float4*>(cr + lane * 4 + c * 256) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    ssq = wave_sum(ssq);
    const float nrm = fmaxf(sqrtf(ssq) * rsqrtf((float)D), eps);
    const float rnrm = __frcp_rn(nrm);                       // one reciprocal per row: a per-element fp32 division is a ~10-instruction VCC-serialised sequence
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int d = lane * 4 + c * 256;
      const float4 v = *reinterpret_cast<const float4*>(cache + d);
      float4 o = make_float4(v.x * rnrm * gq[c].x, v.y * rnrm * gq[c].y, v.z * rnrm * gq[c].z, v.w * rnrm * gq[c].w);   // (written out: scale4 re-orders this kernel's code)
      if (cr) { o.x += cq[c].x; o.y += cq[c].y; o.z += cq[c].z; o.w += cq[c].w; }
      store_lp4<LP_BF16>(h, (long)row * D + d, o);
    }
    return;
  }
  ssq = wave_sum(ssq);
  norm_store<LP_BF16, NCH>(cache, D, ssq, g, cond ? cond + (long)(row / rpc) * D : nullptr, eps, nullptr,
                           (void*)((char*)h + (long)row * D * (LP_BF16 ? 2 : 4)), lane);
}

// Numerics contract of the row-per-workgroup kernels' MoE combine, v = ln_2(u) + sum_j w_j * expert_j(row).  The block is written out in
// combine_norm_row_kernel, head_ddim_row_kernel and head_ddim_guided_row_kernel (a shared helper changed their compiled code, LABNOTES 2026-10-18),
// so a change to it is made in all three:
//   - experts are added in ascending expert id, nx = nx + w * y with separately rounded __fmul_rn / __fadd_rn (never contracted into an fma);
//   - the split-K slabs of the down-projection are added in slice order; YS is a compile-time BOUND on the slab count: slab z >= y_splits is
//     loaded from slab 0 (clamped index) and enters the sum as a selected 0.f;
//   - the fused ln_2 is u * (1 / max(sqrt(sum of partials) * D^-1/2, eps)) * gain: one reciprocal per row, the partials summed in the order of the
//     GEMM-side consumers (row_norm_from_partials);
//   - the row's norm is the cross-wave sum ((w0 + w1) + w2) + w3 of the wave sums, again with one reciprocal per row;
//   - every load is unconditional: columns past D are clamped to column 0 and the result is masked (see below).
//
// Small-batch form (N <= "gemm_skinny_rows" token rows, i.e. B <= 2 environments): ONE WORKGROUP per row, a thread owns 4 columns per 1024,
// so every load of the row (u, gains, conditioning, k x slabs expert rows) is requested at once and the kernel is two dependent round trips
// (routing slots -> rows) plus one cross-wave reduction.  With one wave per row the 14 rows of B = 1 occupied four CUs for 12.7 us.
// Every load of the kernel is unconditional (clamped slab index / column + selects; Y's dtype and the slab count are template parameters): a
// load under a run-time condition compiles into branch + load + s_waitcnt vmcnt(0), i.e. one dependent round trip per load (16 in a row here).
template <bool LP_BF16, int KK, bool FUSED, int NC, bool YBF, int YS>   // NC = ceil(D / 1024) <= 4; YS = slab count bound (1, 2, 4, 8)
__global__ __launch_bounds__(256) void combine_norm_row_kernel(const float* u, const void* __restrict__ Y, int y_splits,
                                                               long y_split_stride, const int* __restrict__ pos, const float* __restrict__ posw, int N,
                                                               int D, const float* __restrict__ g, const float* __restrict__ cond, int rpc, float eps,
                                                               float* x_next, void* h, const float* __restrict__ u_ss, int u_ss_n,
                                                               const float* __restrict__ u_gain) {
  __shared__ float red[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int row = blockIdx.x;
  long prow[KK]; float pw[KK];
#pragma unroll
  for (int j = 0; j < KK; ++j) { prow[j] = (long)pos[(long)row * KK + j] * D; pw[j] = posw[(long)row * KK + j]; }
  float u_nrm = 1.0f;
  if constexpr (FUSED) u_nrm = row_norm_from_partials(u_ss + (long)row * u_ss_n, u_ss_n, D, eps, lane);
  [[maybe_unused]] const float ru_nrm = __frcp_rn(u_nrm);
  const float* cr = cond + (long)(row / rpc) * D;                    // (cond == nullptr: never dereferenced, see `hc` below)
  const bool hc = cond != nullptr, hh = h != nullptr;
  float4 v[NC], gq[NC], cq[NC];
  float ssq = 0.f;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int d = tid * 4 + c * 1024;
    const bool in = d < D;
    const int dc = in ? d : 0;                                       // clamped column: the load always happens, the result is masked
    float4 uu = *reinterpret_cast<const float4*>(u + (long)row * D + dc);
    gq[c] = *reinterpret_cast<const float4*>((hh ? g : u) + dc);
    cq[c] = *reinterpret_cast<const float4*>((hc ? cr : u) + dc);
    float4 gg = make_float4(1.f, 1.f, 1.f, 1.f);
    if constexpr (FUSED) gg = *reinterpret_cast<const float4*>(u_gain + dc);
    float4 ys[KK][YS];
#pragma unroll
    for (int j = 0; j < KK; ++j)
#pragma unroll
      for (int z = 0; z < YS; ++z) {                                 // split-K slabs of the down-projection, all requested together
        const long off = (long)(z < y_splits ? z : 0) * y_split_stride + prow[j] + dc;
        ys[j][z] = load_y4<YBF>(Y, off);
      }
    if constexpr (FUSED) uu = scale4(uu, ru_nrm, gg);
    float4 nx = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int j = 0; j < KK; ++j) {                                   // ascending expert id: next += w * expert(x)   (modedit.py:566)
      float4 y = ys[j][0];
#pragma unroll
      for (int z = 1; z < YS; ++z) {                                 // slabs added in slice order
        const bool on = z < y_splits;
        y.x += on ? ys[j][z].x : 0.f; y.y += on ? ys[j][z].y : 0.f; y.z += on ? ys[j][z].z : 0.f; y.w += on ? ys[j][z].w : 0.f;
      }
      const float w = pw[j];
      nx.x = __fadd_rn(nx.x, __fmul_rn(w, y.x)); nx.y = __fadd_rn(nx.y, __fmul_rn(w, y.y));
      nx.z = __fadd_rn(nx.z, __fmul_rn(w, y.z)); nx.w = __fadd_rn(nx.w, __fmul_rn(w, y.w));
    }
    v[c] = make_float4(uu.x + nx.x, uu.y + nx.y, uu.z + nx.z, uu.w + nx.w);   // x + next_states (:595)
    if (!in) v[c] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (x_next && in) store_out16<StorePolicy::row>(x_next + (long)row * D + d, as_out_u4(v[c]));
    ssq += v[c].x * v[c].x + v[c].y * v[c].y + v[c].z * v[c].z + v[c].w * v[c].w;
  }
  if (!hh) return;
  ssq = wave_sum(ssq);
  if (lane == 0) red[wave] = ssq;
  __syncthreads();
  ssq = ((red[0] + red[1]) + red[2]) + red[3];
  const float rnrm = __frcp_rn(fmaxf(sqrtf(ssq) * rsqrtf((float)D), eps));
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int d = tid * 4 + c * 1024;
    if (d >= D) continue;
    float4 o = scale4(v[c], rnrm, gq[c]);
    if (hc) { o.x += cq[c].x; o.y += cq[c].y; o.z += cq[c].z; o.w += cq[c].w; }
    store_lp4<LP_BF16, StorePolicy::row>(h, (long)row * D + d, o);
  }
}

// --------------------------------------------------------------------------------------------------------------- embed
template <bool LP_BF16, int NCH, int AMAX>   // AMAX: widest action (8 or 32)
__global__ __launch_bounds__(256) void embed_tokens_kernel(const ModeEmbedDesc e) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row = blockIdx.x * ROWS_PER_BLOCK + wave;
  const int D = e.D, T = e.T;
  if (row >= e.B * T) return;
  const int b = row / T, t = row % T;
  float* cache = reinterpret_cast<float*>(smem) + (size_t)wave * D;
  const int t0 = e.use_noise_token ? 1 : 0;            // first goal position
  const int t_img = t0 + 1, t_act = t_img + e.n_img;   // goal_seq_len == 1 on this path
  const float cin = e.c_in ? e.c_in[(long)b * e.c_in_stride] : 1.0f;
  float a[AMAX];
  const int ai = t - t_act;
  if (ai >= 0) {
#pragma unroll
    for (int j = 0; j < AMAX; ++j) a[j] = (j < e.A_dim) ? e.actions[((long)b * e.A_len + ai) * e.A_dim + j] * cin : 0.f;
  }
  float ssq = 0.f;
  for_chunks<NCH>(D, lane, [&](int d) {
    float4 v;
    if (t < t0) {
      v = *reinterpret_cast<const float4*>(e.emb_t + (long)b * e.emb_row_stride + d);
    } else if (t < t_img) {
      const float4 ge = *reinterpret_cast<const float4*>(e.goal_e + (long)b * D + d);
      const float4 pp = *reinterpret_cast<const float4*>(e.pos + d);
      v = make_float4(ge.x + pp.x, ge.y + pp.y, ge.z + pp.z, ge.w + pp.w);
    } else if (t < t_act) {
      const float4 ie = *reinterpret_cast<const float4*>(e.img_e + ((long)b * e.n_img + (t - t_img)) * D + d);
      const float4 pp = *reinterpret_cast<const float4*>(e.pos + D + d);            // both image tokens share pos row 1
      v = make_float4(ie.x + pp.x, ie.y + pp.y, ie.z + pp.z, ie.w + pp.w);
    } else {
      const float4 pp = *reinterpret_cast<const float4*>(e.pos + (long)(1 + ai) * D + d);
      float o[4];
      if (e.A_dim == 7) {
        // rows d..d+3 of w_act [D, 7] are 28 contiguous floats starting at a 16-byte boundary (d % 4 == 0): 7 vector loads instead of 28
        // scalar ones; same fma order as the generic path
        float wv[28];
#pragma unroll
        for (int q = 0; q < 7; ++q) {
          const float4 t4 = *reinterpret_cast<const float4*>(e.w_act + (long)d * 7 + q * 4);
          wv[4 * q] = t4.x; wv[4 * q + 1] = t4.y; wv[4 * q + 2] = t4.z; wv[4 * q + 3] = t4.w;
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          float s_ = 0.f;
#pragma unroll
          for (int j = 0; j < 7; ++j) s_ = fmaf(a[j], wv[c * 7 + j], s_);
          o[c] = s_;
        }
      } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float* wr = e.w_act + (long)(d + c) * e.A_dim;
          float s_ = 0.f;
#pragma unroll
          for (int j = 0; j < AMAX; ++j) if (j < e.A_dim) s_ = fmaf(a[j], wr[j], s_);
          o[c] = s_;
        }
      }
      v = make_float4(o[0] + pp.x, o[1] + pp.y, o[2] + pp.z, o[3] + pp.w);
    }
    *reinterpret_cast<float4*>(cache + d) = v;
    *reinterpret_cast<float4*>(e.x + (long)row * D + d) = v;
    ssq += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
  });
  ssq = wave_sum(ssq);
  norm_store<LP_BF16, NCH>(cache, D, ssq, e.g, e.cond ? e.cond + (long)b * e.cond_row_stride : nullptr, e.eps, nullptr,
                      (void*)((char*)e.h + (long)row * D * (LP_BF16 ? 2 : 4)), lane);
}

// The head kernels' solver update on one output element, given its denoised prediction `den` (guided: already combined): the `denoised` output, then
// DDIM's / the two-point multistep / the two-stage solvers' linear update (ModeHeadDesc).
__device__ __forceinline__ void head_update(const ModeHeadDesc& h, long oidx, float den, float xa, float sc2, float sc3) {
  if (h.denoised) h.denoised[oidx] = den;
  float dd = den;                                     // two-point multistep (DPM-Solver++(2M), gc_sampling.py:724-727): (1 + 1/(2r)) D - (1/(2r)) D_old
  if (h.den_prev && sc3 != 0.0f) dd = (1.0f + sc3) * den - sc3 * h.den_prev[oidx];
  if (h.x_next) {
    if (h.lin) {                                        // two-stage solvers: a linear combination of this stage's input / prediction and two earlier tensors
      float v = __builtin_fmaf(h.lin[0], xa, h.lin[1] * den);
      if (h.aux1) v = __builtin_fmaf(h.lin[2], h.aux1[oidx], v);
      if (h.aux2) v = __builtin_fmaf(h.lin[3], h.aux2[oidx], v);
      h.x_next[oidx] = v;
    } else {
      h.x_next[oidx] = sc2 * xa + (1.0f - sc2) * dd;    // r*x + (1-r)*denoised (gc_sampling.py:948-950)
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- head
template <int NCH, int AMAX>   // NCH > 0: D == 256*NCH, chunk loops fully unrolled (all loads of a phase in flight together); AMAX: widest action (8 or 32)
__global__ __launch_bounds__(256) void head_ddim_kernel(const ModeHeadDesc h) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ar = blockIdx.x * ROWS_PER_BLOCK + wave;          // action-row index in [0, B*A_len)
  if (ar >= h.B * h.A_len) return;
  const int b = ar / h.A_len, ai = ar % h.A_len, D = h.D;
  const long row = (long)b * h.T + (h.T - h.A_len) + ai;      // last A_len tokens (modedit.py:807)
  float* cache = reinterpret_cast<float*>(smem) + (size_t)wave * D;
  const float* ur = h.u + row * D;
  const bool ybf = h.y_dtype == MODE_BF16;
  const float u_nrm = h.u_ss ? row_norm_from_partials(h.u_ss + row * h.u_ss_n, h.u_ss_n, D, h.eps, lane) : 1.0f;
  const float ru_nrm = __frcp_rn(u_nrm);
  // epilogue operands do not depend on the row math: fetch them first
  const bool act_lane = lane < h.A_dim;
  const long oidx = (long)ar * h.A_dim + lane;
  const float bo = act_lane ? h.b_out[lane] : 0.f;
  const float* scp = h.scal ? h.scal + (long)b * h.scal_stride : nullptr;
  const float sc0 = scp ? scp[0] : 0.f, sc1 = scp ? scp[1] : 0.f, sc2 = scp ? scp[2] : 0.f, sc3 = (scp && h.den_prev) ? scp[3] : 0.f;
  const float xa = (scp && act_lane) ? h.x_a[oidx] : 0.f;
  float ssq = 0.f;
  for_chunks<NCH>(D, lane, [&](int d) {
    float4 uu = *reinterpret_cast<const float4*>(ur + d);
    if (h.u_ss) {
      const float4 gg = *reinterpret_cast<const float4*>(h.u_gain + d);
      uu = scale4(uu, ru_nrm, gg);
    }
    float4 nx = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int j = 0; j < h.k; ++j) {
      const long p = h.pos[row * h.k + j];
      const float w = h.posw[row * h.k + j];
      float4 y;
      if (h.y_splits <= 4) {                               // all slabs of the row requested together (a run-time loop waits for each slab's add)
        float4 ys[4];
#pragma unroll
        for (int z = 0; z < 4; ++z)
          ys[z] = z < h.y_splits ? load_y4(h.Y, ybf, (long)z * h.y_split_stride + p * D + d) : make_float4(0.f, 0.f, 0.f, 0.f);
        y = ys[0];
#pragma unroll
        for (int z = 1; z < 4; ++z) { if (z < h.y_splits) { y.x += ys[z].x; y.y += ys[z].y; y.z += ys[z].z; y.w += ys[z].w; } }
      } else {
        y = load_y4(h.Y, ybf, p * D + d);
        for (int z = 1; z < h.y_splits; ++z) {
          const float4 t = load_y4(h.Y, ybf, (long)z * h.y_split_stride + p * D + d);
          y.x += t.x; y.y += t.y; y.z += t.z; y.w += t.w;
        }
      }
      nx.x = __fadd_rn(nx.x, __fmul_rn(w, y.x)); nx.y = __fadd_rn(nx.y, __fmul_rn(w, y.y));
      nx.z = __fadd_rn(nx.z, __fmul_rn(w, y.z)); nx.w = __fadd_rn(nx.w, __fmul_rn(w, y.w));
    }
    const float4 v = make_float4(uu.x + nx.x, uu.y + nx.y, uu.z + nx.z, uu.w + nx.w);
    *reinterpret_cast<float4*>(cache + d) = v;
    ssq += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
  });
  float accv[AMAX];
#pragma unroll
  for (int j = 0; j < AMAX; ++j) accv[j] = 0.f;
  if constexpr (NCH > 0 && AMAX <= 8) {
    // final-norm gain and the 7 head rows for all chunks are requested BEFORE the row reduction (their round trip overlaps it)
    float4 gq[NCH], wq[NCH][AMAX];
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int d = lane * 4 + c * 256;
      gq[c] = *reinterpret_cast<const float4*>(h.g + d);
#pragma unroll
      for (int j = 0; j < AMAX; ++j)
        wq[c][j] = j < h.A_dim ? *reinterpret_cast<const float4*>(h.w_out + (long)j * D + d) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    ssq = wave_sum(ssq);
    const float nrm = fmaxf(sqrtf(ssq) * rsqrtf((float)D), h.eps);
    const float rnrm = __frcp_rn(nrm);                       // one reciprocal per row: a per-element fp32 division is a ~10-instruction VCC-serialised sequence
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const float4 v = *reinterpret_cast<const float4*>(cache + lane * 4 + c * 256);
      const float4 n = scale4(v, rnrm, gq[c]);
#pragma unroll
      for (int j = 0; j < AMAX; ++j)
        if (j < h.A_dim) accv[j] += n.x * wq[c][j].x + n.y * wq[c][j].y + n.z * wq[c][j].z + n.w * wq[c][j].w;
    }
  } else {
    ssq = wave_sum(ssq);
    const float nrm = fmaxf(sqrtf(ssq) * rsqrtf((float)D), h.eps);
    const float rnrm = __frcp_rn(nrm);                       // one reciprocal per row: a per-element fp32 division is a ~10-instruction VCC-serialised sequence
    for (int d = lane * 4; d < D; d += 256) {
      const float4 v = *reinterpret_cast<const float4*>(cache + d);
      const float4 gg = *reinterpret_cast<const float4*>(h.g + d);
      const float4 n = scale4(v, rnrm, gg);
#pragma unroll
      for (int j = 0; j < AMAX; ++j) {
        if (j < h.A_dim) {
          const float4 w = *reinterpret_cast<const float4*>(h.w_out + (long)j * D + d);
          accv[j] += n.x * w.x + n.y * w.y + n.z * w.z + n.w * w.w;
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < AMAX; ++j) accv[j] = wave_sum(accv[j]);
  if (act_lane) {
    float F = 0.f;
#pragma unroll
    for (int j = 0; j < AMAX; ++j) if (lane == j) F = accv[j];
    F += bo;
    if (h.F) h.F[oidx] = F;
    if (scp) {
      const float den = F * sc1 + xa * sc0;               // F*c_out + x*c_skip      (score_wrappers.py:79-80)
      head_update(h, oidx, den, xa, sc2, sc3);
    }
  }
}

__global__ void ddim_edm_step_kernel(const float* F, const float* x_a, const float* scal, long scal_stride, int B,
                                     int per_sample, float* denoised, float* x_next) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)B * per_sample) return;
  const float* sc = scal + (i / per_sample) * scal_stride;
  const float xa = x_a[i];
  const float den = F[i] * sc[1] + xa * sc[0];
  if (denoised) denoised[i] = den;
  if (x_next) x_next[i] = sc[2] * xa + (1.0f - sc[2]) * den;
}

__global__ void sigma_embed_kernel(const float* sigma, const float* w, const float* b, float* e1, int R, int D) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)R * D) return;
  const int r = i / D, d = i % D;
  e1[i] = (logf(sigma[r]) / 4.0f) * w[d] + b[d];             // sigma.log()/4 -> Linear(1, D)   (modedit.py:824-828)
}

}  // namespace mode

using namespace mode;

// Run-time values -> template parameters.  among<V0, V1, ...>(v) names a run-time value and the compile-time constants it may take (the last one
// stands for "anything else"); dispatch(f, among..., among...) calls the generic lambda f with one std::integral_constant per value, so that
// f's body can write kernel<A(), B(), ...>.  Every combination of the lists is instantiated, no other.
template <auto V0, auto... Vs> struct Among { decltype(V0) v; };
template <auto V0, auto... Vs> static Among<V0, Vs...> among(decltype(V0) v) { return {v}; }
template <typename F> static void dispatch(F&& f) { f(); }
template <typename F, auto V0, auto... Vs, typename... Rest>
static void dispatch(F&& f, Among<V0, Vs...> a, Rest... rest) {
  if (sizeof...(Vs) == 0 || a.v == V0) dispatch([&](auto... cs) { f(std::integral_constant<decltype(V0), V0>{}, cs...); }, rest...);
  else if constexpr (sizeof...(Vs) > 0) dispatch(f, Among<Vs...>{a.v}, rest...);
}

template <bool LP>
static void launch_rmsnorm(dim3 grid, size_t lds, hipStream_t st, const float* x, const float* g, const float* cond, int rows, int D, int rpc,
                           float eps, float* y_f32, void* y_lp) {
  switch (D) {
    case 256: hipLaunchKernelGGL((rmsnorm_cond_kernel<LP, 1>), grid, dim3(256), lds, st, x, g, cond, rows, D, rpc, eps, y_f32, y_lp); break;
    case 512: hipLaunchKernelGGL((rmsnorm_cond_kernel<LP, 2>), grid, dim3(256), lds, st, x, g, cond, rows, D, rpc, eps, y_f32, y_lp); break;
    case 1024: hipLaunchKernelGGL((rmsnorm_cond_kernel<LP, 4>), grid, dim3(256), lds, st, x, g, cond, rows, D, rpc, eps, y_f32, y_lp); break;
    default: hipLaunchKernelGGL((rmsnorm_cond_kernel<LP, 0>), grid, dim3(256), lds, st, x, g, cond, rows, D, rpc, eps, y_f32, y_lp);
  }
}

extern "C" int mode_rmsnorm_cond_fwd(const float* x, const float* g, const float* cond, int rows, int D, int rows_per_cond,
                                     float eps, float* y_f32, void* y_lp, int lp_dtype, void* stream) {
  if (!x || !g || rows < 0 || D <= 0 || (D & 3)) return MODE_ERR_BAD_ARG;
  if (rows == 0) return MODE_OK;
  if (rows_per_cond <= 0) rows_per_cond = 1;
  const dim3 grid((rows + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK);
  const size_t lds = (size_t)ROWS_PER_BLOCK * D * 4;
  if (lds > kWaveRowLdsMax) return MODE_ERR_UNSUPPORTED;
  if (lp_dtype == MODE_BF16) launch_rmsnorm<true>(grid, lds, (hipStream_t)stream, x, g, cond, rows, D, rows_per_cond, eps, y_f32, y_lp);
  else launch_rmsnorm<false>(grid, lds, (hipStream_t)stream, x, g, cond, rows, D, rows_per_cond, eps, y_f32, y_lp);
  MODE_LAUNCH_CHECK();
  return MODE_OK;
}

template <bool LP, int NCH>
static void launch_combine_k(dim3 grid, size_t lds, hipStream_t st, const float* u, const void* Y, int ybf, int ys, long yss, const int* pos,
                             const float* posw, int N, int D, int k, const float* g, const float* cond, int rpc, float eps, float* x_next,
                             void* h, const float* u_ss, int u_ss_n, const float* u_gain) {
#define MODE_COMBINE(KK, F, S) hipLaunchKernelGGL((combine_norm_kernel<LP, NCH, KK, F, S>), grid, dim3(256), lds, st, u, Y, ybf, ys, yss, pos, posw, N, D, k, g, cond, rpc, eps, x_next, h, u_ss, u_ss_n, u_gain)
  if (u_ss && k == 2 && (ys == 1 || ys == 2 || ys == 4)) {      // the chain's shapes: slab loop unrolled
    if (ys == 4) MODE_COMBINE(2, true, 4); else if (ys == 2) MODE_COMBINE(2, true, 2); else MODE_COMBINE(2, true, 1);
  } else if (u_ss) { if (k == 2) MODE_COMBINE(2, true, 0); else if (k == 1) MODE_COMBINE(1, true, 0); else MODE_COMBINE(0, true, 0); }
  else { if (k == 2) MODE_COMBINE(2, false, 0); else if (k == 1) MODE_COMBINE(1, false, 0); else MODE_COMBINE(0, false, 0); }
#undef MODE_COMBINE
}

template <bool LP>
static void launch_combine(dim3 grid, size_t lds, hipStream_t st, const float* u, const void* Y, int ybf, int ys, long yss, const int* pos,
                           const float* posw, int N, int D, int k, const float* g, const float* cond, int rpc, float eps, float* x_next, void* h,
                           const float* u_ss, int u_ss_n, const float* u_gain) {
  switch (D) {
    case 256: launch_combine_k<LP, 1>(grid, lds, st, u, Y, ybf, ys, yss, pos, posw, N, D, k, g, cond, rpc, eps, x_next, h, u_ss, u_ss_n, u_gain); break;
    case 512: launch_combine_k<LP, 2>(grid, lds, st, u, Y, ybf, ys, yss, pos, posw, N, D, k, g, cond, rpc, eps, x_next, h, u_ss, u_ss_n, u_gain); break;
    case 1024: launch_combine_k<LP, 4>(grid, lds, st, u, Y, ybf, ys, yss, pos, posw, N, D, k, g, cond, rpc, eps, x_next, h, u_ss, u_ss_n, u_gain); break;
    default: launch_combine_k<LP, 0>(grid, lds, st, u, Y, ybf, ys, yss, pos, posw, N, D, k, g, cond, rpc, eps, x_next, h, u_ss, u_ss_n, u_gain);
  }
}

// "combine_row_max" option: token rows up to which the combine runs one workgroup per row (default: always; 0 = the one-wave-per-row kernel).
// Measured per 10-step chunk: B = 1 12.7 -> 5.4 us per launch, B = 32 10.29 -> 9.62 ms, B = 128 17.94 -> 17.88 ms.  One arithmetic for every
// batch size, so a sample's result stays independent of the batch it is in.
namespace mode { int g_combine_row_max = 0x7fffffff; }

extern "C" int mode_moe_combine_norm_fused_fwd(const float* u, const float* u_ss, int u_ss_n, const float* u_gain, const void* Y, int y_dtype,
                                               int y_splits, int64_t y_split_stride, const int32_t* pos, const float* posw, int N, int D, int k,
                                               const float* g, const float* cond, int rows_per_cond, float eps, float* x_next, void* h,
                                               int h_dtype, void* stream) {
  if (!u || !Y || !pos || !posw || N < 0 || D <= 0 || (D & 3) || k <= 0 || k > 8) return MODE_ERR_BAD_ARG;
  if (h && !g) return MODE_ERR_BAD_ARG;
  if (u_ss && (!u_gain || u_ss_n <= 0)) return MODE_ERR_BAD_ARG;
  if (N == 0) return MODE_OK;
  if (rows_per_cond <= 0) rows_per_cond = 1;
  if (y_splits < 1) y_splits = 1;
  const dim3 grid((N + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK);
  const size_t lds = (size_t)ROWS_PER_BLOCK * D * 4;
  const int ybf = y_dtype == MODE_BF16;
  if (N <= g_combine_row_max && D <= 4096 && y_splits <= 8 && (k == 1 || k == 2)) {   // one workgroup per row
    const hipStream_t st = (hipStream_t)stream;
    const int nc = (D + 1023) / 1024;
    const int ysb = y_splits <= 1 ? 1 : y_splits <= 2 ? 2 : y_splits <= 4 ? 4 : 8;
    dispatch([&](auto LP, auto KK, auto F, auto NC, auto YB, auto YS) {
      hipLaunchKernelGGL((combine_norm_row_kernel<LP(), KK(), F(), NC(), YB(), YS()>), dim3(N), dim3(256), 0, st, u, Y, y_splits, (long)y_split_stride, pos,
                         posw, N, D, g, cond, rows_per_cond, eps, x_next, h, u_ss, u_ss_n, u_gain);
    }, among<true, false>(h_dtype == MODE_BF16), among<2, 1>(k), among<true, false>(u_ss != nullptr), among<1, 2, 4>(nc), among<true, false>(ybf != 0),
       among<1, 2, 4, 8>(ysb));
    MODE_LAUNCH_CHECK();
    return MODE_OK;
  }
  if (lds > kWaveRowLdsMax) return MODE_ERR_UNSUPPORTED;
  if (h_dtype == MODE_BF16)
    launch_combine<true>(grid, lds, (hipStream_t)stream, u, Y, ybf, y_splits, (long)y_split_stride, pos, posw, N, D, k, g, cond, rows_per_cond, eps, x_next, h,
                         u_ss, u_ss_n, u_gain);
  else
    launch_combine<false>(grid, lds, (hipStream_t)stream, u, Y, ybf, y_splits, (long)y_split_stride, pos, posw, N, D, k, g, cond, rows_per_cond, eps, x_next, h,
                          u_ss, u_ss_n, u_gain);
  MODE_LAUNCH_CHECK();
  return MODE_OK;
}

extern "C" int mode_moe_combine_norm_fwd(const float* u, const void* Y, int y_dtype, int y_splits, int64_t y_split_stride, const int32_t* pos,
                                         const float* posw, int N, int D, int k, const float* g, const float* cond, int rows_per_cond,
                                         float eps, float* x_next, void* h, int h_dtype, void* stream) {
  return mode_moe_combine_norm_fused_fwd(u, nullptr, 0, nullptr, Y, y_dtype, y_splits, y_split_stride, pos, posw, N, D, k, g, cond, rows_per_cond,
                                         eps, x_next, h, h_dtype, stream);
}

namespace mode {
// One workgroup per token row (the form of the combine / head row kernels).  The token kind is uniform per workgroup: it selects a source row
// and a positional row by POINTER (dummy = the positional table, masked by selects), so the row's loads are unconditional; only the action
// rows' Linear(A_dim, D) sits behind a (scalar) branch.
//
// GUIDED (classifier-free guidance, ModeEmbedGuidedDesc): the grid has 2 * e.B * T rows; internal sample bi = b + h * e.B reads every input of PAIR b
// (nothing is duplicated in memory), and for h = 1 the goal token's source is a select to zero - the dummy row is loaded, as for an action token.
// Only the conditioning row and the output rows are indexed by the internal sample.
template <bool LP_BF16, int NC, int AMAX, bool GUIDED>   // AMAX: widest action (8 or 32; the instantiation for 8 is the original kernel)
__global__ __launch_bounds__(256) void embed_tokens_row_kernel(const ModeEmbedDesc e) {
  __shared__ float red[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int row = blockIdx.x, D = e.D, T = e.T;
  const int bi = row / T, t = row % T;
  const bool unc = GUIDED && bi >= e.B;                // unconditional branch of pair bi - e.B
  const int b = unc ? bi - e.B : bi;
  const int t0 = e.use_noise_token ? 1 : 0;            // first goal position
  const int t_img = t0 + 1, t_act = t_img + e.n_img;   // goal_seq_len == 1 on this path
  const int ai = t - t_act;
  const bool is_act = ai >= 0, is_noise = t < t0, is_goal = !is_noise && t < t_img;
  const float* src = is_noise ? e.emb_t + (long)b * e.emb_row_stride
                   : is_goal  ? (unc ? e.pos : e.goal_e + (long)b * D)
                   : !is_act  ? e.img_e + ((long)b * e.n_img + (t - t_img)) * D : e.pos;
  const float* pp = is_act ? e.pos + (long)(1 + ai) * D : is_goal ? e.pos : e.pos + D;   // both image tokens share pos row 1; the noise token has none
  const bool has_src = !is_act && !(unc && is_goal), has_pos = !is_noise;   // (no source: the action rows' Linear, or zero when not an action row)
  const float cin = (e.c_in ? e.c_in : e.pos)[e.c_in ? (long)b * e.c_in_stride : 0];
  float a[AMAX];
  {
    const long abase = ((long)b * e.A_len + (is_act ? ai : 0)) * e.A_dim;
#pragma unroll
    for (int j = 0; j < AMAX; ++j) a[j] = e.actions[abase + (j < e.A_dim ? j : 0)];
#pragma unroll
    for (int j = 0; j < AMAX; ++j) a[j] = j < e.A_dim ? a[j] * (e.c_in ? cin : 1.0f) : 0.f;
  }
  const float* cr = e.cond ? e.cond + (long)bi * e.cond_row_stride : e.pos;
  float4 v[NC], gq[NC], cq[NC];
  float ssq = 0.f;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int d = tid * 4 + c * 1024;
    const bool in = d < D;
    const int dc = in ? d : 0;
    const float4 sv = *reinterpret_cast<const float4*>(src + dc), pv = *reinterpret_cast<const float4*>(pp + dc);
    gq[c] = *reinterpret_cast<const float4*>(e.g + dc);
    cq[c] = *reinterpret_cast<const float4*>(cr + dc);
    float o[4] = {0.f, 0.f, 0.f, 0.f};
    if (is_act) {
      if (e.A_dim == 7) {
        // rows d..d+3 of w_act [D, 7] are 28 contiguous floats starting at a 16-byte boundary (d % 4 == 0): 7 vector loads
        float wv[28];
#pragma unroll
        for (int q = 0; q < 7; ++q) {
          const float4 t4 = *reinterpret_cast<const float4*>(e.w_act + (long)dc * 7 + q * 4);
          wv[4 * q] = t4.x; wv[4 * q + 1] = t4.y; wv[4 * q + 2] = t4.z; wv[4 * q + 3] = t4.w;
        }
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) {
          float s_ = 0.f;
#pragma unroll
          for (int j = 0; j < 7; ++j) s_ = fmaf(a[j], wv[cc * 7 + j], s_);
          o[cc] = s_;
        }
      } else {
        float wr[4][AMAX];
#pragma unroll
        for (int cc = 0; cc < 4; ++cc)
#pragma unroll
          for (int j = 0; j < AMAX; ++j) wr[cc][j] = e.w_act[(long)(dc + cc) * e.A_dim + (j < e.A_dim ? j : 0)];
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) {
          float s_ = 0.f;
#pragma unroll
          for (int j = 0; j < AMAX; ++j) s_ = j < e.A_dim ? fmaf(a[j], wr[cc][j], s_) : s_;
          o[cc] = s_;
        }
      }
    }
    const float4 s4 = has_src ? sv : make_float4(o[0], o[1], o[2], o[3]);
    const float4 p4 = has_pos ? pv : make_float4(0.f, 0.f, 0.f, 0.f);
    v[c] = in ? make_float4(s4.x + p4.x, s4.y + p4.y, s4.z + p4.z, s4.w + p4.w) : make_float4(0.f, 0.f, 0.f, 0.f);
    if (in) store_out16<StorePolicy::row>(e.x + (long)row * D + d, as_out_u4(v[c]));
    ssq += v[c].x * v[c].x + v[c].y * v[c].y + v[c].z * v[c].z + v[c].w * v[c].w;
  }
  ssq = wave_sum(ssq);
  if (lane == 0) red[wave] = ssq;
  __syncthreads();
  ssq = ((red[0] + red[1]) + red[2]) + red[3];
  const float rnrm = __frcp_rn(fmaxf(sqrtf(ssq) * rsqrtf((float)D), e.eps));
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int d = tid * 4 + c * 1024;
    if (d >= D) continue;
    float4 o = scale4(v[c], rnrm, gq[c]);
    if (e.cond) { o.x += cq[c].x; o.y += cq[c].y; o.z += cq[c].z; o.w += cq[c].w; }
    store_lp4<LP_BF16, StorePolicy::row>(e.h, (long)row * D + d, o);
  }
}
}  // namespace mode

static bool embed_desc_complete(const ModeEmbedDesc* d) {
  return d && d->goal_e && d->img_e && d->actions && d->w_act && d->pos && d->g && d->x && d->h && (!d->use_noise_token || d->emb_t);
}
static bool embed_desc_supported(const ModeEmbedDesc* d) {
  return !(d->D & 3) && d->A_dim <= kMaxActionDim && d->T == (d->use_noise_token ? 1 : 0) + 1 + d->n_img + d->A_len;
}
// launch the one-workgroup-per-row embed kernel (G: its guided form) on `rows` rows
template <bool G>
static void launch_embed_row(const ModeEmbedDesc* d, int rows, hipStream_t st) {
  dispatch([&](auto LP, auto NC, auto AMAX) {
    hipLaunchKernelGGL((embed_tokens_row_kernel<LP(), NC(), AMAX(), G>), dim3(rows), dim3(256), 0, st, *d);
  }, among<true, false>(d->h_dtype == MODE_BF16), among<1, 2, 4>((d->D + 1023) / 1024), among<32, 8>(d->A_dim > 8 ? 32 : 8));
}

extern "C" int mode_embed_tokens_guided_fwd(const ModeEmbedGuidedDesc* gd, void* stream) {
  const ModeEmbedDesc* d = gd ? &gd->emb : nullptr;
  if (!embed_desc_complete(d)) return MODE_ERR_BAD_ARG;
  if (!embed_desc_supported(d) || d->D > 4096 || d->A_dim < 1) return MODE_ERR_UNSUPPORTED;   // pairs exist in the row kernel only
  const int rows = 2 * d->B * d->T;                                   // both branches of every pair
  if (rows == 0) return MODE_OK;
  launch_embed_row<true>(d, rows, (hipStream_t)stream);
  MODE_LAUNCH_CHECK();
  return MODE_OK;
}

extern "C" int mode_embed_tokens_fwd(const ModeEmbedDesc* d, void* stream) {
  if (!embed_desc_complete(d)) return MODE_ERR_BAD_ARG;
  if (!embed_desc_supported(d)) return MODE_ERR_UNSUPPORTED;
  const int rows = d->B * d->T;
  if (rows == 0) return MODE_OK;
  if (d->D <= 4096 && d->A_dim >= 1) {                               // one workgroup per row
    launch_embed_row<false>(d, rows, (hipStream_t)stream);
    MODE_LAUNCH_CHECK();
    return MODE_OK;
  }
  const dim3 grid((rows + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK);
  const size_t lds = (size_t)ROWS_PER_BLOCK * d->D * 4;
  if (lds > kWaveRowLdsMax) return MODE_ERR_UNSUPPORTED;
  const hipStream_t st = (hipStream_t)stream;
  dispatch([&](auto LP, auto NCH, auto AMAX) {                         // AMAX = 32: the instantiations for A_dim > 8
    hipLaunchKernelGGL((embed_tokens_kernel<LP(), NCH(), AMAX()>), grid, dim3(256), lds, st, *d);
  }, among<true, false>(d->h_dtype == MODE_BF16), among<4, 0>(d->D == 1024 ? 4 : 0), among<32, 8>(d->A_dim > 8 ? 32 : 8));
  MODE_LAUNCH_CHECK();
  return MODE_OK;
}

namespace mode {
// One workgroup per action row (the form of combine_norm_row_kernel): a thread owns 4 columns per 1024; every load of the row - residual, ln_2
// partials and gain, k x slabs expert rows, final-norm gain, the A_dim head rows, bias, EDM scalings, noisy action - is unconditional (clamped
// indices + selects, dtype / slab bound / top-k as template parameters) and requested before the first reduction.  The one-wave-per-row kernel
// above had compiled into ~40 dependent branch + load + wait rounds: 18 us per denoise step whatever the batch.
template <int KK, bool FUSED, bool YBF, int YS, int NC, int AMAX>   // AMAX: widest action (8 or 32; the instantiation for 8 is the original kernel)
__global__ __launch_bounds__(256) void head_ddim_row_kernel(const ModeHeadDesc h) {
  __shared__ float red[4];
  __shared__ float racc[4][AMAX];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ar = blockIdx.x;                                       // action-row index in [0, B*A_len)
  const int b = ar / h.A_len, ai = ar % h.A_len, D = h.D;
  const long row = (long)b * h.T + (h.T - h.A_len) + ai;           // last A_len tokens (modedit.py:807)
  long prow[KK]; float pw[KK];
#pragma unroll
  for (int j = 0; j < KK; ++j) { prow[j] = (long)h.pos[row * KK + j] * D; pw[j] = h.posw[row * KK + j]; }
  float u_nrm = 1.0f;
  if constexpr (FUSED) u_nrm = row_norm_from_partials(h.u_ss + row * h.u_ss_n, h.u_ss_n, D, h.eps, lane);
  [[maybe_unused]] const float ru_nrm = __frcp_rn(u_nrm);
  // epilogue operands (thread j < A_dim finishes output j): clamped, unconditional
  const int jo = tid < h.A_dim ? tid : 0;
  const long oidx = (long)ar * h.A_dim + jo;
  const float bo = h.b_out[jo];
  const bool has_sc = h.scal != nullptr;
  const float* scp = has_sc ? h.scal + (long)b * h.scal_stride : h.b_out;   // (never used when !has_sc)
  const float sc0 = scp[0], sc1 = has_sc ? scp[1] : 0.f, sc2 = has_sc ? scp[2] : 0.f, sc3 = (has_sc && h.den_prev) ? scp[3] : 0.f;
  const float xa = (has_sc ? h.x_a : h.b_out)[has_sc ? oidx : 0];
  constexpr int WQ = AMAX <= 8 ? AMAX : 1;                        // AMAX 8: the head rows are requested with the row's loads; 32: read where used
  float4 v[NC], gq[NC], wq[NC][WQ];
  float ssq = 0.f;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int d = tid * 4 + c * 1024;
    const bool in = d < D;
    const int dc = in ? d : 0;
    float4 uu = *reinterpret_cast<const float4*>(h.u + row * D + dc);
    gq[c] = *reinterpret_cast<const float4*>(h.g + dc);
    if constexpr (AMAX <= 8) {
#pragma unroll
      for (int j = 0; j < AMAX; ++j) wq[c][j] = *reinterpret_cast<const float4*>(h.w_out + (long)(j < h.A_dim ? j : 0) * D + dc);
    }
    float4 gg = make_float4(1.f, 1.f, 1.f, 1.f);
    if constexpr (FUSED) gg = *reinterpret_cast<const float4*>(h.u_gain + dc);
    float4 ys[KK][YS];
#pragma unroll
    for (int j = 0; j < KK; ++j)
#pragma unroll
      for (int z = 0; z < YS; ++z) {
        const long off = (long)(z < h.y_splits ? z : 0) * h.y_split_stride + prow[j] + dc;
        ys[j][z] = load_y4<YBF>(h.Y, off);
      }
    if constexpr (FUSED) uu = scale4(uu, ru_nrm, gg);
    float4 nx = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int j = 0; j < KK; ++j) {
      float4 y = ys[j][0];
#pragma unroll
      for (int z = 1; z < YS; ++z) {
        const bool on = z < h.y_splits;
        y.x += on ? ys[j][z].x : 0.f; y.y += on ? ys[j][z].y : 0.f; y.z += on ? ys[j][z].z : 0.f; y.w += on ? ys[j][z].w : 0.f;
      }
      const float w = pw[j];
      nx.x = __fadd_rn(nx.x, __fmul_rn(w, y.x)); nx.y = __fadd_rn(nx.y, __fmul_rn(w, y.y));
      nx.z = __fadd_rn(nx.z, __fmul_rn(w, y.z)); nx.w = __fadd_rn(nx.w, __fmul_rn(w, y.w));
    }
    v[c] = in ? make_float4(uu.x + nx.x, uu.y + nx.y, uu.z + nx.z, uu.w + nx.w) : make_float4(0.f, 0.f, 0.f, 0.f);
    ssq += v[c].x * v[c].x + v[c].y * v[c].y + v[c].z * v[c].z + v[c].w * v[c].w;
  }
  ssq = wave_sum(ssq);
  if (lane == 0) red[wave] = ssq;
  __syncthreads();
  ssq = ((red[0] + red[1]) + red[2]) + red[3];
  const float rnrm = __frcp_rn(fmaxf(sqrtf(ssq) * rsqrtf((float)D), h.eps));
  float accv[AMAX];
#pragma unroll
  for (int j = 0; j < AMAX; ++j) accv[j] = 0.f;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const float4 n = scale4(v[c], rnrm, gq[c]);   // v = 0 past D
#pragma unroll
    for (int j = 0; j < AMAX; ++j) {
      float4 w;
      if constexpr (AMAX <= 8) w = wq[c][j];
      else w = *reinterpret_cast<const float4*>(h.w_out + (long)(j < h.A_dim ? j : 0) * D + (tid * 4 + c * 1024 < D ? tid * 4 + c * 1024 : 0));
      accv[j] += n.x * w.x + n.y * w.y + n.z * w.z + n.w * w.w;
    }
  }
#pragma unroll
  for (int j = 0; j < AMAX; ++j) accv[j] = wave_sum(accv[j]);
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < AMAX; ++j) racc[wave][j] = accv[j];
  }
  __syncthreads();
  if (tid < h.A_dim) {
    const float F = (((racc[0][tid] + racc[1][tid]) + racc[2][tid]) + racc[3][tid]) + bo;
    if (h.F) h.F[oidx] = F;
    if (has_sc) {
      const float den = F * sc1 + xa * sc0;               // F*c_out + x*c_skip      (score_wrappers.py:79-80)
      head_update(h, oidx, den, xa, sc2, sc3);
    }
  }
}
}  // namespace mode

namespace mode {
// head_ddim_row_kernel for classifier-free guidance (ModeHeadGuidedDesc): one workgroup per action row of a PAIR finishes both of its hidden rows,
// r = 0 the conditional branch (internal sample b), r = 1 the unconditional one (b + B).  What does not depend on the branch - final-norm gain, head
// rows, ln_2 gain, bias, scalings, noisy action, the guidance scale - is loaded once; the two rows' residuals, partials and k x slabs expert rows
// are requested in the same unrolled pass, so both branches' loads are in flight before the first reduction, and the reductions of the two rows share
// their barriers.  Each branch's prediction is formed by the expressions of head_ddim_row_kernel; den = den_u + w (den_c - den_u) then enters
// head_update in the place of `denoised`.
template <int KK, bool FUSED, bool YBF, int YS, int NC, int AMAX>
__global__ __launch_bounds__(256) void head_ddim_guided_row_kernel(const ModeHeadDesc h, const float* __restrict__ scale) {
  __shared__ float red[2][4];
  __shared__ float racc[2][4][AMAX];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ar = blockIdx.x;                                       // action-row index in [0, B*A_len), B pairs
  const int b = ar / h.A_len, ai = ar % h.A_len, D = h.D;
  long row[2], prow[2][KK]; float pw[2][KK], ru_nrm[2];
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    row[r] = (long)(b + r * h.B) * h.T + (h.T - h.A_len) + ai;
#pragma unroll
    for (int j = 0; j < KK; ++j) { prow[r][j] = (long)h.pos[row[r] * KK + j] * D; pw[r][j] = h.posw[row[r] * KK + j]; }
    float u_nrm = 1.0f;
    if constexpr (FUSED) u_nrm = row_norm_from_partials(h.u_ss + row[r] * h.u_ss_n, h.u_ss_n, D, h.eps, lane);
    ru_nrm[r] = __frcp_rn(u_nrm);
  }
  // epilogue operands (thread j < A_dim finishes output j of the pair): clamped, unconditional
  const int jo = tid < h.A_dim ? tid : 0;
  const long oidx = (long)ar * h.A_dim + jo;
  const float bo = h.b_out[jo];
  const float* scp = h.scal + (long)b * h.scal_stride;
  const float sc0 = scp[0], sc1 = scp[1], sc2 = scp[2], sc3 = h.den_prev ? scp[3] : 0.f;
  const float xa = h.x_a[oidx];
  const float gw = scale[0];
  constexpr int WQ = AMAX <= 8 ? AMAX : 1;                        // AMAX 8: the head rows are requested with the rows' loads; 32: read where used
  float4 v[2][NC], gq[NC], wq[NC][WQ];
  float ssq[2] = {0.f, 0.f};
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int d = tid * 4 + c * 1024;
    const bool in = d < D;
    const int dc = in ? d : 0;
    gq[c] = *reinterpret_cast<const float4*>(h.g + dc);
    if constexpr (AMAX <= 8) {
#pragma unroll
      for (int j = 0; j < AMAX; ++j) wq[c][j] = *reinterpret_cast<const float4*>(h.w_out + (long)(j < h.A_dim ? j : 0) * D + dc);
    }
    float4 gg = make_float4(1.f, 1.f, 1.f, 1.f);
    if constexpr (FUSED) gg = *reinterpret_cast<const float4*>(h.u_gain + dc);
    float4 uu[2], ys[2][KK][YS];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      uu[r] = *reinterpret_cast<const float4*>(h.u + row[r] * D + dc);
#pragma unroll
      for (int j = 0; j < KK; ++j)
#pragma unroll
        for (int z = 0; z < YS; ++z) {
          const long off = (long)(z < h.y_splits ? z : 0) * h.y_split_stride + prow[r][j] + dc;
          ys[r][j][z] = load_y4<YBF>(h.Y, off);
        }
    }
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      float4 u4 = uu[r];
      if constexpr (FUSED) u4 = scale4(u4, ru_nrm[r], gg);
      float4 nx = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int j = 0; j < KK; ++j) {
        float4 y = ys[r][j][0];
#pragma unroll
        for (int z = 1; z < YS; ++z) {
          const bool on = z < h.y_splits;
          y.x += on ? ys[r][j][z].x : 0.f; y.y += on ? ys[r][j][z].y : 0.f; y.z += on ? ys[r][j][z].z : 0.f; y.w += on ? ys[r][j][z].w : 0.f;
        }
        const float w = pw[r][j];
        nx.x = __fadd_rn(nx.x, __fmul_rn(w, y.x)); nx.y = __fadd_rn(nx.y, __fmul_rn(w, y.y));
        nx.z = __fadd_rn(nx.z, __fmul_rn(w, y.z)); nx.w = __fadd_rn(nx.w, __fmul_rn(w, y.w));
      }
      v[r][c] = in ? make_float4(u4.x + nx.x, u4.y + nx.y, u4.z + nx.z, u4.w + nx.w) : make_float4(0.f, 0.f, 0.f, 0.f);
      ssq[r] += v[r][c].x * v[r][c].x + v[r][c].y * v[r][c].y + v[r][c].z * v[r][c].z + v[r][c].w * v[r][c].w;
    }
  }
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    ssq[r] = wave_sum(ssq[r]);
    if (lane == 0) red[r][wave] = ssq[r];
  }
  __syncthreads();
  float rnrm[2], accv[2][AMAX];
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    rnrm[r] = __frcp_rn(fmaxf(sqrtf(((red[r][0] + red[r][1]) + red[r][2]) + red[r][3]) * rsqrtf((float)D), h.eps));
#pragma unroll
    for (int j = 0; j < AMAX; ++j) accv[r][j] = 0.f;
  }
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    float4 n[2];
#pragma unroll
    for (int r = 0; r < 2; ++r)                                     // v = 0 past D
      n[r] = scale4(v[r][c], rnrm[r], gq[c]);
#pragma unroll
    for (int j = 0; j < AMAX; ++j) {
      float4 w;
      if constexpr (AMAX <= 8) w = wq[c][j];
      else w = *reinterpret_cast<const float4*>(h.w_out + (long)(j < h.A_dim ? j : 0) * D + (tid * 4 + c * 1024 < D ? tid * 4 + c * 1024 : 0));
#pragma unroll
      for (int r = 0; r < 2; ++r) accv[r][j] += n[r].x * w.x + n[r].y * w.y + n[r].z * w.z + n[r].w * w.w;
    }
  }
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int j = 0; j < AMAX; ++j) accv[r][j] = wave_sum(accv[r][j]);
  if (lane == 0) {
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int j = 0; j < AMAX; ++j) racc[r][wave][j] = accv[r][j];
  }
  __syncthreads();
  if (tid < h.A_dim) {
    float den[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const float F = (((racc[r][0][tid] + racc[r][1][tid]) + racc[r][2][tid]) + racc[r][3][tid]) + bo;
      den[r] = F * sc1 + xa * sc0;                       // F*c_out + x*c_skip of the branch      (score_wrappers.py:79-80)
    }
    head_update(h, oidx, __fadd_rn(den[1], __fmul_rn(gw, __fsub_rn(den[0], den[1]))), xa, sc2, sc3);   // D_u + w (D_c - D_u)
  }
}
}  // namespace mode

static bool head_desc_complete(const ModeHeadDesc* d) {
  return d && d->u && d->Y && d->pos && d->posw && d->g && d->w_out && d->b_out && (!d->scal || d->x_a) && (!d->u_ss || (d->u_gain && d->u_ss_n > 0));
}
static bool head_row_kernel_takes(const ModeHeadDesc* d) {          // shapes of the one-workgroup-per-row head kernels
  return d->D <= 4096 && d->y_splits <= 8 && (d->k == 1 || d->k == 2) && d->A_dim >= 1;
}
// call f with the head row kernels' template parameters <KK, FUSED, YBF, YS, NC, AMAX> for the shapes of d, as compile-time constants
template <typename F>
static void dispatch_head_row(const ModeHeadDesc* d, F&& f) {
  dispatch(f, among<2, 1>(d->k), among<true, false>(d->u_ss != nullptr), among<true, false>(d->y_dtype == MODE_BF16),
           among<1, 2, 4, 8>(d->y_splits <= 1 ? 1 : d->y_splits <= 2 ? 2 : d->y_splits <= 4 ? 4 : 8), among<1, 2, 4>((d->D + 1023) / 1024),
           among<32, 8>(d->A_dim > 8 ? 32 : 8));
}

extern "C" int mode_head_ddim_guided_fwd(const ModeHeadGuidedDesc* gd, void* stream) {
  const ModeHeadDesc* d = gd ? &gd->head : nullptr;
  if (!head_desc_complete(d) || !gd->scale || !d->scal || d->F) return MODE_ERR_BAD_ARG;   // the raw output F has no guided form
  if ((d->D & 3) || d->A_dim > kMaxActionDim || !head_row_kernel_takes(d)) return MODE_ERR_UNSUPPORTED;   // pairs exist in the row kernel only
  const int rows = d->B * d->A_len;
  if (rows == 0) return MODE_OK;
  dispatch_head_row(d, [&](auto KK, auto F, auto YB, auto YS, auto NC, auto AMAX) {
    hipLaunchKernelGGL((head_ddim_guided_row_kernel<KK(), F(), YB(), YS(), NC(), AMAX()>), dim3(rows), dim3(256), 0, (hipStream_t)stream, *d, gd->scale);
  });
  MODE_LAUNCH_CHECK();
  return MODE_OK;
}

extern "C" int mode_head_ddim_fwd(const ModeHeadDesc* d, void* stream) {
  if (!head_desc_complete(d)) return MODE_ERR_BAD_ARG;
  if ((d->D & 3) || d->A_dim > kMaxActionDim) return MODE_ERR_UNSUPPORTED;
  const int rows = d->B * d->A_len;
  if (rows == 0) return MODE_OK;
  if (head_row_kernel_takes(d)) {                                     // one workgroup per row
    dispatch_head_row(d, [&](auto KK, auto F, auto YB, auto YS, auto NC, auto AMAX) {
      hipLaunchKernelGGL((head_ddim_row_kernel<KK(), F(), YB(), YS(), NC(), AMAX()>), dim3(rows), dim3(256), 0, (hipStream_t)stream, *d);
    });
    MODE_LAUNCH_CHECK();
    return MODE_OK;
  }
  const dim3 grid((rows + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK);
  const size_t lds = (size_t)ROWS_PER_BLOCK * d->D * 4;
  if (lds > kWaveRowLdsMax) return MODE_ERR_UNSUPPORTED;
  const hipStream_t st = (hipStream_t)stream;
  dispatch([&](auto NCH, auto AMAX) {                                  // AMAX = 32: the instantiations for A_dim > 8
    hipLaunchKernelGGL((head_ddim_kernel<NCH(), AMAX()>), grid, dim3(256), lds, st, *d);
  }, among<4, 0>(d->D == 1024 ? 4 : 0), among<32, 8>(d->A_dim > 8 ? 32 : 8));
  MODE_LAUNCH_CHECK();
  return MODE_OK;
}

extern "C" int mode_ddim_edm_step(const float* F, const float* x_a, const float* scal, int64_t scal_stride, int B, int per_sample,
                                  float* denoised, float* x_next, void* stream) {
  if (!F || !x_a || !scal) return MODE_ERR_BAD_ARG;
  const long n = (long)B * per_sample;
  if (n == 0) return MODE_OK;
  hipLaunchKernelGGL(ddim_edm_step_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, F, x_a, scal, (long)scal_stride, B,
                     per_sample, denoised, x_next);
  MODE_LAUNCH_CHECK();
  return MODE_OK;
}

extern "C" int mode_sigma_embed(const float* sigma, const float* w, const float* b, float* e1, int R, int D, void* stream) {
  if (!sigma || !w || !b || !e1) return MODE_ERR_BAD_ARG;
  const long n = (long)R * D;
  if (n == 0) return MODE_OK;
  hipLaunchKernelGGL(sigma_embed_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, sigma, w, b, e1, R, D);
  MODE_LAUNCH_CHECK();
  return MODE_OK;
}
