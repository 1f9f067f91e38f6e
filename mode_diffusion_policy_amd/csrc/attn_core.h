// The wave-level body of the tiny-T causal attention (see attn.hip for the layout story), shared by the stand-alone kernel (operands from the
// packed qkv buffer in global memory) and the fused QKV-projection + attention kernel (qkv_attn.hip: operands from the bf16 q | k | v tile the GEMM
// epilogue left in LDS).  ONE definition so that both produce the same bits: a sample's result must not depend on which chain its batch size selects
// (tests/test_gpu_model.py::test_c2_full_size_properties).
// Also what the attention family defines ONCE: the entry points that cross translation units, the LDS layouts of the backward kernels and the long fp32 forward
// (carved by the kernel, sized by its launcher), and the phases that the two backward kernels (attn.hip: T <= 16, attn_long.hip: T <= 64) have in common.
#pragma once
#include <type_traits>

#include "mode_common.h"

namespace mode {

// ---- host: entry points and the option used across translation units (defined in attn.hip / attn_long.hip; called from there, dit.hip, dit_train.hip)
extern int g_attn_bwd_mfma;   // "attn_bwd_mfma" option: 1 = the attention backward's matrix products on fp32 MFMA (head_dim % 16 == 0), 0 = the VALU form
// dbias_partial (optional): [B][3 D] fp32, row b = sample b's share of the packed QKV bias gradient (dit_train.hip adds the rows)
int attn_block_bwd_launch(const void* qkv, const float* q_gain, const float* k_gain, const void* dy, void* dqkv, float* dgq_partial, float* dgk_partial, int dtype, int B,
                          int T, int H, int head_dim, float eps, uint32_t seed, float p_drop, float* dbias_partial, void* stream);
// attn_long.hip: the kernels for 16 < T <= 64 (taken by both entry points of attn.hip when T > 16)
int attn_long_fwd_launch(const void* qkv, const float* qg, const float* kg, void* y, int dtype, int B, int T, int H, int HD, float eps, uint32_t seed,
                         uint32_t thresh, float inv_keep, hipStream_t s);
int attn_long_bwd_launch(const void* qkv, const float* qg, const float* kg, const void* dy, void* dqkv, float* dgq_partial, float* dgk_partial, int dtype,
                         int B, int T, int H, int HD, float eps, uint32_t seed, uint32_t thresh, float inv_keep, float* dbias_partial, hipStream_t s);
// 32*(NKS-1) < head_dim <= 32*NKS of the bf16 forward kernels: LAUNCH(NKS) for head_dim in 1..128
#define MODE_ATTN_NKS_DISPATCH(head_dim, LAUNCH) \
  switch (((head_dim) + 31) / 32) { case 1: LAUNCH(1); break; case 2: LAUNCH(2); break; case 3: LAUNCH(3); break; default: LAUNCH(4); break; }

// ---- LDS layouts: byte offsets of a kernel's arrays in its dynamic LDS, from the kernel's shape arguments.  The kernel takes its pointers from the struct and
// the launcher passes `bytes` (the end of the last array) as the launch's LDS size, so the two cannot disagree.  `bytes` is exact - the arrays plus the alignment
// gaps the kernel really has - and so never above the rounded-up formulas the launchers used to carry.  Plain sums of products of the shape (int: callers bound T and
// head_dim first), rounded up only where the kernel pads: and-masks on the running offset cost attn_bwd_kernel<bf16, VALU> 24 bytes of scratch.
constexpr __host__ __device__ int pad16(int bytes) { return (bytes + 15) & ~15; }
constexpr __host__ __device__ int lds_take(int& end, int bytes) { end += bytes; return end - bytes; }   // the next array's offset; `end` moves past it
template <class E> __device__ __forceinline__ E* lds_at(char* smem, int off) { return reinterpret_cast<E*>(smem + off); }

// attn_f32_kernel and attn_long_bf16_kernel keep their carve-ups and their launchers' formulas by hand: with a layout struct the same arithmetic was scheduled
// differently and measured 1.2 % and 0.8 % slower (profiles/attention_refactor.txt).
struct AttnLongF32Lds {      // attn_long_f32_kernel: q, k, v [T][HP], p [T][TP]
  int HP = 0, TP = 0;
  int q = 0, k = 0, v = 0, p = 0, bytes = 0;
  constexpr __host__ __device__ AttnLongF32Lds(int T, int HD) : HP(HD + 1), TP(T + 1) {
    q = lds_take(bytes, T * HP * 4); k = lds_take(bytes, T * HP * 4); v = lds_take(bytes, T * HP * 4); p = lds_take(bytes, T * TP * 4);
  }
};
// The backward kernels keep v / dO (and dV, which replaces v) in the INPUT dtype (esize 2: bf16 bits, 4: fp32), fp32 for everything else.
struct AttnBwdLds {          // attn_bwd_kernel<T2, MF>
  int HP = 0, HV = 0;        // row strides: HP fp32 tiles (padded: bank-conflict-free column walks), HV the v / dO tiles (bf16: 16-byte aligned rows, 4 banks of skew)
  int ntile = 0;             // 16 x 16 coefficient tiles, contiguous from p (zeroed in one loop)
  int q = 0, k = 0, qh = 0, kh = 0, p = 0, ds = 0, pdT = 0, dsT = 0, rq = 0, rk = 0, gq = 0, gk = 0, v = 0, dO = 0, bytes = 0;
  constexpr __host__ __device__ AttnBwdLds(int T, int HD, int esize, bool mf) : HP(HD + 1), HV(esize == 2 ? HD + 8 : HD + 1), ntile(mf ? 3 : 4) {
    const int row = T * HP * 4, tile = 256 * 4;
    q = lds_take(bytes, row); k = lds_take(bytes, row);       // raw q, k  [T][HP]
    qh = lds_take(bytes, row); kh = lds_take(bytes, row);     // q_hat / k_hat, later d q_hat / d k_hat
    // probability-sized tiles are zero-padded to 16 x 16 (row stride 16): branch-free 16-term dot products, float4 broadcast reads
    p = lds_take(bytes, tile);                                // P [query][key]   (16-byte aligned: four rows of 4-byte elements before it)
    ds = lds_take(bytes, tile);                               // dPd, then dS   [query][key]
    if (!mf) pdT = lds_take(bytes, tile);                     // dropped probabilities, transposed [key][query]   (VALU form only: the MFMA form keeps them in p)
    dsT = lds_take(bytes, tile);                              // dS transposed  [key][query]
    rq = lds_take(bytes, pad16(2 * T * 4)); rk = rq + T * 4;  // 1/norm per token: q [T], k [T], padded to 16 bytes
    gq = lds_take(bytes, HD * 4); gk = lds_take(bytes, HD * 4);   // qk-norm gains [HD] (read per element in three phases: from LDS, not through the vector cache)
    v = lds_take(bytes, T * HV * esize);                      // v, later dV   [T][HV]   (16-byte aligned: HD % 2 == 0)
    dO = lds_take(bytes, T * HV * esize);
  }
};
// The training shape (bf16, T = 14, head_dim 128, MFMA form) must stay under 40 KiB: four workgroups per CU, the whole grid of B*H = 1024 in one round.
static_assert(AttnBwdLds(14, 128, 2, true).bytes <= 40960, "attn_bwd_kernel: the training shape no longer fits four workgroups per CU");
struct AttnLongBwdLds {      // attn_long_bwd_kernel<T2>: P and dS as lower triangles so that T = 64, head_dim = 128 in fp32 fits one CU's LDS
  int HP = 0, HV = 0, ntri = 0;
  int qh = 0, kh = 0, p = 0, ds = 0, rq = 0, rk = 0, v = 0, dO = 0, bytes = 0;
  constexpr __host__ __device__ AttnLongBwdLds(int T, int HD, int esize) : HP(HD + 1), HV(esize == 2 ? HD + 8 : HD + 1), ntri(T * (T + 1) / 2) {
    qh = lds_take(bytes, T * HP * 4); kh = lds_take(bytes, T * HP * 4);   // q_hat, later d q_hat, later dq   [T][HP]
    p = lds_take(bytes, ntri * 4); ds = lds_take(bytes, ntri * 4);        // P, later Pd; dPd, later dS       [tri]
    rq = lds_take(bytes, T * 4); rk = lds_take(bytes, T * 4); // 1/norm per token
    bytes = pad16(bytes);
    v = lds_take(bytes, T * HV * esize);                      // v, later dV    [T][HV]   (16-byte aligned)
    dO = lds_take(bytes, T * HV * esize);
  }
};

// attention-dropout keep mask (SDPA dropout_p, modedit.py:149): element (problem, query, key) of stream `seed`
__device__ __forceinline__ bool attn_keep(uint32_t seed, int prob, int T, int q, int k, uint32_t thresh) {
  return hash_u32(hash_u32((uint32_t)((prob * T + q) * T + k) ^ seed) + 0x9e3779b9U) >= thresh;
}

// Operand sources: q / k / v (token row, first dim) -> the 8 bf16 at dims d0 .. d0+7 of that row of this (sample, head).
struct AttnGlobalSrc {
  const uint16_t* base;   // qkv + (b * T) * ld + h * HD
  long ld; int D;
  __device__ __forceinline__ uint4 q(int row, int d0) const { return *reinterpret_cast<const uint4*>(base + (long)row * ld + d0); }
  __device__ __forceinline__ uint4 k(int row, int d0) const { return *reinterpret_cast<const uint4*>(base + (long)row * ld + D + d0); }
  __device__ __forceinline__ uint4 v(int row, int d0) const { return *reinterpret_cast<const uint4*>(base + (long)row * ld + 2L * D + d0); }
};

// One wave64 = one (sample, head): T <= 16 tokens, 32*(NKS-1) < HD <= 32*NKS, HD % 16 == 0 (dims past HD are zero k-slots).  `prob` only feeds the
// dropout hash.  y0 = output row of token 0 of this sample at this head's first column, ldy its row stride (elements).
template <int NKS, class Src>
__device__ __forceinline__ void attn_wave_bf16(const Src& src, const float* __restrict__ qg, const float* __restrict__ kg, uint16_t* __restrict__ y0,
                                               long ldy, int T, int HD, float eps, uint32_t seed, uint32_t thresh, float inv_keep, int prob, int lane) {
  const int fr = lane & 15, fq = lane >> 4;
  const bool tv = fr < T;
  const int rrow = tv ? fr : 0;

  // ---- V rows first (requested before anything else: the global latency hides under QK^T / softmax): FOUR 16-byte loads per lane, keys
  // fq*4 + j, dims fr*8 .. fr*8+7.  Branch-free (clamped address + select): as predicated 2-byte loads this block compiled into 16 serial
  // branch + s_waitcnt vmcnt(0) pairs, 7.4 us of dependent round trips per launch whatever the batch.
  uint4 vr[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int key = fq * 4 + j;
    vr[j] = src.v(min(key, T - 1), min(fr * 8, HD - 8));   // masked where it is used
  }

  // ---- qk-norm gains: independent of everything else, fetched up front (their round trip used to follow the row-norm reduction)
  float4 gq4[NKS][2], gk4[NKS][2];
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) {
    const int dg = (ks * 32 + fq * 8 < HD) ? ks * 32 + fq * 8 : 0;      // padded k-slots carry zeros; any valid gain address works
    gq4[ks][0] = *reinterpret_cast<const float4*>(qg + dg); gq4[ks][1] = *reinterpret_cast<const float4*>(qg + dg + 4);
    gk4[ks][0] = *reinterpret_cast<const float4*>(kg + dg); gk4[ks][1] = *reinterpret_cast<const float4*>(kg + dg + 4);
  }

  // ---- load q / k fragments: token row fr, dims ks*32 + fq*8 + [0,8).  All loads of the kernel are requested here, ahead of any use; the
  // scheduling barrier keeps the compiler from sinking them to their use sites (it did: ~20 waits on partial results in a row)
  uint4 tq_[NKS], tk_[NKS];
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) {
    const int dq = (ks * 32 + fq * 8 < HD) ? ks * 32 : 0;     // clamped address + select below: no branch around the loads
    tq_[ks] = src.q(rrow, fq * 8 + dq); tk_[ks] = src.k(rrow, fq * 8 + dq);
  }
  // (an empty asm that "modifies" every loaded register: the loads cannot move below it, so the kernel has ONE wait for one round trip)
#define MODE_PIN4(v) asm volatile("" : "+v"((v).x), "+v"((v).y), "+v"((v).z), "+v"((v).w))
#pragma unroll
  for (int j = 0; j < 4; ++j) MODE_PIN4(vr[j]);
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) {
    MODE_PIN4(gq4[ks][0]); MODE_PIN4(gq4[ks][1]); MODE_PIN4(gk4[ks][0]); MODE_PIN4(gk4[ks][1]); MODE_PIN4(tq_[ks]); MODE_PIN4(tk_[ks]);
  }
#undef MODE_PIN4
  float qf[NKS][8], kf[NKS][8];
  float qss = 0.f, kss = 0.f;
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) {
    const bool okq = tv && ks * 32 + fq * 8 < HD;
    const uint4 rq = make_uint4(okq ? tq_[ks].x : 0u, okq ? tq_[ks].y : 0u, okq ? tq_[ks].z : 0u, okq ? tq_[ks].w : 0u);
    const uint4 rk = make_uint4(okq ? tk_[ks].x : 0u, okq ? tk_[ks].y : 0u, okq ? tk_[ks].z : 0u, okq ? tk_[ks].w : 0u);
    const uint32_t uq[4] = {rq.x, rq.y, rq.z, rq.w}, uk[4] = {rk.x, rk.y, rk.z, rk.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      qf[ks][2 * i] = bf16_bits_to_f32(uq[i] & 0xffff); qf[ks][2 * i + 1] = bf16_bits_to_f32(uq[i] >> 16);
      kf[ks][2 * i] = bf16_bits_to_f32(uk[i] & 0xffff); kf[ks][2 * i + 1] = bf16_bits_to_f32(uk[i] >> 16);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) { qss += qf[ks][i] * qf[ks][i]; kss += kf[ks][i] * kf[ks][i]; }
  }
  // row norm: the 4 lane groups (fq) of a token hold disjoint dims -> xor 16, 32
  qss += __shfl_xor(qss, 16, 64); qss += __shfl_xor(qss, 32, 64);
  kss += __shfl_xor(kss, 16, 64); kss += __shfl_xor(kss, 32, 64);
  const float qn = fmaxf(sqrtf(qss) * rsqrtf((float)HD), eps), kn = fmaxf(sqrtf(kss) * rsqrtf((float)HD), eps);
  const float rqn = __frcp_rn(qn), rkn = __frcp_rn(kn);      // one reciprocal per row (64 per-element fp32 divisions per lane were ~2 us of this kernel)

  bf16x8 qfrag[NKS], kfrag[NKS];
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) {
    const float4 g0 = gq4[ks][0], g1 = gq4[ks][1], h0 = gk4[ks][0], h1 = gk4[ks][1];
    const float gq[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w}, gk[8] = {h0.x, h0.y, h0.z, h0.w, h1.x, h1.y, h1.z, h1.w};
    uint32_t pq[4], pk[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      pq[i] = pack_bf16x2(qf[ks][2 * i] * rqn * gq[2 * i], qf[ks][2 * i + 1] * rqn * gq[2 * i + 1]);
      pk[i] = pack_bf16x2(kf[ks][2 * i] * rkn * gk[2 * i], kf[ks][2 * i + 1] * rkn * gk[2 * i + 1]);
    }
    uint4 tq = make_uint4(pq[0], pq[1], pq[2], pq[3]), tk = make_uint4(pk[0], pk[1], pk[2], pk[3]);
    qfrag[ks] = *reinterpret_cast<bf16x8*>(&tq);
    kfrag[ks] = *reinterpret_cast<bf16x8*>(&tk);
  }

  // ---- S^T[key][query] = sum_d K[key][d] Q[query][d]; lane: query = fr, keys = fq*4 + r
  f32x4 st = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) st = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kfrag[ks], qfrag[ks], st, 0, 0, 0);
  const float scale = rsqrtf((float)HD);
  float s[4], mx = -INFINITY;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int key = fq * 4 + r;
    s[r] = (key <= fr && key < T) ? st[r] * scale : -INFINITY;     // is_causal=True (modedit.py:149)
    mx = fmaxf(mx, s[r]);
  }
  mx = fmaxf(mx, __shfl_xor(mx, 16, 64)); mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
  float p[4], sum = 0.f;
#pragma unroll
  for (int r = 0; r < 4; ++r) { p[r] = (s[r] == -INFINITY) ? 0.f : __expf(s[r] - mx); sum += p[r]; }
  sum += __shfl_xor(sum, 16, 64); sum += __shfl_xor(sum, 32, 64);
  const float inv = 1.0f / sum;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    p[r] *= inv;
    if (thresh) p[r] = attn_keep(seed, prob, T, fr, fq * 4 + r, thresh) ? p[r] * inv_keep : 0.f;
  }
  uint4 tp = make_uint4(pack_bf16x2(p[0], p[1]), pack_bf16x2(p[2], p[3]), 0u, 0u);
  const bf16x8 pfrag = *reinterpret_cast<bf16x8*>(&tp);          // B operand: slots 0..3 = keys fq*4+r, slots 4..7 = 0

  // ---- O^T[row][query] = sum_key V[key][dim(row)] P[query][key].  MFMA i (0..7) takes as its 16 rows the dims fr*8 + i - element i of each
  // lane's four V vectors is its A operand (k-slots j < 4 = keys fq*4+j, slots 4..7 zero) - so that a lane ends up with 8 CONSECUTIVE dims
  // (fq*4+r)*8 .. +7 of its query per accumulator register r: four 16-byte stores.
  uint32_t vd[4][4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const bool okv = fq * 4 + j < T && fr * 8 < HD;               // keys past T / dims past head_dim (clamped loads above) are zero operands
    vd[j][0] = okv ? vr[j].x : 0u; vd[j][1] = okv ? vr[j].y : 0u; vd[j][2] = okv ? vr[j].z : 0u; vd[j][3] = okv ? vr[j].w : 0u;
  }
  float ov[4][8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int dw = i >> 1, sh = (i & 1) * 16;
    const uint32_t e0 = (vd[0][dw] >> sh) & 0xffffu, e1 = (vd[1][dw] >> sh) & 0xffffu, e2 = (vd[2][dw] >> sh) & 0xffffu, e3 = (vd[3][dw] >> sh) & 0xffffu;
    uint4 tvv = make_uint4(e0 | (e1 << 16), e2 | (e3 << 16), 0u, 0u);
    const bf16x8 vfrag = *reinterpret_cast<bf16x8*>(&tvv);
    f32x4 o = f32x4{0.f, 0.f, 0.f, 0.f};
    o = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vfrag, pfrag, o, 0, 0, 0);     // D[row = fq*4 + r][col = query fr]
#pragma unroll
    for (int r = 0; r < 4; ++r) ov[r][i] = o[r];
  }
  uint16_t* yrow = y0 + (long)fr * ldy;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int d0 = (fq * 4 + r) * 8;
    if (tv && d0 < HD)
      store_out16<StorePolicy::attn>(yrow + d0, out_u4{pack_bf16x2(ov[r][0], ov[r][1]), pack_bf16x2(ov[r][2], ov[r][3]),
                                                        pack_bf16x2(ov[r][4], ov[r][5]), pack_bf16x2(ov[r][6], ov[r][7])});
  }
}

// ---- backward: the phases that attn_bwd_kernel (attn.hip) and attn_long_bwd_kernel (attn_long.hip) share.  One 256-thread workgroup per (sample, head); T2 =
// uint16_t (bf16 bits) or float is the dtype of qkv / dY / dqkv, TV the type v / dO / dV have in LDS (see AttnBwdLds).  The S / dPd products, the softmax + dS
// pass and the three token-dimension products differ between the kernels and stay with them.
template <typename T2> using attn_tv_t = typename std::conditional<sizeof(T2) == 2, uint16_t, float>::type;
template <typename TV>
__device__ __forceinline__ float attn_tvf(TV x) { if constexpr (sizeof(TV) == 2) return bf16_bits_to_f32(x); else return x; }

// one 16-byte chunk <-> its 16 / sizeof(T2) fp32 values
template <typename T2>
__device__ __forceinline__ void attn_unpack16(const uint4& u, float* dst) {
  if constexpr (sizeof(T2) == 2) {
    const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) { dst[2 * j] = bf16_bits_to_f32(w[j] & 0xffff); dst[2 * j + 1] = bf16_bits_to_f32(w[j] >> 16); }
  } else {
    dst[0] = __uint_as_float(u.x); dst[1] = __uint_as_float(u.y); dst[2] = __uint_as_float(u.z); dst[3] = __uint_as_float(u.w);
  }
}
template <typename T2>
__device__ __forceinline__ uint4 attn_pack16(const float* src) {
  uint4 u;
  if constexpr (sizeof(T2) == 2) {
    u.x = pack_bf16x2(src[0], src[1]); u.y = pack_bf16x2(src[2], src[3]); u.z = pack_bf16x2(src[4], src[5]); u.w = pack_bf16x2(src[6], src[7]);
  } else {
    u.x = __float_as_uint(src[0]); u.y = __float_as_uint(src[1]); u.z = __float_as_uint(src[2]); u.w = __float_as_uint(src[3]);
  }
  return u;
}

// Stage q | k (fp32, row stride HP) and v | dO (TV, row stride HV) of this (sample, head) into LDS.  qkv0 / dy0: token 0 at this head's first column (row strides
// ld / D elements).  16-byte global loads, all four tensors of a thread's chunk requested before the first use (one memory round trip per workgroup - a per-
// element loop serialises T*HD/256 dependent round trips and was 80 % of the short kernel's time).
template <typename T2>
__device__ __forceinline__ void attn_bwd_stage(const T2* __restrict__ qkv0, const T2* __restrict__ dy0, long ld, int D, int T, int HD, float* sq, float* sk, int HP,
                                               attn_tv_t<T2>* sv, attn_tv_t<T2>* sdo, int HV, int tid) {
  constexpr int VE = 16 / (int)sizeof(T2);              // elements per 16-byte chunk
  const int cpr = HD / VE;                              // chunks per token row
  for (int i = tid; i < T * cpr; i += 256) {
    const int t = i / cpr, d = (i % cpr) * VE;
    const T2* r = qkv0 + (long)t * ld + d;
    const uint4 uq = *reinterpret_cast<const uint4*>(r), uk = *reinterpret_cast<const uint4*>(r + D), uv = *reinterpret_cast<const uint4*>(r + 2 * D);
    const uint4 ud = *reinterpret_cast<const uint4*>(dy0 + (long)t * D + d);
    float fq_[VE], fk_[VE];
    attn_unpack16<T2>(uq, fq_); attn_unpack16<T2>(uk, fk_);
#pragma unroll
    for (int j = 0; j < VE; ++j) { sq[t * HP + d + j] = fq_[j]; sk[t * HP + d + j] = fk_[j]; }
    if constexpr (sizeof(T2) == 2) {                    // bf16: the 16-byte chunks go to LDS as they are
      *reinterpret_cast<uint4*>(sv + t * HV + d) = uv; *reinterpret_cast<uint4*>(sdo + t * HV + d) = ud;
    } else {
      float fv_[VE], fd_[VE];
      attn_unpack16<T2>(uv, fv_); attn_unpack16<T2>(ud, fd_);
#pragma unroll
      for (int j = 0; j < VE; ++j) { sv[t * HV + d + j] = fv_[j]; sdo[t * HV + d + j] = fd_[j]; }
    }
  }
}

// 1 / max(||x|| * HD^-1/2, eps) from the row's sum of squares (the backward kernels' form; the fp32 forward kernels divide by the norm, which rounds differently)
__device__ __forceinline__ float attn_bwd_rnorm(float ss, int HD, float eps) { return 1.0f / fmaxf(sqrtf(ss) * rsqrtf((float)HD), eps); }

// Where the norm backward finds raw q / k element (t, d) and the gains gq / gk [HD]: the short kernel's LDS copies, or the long kernel's re-read of global
// memory (L2).
struct AttnRawLds {
  const float *sq, *sk, *gq, *gk; int HP;
  __device__ __forceinline__ float q(int t, int d) const { return sq[t * HP + d]; }
  __device__ __forceinline__ float k(int t, int d) const { return sk[t * HP + d]; }
};
template <typename T2>
struct AttnRawGlobal {
  const T2* qkv0; long ld; int D;                       // raw q of token t at qkv0 + t*ld, k at + D
  const float *gq, *gk;
  __device__ __forceinline__ float q(int t, int d) const { return attn_tvf(qkv0[(long)t * ld + d]); }
  __device__ __forceinline__ float k(int t, int d) const { return attn_tvf(qkv0[(long)t * ld + D + d]); }
};

// gain-gradient partials of this (sample, head): dgq / dgk = its rows [HD] of the partial buffers; sqh / skh hold d q_hat / d k_hat
template <class Raw>
__device__ __forceinline__ void attn_bwd_gain_partials(const Raw& raw, const float* sqh, const float* skh, int HP, const float* srq, const float* srk,
                                                       float* __restrict__ dgq, float* __restrict__ dgk, int T, int HD, int tid) {
  for (int d = tid; d < HD; d += 256) {
    float a = 0.f, c = 0.f;
    for (int t = 0; t < T; ++t) { a += sqh[t * HP + d] * raw.q(t, d) * srq[t]; c += skh[t * HP + d] * raw.k(t, d) * srk[t]; }
    dgq[d] = a; dgk[d] = c;
  }
}

// qk-RMSNorm backward of token t (x_hat = x * r * g): dx = g*dxh*r - x * <g*dxh, x> * r^3 / HD  (clamped rows: dx = g*dxh/eps); in place over d x_hat.
// 16 lanes (l16) per token with 4-step xor-shuffle reductions: every thread of the wave calls it, t >= T idles.
template <class Raw>
__device__ __forceinline__ void attn_bwd_norm_token(const Raw& raw, float* sqh, float* skh, int HP, const float* srq, const float* srk, int t, int l16, int T, int HD,
                                                    float eps) {
  float cq = 0.f, ck = 0.f;
  if (t < T) {
#pragma unroll 4
    for (int d = l16; d < HD; d += 16) { cq += raw.gq[d] * sqh[t * HP + d] * raw.q(t, d); ck += raw.gk[d] * skh[t * HP + d] * raw.k(t, d); }
  }
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) { cq += __shfl_xor(cq, o, 64); ck += __shfl_xor(ck, o, 64); }
  if (t < T) {
    const float rq = srq[t], rk = srk[t];
    const bool clq = rq >= 1.0f / eps, clk = rk >= 1.0f / eps;
    const float cqs = clq ? 0.f : cq * rq * rq * rq / (float)HD, cks = clk ? 0.f : ck * rk * rk * rk / (float)HD;   // per token, not per element (a division each)
#pragma unroll 4
    for (int d = l16; d < HD; d += 16) {
      sqh[t * HP + d] = raw.gq[d] * sqh[t * HP + d] * rq - raw.q(t, d) * cqs;
      skh[t * HP + d] = raw.gk[d] * skh[t * HP + d] * rk - raw.k(t, d) * cks;
    }
  }
}

// Write-out tail: dq | dk (fp32 in LDS, row stride HP) and dV (TV, row stride HV) -> dqkv0 (token 0 at this head's first column, row stride ld) in 16-byte stores.
// dbias0 (optional): this (sample, head)'s columns of the sample's share [3 D] of the packed QKV projection's bias gradient = column sums of dqkv over its T
// tokens, from the values AS STORED (bf16-rounded on the bf16 path, like a separate column sum over dqkv); the caller adds the B rows with one small column sum.
template <typename T2>
__device__ __forceinline__ void attn_bwd_write(const float* sdq, const float* sdk, int HP, const attn_tv_t<T2>* sdv, int HV, T2* __restrict__ dqkv0,
                                               float* __restrict__ dbias0, long ld, int D, int T, int HD, int tid) {
  constexpr int VE = 16 / (int)sizeof(T2);
  const int cpr = HD / VE;
  if (dbias0) {
    for (int c = tid; c < 3 * HD; c += 256) {
      const int which = c / HD, d = c - which * HD;
      float sacc = 0.f;
      for (int t = 0; t < T; ++t) {
        float v = which == 0 ? sdq[t * HP + d] : which == 1 ? sdk[t * HP + d] : attn_tvf(sdv[t * HV + d]);
        if constexpr (sizeof(T2) == 2) v = bf16_bits_to_f32(f32_to_bf16_bits(v));
        sacc += v;
      }
      dbias0[(long)which * D + d] = sacc;
    }
  }
  for (int i = tid; i < T * cpr; i += 256) {
    const int t = i / cpr, d = (i % cpr) * VE;
    T2* o = dqkv0 + (long)t * ld + d;
    *reinterpret_cast<uint4*>(o) = attn_pack16<T2>(sdq + t * HP + d);
    *reinterpret_cast<uint4*>(o + D) = attn_pack16<T2>(sdk + t * HP + d);
    if constexpr (sizeof(T2) == 2) *reinterpret_cast<uint4*>(o + 2 * D) = *reinterpret_cast<const uint4*>(sdv + t * HV + d);
    else *reinterpret_cast<uint4*>(o + 2 * D) = attn_pack16<T2>(reinterpret_cast<const float*>(sdv) + t * HV + d);
  }
}

}  // namespace mode
