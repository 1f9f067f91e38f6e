// Causal attention for 16 < T <= 64 tokens per sample (action chunks longer than the 14-token default): selected inside mode_attn_block_fwd /
// mode_attn_block_bwd / attn_block_bwd_launch when T > 16.  The tiny-T kernels (attn.hip, attn_core.h) stay as they are for T <= 16.  attn_core.h also
// holds the LDS layouts of this file's fp32 forward and backward and the backward phases this file shares with attn.hip (staging, gain partials, norm backward, write-out).
//
// bf16 forward: one workgroup per (sample, head), one wave per 16-query tile (ceil(T/16) waves).  Wave w normalises rows 16w .. 16w+15 of q and k
// exactly like attn_core.h's body (fragment loads, 4-lane-group shuffle reduction, one reciprocal per row), keeps its q_hat fragments in registers and
// publishes k_hat and raw v rows to LDS.  Then S^T = K Q^T on v_mfma_f32_16x16x32_bf16 for key tiles 0..w only (causal), an exact two-pass softmax over
// the <= 64 keys of a query (16 values per lane + two xor-shuffles), and O^T = V^T P^T with two key tiles per MFMA (k-slots 0..3 = tile 2m, 4..7 =
// tile 2m+1 of the lane group's 4 keys): each lane ends up with 8 consecutive head dims of its query per accumulator register -> 16-byte stores.
// fp32 parity forward and the backward (both dtypes): one 256-thread workgroup per (sample, head), everything staged in LDS, fp32 VALU math; the
// backward keeps P and dS as lower triangles so that T = 64, head_dim = 128 in fp32 fits one CU's LDS.
#include "mode_common.h"
#include "attn_core.h"

namespace mode {

constexpr int kLongTMax = kMaxTokens;

// ---------------------------------------------------------------------------------------------------------------- forward, bf16 (MFMA)
template <int NKS>   // 32*(NKS-1) < head_dim <= 32*NKS, head_dim % 16 == 0
__global__ __launch_bounds__(256) void attn_long_bf16_kernel(const uint16_t* __restrict__ qkv, const float* __restrict__ qg, const float* __restrict__ kg,
                                                             uint16_t* __restrict__ y, int T, int H, int HD, float eps, uint32_t seed, uint32_t thresh,
                                                             float inv_keep) {
  constexpr int KS = NKS * 32 + 8;                     // k_hat row stride (bf16): 16-byte rows, 4 banks of skew
  constexpr int VS = 128 + 8;                          // v row stride (bf16)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int nt = blockDim.x >> 6;                      // 16-token tiles
  uint16_t* sk = reinterpret_cast<uint16_t*>(smem);    // [nt*16][KS]
  uint16_t* sv = sk + nt * 16 * KS;                    // [nt*16][VS]
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  const int prob = blockIdx.x, b = prob / H, h = prob % H, D = H * HD;
  const long ld = 3L * D;
  const uint16_t* base = qkv + (long)b * T * ld + h * HD;
  const int row = w * 16 + fr;                         // this lane's q / k row (query of the S^T column it owns)
  const bool tv = row < T;
  const int rrow = tv ? row : T - 1;

  // v rows of this tile: keys 16w + fq*4 + j, dims fr*8 .. fr*8+7 (clamped address + select, as in attn_core.h)
  uint4 vr[4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
    vr[j] = *reinterpret_cast<const uint4*>(base + (long)min(w * 16 + fq * 4 + j, T - 1) * ld + 2L * D + min(fr * 8, HD - 8));
  float4 gq4[NKS][2], gk4[NKS][2];
  uint4 tq_[NKS], tk_[NKS];
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) {
    const int dg = (ks * 32 + fq * 8 < HD) ? ks * 32 + fq * 8 : 0;
    gq4[ks][0] = *reinterpret_cast<const float4*>(qg + dg); gq4[ks][1] = *reinterpret_cast<const float4*>(qg + dg + 4);
    gk4[ks][0] = *reinterpret_cast<const float4*>(kg + dg); gk4[ks][1] = *reinterpret_cast<const float4*>(kg + dg + 4);
    tq_[ks] = *reinterpret_cast<const uint4*>(base + (long)rrow * ld + dg);
    tk_[ks] = *reinterpret_cast<const uint4*>(base + (long)rrow * ld + D + dg);
  }
  // qk-RMSNorm on the fragments: a copy of attn_wave_bf16's (attn_core.h) arithmetic, rows past T and dims past head_dim zeros.  Kept as a copy on purpose:
  // sharing the body changed the register allocation of attn_bf16_kernel and of all qkv_attn_kernel instantiations
  float qf[NKS][8], kf[NKS][8];
  float qss = 0.f, kss = 0.f;
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) {
    const bool ok = tv && ks * 32 + fq * 8 < HD;
    const uint32_t uq[4] = {ok ? tq_[ks].x : 0u, ok ? tq_[ks].y : 0u, ok ? tq_[ks].z : 0u, ok ? tq_[ks].w : 0u};
    const uint32_t uk[4] = {ok ? tk_[ks].x : 0u, ok ? tk_[ks].y : 0u, ok ? tk_[ks].z : 0u, ok ? tk_[ks].w : 0u};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      qf[ks][2 * i] = bf16_bits_to_f32(uq[i] & 0xffff); qf[ks][2 * i + 1] = bf16_bits_to_f32(uq[i] >> 16);
      kf[ks][2 * i] = bf16_bits_to_f32(uk[i] & 0xffff); kf[ks][2 * i + 1] = bf16_bits_to_f32(uk[i] >> 16);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) { qss += qf[ks][i] * qf[ks][i]; kss += kf[ks][i] * kf[ks][i]; }
  }
  qss += __shfl_xor(qss, 16, 64); qss += __shfl_xor(qss, 32, 64);
  kss += __shfl_xor(kss, 16, 64); kss += __shfl_xor(kss, 32, 64);
  const float rqn = __frcp_rn(fmaxf(sqrtf(qss) * rsqrtf((float)HD), eps)), rkn = __frcp_rn(fmaxf(sqrtf(kss) * rsqrtf((float)HD), eps));
  bf16x8 qfrag[NKS];
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
    uint4 tq = make_uint4(pq[0], pq[1], pq[2], pq[3]);
    qfrag[ks] = *reinterpret_cast<bf16x8*>(&tq);
    *reinterpret_cast<uint4*>(sk + row * KS + ks * 32 + fq * 8) = make_uint4(pk[0], pk[1], pk[2], pk[3]);
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const bool okv = w * 16 + fq * 4 + j < T && fr * 8 < HD;
    *reinterpret_cast<uint4*>(sv + (w * 16 + fq * 4 + j) * VS + fr * 8) = okv ? vr[j] : make_uint4(0u, 0u, 0u, 0u);
  }
  __syncthreads();

  // S^T[key][query] for key tiles kt <= w; lane: query 16w + fr, keys 16kt + fq*4 + r
  const float scale = rsqrtf((float)HD);
  float p[4][4], mx = -INFINITY;
#pragma unroll
  for (int kt = 0; kt < 4; ++kt) {
    f32x4 st = f32x4{0.f, 0.f, 0.f, 0.f};
    if (kt <= w) {
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks) {
        const uint4 kk = *reinterpret_cast<const uint4*>(sk + (kt * 16 + fr) * KS + ks * 32 + fq * 8);
        st = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8*>(&kk), qfrag[ks], st, 0, 0, 0);
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int key = kt * 16 + fq * 4 + r;
      p[kt][r] = (kt <= w && key <= row && key < T) ? st[r] * scale : -INFINITY;     // is_causal=True
      mx = fmaxf(mx, p[kt][r]);
    }
  }
  mx = fmaxf(mx, __shfl_xor(mx, 16, 64)); mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
  float sum = 0.f;
#pragma unroll
  for (int kt = 0; kt < 4; ++kt)
#pragma unroll
    for (int r = 0; r < 4; ++r) { p[kt][r] = (p[kt][r] == -INFINITY) ? 0.f : __expf(p[kt][r] - mx); sum += p[kt][r]; }
  sum += __shfl_xor(sum, 16, 64); sum += __shfl_xor(sum, 32, 64);
  const float inv = 1.0f / sum;
#pragma unroll
  for (int kt = 0; kt < 4; ++kt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      p[kt][r] *= inv;
      if (thresh) p[kt][r] = attn_keep(seed, prob, T, row, kt * 16 + fq * 4 + r, thresh) ? p[kt][r] * inv_keep : 0.f;
    }

  // O^T[dim][query] = sum_key V[key][dim] P[query][key]: MFMA i takes the dims fr*8 + i as its rows (attn_core.h's layout), two key tiles per MFMA
  f32x4 o[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) o[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    if (2 * m > w) continue;
    const bool hi = 2 * m + 1 <= w;
    uint4 tp = make_uint4(pack_bf16x2(p[2 * m][0], p[2 * m][1]), pack_bf16x2(p[2 * m][2], p[2 * m][3]),
                          pack_bf16x2(p[2 * m + 1][0], p[2 * m + 1][1]), pack_bf16x2(p[2 * m + 1][2], p[2 * m + 1][3]));
    const bf16x8 pfrag = *reinterpret_cast<bf16x8*>(&tp);
    uint32_t vl[4][4], vh[4][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint4 a = *reinterpret_cast<const uint4*>(sv + (32 * m + fq * 4 + j) * VS + fr * 8);
      const uint4 c = hi ? *reinterpret_cast<const uint4*>(sv + (32 * m + 16 + fq * 4 + j) * VS + fr * 8) : make_uint4(0u, 0u, 0u, 0u);
      vl[j][0] = a.x; vl[j][1] = a.y; vl[j][2] = a.z; vl[j][3] = a.w;
      vh[j][0] = c.x; vh[j][1] = c.y; vh[j][2] = c.z; vh[j][3] = c.w;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int dw = i >> 1, sh = (i & 1) * 16;
      auto e = [&](const uint32_t (&v)[4][4], int j) { return (v[j][dw] >> sh) & 0xffffu; };
      uint4 tvv = make_uint4(e(vl, 0) | (e(vl, 1) << 16), e(vl, 2) | (e(vl, 3) << 16), e(vh, 0) | (e(vh, 1) << 16), e(vh, 2) | (e(vh, 3) << 16));
      o[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8*>(&tvv), pfrag, o[i], 0, 0, 0);   // D[dim row fq*4+r][query fr]
    }
  }
  uint16_t* yrow = y + ((long)b * T + row) * D + h * HD;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int d0 = (fq * 4 + r) * 8;
    if (tv && d0 < HD)
      *reinterpret_cast<uint4*>(yrow + d0) = make_uint4(pack_bf16x2(o[0][r], o[1][r]), pack_bf16x2(o[2][r], o[3][r]),
                                                        pack_bf16x2(o[4][r], o[5][r]), pack_bf16x2(o[6][r], o[7][r]));
  }
}

// ---------------------------------------------------------------------------------------------------------------- forward, fp32 parity
// Plain VALU in the reference's order (norm, q k^T * scale, masked softmax, P V); 256 threads, one wave per softmax row (lane = key, T <= 64).
__global__ __launch_bounds__(256) void attn_long_f32_kernel(const float* __restrict__ qkv, const float* __restrict__ qg, const float* __restrict__ kg,
                                                            float* __restrict__ y, int T, int H, int HD, float eps, uint32_t seed, uint32_t thresh,
                                                            float inv_keep) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const AttnLongF32Lds L(T, HD);
  const int HP = L.HP, TP = L.TP;
  float *sq = lds_at<float>(smem, L.q), *sk = lds_at<float>(smem, L.k), *sv = lds_at<float>(smem, L.v), *sp = lds_at<float>(smem, L.p);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int prob = blockIdx.x, b = prob / H, h = prob % H, D = H * HD;
  const long ld = 3L * D;
  for (int i = tid; i < T * HD; i += 256) {
    const int t = i / HD, d = i % HD;
    const float* r = qkv + ((long)b * T + t) * ld + h * HD + d;
    sq[t * HP + d] = r[0]; sk[t * HP + d] = r[D]; sv[t * HP + d] = r[2 * D];
  }
  __syncthreads();
  for (int t = wave; t < T; t += 4) {                  // qk-RMSNorm
    float a = 0.f, c = 0.f;
    for (int d = lane; d < HD; d += 64) { a += sq[t * HP + d] * sq[t * HP + d]; c += sk[t * HP + d] * sk[t * HP + d]; }
    a = wave_sum(a); c = wave_sum(c);
    const float qn = fmaxf(sqrtf(a) * rsqrtf((float)HD), eps), kn = fmaxf(sqrtf(c) * rsqrtf((float)HD), eps);
    for (int d = lane; d < HD; d += 64) { sq[t * HP + d] = sq[t * HP + d] / qn * qg[d]; sk[t * HP + d] = sk[t * HP + d] / kn * kg[d]; }
  }
  __syncthreads();
  const float scale = rsqrtf((float)HD);
  for (int i = tid; i < T * T; i += 256) {
    const int qi = i / T, ki = i % T;
    if (ki > qi) continue;
    float a = 0.f;
    for (int d = 0; d < HD; ++d) a = fmaf(sq[qi * HP + d], sk[ki * HP + d], a);
    sp[qi * TP + ki] = a * scale;
  }
  __syncthreads();
  for (int qi = wave; qi < T; qi += 4) {
    const bool valid = lane <= qi;
    const float s = valid ? sp[qi * TP + lane] : -INFINITY;
    const float mx = wave_max(s);
    const float e = valid ? expf(s - mx) : 0.f;
    const float sum = wave_sum(e);
    float pv = e / sum;
    if (thresh && valid) pv = attn_keep(seed, prob, T, qi, lane, thresh) ? pv * inv_keep : 0.f;
    if (lane < T) sp[qi * TP + lane] = pv;
  }
  __syncthreads();
  for (int i = tid; i < T * HD; i += 256) {
    const int qi = i / HD, d = i % HD;
    float a = 0.f;
    for (int ki = 0; ki <= qi; ++ki) a = fmaf(sp[qi * TP + ki], sv[ki * HP + d], a);
    y[((long)b * T + qi) * D + h * HD + d] = a;
  }
}

// ---------------------------------------------------------------------------------------------------------------- backward (both dtypes)
// dY [B*T, D] -> dqkv [B*T, 3D], gain partials dgq/dgk [B*H, HD], optional per-sample QKV bias partial [B][3D].  Same math as attn.hip's backward:
//   P = softmax(q_hat k_hat^T * scale) (causal), Pd = P * keep / (1-p);  dV = Pd^T dO;  dP = (dO V^T) * keep / (1-p);  dS = P (dP - rowsum(dP P)) * scale;
//   dq_hat = dS k_hat;  dk_hat = dS^T q_hat;  then the qk-RMSNorm backward.  Raw q / k are re-read from global memory (L2) where the norm backward needs them.
__device__ __forceinline__ int tri_idx(int i, int j) { return i * (i + 1) / 2 + j; }   // lower triangle, j <= i

template <typename T2>
__global__ __launch_bounds__(256) void attn_long_bwd_kernel(const T2* __restrict__ qkv, const float* __restrict__ qg, const float* __restrict__ kg,
                                                            const T2* __restrict__ dY, T2* __restrict__ dqkv, float* __restrict__ dgq_part,
                                                            float* __restrict__ dgk_part, int T, int H, int HD, float eps, uint32_t seed, uint32_t thresh,
                                                            float inv_keep, float* __restrict__ dbias_part) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  typedef attn_tv_t<T2> TV;
  constexpr int MAXE = kLongTMax * 128 / 256;           // outputs per thread and tensor at T = 64, head_dim = 128
  const AttnLongBwdLds L(T, HD, sizeof(T2));
  const int HP = L.HP, HV = L.HV, NTRI = L.ntri;
  float *sqh = lds_at<float>(smem, L.qh), *skh = lds_at<float>(smem, L.kh), *sP = lds_at<float>(smem, L.p), *sdS = lds_at<float>(smem, L.ds);
  float *srq = lds_at<float>(smem, L.rq), *srk = lds_at<float>(smem, L.rk);
  TV *sv = lds_at<TV>(smem, L.v), *sdo = lds_at<TV>(smem, L.dO);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int prob = blockIdx.x, b = prob / H, h = prob % H, D = H * HD;
  const long ld = 3L * D;
  const T2* qrow0 = qkv + (long)b * T * ld + h * HD;    // raw q of token t at qrow0 + t*ld, k at + D, v at + 2D
  attn_bwd_stage<T2>(qrow0, dY + (long)b * T * D + h * HD, ld, D, T, HD, sqh, skh, HP, sv, sdo, HV, tid);   // raw q / k where q_hat / k_hat replace them
  __syncthreads();
  for (int t = wave; t < T; t += 4) {                   // row norms, then q_hat / k_hat in place
    float a = 0.f, c = 0.f;
    for (int d = lane; d < HD; d += 64) { a += sqh[t * HP + d] * sqh[t * HP + d]; c += skh[t * HP + d] * skh[t * HP + d]; }
    a = wave_sum(a); c = wave_sum(c);
    const float rq = attn_bwd_rnorm(a, HD, eps), rk = attn_bwd_rnorm(c, HD, eps);
    if (lane == 0) { srq[t] = rq; srk[t] = rk; }
    for (int d = lane; d < HD; d += 64) { sqh[t * HP + d] = sqh[t * HP + d] * rq * qg[d]; skh[t * HP + d] = skh[t * HP + d] * rk * kg[d]; }
  }
  __syncthreads();
  const float scale = rsqrtf((float)HD);
  for (int i = tid; i < NTRI; i += 256) {               // S = q_hat k_hat^T * scale and dPd = dO V^T on the lower triangle
    int qi = (int)((sqrtf(8.0f * (float)i + 1.0f) - 1.0f) * 0.5f);
    while (tri_idx(qi, 0) > i) --qi;
    while (tri_idx(qi + 1, 0) <= i) ++qi;
    const int ki = i - tri_idx(qi, 0);
    float s = 0.f, dp = 0.f;
    for (int d = 0; d < HD; ++d) {
      s = fmaf(sqh[qi * HP + d], skh[ki * HP + d], s);
      dp = fmaf(attn_tvf(sdo[qi * HV + d]), attn_tvf(sv[ki * HV + d]), dp);
    }
    sP[i] = s * scale; sdS[i] = dp;
  }
  __syncthreads();
  for (int qi = wave; qi < T; qi += 4) {                // softmax rows, dropout, dS: one wave per query, lane = key
    const bool valid = lane <= qi;
    const int ti = tri_idx(qi, valid ? lane : 0);
    const float s = valid ? sP[ti] : -INFINITY;
    const float mx = wave_max(s);
    const float e = valid ? expf(s - mx) : 0.f;
    const float sum = wave_sum(e);
    const float pv = valid ? e / sum : 0.f;
    float m = 1.0f;
    if (thresh && valid) m = attn_keep(seed, prob, T, qi, lane, thresh) ? inv_keep : 0.f;
    const float dP = valid ? sdS[ti] * m : 0.f;
    const float rs = wave_sum(dP * pv);
    const float dS = pv * (dP - rs) * scale;
    if (valid) { sP[ti] = pv * m; sdS[ti] = dS; }
  }
  __syncthreads();
  // dq_hat[t][d] = sum_{j<=t} dS[t][j] k_hat[j][d];  dk_hat[t][d] = sum_{i>=t} dS[i][t] q_hat[i][d];  dV[t][d] = sum_{i>=t} Pd[i][t] dO[i][d]
  {
    // dV needs no v: it replaces v at once; dq_hat / dk_hat read each other's inputs, so they wait in registers for the barrier
    float aq[MAXE], ak[MAXE];
#pragma unroll
    for (int u = 0; u < MAXE; ++u) {
      aq[u] = 0.f; ak[u] = 0.f;
      const int e = tid + 256 * u;
      if (e < T * HD) {
        const int t = e / HD, d = e % HD;
        float a = 0.f;
        for (int j = 0; j <= t; ++j) a = fmaf(sdS[tri_idx(t, j)], skh[j * HP + d], a);
        float c = 0.f, v = 0.f;
        for (int i = t; i < T; ++i) {
          const int ti = tri_idx(i, t);
          c = fmaf(sdS[ti], sqh[i * HP + d], c);
          v = fmaf(sP[ti], attn_tvf(sdo[i * HV + d]), v);
        }
        aq[u] = a; ak[u] = c;
        if constexpr (sizeof(TV) == 2) sv[t * HV + d] = f32_to_bf16_bits(v); else sv[t * HV + d] = v;
      }
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < MAXE; ++u) {
      const int e = tid + 256 * u;
      if (e < T * HD) {
        const int t = e / HD, d = e % HD;
        sqh[t * HP + d] = aq[u]; skh[t * HP + d] = ak[u];
      }
    }
  }
  __syncthreads();
  const AttnRawGlobal<T2> raw{qrow0, ld, D, qg, kg};
  attn_bwd_gain_partials(raw, sqh, skh, HP, srq, srk, dgq_part + (long)prob * HD, dgk_part + (long)prob * HD, T, HD, tid);
  __syncthreads();
  for (int t0 = 0; t0 < T; t0 += 16) attn_bwd_norm_token(raw, sqh, skh, HP, srq, srk, t0 + (tid >> 4), tid & 15, T, HD, eps);   // 16 tokens per pass
  __syncthreads();
  attn_bwd_write<T2>(sqh, skh, HP, sv, HV, dqkv + (long)b * T * ld + h * HD, dbias_part ? dbias_part + (long)b * 3 * D + h * HD : nullptr, ld, D, T, HD, tid);
}

// ---------------------------------------------------------------------------------------------------------------- host
constexpr int kLdsMax = 160 * 1024;

static LdsLimitOnce g_lds_f32_fwd, g_lds_bwd_bf16, g_lds_bwd_f32;   // one per kernel instantiation
static int ensure_lds(const void* kern, size_t bytes, LdsLimitOnce& once) {
  return bytes <= 64 * 1024 ? MODE_OK : once.ensure(kern, kLdsMax);
}

int attn_long_fwd_launch(const void* qkv, const float* qg, const float* kg, void* y, int dtype, int B, int T, int H, int HD, float eps, uint32_t seed,
                         uint32_t thresh, float inv_keep, hipStream_t s) {
  if (T > kLongTMax || HD <= 0 || HD > 128) return MODE_ERR_UNSUPPORTED;
  const dim3 grid(B * H);
  if (dtype == MODE_BF16) {
    if (HD % 16) return MODE_ERR_UNSUPPORTED;
    const int nt = (T + 15) / 16;
    const uint16_t* in = (const uint16_t*)qkv; uint16_t* out = (uint16_t*)y;
    // attn_long_bf16_kernel<NK>'s carve-up (kept by hand: see the LDS layouts in attn_core.h)
#define MODE_ALF(NK) \
  hipLaunchKernelGGL(attn_long_bf16_kernel<NK>, grid, dim3(64 * nt), (size_t)nt * 16 * ((NK * 32 + 8) + (128 + 8)) * 2, s, in, qg, kg, out, T, H, HD, eps, seed, thresh, inv_keep)
    MODE_ATTN_NKS_DISPATCH(HD, MODE_ALF)
#undef MODE_ALF
  } else {
    const size_t lds = AttnLongF32Lds(T, HD).bytes;
    int rc = ensure_lds(reinterpret_cast<const void*>(attn_long_f32_kernel), lds, g_lds_f32_fwd);
    if (rc) return rc;
    hipLaunchKernelGGL(attn_long_f32_kernel, grid, dim3(256), lds, s, (const float*)qkv, qg, kg, (float*)y, T, H, HD, eps, seed, thresh, inv_keep);
  }
  MODE_LAUNCH_CHECK();
  return MODE_OK;
}

int attn_long_bwd_launch(const void* qkv, const float* qg, const float* kg, const void* dy, void* dqkv, float* dgq_partial, float* dgk_partial, int dtype,
                         int B, int T, int H, int HD, float eps, uint32_t seed, uint32_t thresh, float inv_keep, float* dbias_partial, hipStream_t s) {
  if (T > kLongTMax || HD <= 0 || HD > 128 || HD % (dtype == MODE_BF16 ? 8 : 4)) return MODE_ERR_UNSUPPORTED;
  const size_t lds = AttnLongBwdLds(T, HD, dtype == MODE_BF16 ? 2 : 4).bytes;   // at most 149,248 bytes (fp32, T = 64, head_dim 128)
  if (lds > (size_t)kLdsMax) return MODE_ERR_UNSUPPORTED;
  int rc;
#define MODE_ALB(T2, ONCE)                                                                                                                                  \
  do {                                                                                                                                                   \
    if ((rc = ensure_lds(reinterpret_cast<const void*>(attn_long_bwd_kernel<T2>), lds, ONCE))) return rc;                                                                                     \
    hipLaunchKernelGGL(attn_long_bwd_kernel<T2>, dim3(B * H), dim3(256), lds, s, (const T2*)qkv, qg, kg, (const T2*)dy, (T2*)dqkv, dgq_partial,         \
                       dgk_partial, T, H, HD, eps, seed, thresh, inv_keep, dbias_partial);                                                               \
  } while (0)
  if (dtype == MODE_BF16) MODE_ALB(uint16_t, g_lds_bwd_bf16); else MODE_ALB(float, g_lds_bwd_f32);
#undef MODE_ALB
  MODE_LAUNCH_CHECK();
  return MODE_OK;
}

}  // namespace mode
