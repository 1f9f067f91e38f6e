// Tiny-T causal attention for the 14-token MoDE sequence (modedit.py:125-127, 145-165): B*H independent problems of
// T <= 16 tokens, head_dim 32..128.  One wave64 per (sample, head), four per workgroup, no LDS at all:
//   * q/k rows are read straight into MFMA fragments (16 B per lane), qk-RMSNorm is a 4-lane-group shuffle reduction on those
//     fragments, S^T = K Q^T runs on v_mfma_f32_16x16x32_bf16 (T padded to 16) so that each lane ends up owning one
//     QUERY column and 4 key rows: the causal softmax is 4 local values + two xor-shuffles,
//   * the probabilities are already laid out as the B operand of  O^T = V^T P^T  (k-slots 4..7 of each lane group are zero
//     padding), so P never moves between lanes; each lane then owns 4 consecutive head-dim outputs of one query -> 8-byte stores.
// fp32 parity mode: a plain VALU kernel with the same math (one wave per (sample, head), LDS-staged q/k/v).
// Backward (training, both dtypes): attn_bwd_kernel below, one 256-thread workgroup per (sample, head), in an MFMA and a VALU form of its matrix products.
// Both entry points hand T > 16 to attn_long.hip.  attn_core.h holds the bf16 forward's wave body (shared with qkv_attn.hip), the LDS layouts of the backward kernels and
// the backward phases shared with attn_long.hip (staging, gain partials, norm backward, write-out).
#include "mode_common.h"
#include "attn_core.h"

namespace mode {

template <int NKS>   // 32*(NKS-1) < head_dim <= 32*NKS, head_dim % 16 == 0 (dims past head_dim are zero k-slots)
__global__ __launch_bounds__(256) void attn_bf16_kernel(const uint16_t* __restrict__ qkv, const float* __restrict__ qg,
                                                        const float* __restrict__ kg, uint16_t* __restrict__ y, int B, int T,
                                                        int H, int HD, float eps, uint32_t seed, uint32_t thresh, float inv_keep) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int prob = blockIdx.x * 4 + wave;
  if (prob >= B * H) return;
  const int b = prob / H, h = prob % H;
  const int D = H * HD;
  const long ld = 3L * D;
  const AttnGlobalSrc src{qkv + (long)b * T * ld + h * HD, ld, D};
  attn_wave_bf16<NKS>(src, qg, kg, y + (long)b * T * D + h * HD, D, T, HD, eps, seed, thresh, inv_keep, prob, lane);   // attn_core.h
}

// fp32 parity kernel: one wave per (b,h); q,k,v rows staged in LDS; plain VALU math in the reference's order.
__global__ __launch_bounds__(64) void attn_f32_kernel(const float* __restrict__ qkv, const float* __restrict__ qg,
                                                      const float* __restrict__ kg, float* __restrict__ y, int B, int T, int H,
                                                      int HD, float eps, uint32_t seed, uint32_t thresh, float inv_keep) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* sq = reinterpret_cast<float*>(smem);          // [T][HD]
  float* sk = sq + T * HD;
  float* sv = sk + T * HD;
  float* sp = sv + T * HD;                             // [T][T]
  const int lane = threadIdx.x, b = blockIdx.x / H, h = blockIdx.x % H, D = H * HD;
  const long ld = 3L * D;
  for (int i = lane; i < T * HD; i += 64) {
    const int t = i / HD, d = i % HD;
    const float* r = qkv + ((long)b * T + t) * ld + h * HD + d;
    sq[i] = r[0]; sk[i] = r[D]; sv[i] = r[2 * D];
  }
  __syncthreads();
  for (int t = 0; t < T; ++t) {                        // qk-RMSNorm (modedit.py:126-127, 145-146)
    float a = 0.f, c = 0.f;
    for (int d = lane; d < HD; d += 64) { a += sq[t * HD + d] * sq[t * HD + d]; c += sk[t * HD + d] * sk[t * HD + d]; }
    a = wave_sum(a); c = wave_sum(c);
    const float qn = fmaxf(sqrtf(a) * rsqrtf((float)HD), eps), kn = fmaxf(sqrtf(c) * rsqrtf((float)HD), eps);
    for (int d = lane; d < HD; d += 64) { sq[t * HD + d] = sq[t * HD + d] / qn * qg[d]; sk[t * HD + d] = sk[t * HD + d] / kn * kg[d]; }
  }
  __syncthreads();
  const float scale = rsqrtf((float)HD);
  for (int i = lane; i < T * T; i += 64) {
    const int qi = i / T, ki = i % T;
    float a = -INFINITY;
    if (ki <= qi) {
      a = 0.f;
      for (int d = 0; d < HD; ++d) a = fmaf(sq[qi * HD + d], sk[ki * HD + d], a);
      a *= scale;
    }
    sp[i] = a;
  }
  __syncthreads();
  if (lane < T) {
    float mx = -INFINITY;
    for (int ki = 0; ki <= lane; ++ki) mx = fmaxf(mx, sp[lane * T + ki]);
    float sum = 0.f;
    for (int ki = 0; ki < T; ++ki) { const float e = (ki <= lane) ? expf(sp[lane * T + ki] - mx) : 0.f; sp[lane * T + ki] = e; sum += e; }
    for (int ki = 0; ki < T; ++ki) {
      float pv = sp[lane * T + ki] / sum;
      if (thresh) pv = attn_keep(seed, blockIdx.x, T, lane, ki, thresh) ? pv * inv_keep : 0.f;
      sp[lane * T + ki] = pv;
    }
  }
  __syncthreads();
  for (int i = lane; i < T * HD; i += 64) {
    const int qi = i / HD, d = i % HD;
    float a = 0.f;
    for (int ki = 0; ki <= qi; ++ki) a = fmaf(sp[qi * T + ki], sv[ki * HD + d], a);
    y[((long)b * T + qi) * D + h * HD + d] = a;
  }
}

// ---- backward (training): one 256-thread workgroup per (sample, head), everything in LDS, fp32 VALU in the forward's order.
// dY [B*T, D] (T2 = bf16/f32) -> dqkv [B*T, 3D]; per-workgroup partial gradients of the qk-norm gains: dgq/dgk [B*H, HD].
// MF: the five small matrix products (S = q_hat k_hat^T and dPd = dO V^T over the head dim; dq_hat = dS k_hat, dk_hat = dS^T q_hat, dV = Pd^T dO over the tokens) on
// v_mfma_f32_16x16x4_f32 - exact fp32 like the VALU form, but an operand element is read from LDS once per 16 outputs: the VALU form moved ~0.8 MB of LDS
// reads per (sample, head) - with four workgroups per CU these two phases were LDS-bandwidth-bound and two thirds of the kernel's 38 us.  head_dim % 16 == 0.
template <typename T2, bool MF>
__global__ __launch_bounds__(256, 4) void attn_bwd_kernel(const T2* __restrict__ qkv, const float* __restrict__ qg, const float* __restrict__ kg,
                                                       const T2* __restrict__ dY, T2* __restrict__ dqkv, float* __restrict__ dgq_part,
                                                       float* __restrict__ dgk_part, int B, int T, int H, int HD, float eps, uint32_t seed,
                                                       uint32_t thresh, float inv_keep, float* __restrict__ dbias_part) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // v / dO (and dV, which replaces v) in the INPUT dtype: for bf16 that is exact (the inputs are bf16, dV is rounded to bf16 on its way out anyway) and
  // brings the workgroup under 40 KB of LDS (attn_core.h: AttnBwdLds)
  typedef attn_tv_t<T2> TV;
  const AttnBwdLds L(T, HD, sizeof(T2), MF);
  const int HP = L.HP, HV = L.HV;
  float *sq = lds_at<float>(smem, L.q), *sk = lds_at<float>(smem, L.k), *sqh = lds_at<float>(smem, L.qh), *skh = lds_at<float>(smem, L.kh);
  float *sp = lds_at<float>(smem, L.p), *sds = lds_at<float>(smem, L.ds), *spdT = lds_at<float>(smem, L.pdT), *sdsT = lds_at<float>(smem, L.dsT);
  float *srq = lds_at<float>(smem, L.rq), *srk = lds_at<float>(smem, L.rk), *sgq = lds_at<float>(smem, L.gq), *sgk = lds_at<float>(smem, L.gk);
  TV *sv = lds_at<TV>(smem, L.v), *sdo = lds_at<TV>(smem, L.dO);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int prob = blockIdx.x, b = prob / H, h = prob % H, D = H * HD;
  const long ld = 3L * D;
  for (int i = tid; i < L.ntile * 256; i += 256) sp[i] = 0.f;   // zero padding of the 16x16 tiles (written sparsely below)
  for (int d = tid; d < HD; d += 256) { sgq[d] = qg[d]; sgk[d] = kg[d]; }
  attn_bwd_stage<T2>(qkv + (long)b * T * ld + h * HD, dY + (long)b * T * D + h * HD, ld, D, T, HD, sq, sk, HP, sv, sdo, HV, tid);
  __syncthreads();
  for (int t = wave; t < T; t += 4) {                  // one wave per token: row norms
    float a = 0.f, c = 0.f;
    for (int d = lane; d < HD; d += 64) { a += sq[t * HP + d] * sq[t * HP + d]; c += sk[t * HP + d] * sk[t * HP + d]; }
    a = wave_sum(a); c = wave_sum(c);
    if (lane == 0) { srq[t] = attn_bwd_rnorm(a, HD, eps); srk[t] = attn_bwd_rnorm(c, HD, eps); }
  }
  __syncthreads();
  for (int i = tid; i < T * HD; i += 256) {
    const int t = i / HD, d = i % HD;
    sqh[t * HP + d] = sq[t * HP + d] * srq[t] * sgq[d];
    skh[t * HP + d] = sk[t * HP + d] * srk[t] * sgk[d];
  }
  __syncthreads();
  const float scale = rsqrtf((float)HD);
  if constexpr (MF) {
    // wave 0: S = q_hat k_hat^T * scale, wave 1: dPd = dO V^T - D[i][j] += A[i][d] B[d][j], four head dims per instruction; a lane supplies A[i = l & 15][d0 + (l >> 4)]
    // and B[..][j = l & 15] and ends up with rows i = 4 (l >> 4) + r of column j.  Rows / columns >= T read a clamped (finite) row: their outputs are not stored.
    if (wave < 2) {
      const int fr = min(lane & 15, T - 1), fq = lane >> 4;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      if (wave == 0) {
        const float* qa = sqh + fr * HP + fq; const float* kb = skh + fr * HP + fq;
        for (int d0 = 0; d0 < HD; d0 += 16) {
          float a[4], bv[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) { a[u] = qa[d0 + 4 * u]; bv[u] = kb[d0 + 4 * u]; }
#pragma unroll
          for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u], bv[u], acc, 0, 0, 0);
        }
      } else {
        const TV* oa = sdo + fr * HV + fq; const TV* vb = sv + fr * HV + fq;
        for (int d0 = 0; d0 < HD; d0 += 16) {
          float a[4], bv[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) { a[u] = attn_tvf(oa[d0 + 4 * u]); bv[u] = attn_tvf(vb[d0 + 4 * u]); }
#pragma unroll
          for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u], bv[u], acc, 0, 0, 0);
        }
      }
      const int ki = lane & 15;
      float* dst = wave == 0 ? sp : sds;
      const float mul = wave == 0 ? scale : 1.0f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int qi = 4 * (lane >> 4) + r;
        if (qi < T && ki <= qi) dst[qi * 16 + ki] = acc[r] * mul;
      }
    }
  } else
  // S = q_hat k_hat^T * scale (causal) and dPd = dO V^T: four lanes per (query, key) pair, each a quarter of the head dim with two
  // independent accumulator pairs (the one-thread-per-pair loop was a 128-deep chain of dependent LDS reads), xor-shuffle combine
  {
    // thread = (query qi, group of 4 keys, quarter of the head dim): the q / dO values are loaded once per 4 keys (10 LDS reads per 8 FMAs),
    // 14 x 4 x 4 = 224 threads cover the whole [T][T] tile in one pass; quarter sums are combined by xor-shuffles
    const int part = tid & 3, kgrp = (tid >> 2) & 3, qi = tid >> 4;
    float sa[4] = {0.f, 0.f, 0.f, 0.f}, pa[4] = {0.f, 0.f, 0.f, 0.f};
    const bool act = qi < T && kgrp * 4 <= qi;
    if (act) {
      const float* qr = sqh + qi * HP; const TV* orow = sdo + qi * HV;
      const int k0 = kgrp * 4;
      const float* kr[4]; const TV* vr[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) { const int kk = min(k0 + j, T - 1); kr[j] = skh + kk * HP; vr[j] = sv + kk * HV; }
#pragma unroll 4
      for (int d = part; d < HD; d += 4) {                  // lanes interleave d: consecutive banks; unrolled: 40 LDS reads in flight
        const float qv = qr[d], ov = attn_tvf(orow[d]);
#pragma unroll
        for (int j = 0; j < 4; ++j) { sa[j] = fmaf(qv, kr[j][d], sa[j]); pa[j] = fmaf(ov, attn_tvf(vr[j][d]), pa[j]); }
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      sa[j] += __shfl_xor(sa[j], 1, 64); sa[j] += __shfl_xor(sa[j], 2, 64);
      pa[j] += __shfl_xor(pa[j], 1, 64); pa[j] += __shfl_xor(pa[j], 2, 64);
    }
    if (act && part == 0) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int ki = kgrp * 4 + j;
        if (ki <= qi) { sp[qi * 16 + ki] = sa[j] * scale; sds[qi * 16 + ki] = pa[j]; }
      }
    }
  }
  __syncthreads();
  {                                                     // softmax rows, dropout, dS = P * (dP - sum(dP*P)) * scale: 16 lanes per query row
    const int qi = wave * 4 + (lane >> 4), ki = lane & 15;
    const bool valid = qi < T && ki <= qi;
    const float sv_ = valid ? sp[qi * 16 + ki] : -INFINITY;
    float mx = sv_;
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    const float e = valid ? expf(sv_ - mx) : 0.f;
    float sum = e;
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) sum += __shfl_xor(sum, o, 64);
    const float pv = valid ? e / sum : 0.f;
    float m = 1.0f;
    if (thresh && valid) m = attn_keep(seed, prob, T, qi, ki, thresh) ? inv_keep : 0.f;
    const float dP = valid ? sds[qi * 16 + ki] * m : 0.f;   // gradient wrt the un-dropped probability
    float rs = dP * pv;
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) rs += __shfl_xor(rs, o, 64);
    const float dS = pv * (dP - rs) * scale;
    if (qi < T && ki < T) {
      if constexpr (MF) sp[qi * 16 + ki] = pv * m;               // the MFMA form reads the dropped probabilities [query][key]
      else { sp[qi * 16 + ki] = pv; spdT[ki * 16 + qi] = pv * m; }
      sds[qi * 16 + ki] = dS; sdsT[ki * 16 + qi] = dS;
    }
  }
  __syncthreads();
  // dV[j][d] = sum_{i>=j} Pd[i][j] dO[i][d];  dq_hat[i][d] = sum_{j<=i} dS[i][j] k_hat[j][d];  dk_hat[j][d] = sum_{i>=j} dS[i][j] q_hat[i][d].
  // One thread per (role, head-dim column) — role 0: dq_hat, role 1: dV and dk_hat.  The T column values a thread needs are read from
  // LDS once into registers, the P / dS coefficients are wave-uniform broadcast reads, so the FMAs are independent of LDS latency.
  // Results stay in registers across the barrier: they overwrite q_hat / k_hat / v in place.   (host side guarantees 2*HD <= 256, T <= 16)
  if constexpr (MF) {
    // 16-column tiles of the head dim, tile t on wave t % 4 (head_dim <= 128: at most two per wave); per tile three products over the token index k (four per
    // instruction): dq_hat[i][d] = dS[i][k] k_hat[k][d], dk_hat[j][d] = dS[k][j] q_hat[k][d], dV[j][d] = Pd[k][j] dO[k][d].  The coefficient tiles are zero beyond
    // T and above the diagonal; the other operand's rows k >= T are clamped (0 x finite).  Results wait in registers for the barrier, then replace q_hat / k_hat / v.
    const int fr = lane & 15, fq = lane >> 4, nt = HD / 16;
    f32x4 rq[2], rk[2], rv[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      rq[u] = f32x4{0.f, 0.f, 0.f, 0.f}; rk[u] = rq[u]; rv[u] = rq[u];
      const int t = wave + 4 * u;
      if (t < nt) {
        const int d = t * 16 + fr;
#pragma unroll
        for (int k0 = 0; k0 < 16; k0 += 4) {
          const int k = k0 + fq, kc = min(k, T - 1);
          const float a_dq = sdsT[k * 16 + fr], a_dk = sds[k * 16 + fr], a_dv = sp[k * 16 + fr];
          const float b_k = skh[kc * HP + d], b_q = sqh[kc * HP + d], b_o = attn_tvf(sdo[kc * HV + d]);
          rq[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_dq, b_k, rq[u], 0, 0, 0);
          rk[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_dk, b_q, rk[u], 0, 0, 0);
          rv[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_dv, b_o, rv[u], 0, 0, 0);
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int t = wave + 4 * u;
      if (t < nt) {
        const int d = t * 16 + fr;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = 4 * fq + r;
          if (row < T) {
            sqh[row * HP + d] = rq[u][r]; skh[row * HP + d] = rk[u][r];
            if constexpr (sizeof(TV) == 2) sv[row * HV + d] = f32_to_bf16_bits(rv[u][r]); else sv[row * HV + d] = rv[u][r];
          }
        }
      }
    }
  } else
  {
    constexpr int TMAX = 16;
    const int role = tid / HD, d = tid % HD;
    const bool act = tid < 2 * HD;
    float o0[TMAX], o1[TMAX];
#pragma unroll
    for (int t = 0; t < TMAX; ++t) { o0[t] = 0.f; o1[t] = 0.f; }
    auto dot16 = [](const float* row, const float* col) {   // row: 16 floats in LDS (wave-uniform address -> broadcast), col: registers
      const float4 a = *reinterpret_cast<const float4*>(row), b4 = *reinterpret_cast<const float4*>(row + 4);
      const float4 c = *reinterpret_cast<const float4*>(row + 8), e = *reinterpret_cast<const float4*>(row + 12);
      float r0 = a.x * col[0], r1 = a.y * col[1], r2 = a.z * col[2], r3 = a.w * col[3];
      r0 = fmaf(b4.x, col[4], r0); r1 = fmaf(b4.y, col[5], r1); r2 = fmaf(b4.z, col[6], r2); r3 = fmaf(b4.w, col[7], r3);
      r0 = fmaf(c.x, col[8], r0); r1 = fmaf(c.y, col[9], r1); r2 = fmaf(c.z, col[10], r2); r3 = fmaf(c.w, col[11], r3);
      r0 = fmaf(e.x, col[12], r0); r1 = fmaf(e.y, col[13], r1); r2 = fmaf(e.z, col[14], r2); r3 = fmaf(e.w, col[15], r3);
      return (r0 + r1) + (r2 + r3);
    };
    if (act && role == 0) {
      float kc[TMAX];
#pragma unroll
      for (int u = 0; u < TMAX; ++u) kc[u] = u < T ? skh[u * HP + d] : 0.f;
#pragma unroll
      for (int t = 0; t < TMAX; ++t) o0[t] = dot16(sds + t * 16, kc);          // causal zeros are in the tile
    } else if (act) {
      float oc[TMAX], qc[TMAX];
#pragma unroll
      for (int u = 0; u < TMAX; ++u) { oc[u] = u < T ? attn_tvf(sdo[u * HV + d]) : 0.f; qc[u] = u < T ? sqh[u * HP + d] : 0.f; }
#pragma unroll
      for (int j = 0; j < TMAX; ++j) { o0[j] = dot16(spdT + j * 16, oc); o1[j] = dot16(sdsT + j * 16, qc); }
    }
    __syncthreads();
    if (act && role == 0) {
#pragma unroll
      for (int t = 0; t < TMAX; ++t) if (t < T) sqh[t * HP + d] = o0[t];
    } else if (act) {
#pragma unroll
      for (int j = 0; j < TMAX; ++j) if (j < T) {
        if constexpr (sizeof(TV) == 2) sv[j * HV + d] = f32_to_bf16_bits(o0[j]); else sv[j * HV + d] = o0[j];
        skh[j * HP + d] = o1[j];
      }
    }
  }
  __syncthreads();
  const AttnRawLds raw{sq, sk, sgq, sgk, HP};
  attn_bwd_gain_partials(raw, sqh, skh, HP, srq, srk, dgq_part + (long)prob * HD, dgk_part + (long)prob * HD, T, HD, tid);
  __syncthreads();
  attn_bwd_norm_token(raw, sqh, skh, HP, srq, srk, tid >> 4, tid & 15, T, HD, eps);   // all T <= 16 tokens in one pass
  __syncthreads();
  attn_bwd_write<T2>(sqh, skh, HP, sv, HV, dqkv + (long)b * T * ld + h * HD, dbias_part ? dbias_part + (long)b * 3 * D + h * HD : nullptr, ld, D, T, HD, tid);
}

}  // namespace mode

using namespace mode;

extern "C" int mode_attn_block_fwd(const void* qkv, const float* q_gain, const float* k_gain, void* y, int dtype, int B, int T, int H,
                                   int head_dim, float eps, uint32_t seed, float p_drop, void* stream) {
  if (!qkv || !q_gain || !k_gain || !y || B < 0 || T <= 0 || H <= 0) return MODE_ERR_BAD_ARG;
  if (B == 0) return MODE_OK;
  if (p_drop < 0.f || p_drop >= 1.f) return MODE_ERR_BAD_ARG;
  const uint32_t th = dropout_thresh(p_drop); const float ik = 1.0f / (1.0f - p_drop);
  hipStream_t s = (hipStream_t)stream;
  if (T > 16) return attn_long_fwd_launch(qkv, q_gain, k_gain, y, dtype, B, T, H, head_dim, eps, seed, th, ik, s);
  if (dtype == MODE_BF16) {
    if (head_dim <= 0 || head_dim % 16 != 0 || head_dim > 128) return MODE_ERR_UNSUPPORTED;
    const dim3 grid((B * H + 3) / 4), blk(256);
    const uint16_t* in = (const uint16_t*)qkv; uint16_t* out = (uint16_t*)y;
#define MODE_ASF(NK) hipLaunchKernelGGL(attn_bf16_kernel<NK>, grid, blk, 0, s, in, q_gain, k_gain, out, B, T, H, head_dim, eps, seed, th, ik)
    MODE_ATTN_NKS_DISPATCH(head_dim, MODE_ASF)
#undef MODE_ASF
  } else {
    const size_t lds = ((size_t)3 * T * head_dim + (size_t)T * T) * 4;   // attn_f32_kernel's carve-up (kept by hand: see the LDS layouts in attn_core.h)
    if (lds > 64 * 1024) return MODE_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(attn_f32_kernel, dim3(B * H), dim3(64), lds, s, (const float*)qkv, q_gain, k_gain, (float*)y, B, T, H, head_dim, eps, seed, th, ik);
  }
  MODE_LAUNCH_CHECK();
  return MODE_OK;
}

namespace mode {
int g_attn_bwd_mfma = 1;
int attn_block_bwd_launch(const void* qkv, const float* q_gain, const float* k_gain, const void* dy, void* dqkv, float* dgq_partial,
                          float* dgk_partial, int dtype, int B, int T, int H, int head_dim, float eps, uint32_t seed, float p_drop, float* dbias_partial,
                          void* stream) {
  if (!qkv || !q_gain || !k_gain || !dy || !dqkv || !dgq_partial || !dgk_partial || B < 0 || T <= 0 || H <= 0) return MODE_ERR_BAD_ARG;
  if (p_drop < 0.f || p_drop >= 1.f) return MODE_ERR_BAD_ARG;
  if (B == 0) return MODE_OK;
  if (T > 16)
    return attn_long_bwd_launch(qkv, q_gain, k_gain, dy, dqkv, dgq_partial, dgk_partial, dtype, B, T, H, head_dim, eps, seed, dropout_thresh(p_drop),
                                1.0f / (1.0f - p_drop), dbias_partial, (hipStream_t)stream);
  const bool mf = head_dim % 16 == 0 && g_attn_bwd_mfma;
  if (head_dim > 128 || head_dim % (dtype == MODE_BF16 ? 8 : 4)) return MODE_ERR_UNSUPPORTED;
  const size_t lds = AttnBwdLds(T, head_dim, dtype == MODE_BF16 ? 2 : 4, mf).bytes;   // at most 54,784 bytes (fp32, T = 16, head_dim 128, VALU form)
  if (lds > 64 * 1024) return MODE_ERR_UNSUPPORTED;
  const uint32_t th = dropout_thresh(p_drop); const float ik = 1.0f / (1.0f - p_drop);
  hipStream_t s = (hipStream_t)stream;
#define MODE_ATTN_BWD(T2, MF) hipLaunchKernelGGL((attn_bwd_kernel<T2, MF>), dim3(B * H), dim3(256), lds, s, (const T2*)qkv, q_gain, k_gain, (const T2*)dy, (T2*)dqkv, \
                                                 dgq_partial, dgk_partial, B, T, H, head_dim, eps, seed, th, ik, dbias_partial)
  if (dtype == MODE_BF16) { if (mf) MODE_ATTN_BWD(uint16_t, true); else MODE_ATTN_BWD(uint16_t, false); }
  else { if (mf) MODE_ATTN_BWD(float, true); else MODE_ATTN_BWD(float, false); }
#undef MODE_ATTN_BWD
  MODE_LAUNCH_CHECK();
  return MODE_OK;
}
}  // namespace mode

extern "C" int mode_attn_block_bwd(const void* qkv, const float* q_gain, const float* k_gain, const void* dy, void* dqkv, float* dgq_partial,
                                   float* dgk_partial, int dtype, int B, int T, int H, int head_dim, float eps, uint32_t seed, float p_drop,
                                   void* stream) {
  return mode::attn_block_bwd_launch(qkv, q_gain, k_gain, dy, dqkv, dgq_partial, dgk_partial, dtype, B, T, H, head_dim, eps, seed, p_drop, nullptr, stream);
}
