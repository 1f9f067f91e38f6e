// LoRA training without the dense weight gradient (include/mode_hip.h "LoRA adapters", ModeLoraFactDesc): with Y = X W_eff^T, W_eff = W + s B A,
//   T = dY B   [M, r]        U = X A^T   [M, r]              (down: contraction over rows resp. cols)
//   dA = s T^T X  [r, cols]  dB = s dY^T U  [rows, r]        (up: contraction over the M rows of a group)
// X and dY are the bf16 operands of the dense weight-gradient GEMM this replaces; they expand exactly to fp32, A and B stay fp32, and every product
// runs on the exact fp32-input MFMA (v_mfma_f32_16x16x4_f32: a k-ordered fp32 fma chain).  No atomics and no grid-dependent order: the down stage
// splits its contraction over the four waves of a workgroup and adds the four shares in wave order, the up stage cuts every group into blocks of
// LF_RB rows counted from the group's first row, and a finishing pass adds the blocks' shares in ascending order, scales and stores.
#include "mode_common.h"

namespace mode {

typedef float lf_f4 __attribute__((ext_vector_type(4)));
typedef uint16_t lf_u16x8 __attribute__((ext_vector_type(8)));

constexpr int LF_DOWN_ROWS = 16;       // down: rows of T / U per workgroup (one MFMA tile); its four waves take every fourth 32-deep step
constexpr int LF_RB = 128;             // up: rows per block, a function of nothing
constexpr int LF_STRIP = 128;          // up: columns per wave (eight 16-wide MFMA tiles interleaved, so that a lane loads and stores 8 in a row)

struct LfGroup { int lo, hi; };
// rows [lo, hi) of group g, forced into [0, M] whatever the device holds
__device__ __forceinline__ LfGroup lf_group(const ModeLoraFactDesc& d, int g) {
  if (!d.group_offsets) return LfGroup{0, d.M};
  int lo = d.group_offsets[g], hi = d.group_offsets[g + 1];
  lo = min(max(lo, 0), d.M);
  hi = min(max(hi, lo), d.M);
  return LfGroup{lo, hi};
}
// first slot of group g's row-block shares: disjoint for ascending offsets, below M / LF_RB + G + 1 always
__device__ __forceinline__ int lf_slot0(const LfGroup& q, int g) { return q.lo / LF_RB + g; }

// ---- down -------------------------------------------------------------------------------------------------------------------------------
// blockIdx = (16-row tile of the group, side, group).  side 0: T = dY B, side 1: U = X A^T.  Lane (row = lane % 16, q = lane / 16) loads 8
// consecutive bf16 of its row per step; MFMA e of the step contracts elements 8 q' + e, q' = 0 .. 3, so the fp32 operand of lane (c, q) is
// B[i0 + 8 q + e][k0 + c] resp. A[k0 + c][i0 + 8 q + e].
template <int RT>
__global__ __launch_bounds__(256) void lora_fact_down_kernel(const ModeLoraFactDesc d, float* __restrict__ T, float* __restrict__ U) {
  __shared__ float red[4 * LF_DOWN_ROWS * RT * 16];
  const int g = blockIdx.z, side = blockIdx.y;
  const LfGroup grp = lf_group(d, g);
  const int m0 = grp.lo + (int)blockIdx.x * LF_DOWN_ROWS;
  if (m0 >= grp.hi) return;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 15, q = lane >> 4;
  const int r = d.r, rows = d.rows, cols = d.cols;
  const int K = side ? cols : rows;
  const int m = m0 + c;
  const bool mlive = m < grp.hi;
  const uint16_t* src = nullptr;
  if (mlive) {
    if (side) src = reinterpret_cast<const uint16_t*>(d.X) + (long)(d.x_rows ? d.x_rows[m] : m) * d.ld_x;
    else src = reinterpret_cast<const uint16_t*>(d.dY) + (long)m * d.ld_dy;
  }
  const float* __restrict__ Wm = side ? d.A + (long)g * r * cols : d.B + (long)g * rows * r;

  lf_f4 acc[RT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) acc[rt] = lf_f4{0.f, 0.f, 0.f, 0.f};
  const int nstep = (K + 31) / 32;
  for (int st = wave; st < nstep; st += 4) {
    const int i8 = st * 32 + 8 * q;
    const bool ilive = i8 < K;                           // K % 8 == 0: a lane's 8 elements are inside or outside together
    lf_u16x8 a = {0, 0, 0, 0, 0, 0, 0, 0};
    if (mlive && ilive) a = *reinterpret_cast<const lf_u16x8*>(src + i8);
    float w[RT][8];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      const int k = rt * 16 + c;
#pragma unroll
      for (int e = 0; e < 8; ++e) w[rt][e] = 0.f;
      if (k < r && ilive) {
        if (side) {
          const lf_f4 lo = *reinterpret_cast<const lf_f4*>(Wm + (long)k * cols + i8);
          const lf_f4 hi = *reinterpret_cast<const lf_f4*>(Wm + (long)k * cols + i8 + 4);
#pragma unroll
          for (int e = 0; e < 4; ++e) { w[rt][e] = lo[e]; w[rt][4 + e] = hi[e]; }
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e) w[rt][e] = Wm[(long)(i8 + e) * r + k];
        }
      }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float af = bf16_bits_to_f32(a[e]);
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) acc[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(af, w[rt][e], acc[rt], 0, 0, 0);
    }
  }
  // accumulator: row 4 q + reg of the tile, column rt * 16 + c of the rank
  constexpr int RW = RT * 16;
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) red[(wave * LF_DOWN_ROWS + 4 * q + reg) * RW + rt * 16 + c] = acc[rt][reg];
  __syncthreads();
  float* __restrict__ out = side ? U : T;
  for (int t = tid; t < LF_DOWN_ROWS * RW; t += 256) {
    const int row = t / RW, k = t - row * RW;
    if (m0 + row < grp.hi && k < r) {
      float v = red[t];
      v = __fadd_rn(v, red[LF_DOWN_ROWS * RW + t]);
      v = __fadd_rn(v, red[2 * LF_DOWN_ROWS * RW + t]);
      v = __fadd_rn(v, red[3 * LF_DOWN_ROWS * RW + t]);
      out[(long)(m0 + row) * r + k] = v;
    }
  }
}

// ---- up ---------------------------------------------------------------------------------------------------------------------------------
// One wave per workgroup; blockIdx = (strip, row block of the group, group).  Strips 0 .. SA-1 are 128 columns of dA^ = T^T X, the rest 128 rows of
// dB^T = U^T dY: both are [r, n] = P^T S with P = T or U [M, r] fp32 and S = X or dY [M, n] bf16.  A step contracts 4 rows: lane (c, q) holds
// P[m + q][k0 + c] and the 8 elements S[m + q][j0 + 8 c .. + 7]; MFMA e takes element e, so tile e owns columns j0 + 8 c + e and a lane ends up
// with 8 consecutive columns of rank rows rt * 16 + 4 q + reg.  The block's share goes to its slot of the workspace as [r][cols] ++ [r][rows].
template <int RT>
__global__ __launch_bounds__(64) void lora_fact_up_kernel(const ModeLoraFactDesc d, const float* __restrict__ T, const float* __restrict__ U,
                                                           float* __restrict__ partial, int SA) {
  const int g = blockIdx.z;
  const LfGroup grp = lf_group(d, g);
  const int start = grp.lo + (int)blockIdx.y * LF_RB;
  if (start >= grp.hi) return;
  const int end = min(grp.hi, start + LF_RB);
  const int lane = threadIdx.x, c = lane & 15, q = lane >> 4;
  const int r = d.r, rows = d.rows, cols = d.cols;
  const bool bside = (int)blockIdx.x >= SA;
  const int n = bside ? rows : cols;
  const int jc = ((int)blockIdx.x - (bside ? SA : 0)) * LF_STRIP + 8 * c;
  const bool jlive = jc < n;                             // n % 8 == 0
  const uint16_t* S = reinterpret_cast<const uint16_t*>(bside ? d.dY : d.X);
  const long ld = bside ? d.ld_dy : d.ld_x;
  const int32_t* rowmap = bside ? nullptr : d.x_rows;
  const float* __restrict__ P = bside ? U : T;

  lf_f4 acc[RT][8];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[rt][e] = lf_f4{0.f, 0.f, 0.f, 0.f};
  for (int m4 = start; m4 < end; m4 += 4) {
    const int m = m4 + q;
    const bool live = m < end;
    lf_u16x8 x = {0, 0, 0, 0, 0, 0, 0, 0};
    if (live && jlive) x = *reinterpret_cast<const lf_u16x8*>(S + (long)(rowmap ? rowmap[m] : m) * ld + jc);
    float p[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      const int k = rt * 16 + c;
      p[rt] = (live && k < r) ? P[(long)m * r + k] : 0.f;
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float xf = bf16_bits_to_f32(x[e]);
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) acc[rt][e] = __builtin_amdgcn_mfma_f32_16x16x4f32(p[rt], xf, acc[rt][e], 0, 0, 0);
    }
  }
  if (!jlive) return;
  const long per_slot = (long)r * (cols + rows);
  float* dst = partial + (long)(lf_slot0(grp, g) + (int)blockIdx.y) * per_slot + (bside ? (long)r * cols : 0);
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int k = rt * 16 + 4 * q + reg;
      if (k < r) {
        float* o = dst + (long)k * n + jc;
        *reinterpret_cast<lf_f4*>(o) = lf_f4{acc[rt][0][reg], acc[rt][1][reg], acc[rt][2][reg], acc[rt][3][reg]};
        *reinterpret_cast<lf_f4*>(o + 4) = lf_f4{acc[rt][4][reg], acc[rt][5][reg], acc[rt][6][reg], acc[rt][7][reg]};
      }
    }
}

// ---- finish: dA[g][k][j] = s * (share_0 + share_1 + ...), dB[g][i][k] likewise from the [r][rows] half; a group without rows gets +0.0
__global__ __launch_bounds__(256) void lora_fact_finish_kernel(const ModeLoraFactDesc d, const float* __restrict__ partial) {
  const int r = d.r, rows = d.rows, cols = d.cols;
  const long na = (long)r * cols, per_slot = na + (long)rows * r, total = (long)d.G * per_slot;
  const float s = d.scale[0];
  for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long)gridDim.x * 256) {
    const int g = (int)(t / per_slot);
    const long e = t - (long)g * per_slot;
    const LfGroup grp = lf_group(d, g);
    const int nb = (grp.hi - grp.lo + LF_RB - 1) / LF_RB;
    long src;
    float* out;
    if (e < na) {
      src = e;
      out = d.dA + (long)g * na + e;
    } else {                                             // dB is [rows][r], its shares [r][rows]
      const long f = e - na;
      const int i = (int)(f / r), k = (int)(f - (long)i * r);
      src = na + (long)k * rows + i;
      out = d.dB + (long)g * rows * r + f;
    }
    float v = 0.f;
    if (nb > 0) {
      const float* p = partial + (long)lf_slot0(grp, g) * per_slot + src;
      float sum = p[0];
      for (int b = 1; b < nb; ++b) sum = __fadd_rn(sum, p[(long)b * per_slot]);
      v = __fmul_rn(s, sum);
    }
    *out = v;
  }
}

struct LfWs { size_t t, u, partial, total; };
static inline size_t lf_up(size_t v) { return (v + 255) & ~(size_t)255; }
static LfWs lf_ws(const ModeLoraFactDesc* d) {
  LfWs w;
  const size_t tu = lf_up((size_t)d->M * d->r * sizeof(float));
  const size_t slots = (size_t)d->M / LF_RB + d->G + 1;
  w.t = 0; w.u = tu; w.partial = 2 * tu;
  w.total = 2 * tu + lf_up(slots * d->r * ((size_t)d->cols + d->rows) * sizeof(float));
  return w;
}
static int lf_check_shape(const ModeLoraFactDesc* d) {
  if (!d || d->G < 1 || d->G > 65535 || d->M < 0) return MODE_ERR_BAD_ARG;
  if (d->r < 1 || d->r > MODE_LORA_MAX_RANK || d->rows < 8 || d->cols < 8 || d->rows % 8 || d->cols % 8 || d->dtype != MODE_BF16) return MODE_ERR_UNSUPPORTED;
  if ((d->M + LF_RB - 1) / LF_RB > 65535) return MODE_ERR_UNSUPPORTED;
  return MODE_OK;
}
static inline bool lf_al(const void* p, uintptr_t a) { return p && !((uintptr_t)p & (a - 1)); }

}  // namespace mode

using namespace mode;

extern "C" size_t mode_lora_fact_workspace_bytes(const ModeLoraFactDesc* d) {
  if (lf_check_shape(d) != MODE_OK) return 0;
  return lf_ws(d).total;
}

extern "C" int mode_lora_fact_grad(const ModeLoraFactDesc* d, void* workspace, size_t workspace_bytes, void* stream) {
  const int rc = lf_check_shape(d);
  if (rc != MODE_OK) return rc;
  if (!lf_al(d->X, 16) || !lf_al(d->dY, 16) || !lf_al(d->A, 16) || !lf_al(d->B, 16) || !lf_al(d->dA, 16) || !lf_al(d->dB, 16) || !lf_al(d->scale, 4))
    return MODE_ERR_BAD_ARG;
  if (d->ld_x % 8 || d->ld_dy % 8 || d->ld_x < d->cols || d->ld_dy < d->rows) return MODE_ERR_BAD_ARG;
  if (d->x_rows && ((uintptr_t)d->x_rows & 3)) return MODE_ERR_BAD_ARG;
  if (d->group_offsets ? ((uintptr_t)d->group_offsets & 3) != 0 : d->G != 1) return MODE_ERR_BAD_ARG;
  if (!lf_al(workspace, 16)) return MODE_ERR_BAD_ARG;
  const LfWs W = lf_ws(d);
  if (workspace_bytes < W.total) return MODE_ERR_WORKSPACE;
  hipStream_t hs = (hipStream_t)stream;
  float* T = reinterpret_cast<float*>((char*)workspace + W.t);
  float* U = reinterpret_cast<float*>((char*)workspace + W.u);
  float* partial = reinterpret_cast<float*>((char*)workspace + W.partial);
  const int RT = (d->r + 15) / 16;
  if (d->M > 0) {
    const dim3 gd((d->M + LF_DOWN_ROWS - 1) / LF_DOWN_ROWS, 2, d->G);
    switch (RT) {
      case 1: hipLaunchKernelGGL(lora_fact_down_kernel<1>, gd, dim3(256), 0, hs, *d, T, U); break;
      case 2: hipLaunchKernelGGL(lora_fact_down_kernel<2>, gd, dim3(256), 0, hs, *d, T, U); break;
      case 3: hipLaunchKernelGGL(lora_fact_down_kernel<3>, gd, dim3(256), 0, hs, *d, T, U); break;
      default: hipLaunchKernelGGL(lora_fact_down_kernel<4>, gd, dim3(256), 0, hs, *d, T, U); break;
    }
    MODE_LAUNCH_CHECK();
    const int SA = (d->cols + LF_STRIP - 1) / LF_STRIP, SB = (d->rows + LF_STRIP - 1) / LF_STRIP;
    const dim3 gu(SA + SB, (d->M + LF_RB - 1) / LF_RB, d->G);
    switch (RT) {
      case 1: hipLaunchKernelGGL(lora_fact_up_kernel<1>, gu, dim3(64), 0, hs, *d, T, U, partial, SA); break;
      case 2: hipLaunchKernelGGL(lora_fact_up_kernel<2>, gu, dim3(64), 0, hs, *d, T, U, partial, SA); break;
      case 3: hipLaunchKernelGGL(lora_fact_up_kernel<3>, gu, dim3(64), 0, hs, *d, T, U, partial, SA); break;
      default: hipLaunchKernelGGL(lora_fact_up_kernel<4>, gu, dim3(64), 0, hs, *d, T, U, partial, SA); break;
    }
    MODE_LAUNCH_CHECK();
  }
  const long total = (long)d->G * d->r * ((long)d->cols + d->rows);
  const int fblocks = (int)std::min<long>((total + 255) / 256, 2048);
  hipLaunchKernelGGL(lora_fact_finish_kernel, dim3(fblocks), dim3(256), 0, hs, *d, partial);
  MODE_LAUNCH_CHECK();
  return MODE_OK;
}
