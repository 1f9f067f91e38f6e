// LoRA adapters on a frozen base (include/mode_hip.h "LoRA adapters"): the merge W + s B A into the bf16 compute shadow (or in place over the fp32
// master) and the projection of the backward chain's dense weight gradient onto the adapter, dA = s B^T dW and dB = s dW A^T.  Stand-alone
// kernels around the unchanged launch chains; fp32 VALU products, no atomics: every output is a fixed expression of its inputs, whatever the grid.
#include "mode_common.h"

namespace mode {

typedef float lr_f4 __attribute__((ext_vector_type(4)));

constexpr int LR_THREADS = 256;
constexpr int LM_ROWS = 64, LM_COLS = 128;             // merge: one workgroup per 64 x 128 tile, a thread owns 4 rows x 8 columns
constexpr int LG_ROWS = 64, LG_COLS = 64;              // projection: row blocks of 64 (the unit dA's partials are indexed by), column steps of 64
constexpr int LG_LD = LG_COLS + 4;                     // padded LDS row of the dW / A tiles (16-byte aligned, rows 4 banks apart)

// ---- merge -----------------------------------------------------------------------------------------------------------------------------
// out[i][j] = W[i][j] + s * acc, acc <- acc + B[i][k] * A[k][j] over k = 0 .. r-1 from acc = 0, EVERY product and sum rounded to fp32 on its own
// (contraction is switched off for this kernel: left on, the compiler fuses even __fadd_rn(x, __fmul_rn(y, z)) into one fma).  The header states
// this, and the same expression written with separate fp32 tensor operations gives the same bits (tests/test_gpu_lora_model.py compares against
// exactly that).
// LDS: the A tile [r][128] and the B tile transposed [r][64]; per k a thread reads 8 + 4 staged values for 32 products.  W is read once (the loads are
// issued ahead of the k loop), out written once, both as 16-byte accesses.  W and out may alias (in place over the master): no __restrict__.
template <bool OUT_BF16>
__global__ __launch_bounds__(LR_THREADS) void lora_merge_kernel(const ModeLoraDesc d) {
#pragma clang fp contract(off)
  extern __shared__ float lora_lds[];
  const int r = d.r, cols = d.cols, rows = d.rows;
  float* As = lora_lds;                                // [r][LM_COLS]
  float* Bs = lora_lds + r * LM_COLS;                  // [r][LM_ROWS]
  const int tid = threadIdx.x, g = blockIdx.z;
  const int row0 = blockIdx.y * LM_ROWS, col0 = blockIdx.x * LM_COLS;
  const float* A = d.A + (long)g * r * cols;
  const float* B = d.B + (long)g * rows * r;
  const int nrow = min(LM_ROWS, rows - row0);

  const int c8 = (tid & 15) * 8, rg = (tid >> 4) * 4;
  const int col = col0 + c8;
  const bool live = col < cols;                        // cols % 8 == 0: a thread's 8 columns are inside or outside together
  const float* Wg = d.W + (long)g * d.w_stride;
  lr_f4 w[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    w[i][0] = w[i][1] = lr_f4{0.f, 0.f, 0.f, 0.f};
    if (live && rg + i < nrow) {
      const float* src = Wg + (long)(row0 + rg + i) * cols + col;
      w[i][0] = *reinterpret_cast<const lr_f4*>(src);
      w[i][1] = *reinterpret_cast<const lr_f4*>(src + 4);
    }
  }
  for (int t = tid; t < r * (LM_COLS / 4); t += LR_THREADS) {
    const int k = t / (LM_COLS / 4), c = (t % (LM_COLS / 4)) * 4;
    lr_f4 v = {0.f, 0.f, 0.f, 0.f};
    if (col0 + c < cols) v = *reinterpret_cast<const lr_f4*>(A + (long)k * cols + col0 + c);
    *reinterpret_cast<lr_f4*>(As + k * LM_COLS + c) = v;
  }
  for (int t = tid; t < LM_ROWS * r; t += LR_THREADS) {                 // the tile's rows are one contiguous run of B
    const int i = t / r, k = t - i * r;
    Bs[k * LM_ROWS + i] = i < nrow ? B[(long)row0 * r + t] : 0.f;
  }
  __syncthreads();
  if (!live) return;

  float acc[4][8];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[i][j] = 0.f;
  for (int k = 0; k < r; ++k) {
    const lr_f4 a0 = *reinterpret_cast<const lr_f4*>(As + k * LM_COLS + c8);
    const lr_f4 a1 = *reinterpret_cast<const lr_f4*>(As + k * LM_COLS + c8 + 4);
    const lr_f4 b = *reinterpret_cast<const lr_f4*>(Bs + k * LM_ROWS + rg);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float p0 = b[i] * a0[j], p1 = b[i] * a1[j];
        acc[i][j] = acc[i][j] + p0;
        acc[i][4 + j] = acc[i][4 + j] + p1;
      }
    }
  }
  const float s = d.scale[0];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (rg + i >= nrow) continue;
    float v[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float q0 = s * acc[i][j], q1 = s * acc[i][4 + j];
      v[j] = w[i][0][j] + q0;
      v[4 + j] = w[i][1][j] + q1;
    }
    const long off = (long)g * d.w_stride + (long)(row0 + rg + i) * cols + col;
    if constexpr (OUT_BF16) {
      out_u4 o = {pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]), pack_bf16x2(v[6], v[7])};
      *reinterpret_cast<out_u4*>(reinterpret_cast<uint16_t*>(d.out) + off) = o;
    } else {
      float* dst = reinterpret_cast<float*>(d.out) + off;
      *reinterpret_cast<lr_f4*>(dst) = lr_f4{v[0], v[1], v[2], v[3]};
      *reinterpret_cast<lr_f4*>(dst + 4) = lr_f4{v[4], v[5], v[6], v[7]};
    }
  }
}

// ---- projection, stage 1 ---------------------------------------------------------------------------------------------------------------
// One work item = (matrix g, row block rb of 64 rows); a workgroup walks the block's columns in steps of 64, so every element of dW is read from
// HBM once and feeds both products from LDS:
//   partial[g][rb][k][j] = sum over the block's rows i (ascending) of B[i][k] dW[i][j]          (one fma chain from 0; written per column step)
//   dB[i][k]             = s * sum over ALL columns j (ascending) of dW[i][j] A[k][j]           (one fma chain from 0 across the column steps)
// RT = ceil(r / 16): thread (c4 = tid % 16, kq = tid / 16) owns columns 4 c4 .. + 3 of adapter rows kq + 16 m of the first product and thread
// (row = tid / 4, kq = tid % 4) owns adapter columns kq + 4 m of one dW row of the second, m < RT resp. 4 RT.
template <int RT>
__global__ __launch_bounds__(LR_THREADS) void lora_grad_kernel(const ModeLoraDesc d, float* __restrict__ partial, int nrb) {
  extern __shared__ float lora_lds[];
  const int r = d.r, cols = d.cols, rows = d.rows, ldb = r + 1;
  float* Ds = lora_lds;                                // [64][LG_LD]   dW tile
  float* As = Ds + LG_ROWS * LG_LD;                    // [r][LG_LD]    A tile
  float* Bs = As + r * LG_LD;                          // [64][r + 1]   the row block of B
  const int tid = threadIdx.x;
  const int c4 = (tid & 15) * 4, kq1 = tid >> 4;
  const int row2 = tid >> 2, kq2 = tid & 3;
  for (int item = blockIdx.x; item < d.G * nrb; item += gridDim.x) {
    const int g = item / nrb, rb = item - g * nrb;
    const int row0 = rb * LG_ROWS, nrow = min(LG_ROWS, rows - row0);
    const float* __restrict__ dW = d.dW + (long)g * d.w_stride + (long)row0 * cols;
    const float* __restrict__ A = d.A + (long)g * r * cols;
    const float* __restrict__ B = d.B + ((long)g * rows + row0) * r;
    for (int t = tid; t < LG_ROWS * r; t += LR_THREADS) {
      const int i = t / r, k = t - i * r;
      Bs[i * ldb + k] = i < nrow ? B[t] : 0.f;
    }
    float accB[4 * RT];
#pragma unroll
    for (int m = 0; m < 4 * RT; ++m) accB[m] = 0.f;
    // the next column step's dW and A tiles travel in registers while this one is computed on: a step's global latency is hidden behind the
    // previous step's products (one workgroup walks up to 64 steps, and the small targets give the part only 16 - 64 workgroups)
    constexpr int DU = LG_ROWS * (LG_COLS / 4) / LR_THREADS;
    lr_f4 dreg[DU], areg[RT];
    auto fetch = [&](int col0) {
#pragma unroll
      for (int u = 0; u < DU; ++u) {
        const int t = u * LR_THREADS + tid, i = t >> 4, c = (t & 15) * 4;
        dreg[u] = lr_f4{0.f, 0.f, 0.f, 0.f};
        if (i < nrow && col0 + c < cols) dreg[u] = *reinterpret_cast<const lr_f4*>(dW + (long)i * cols + col0 + c);
      }
#pragma unroll
      for (int u = 0; u < RT; ++u) {
        const int t = u * LR_THREADS + tid, k = t >> 4, c = (t & 15) * 4;
        areg[u] = lr_f4{0.f, 0.f, 0.f, 0.f};
        if (k < r && col0 + c < cols) areg[u] = *reinterpret_cast<const lr_f4*>(A + (long)k * cols + col0 + c);
      }
    };
    fetch(0);
    for (int col0 = 0; col0 < cols; col0 += LG_COLS) {
      __syncthreads();                                 // the previous step's readers are done with Ds / As (and Bs is staged before the first)
#pragma unroll
      for (int u = 0; u < DU; ++u) {
        const int t = u * LR_THREADS + tid, i = t >> 4, c = (t & 15) * 4;
        *reinterpret_cast<lr_f4*>(Ds + i * LG_LD + c) = dreg[u];
      }
#pragma unroll
      for (int u = 0; u < RT; ++u) {
        const int t = u * LR_THREADS + tid, k = t >> 4, c = (t & 15) * 4;
        if (k < r) *reinterpret_cast<lr_f4*>(As + k * LG_LD + c) = areg[u];
      }
      __syncthreads();
      if (col0 + LG_COLS < cols) fetch(col0 + LG_COLS);
      // product 1: this row block's share of dA, columns col0 .. col0 + 63
      lr_f4 acc[RT];
#pragma unroll
      for (int m = 0; m < RT; ++m) acc[m] = lr_f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
      for (int i = 0; i < LG_ROWS; ++i) {
        const lr_f4 dv = *reinterpret_cast<const lr_f4*>(Ds + i * LG_LD + c4);
#pragma unroll
        for (int m = 0; m < RT; ++m) {
          const int k = kq1 + 16 * m;
          if (k < r) {
            const float b = Bs[i * ldb + k];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[m][j] = __builtin_fmaf(b, dv[j], acc[m][j]);
          }
        }
      }
      if (col0 + c4 < cols) {
#pragma unroll
        for (int m = 0; m < RT; ++m) {
          const int k = kq1 + 16 * m;
          if (k < r) *reinterpret_cast<lr_f4*>(partial + (((long)g * nrb + rb) * r + k) * cols + col0 + c4) = acc[m];
        }
      }
      // product 2: dB of this row block, continued over the column steps
#pragma unroll 4
      for (int j4 = 0; j4 < LG_COLS; j4 += 4) {
        const lr_f4 dv = *reinterpret_cast<const lr_f4*>(Ds + row2 * LG_LD + j4);
#pragma unroll
        for (int m = 0; m < 4 * RT; ++m) {
          const int k = kq2 + 4 * m;
          if (k < r) {
            const lr_f4 av = *reinterpret_cast<const lr_f4*>(As + k * LG_LD + j4);
#pragma unroll
            for (int j = 0; j < 4; ++j) accB[m] = __builtin_fmaf(dv[j], av[j], accB[m]);
          }
        }
      }
    }
    if (row2 < nrow) {
      const float s = d.scale[0];
      float* dst = d.dB + ((long)g * rows + row0 + row2) * r;
#pragma unroll
      for (int m = 0; m < 4 * RT; ++m) {
        const int k = kq2 + 4 * m;
        if (k < r) {
          const float v = __fmul_rn(s, accB[m]);
          dst[k] = d.accumulate ? __fadd_rn(dst[k], v) : v;
        }
      }
    }
    __syncthreads();                                   // Bs / Ds / As are restaged by the next item
  }
}

// ---- projection, stage 2: dA[g][k][j] = s * (partial[g][0][k][j] + partial[g][1][k][j] + ...), ascending row block, one thread per 4 columns
__global__ __launch_bounds__(LR_THREADS) void lora_grad_finish_kernel(const ModeLoraDesc d, const float* __restrict__ partial, int nrb) {
  const long per_g = (long)d.r * d.cols;
  const long n4 = (long)d.G * per_g / 4;
  const float s = d.scale[0];
  for (long t = (long)blockIdx.x * LR_THREADS + threadIdx.x; t < n4; t += (long)gridDim.x * LR_THREADS) {
    const long e = t * 4;
    const long g = e / per_g, rem = e - g * per_g;
    const float* p = partial + g * nrb * per_g + rem;
    lr_f4 sum = *reinterpret_cast<const lr_f4*>(p);
    int rb = 1;
    for (; rb + 8 <= nrb; rb += 8) {                   // 8 loads in flight, then the additions in ascending order
      lr_f4 v[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] = *reinterpret_cast<const lr_f4*>(p + (long)(rb + q) * per_g);
#pragma unroll
      for (int q = 0; q < 8; ++q)
#pragma unroll
        for (int j = 0; j < 4; ++j) sum[j] = __fadd_rn(sum[j], v[q][j]);
    }
    for (; rb < nrb; ++rb) {
      const lr_f4 v = *reinterpret_cast<const lr_f4*>(p + (long)rb * per_g);
#pragma unroll
      for (int j = 0; j < 4; ++j) sum[j] = __fadd_rn(sum[j], v[j]);
    }
    lr_f4* dst = reinterpret_cast<lr_f4*>(d.dA + e);
    lr_f4 o;
    if (d.accumulate) {
      const lr_f4 old = *dst;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = __fadd_rn(old[j], __fmul_rn(s, sum[j]));
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = __fmul_rn(s, sum[j]);
    }
    *dst = o;
  }
}

// shape rules shared by the three entry points
static int lora_check_shape(const ModeLoraDesc* d) {
  if (!d || d->G < 1 || d->rows < 1 || d->cols < 1 || d->G > 65535) return MODE_ERR_BAD_ARG;
  if (d->r < 1 || d->r > MODE_LORA_MAX_RANK || d->cols % 8) return MODE_ERR_UNSUPPORTED;
  if (d->w_stride % 8 || (d->G > 1 && d->w_stride < (int64_t)d->rows * d->cols)) return MODE_ERR_BAD_ARG;
  return MODE_OK;
}
static inline bool lora_al16(const void* p) { return p && !((uintptr_t)p & 15); }

}  // namespace mode

using namespace mode;

extern "C" int mode_lora_merge(const ModeLoraDesc* d, void* stream) {
  const int rc = lora_check_shape(d);
  if (rc != MODE_OK) return rc;
  if (!lora_al16(d->W) || !lora_al16(d->A) || !lora_al16(d->out) || !d->B || !d->scale || ((uintptr_t)d->B & 3) || ((uintptr_t)d->scale & 3))
    return MODE_ERR_BAD_ARG;
  if (d->out_dtype != MODE_BF16 && d->out_dtype != MODE_F32) return MODE_ERR_BAD_ARG;
  const dim3 grid((d->cols + LM_COLS - 1) / LM_COLS, (d->rows + LM_ROWS - 1) / LM_ROWS, d->G);
  if (grid.y > 65535) return MODE_ERR_UNSUPPORTED;
  const size_t lds = (size_t)d->r * (LM_COLS + LM_ROWS) * sizeof(float);            // <= 48 KiB at r = 64
  if (d->out_dtype == MODE_BF16)
    hipLaunchKernelGGL(lora_merge_kernel<true>, grid, dim3(LR_THREADS), lds, (hipStream_t)stream, *d);
  else
    hipLaunchKernelGGL(lora_merge_kernel<false>, grid, dim3(LR_THREADS), lds, (hipStream_t)stream, *d);
  MODE_LAUNCH_CHECK();
  return MODE_OK;
}

extern "C" size_t mode_lora_grad_workspace_bytes(const ModeLoraDesc* d) {
  if (lora_check_shape(d) != MODE_OK) return 0;
  const size_t nrb = ((size_t)d->rows + LG_ROWS - 1) / LG_ROWS;
  return (size_t)d->G * nrb * d->r * d->cols * sizeof(float);
}

extern "C" int mode_lora_grad(const ModeLoraDesc* d, void* workspace, size_t workspace_bytes, void* stream) {
  const int rc = lora_check_shape(d);
  if (rc != MODE_OK) return rc;
  if (!lora_al16(d->dW) || !lora_al16(d->A) || !lora_al16(d->dA) || !d->B || !d->dB || !d->scale || ((uintptr_t)d->B & 3) || ((uintptr_t)d->dB & 3) ||
      ((uintptr_t)d->scale & 3))
    return MODE_ERR_BAD_ARG;
  if (!lora_al16(workspace)) return MODE_ERR_BAD_ARG;
  if (workspace_bytes < mode_lora_grad_workspace_bytes(d)) return MODE_ERR_WORKSPACE;
  const int nrb = (d->rows + LG_ROWS - 1) / LG_ROWS;
  if ((int64_t)d->G * nrb > 0x7fffffff) return MODE_ERR_UNSUPPORTED;
  float* partial = reinterpret_cast<float*>(workspace);
  const int blocks = std::min(d->G * nrb, 4096);                                     // the rest by grid stride: the result does not depend on it
  const size_t lds = ((size_t)LG_ROWS * LG_LD + (size_t)d->r * LG_LD + (size_t)LG_ROWS * (d->r + 1)) * sizeof(float);      // <= 50.3 KiB at r = 64
  switch ((d->r + 15) / 16) {
    case 1: hipLaunchKernelGGL(lora_grad_kernel<1>, dim3(blocks), dim3(LR_THREADS), lds, (hipStream_t)stream, *d, partial, nrb); break;
    case 2: hipLaunchKernelGGL(lora_grad_kernel<2>, dim3(blocks), dim3(LR_THREADS), lds, (hipStream_t)stream, *d, partial, nrb); break;
    case 3: hipLaunchKernelGGL(lora_grad_kernel<3>, dim3(blocks), dim3(LR_THREADS), lds, (hipStream_t)stream, *d, partial, nrb); break;
    default: hipLaunchKernelGGL(lora_grad_kernel<4>, dim3(blocks), dim3(LR_THREADS), lds, (hipStream_t)stream, *d, partial, nrb); break;
  }
  MODE_LAUNCH_CHECK();
  const long n4 = (long)d->G * d->r * d->cols / 4;
  const int fblocks = (int)std::min<long>((n4 + LR_THREADS - 1) / LR_THREADS, 2048);
  hipLaunchKernelGGL(lora_grad_finish_kernel, dim3(fblocks), dim3(LR_THREADS), 0, (hipStream_t)stream, *d, partial, nrb);
  MODE_LAUNCH_CHECK();
  return MODE_OK;
}
