// Device-side gradient norms (include/mode_hip.h "Device-side gradient norms"): a deterministic sum of squares over flat fp32 gradient
// buffers in two stages, and the clip / skip state the AdamW launches read on the device.  Streaming kernels, no float atomics: every
// chunk's partial is a fixed expression of the chunk's data, so the result is the same bits for any grid, any split into launches, any run.
#include "mode_common.h"

namespace mode {

typedef float gn_f4 __attribute__((ext_vector_type(4)));

constexpr int GN_THREADS = 256;                                        // 4 waves
constexpr int GN_GROUPS = MODE_GRAD_CHUNK / 4 / GN_THREADS;            // 16-byte groups per thread and chunk (16)
static_assert(MODE_GRAD_CHUNK % (4 * GN_THREADS) == 0, "a chunk is a whole number of 16-byte groups per thread");

// stage 1.  Additions on the longest path from an element to partial[c]: GN_GROUPS (per-lane accumulators) + 2 (lane pairs) + 6 (wave
// butterfly) + 3 (cross-wave) = 27 at MODE_GRAD_CHUNK = 16384 - tests/grad_norm_refs.py derives its bound from exactly this structure.
__global__ __launch_bounds__(GN_THREADS) void grad_sumsq_kernel(const float* __restrict__ g, const ModeGradChunk* __restrict__ chunks, int first, int count,
                                                                float* __restrict__ partial) {
  __shared__ float wsum[GN_THREADS / 64];
  const int tid = threadIdx.x;
  for (int c = first + blockIdx.x; c < first + count; c += gridDim.x) {
    const ModeGradChunk ch = chunks[c];
    const int n = min(max(ch.n, 0), MODE_GRAD_CHUNK);                  // a corrupt table cannot widen the walk
    const float* __restrict__ src = g + ch.lo;
    gn_f4 x[GN_GROUPS];
#pragma unroll
    for (int k = 0; k < GN_GROUPS; ++k) {                              // every load of the chunk in flight before the first square
      const int e = (k * GN_THREADS + tid) * 4;
      gn_f4 v = {0.f, 0.f, 0.f, 0.f};
      if (e + 4 <= n) {
        v = *reinterpret_cast<const gn_f4*>(src + e);
      } else if (e < n) {                                              // the one ragged group of the chunk: element by element, nothing at or past lo + n
        v[0] = src[e];
        if (e + 1 < n) v[1] = src[e + 1];
        if (e + 2 < n) v[2] = src[e + 2];
      }
      x[k] = v;
    }
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
    for (int k = 0; k < GN_GROUPS; ++k) {                              // explicit roundings: square to fp32, then add (no contraction into an fma)
      a0 = __fadd_rn(a0, __fmul_rn(x[k][0], x[k][0]));
      a1 = __fadd_rn(a1, __fmul_rn(x[k][1], x[k][1]));
      a2 = __fadd_rn(a2, __fmul_rn(x[k][2], x[k][2]));
      a3 = __fadd_rn(a3, __fmul_rn(x[k][3], x[k][3]));
    }
    float s = __fadd_rn(__fadd_rn(a0, a1), __fadd_rn(a2, a3));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s = __fadd_rn(s, __shfl_xor(s, o, 64));     // fixed butterfly: lane i and lane i ^ o form the same sum
    if ((tid & 63) == 0) wsum[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) partial[c] = __fadd_rn(__fadd_rn(__fadd_rn(wsum[0], wsum[1]), wsum[2]), wsum[3]);
    __syncthreads();                                                   // wsum is reused by the next chunk of this workgroup
  }
}

// stage 2: one workgroup.  Thread t sums tensor t, t + 1024, ... (ascending chunk order, fp64); thread 0 adds the tensors' sums in
// ascending tensor order and writes the state.
constexpr int GF_THREADS = 1024;

__global__ __launch_bounds__(GF_THREADS) void grad_clip_finish_kernel(const float* __restrict__ partial, const int32_t* __restrict__ begin, int n_tensors,
                                                                      float max_norm, float grad_scale, int skip_nonfinite, float* __restrict__ tensor_sq,
                                                                      ModeGradClipState* __restrict__ st) {
  __shared__ double tsum[GF_THREADS];
  const int tid = threadIdx.x;
  double total = 0.0;                                                  // thread 0's
  for (int t0 = 0; t0 < n_tensors; t0 += GF_THREADS) {
    const int t = t0 + tid;
    double s = 0.0;
    if (t < n_tensors) {
      const int c1 = begin[t + 1];
      int c = begin[t];
      for (; c + 16 <= c1; c += 16) {                                  // 16 loads in flight, then the additions in ascending order (a large expert matrix owns
        float v[16];                                                   // hundreds of partials: one load latency per addition would dominate the launch)
#pragma unroll
        for (int i = 0; i < 16; ++i) v[i] = partial[c + i];
#pragma unroll
        for (int i = 0; i < 16; ++i) s += (double)v[i];
      }
      for (; c < c1; ++c) s += (double)partial[c];
      tensor_sq[t] = (float)s;
    }
    tsum[tid] = s;
    __syncthreads();
    if (tid == 0) {
      const int m = min(GF_THREADS, n_tensors - t0);
      for (int i = 0; i < m; ++i) total += tsum[i];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const float total_norm = fabsf(grad_scale) * (float)sqrt(total);
    float coef = 1.f;
    if (max_norm > 0.f) coef = fminf(1.f, max_norm / (total_norm + 1e-6f));
    const int nonfinite = !isfinite(total_norm);
    const int skip = nonfinite && skip_nonfinite;
    st->total_norm = total_norm;
    st->coef = coef;
    st->scale = __fmul_rn(grad_scale, coef);
    st->nonfinite = nonfinite;
    st->skip = skip;
    st->skipped += skip;
  }
}

}  // namespace mode

using namespace mode;

extern "C" int mode_grad_sumsq(const float* g, const ModeGradChunk* chunks, int first, int count, float* partial, void* stream) {
  if (first < 0 || count < 0) return MODE_ERR_BAD_ARG;
  if (count == 0) return MODE_OK;
  if (!g || !chunks || !partial || ((uintptr_t)g & 15) || ((uintptr_t)chunks & 7)) return MODE_ERR_BAD_ARG;
  const int blocks = std::min(count, 2048);                           // 8 workgroups of 4 waves per CU; the rest by grid stride
  hipLaunchKernelGGL(grad_sumsq_kernel, dim3(blocks), dim3(GN_THREADS), 0, (hipStream_t)stream, g, chunks, first, count, partial);
  MODE_LAUNCH_CHECK();
  return MODE_OK;
}

extern "C" int mode_grad_clip_finish(const float* partial, const int32_t* tensor_chunk_begin, int n_tensors, float max_norm, float grad_scale,
                                     int skip_nonfinite, float* tensor_sq, ModeGradClipState* st, void* stream) {
  if (!st || n_tensors < 0 || ((uintptr_t)st & 3)) return MODE_ERR_BAD_ARG;
  if (n_tensors > 0 && (!partial || !tensor_chunk_begin || !tensor_sq)) return MODE_ERR_BAD_ARG;
  hipLaunchKernelGGL(grad_clip_finish_kernel, dim3(1), dim3(GF_THREADS), 0, (hipStream_t)stream, partial, tensor_chunk_begin, n_tensors, max_norm,
                     grad_scale, skip_nonfinite, tensor_sq, st);
  MODE_LAUNCH_CHECK();
  return MODE_OK;
}
