// Device-resident episode store -> the training batch of one step (include/mode_hip.h: mode_data_sample_windows; data.EpisodeStore /
// data.WindowStream).  Sample j of step t is a pure function of (seed, t, j) and the store: a counter-based draw of a window start, a binary search
// of the start among the episodes' prefix sums, and the gather of W action rows (normalised, the last row held past the episode's end with a
// zero mask), the episode's goal row, the sample's noise row of the environment noise stream, its sigma uniform and its cameras' integer shifts.
//
// grid (B), 256 threads: workgroup j owns output row j.  Every thread runs the (uniform) draw and search itself - <= 31 dependent 4-byte loads
// of a table that is L2-resident after the first workgroups - and the threads then share the row's W * A + G elements.  A batch moves
// B * (2 W A + G) floats, ~300 KB at B = 128: latency-bound, plain loops, no LDS, no atomics.  Every index is clamped into its table before it
// becomes an address.
#include "mode_common.h"

namespace mode {

// (x - lo) * scale - 1 in three roundings.  The pragma is what keeps them three: the __f*_rn intrinsics are plain operators to this compiler, and
// left alone it contracts the product into the last difference (seen: normalised values up to 10 ulp from the unfused ones near 0).
__device__ __forceinline__ float normalise_unfused(float x, float lo, float scale) {
#pragma clang fp contract(off)
  const float t = (x - lo) * scale;
  return t - 1.0f;
}

__global__ __launch_bounds__(256) void data_sample_windows_kernel(ModeDataStreamDesc d) {
  const int j = blockIdx.x, tid = threadIdx.x;
  const uint32_t uj = (uint32_t)j;
  const uint32_t k = mode_stream_seed(d.seed, d.step);
  uint32_t g = (uint32_t)(((uint64_t)hash_u32(k ^ uj) * (uint64_t)(uint32_t)d.n_total) >> 32);
  g = min(g, (uint32_t)d.n_total - 1u);
  int lo = 0, hi = d.E;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if ((uint32_t)d.starts[mid] <= g) lo = mid; else hi = mid;
  }
  const int e = min(max(lo, 0), d.E - 1);
  const int first = min(max(d.ep_begin[e], 0), d.S - 1);
  const int last = min(max(d.ep_begin[e + 1] - 1, first), d.S - 1);
  const long want = (long)d.ep_begin[e] + ((long)g - (long)d.starts[e]);
  const int start = (int)min(max(want, (long)first), (long)last);

  const int A = d.A, WA = d.W * d.A;
  const bool norm = d.lo != nullptr;
  float* oa = d.out_actions + (long)j * WA;
  for (int i = tid; i < WA; i += 256) {
    const int w = i / A, a = i - w * A;
    const float x = d.actions[min((long)start + w, (long)last) * A + a];
    oa[i] = norm ? normalise_unfused(x, d.lo[a], d.scale[a]) : x;
  }
  for (int w = tid; w < d.W; w += 256) d.action_mask[(long)j * d.W + w] = (long)start + w <= (long)last ? 1.0f : 0.0f;
  {
    const float* src = d.goals + (long)e * d.G;
    float* dst = d.latent_goal + (long)j * d.G;
    for (int i = tid; i < d.G; i += 256) dst[i] = src[i];
  }
  if (d.noise) {
    const uint32_t kn = mode_stream_seed(d.seed + 1u + uj * 0x9E3779B9u, d.step);
    float* dst = d.noise + (long)j * WA;
    for (int i = tid; i < WA; i += 256) dst[i] = env_normal(kn, (uint32_t)i);
  }
  if (tid == 0) {
    d.index[j] = start;
    d.episode[j] = e;
    if (d.u) {
      const uint32_t k2 = mode_stream_seed(d.seed + 2u, d.step);
      d.u[j] = ((double)(hash_u32(k2 ^ uj) >> 8) + 0.5) * 0x1p-24;
    }
  }
  if (tid < 4) {
    const int q = tid >> 1, c = tid & 1;
    int32_t* sh = q == 0 ? d.shifts[0] : d.shifts[1];                       // (no dynamic index into the argument block)
    const int pad = q == 0 ? d.shift_pad[0] : d.shift_pad[1];
    if (sh) {
      const uint32_t k3 = mode_stream_seed(d.seed + 3u, d.step);
      sh[2 * (long)j + c] = (int32_t)(((uint64_t)hash_u32(k3 ^ (4u * uj + 2u * (uint32_t)q + (uint32_t)c)) * (uint64_t)(2 * pad + 1)) >> 32);
    }
  }
}

}  // namespace mode

using namespace mode;

extern "C" int mode_data_sample_windows(const ModeDataStreamDesc* d, void* stream) {
  if (!d || !d->actions || !d->ep_begin || !d->starts || !d->goals || !d->out_actions || !d->action_mask || !d->latent_goal || !d->index || !d->episode)
    return MODE_ERR_BAD_ARG;
  if ((d->lo == nullptr) != (d->scale == nullptr)) return MODE_ERR_BAD_ARG;
  if (d->S <= 0 || d->E <= 0 || d->A <= 0 || d->G <= 0 || d->W <= 0 || d->B <= 0 || d->n_total <= 0 || d->n_total > d->S || d->E > d->S) return MODE_ERR_BAD_ARG;
  for (int q = 0; q < 2; ++q)
    if (d->shift_pad[q] < 0 || d->shift_pad[q] > 16384 || (d->shifts[q] && d->shift_pad[q] == 0)) return MODE_ERR_BAD_ARG;
  if (d->B > 65535 || (long)d->W * d->A > 4096 || d->G > 4096) return MODE_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(data_sample_windows_kernel, dim3(d->B), dim3(256), 0, (hipStream_t)stream, *d);
  MODE_LAUNCH_CHECK();
  return MODE_OK;
}
