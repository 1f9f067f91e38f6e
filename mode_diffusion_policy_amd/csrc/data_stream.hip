// Device-resident episode store -> the training batch of one step (include/mode_hip.h: mode_data_sample_windows; data.EpisodeStore /
// data.WindowStream).  Sample j of step t is a pure function of (seed, t, j) and the store: a counter-based draw of a window start, a binary search
// of the start among the episodes' prefix sums, and the gather of W action rows (normalised, the last row held past the episode's end with a
// zero mask), the episode's goal row, the sample's noise row of the environment noise stream, its sigma uniform and its cameras' integer shifts.
//
// grid (B), 256 threads: workgroup j owns output row j.  Every thread runs the (uniform) draw and search itself - <= 31 dependent 4-byte loads
// of a table that is L2-resident after the first workgroups - and the threads then share the row's W * A + G elements.  A batch moves
// B * (2 W A + G) floats, ~300 KB at B = 128: latency-bound, plain loops, no LDS, no atomics.  Every index is clamped into its table before it
// becomes an address.
//
// Validation reads the same store (include/mode_hip.h: mode_data_sweep_windows, mode_action_error; data.WindowSweep, validation.Validator): the sweep
// kernel enumerates the windows instead of drawing them and shares the located-window row body with the kernel above, and the error kernel sums the
// masked squared / absolute difference of two chunks into fp64 accumulators, one wave per element, in an order fixed by the shape.
//
// The held-out denoising error per noise level (include/mode_hip.h: mode_val_noise_levels, mode_level_error; validation.LevelValidator): a prep
// launch gives every swept window a level of a sigma table and its noised input, and the error kernel's body, shared, sums per level.
//
// Hindsight goals (include/mode_hip.h: mode_data_relabel_goals): a second launch behind either sampling kernel replaces a drawn share of the rows'
// episode goals by the stored embedding of a step a drawn number of steps ahead in the same episode.
//
// Ordered draws (include/mode_hip.h: mode_data_sample_windows_ordered; data.WindowStream(order="epoch") / (episode_weights=)): a third sampling kernel
// that locates row j's window another way - by a keyed permutation of the epoch's positions, or by an episode drawn from a table of weights - and then
// runs the same located-window row body and the same noise / u / shifts tail as the i.i.d. kernel: ONE definition of each.
#include "mode_common.h"

namespace mode {

// (x - lo) * scale - 1 in three roundings.  The pragma is what keeps them three: the __f*_rn intrinsics are plain operators to this compiler, and
// left alone it contracts the product into the last difference (seen: normalised values up to 10 ulp from the unfused ones near 0).
__device__ __forceinline__ float normalise_unfused(float x, float lo, float scale) {
#pragma clang fp contract(off)
  const float t = (x - lo) * scale;
  return t - 1.0f;
}

// What a located window needs of either descriptor (ModeDataStreamDesc, ModeDataSweepDesc): the store's tables and the row outputs.
struct WindowTables {
  const float* actions; const int32_t* ep_begin; const float* goals; const float* lo; const float* scale;
  int S, E, A, G, W;
  float* out_actions; float* action_mask; float* latent_goal; int32_t* index; int32_t* episode;
};
template <class Desc>
__device__ __forceinline__ WindowTables window_tables(const Desc& d) {
  return {d.actions, d.ep_begin, d.goals, d.lo, d.scale, d.S, d.E, d.A, d.G, d.W, d.out_actions, d.action_mask, d.latent_goal, d.index, d.episode};
}

// The episode of window number g: the largest e with starts[e] <= g (the header's binary search), clamped into [0, E).  The table's elements are
// int32 window numbers (starts) or int64 cuts of [0, 2^32] (mode_data_sample_windows_ordered's cut): never negative, compared unsigned in their width.
template <class T>
__device__ __forceinline__ int locate_episode(const T* starts, int E, uint32_t g) {
  int lo = 0, hi = E;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if ((typename std::make_unsigned<T>::type)starts[mid] <= g) lo = mid; else hi = mid;
  }
  return min(max(lo, 0), E - 1);
}

// Output row j of a located window - step p of episode e: index / episode, the gather of W action rows (normalised, the last row held past the
// episode's end), the step mask (all zero unless `live`) and the episode's goal row.  ONE body for the training stream and the sweep.
__device__ __forceinline__ void window_row(const WindowTables& t, int j, int e, long p, bool live, int tid) {
  const int first = min(max(t.ep_begin[e], 0), t.S - 1);
  const int last = min(max(t.ep_begin[e + 1] - 1, first), t.S - 1);
  const long want = (long)t.ep_begin[e] + p;
  const int start = (int)min(max(want, (long)first), (long)last);

  const int A = t.A, WA = t.W * t.A;
  const bool norm = t.lo != nullptr;
  float* oa = t.out_actions + (long)j * WA;
  for (int i = tid; i < WA; i += 256) {
    const int w = i / A, a = i - w * A;
    const float x = t.actions[min((long)start + w, (long)last) * A + a];
    oa[i] = norm ? normalise_unfused(x, t.lo[a], t.scale[a]) : x;
  }
  for (int w = tid; w < t.W; w += 256) t.action_mask[(long)j * t.W + w] = live && (long)start + w <= (long)last ? 1.0f : 0.0f;
  {
    const float* src = t.goals + (long)e * t.G;
    float* dst = t.latent_goal + (long)j * t.G;
    for (int i = tid; i < t.G; i += 256) dst[i] = src[i];
  }
  if (tid == 0) {
    t.index[j] = start;
    t.episode[j] = e;
  }
}

// What follows the located window in row j of a training batch - the noise row, the sigma uniform and the cameras' shifts, keyed by (seed, step, j)
// whatever located the window.  ONE body for the i.i.d. and the ordered kernel.
__device__ __forceinline__ void stream_row_tail(const ModeDataStreamDesc& d, int j, int tid) {
  const uint32_t uj = (uint32_t)j;
  const int WA = d.W * d.A;
  if (d.noise) {
    const uint32_t kn = mode_stream_seed(d.seed + 1u + uj * 0x9E3779B9u, d.step);
    float* dst = d.noise + (long)j * WA;
    for (int i = tid; i < WA; i += 256) dst[i] = env_normal(kn, (uint32_t)i);
  }
  if (tid == 0 && d.u) {
    const uint32_t k2 = mode_stream_seed(d.seed + 2u, d.step);
    d.u[j] = ((double)(hash_u32(k2 ^ uj) >> 8) + 0.5) * 0x1p-24;
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

__global__ __launch_bounds__(256) void data_sample_windows_kernel(ModeDataStreamDesc d) {
  const int j = blockIdx.x, tid = threadIdx.x;
  const uint32_t uj = (uint32_t)j;
  const uint32_t k = mode_stream_seed(d.seed, d.step);
  uint32_t g = (uint32_t)(((uint64_t)hash_u32(k ^ uj) * (uint64_t)(uint32_t)d.n_total) >> 32);
  g = min(g, (uint32_t)d.n_total - 1u);
  const int e = locate_episode(d.starts, d.E, g);
  window_row(window_tables(d), j, e, (long)g - (long)d.starts[e], true, tid);
  stream_row_tail(d, j, tid);
}

// The epoch permutation (include/mode_hip.h states it bit for bit): a balanced Feistel network on the smallest even number of bits that holds n - 1,
// MODE_PERM_ROUNDS rounds keyed by the epoch, applied again while the result is >= n (cycle walking: a walk that starts inside [0, n) returns there,
// and the map it induces on [0, n) is a bijection).  The domain is < 4 n, so a walk takes 4 applications on average at worst.  The bound of 2^bits
// applications is the length of the longest cycle the domain can hold: no value inside [0, n) reaches it, it only keeps a coding error from hanging
// the device, and the clamp behind it keeps the result an index.  Every thread of the workgroup walks the same q: the trip count is uniform.
__device__ __forceinline__ uint32_t epoch_perm(uint32_t ke, uint32_t n, uint32_t q) {
  const int nb = 32 - __clz((int)max(n - 1u, 1u));                         // bit length of n - 1, at least 1
  const int h = max(1, (nb + 1) >> 1);                                     // bits = 2 h: the smallest even number >= max(2, nb); h <= 16
  const uint32_t mask = (1u << h) - 1u;
  const uint64_t cap = 1ull << (2 * h);
  uint32_t v = min(q, n - 1u);
  for (uint64_t it = 0; it < cap; ++it) {
    uint32_t L = v >> h, R = v & mask;
#pragma unroll
    for (uint32_t r = 0; r < (uint32_t)MODE_PERM_ROUNDS; ++r) {
      const uint32_t t = L ^ (hash_u32(ke ^ (R | (r << 16))) & mask);
      L = R;
      R = t;
    }
    v = (L << h) | R;
    if (v < n) break;
  }
  return min(v, n - 1u);
}

// Row j of an ordered batch (include/mode_hip.h: mode_data_sample_windows_ordered).  The same grid as the kernel above; every thread locates the row's
// window itself (uniform over the workgroup): MODE_ORDER_EPOCH walks the permutation of the row's epoch and searches `starts`, MODE_ORDER_WEIGHTED
// searches `cut` for the episode (<= 31 dependent 8-byte loads of an L2-resident table) and draws the start within it.  No LDS, no atomics.
__global__ __launch_bounds__(256) void data_sample_windows_ordered_kernel(ModeDataOrderDesc o) {
  const ModeDataStreamDesc& d = o.s;
  const int j = blockIdx.x, tid = threadIdx.x;
  const uint32_t uj = (uint32_t)j, n = (uint32_t)d.n_total;
  int e;
  long p;
  if (o.mode == MODE_ORDER_EPOCH) {
    const uint64_t P = (uint64_t)d.step * (uint64_t)(uint32_t)d.B + (uint64_t)uj;
    const uint64_t ep = P / n;
    const uint32_t q = (uint32_t)(P - ep * n);
    const uint32_t ke = mode_stream_seed(d.seed + 6u + (uint32_t)(ep >> 32) * 0x9E3779B9u, (uint32_t)ep);
    const uint32_t g = epoch_perm(ke, n, q);
    e = locate_episode(d.starts, d.E, g);
    p = (long)g - (long)d.starts[e];
    if (tid == 0) {
      o.epoch[j] = (int64_t)ep;
      o.position[j] = (int64_t)q;
    }
  } else {
    const uint32_t r1 = hash_u32(mode_stream_seed(d.seed, d.step) ^ uj);
    const uint32_t r2 = hash_u32(mode_stream_seed(d.seed + 7u, d.step) ^ uj);
    e = locate_episode(o.cut, d.E, r1);
    const long n_e = max((long)d.starts[e + 1] - (long)d.starts[e], 1l);
    p = min((long)(((uint64_t)r2 * (uint64_t)n_e) >> 32), n_e - 1);
  }
  window_row(window_tables(d), j, e, p, true, tid);
  stream_row_tail(d, j, tid);
}

// The sweep (include/mode_hip.h: mode_data_sweep_windows; data.WindowSweep): row j is window first + j of the fixed enumeration instead of a
// draw - the same grid, search and row body; a row past the end repeats the last window with valid = 0 and a zero mask.  The noise row is keyed
// by the window's number, so a window carries its noise whatever batch size it is swept with.
__global__ __launch_bounds__(256) void data_sweep_windows_kernel(ModeDataSweepDesc d) {
  const int j = blockIdx.x, tid = threadIdx.x;
  const long want = (long)d.first + j;
  const bool live = want < (long)d.n_total;
  const uint32_t g = (uint32_t)min(max(want, 0l), (long)d.n_total - 1);
  const int e = locate_episode(d.starts, d.E, g);
  window_row(window_tables(d), j, e, (long)d.stride * ((long)g - (long)d.starts[e]), live, tid);
  if (tid == 0) {
    d.valid[j] = live ? 1.0f : 0.0f;
    d.window[j] = (int32_t)g;
  }
  if (d.noise) {
    const int WA = d.W * d.A;
    const uint32_t kn = mode_stream_seed(d.seed + 1u + g * 0x9E3779B9u, d.draw);
    float* dst = d.noise + (long)j * WA;
    for (int i = tid; i < WA; i += 256) dst[i] = d.noise_scale * env_normal(kn, (uint32_t)i);
  }
}

// Hindsight goal relabelling (include/mode_hip.h: mode_data_relabel_goals; data.WindowStream / data.WindowSweep with goal="hindsight"): runs after
// either sampling kernel on its index / episode.  grid (B), 256 threads like them: every thread runs the row's two (uniform) draws and clamps, thread
// 0 stores the three scalars, and a chosen row's G elements are shared - 16 bytes per thread where the row allows it (G = 512 fp32: 128 threads,
// one load and one store each).  A row that is not chosen leaves latent_goal alone.  Latency-bound like the kernels above: no LDS, no atomics.
__device__ __forceinline__ float bf16_bits_to_f32(uint32_t bits16) { return __builtin_bit_cast(float, bits16 << 16); }

__global__ __launch_bounds__(256) void data_relabel_goals_kernel(ModeDataGoalDesc d) {
  const int j = blockIdx.x, tid = threadIdx.x, G = d.G;
  const uint32_t id = d.ids ? (uint32_t)d.ids[j] : (uint32_t)j;
  const bool kind = (uint64_t)hash_u32(mode_stream_seed(d.seed + 5u, d.step) ^ id) < d.thresh;
  const uint64_t span = (uint64_t)((long)d.hi - (long)d.lo + 1);
  const long off = (long)d.lo + (long)(((uint64_t)hash_u32(mode_stream_seed(d.seed + 4u, d.step) ^ id) * span) >> 32);

  const int e = min(max(d.episode[j], 0), d.E - 1);
  const int first = min(max(d.ep_begin[e], 0), d.S - 1);
  const int last = min(max(d.ep_begin[e + 1] - 1, first), d.S - 1);
  const int start = min(max(d.index[j], first), last);
  const int r = (int)min((long)start + off, (long)last);                      // off >= 0: start <= r <= last
  if (tid == 0) {
    if (d.goal_index) d.goal_index[j] = r;
    if (d.goal_offset) d.goal_offset[j] = r - start;
    if (d.goal_kind) d.goal_kind[j] = kind ? 1.0f : 0.0f;
  }
  if (!kind) return;                                                           // (uniform over the workgroup)

  float* dst = d.latent_goal + (long)j * G;
  const bool aligned = ((((uintptr_t)d.step_goals) | ((uintptr_t)d.latent_goal)) & 15u) == 0;
  if (d.goal_dtype == MODE_F32) {
    const uint32_t* src = (const uint32_t*)d.step_goals + (long)r * G;
    if (aligned && (G & 3) == 0) {
      for (int i = tid; i < (G >> 2); i += 256) ((uint4*)dst)[i] = ((const uint4*)src)[i];
    } else {
      for (int i = tid; i < G; i += 256) ((uint32_t*)dst)[i] = src[i];
    }
  } else {
    const uint16_t* src = (const uint16_t*)d.step_goals + (long)r * G;
    if (aligned && (G & 7) == 0) {
      for (int i = tid; i < (G >> 3); i += 256) {
        const uint4 v = ((const uint4*)src)[i];                                // 8 bf16, element 2 c in the low half of word c
        ((float4*)dst)[2 * i] = make_float4(bf16_bits_to_f32(v.x & 0xffffu), bf16_bits_to_f32(v.x >> 16), bf16_bits_to_f32(v.y & 0xffffu), bf16_bits_to_f32(v.y >> 16));
        ((float4*)dst)[2 * i + 1] = make_float4(bf16_bits_to_f32(v.z & 0xffffu), bf16_bits_to_f32(v.z >> 16), bf16_bits_to_f32(v.w & 0xffffu), bf16_bits_to_f32(v.w >> 16));
      }
    } else {
      for (int i = tid; i < G; i += 256) dst[i] = bf16_bits_to_f32(src[i]);
    }
  }
}

// Masked error between two chunks, accumulated in fp64 (include/mode_hip.h: mode_action_error states the terms and the summation order).  256
// threads = 4 waves, one wave per element i = w * A + a; its lanes stride the batch, so the loads of a wave are W * A floats apart - a validation
// batch is a few thousand elements, latency-bound like the loss kernels.  No fused multiply-add anywhere: numpy fp64 reproduces every bit.
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o, 64);
  return v;
}

// One lane's share of element i = w * A + a and the butterfly over the wave: ONE body for mode_action_error and mode_level_error, so the two kernels
// cannot drift apart in a rounding.  `level` (or nullptr: every row) restricts the rows to those of level k; `unit` (or nullptr) is mode_action_error's.
struct ErrorSums { double sq, ab, cn; };
__device__ __forceinline__ ErrorSums masked_error_sums(const float* pred, const float* target, const float* mask, const float* weight, const double* unit,
                                                       const int32_t* level, int k, int B, int W, int A, int i, int lane) {
#pragma clang fp contract(off)
  const int WA = W * A, w = i / A, a = i - w * A;
  const double un = unit ? unit[a] : 1.0;
  double sq = 0.0, ab = 0.0, cn = 0.0;
  for (int b = lane; b < B; b += 64) {
    if (level && level[b] != k) continue;                                    // another level's row: nothing of it is read
    const float mr = mask ? mask[(long)b * W + w] : 1.f, m = mr > 0.f ? mr : 0.f;
    const float wr = weight ? weight[b] : 1.f, wt = wr > 0.f ? wr : 0.f;
    const float cf = wt * m;
    if (!(cf > 0.f)) continue;                                               // c == 0: the term is skipped, not multiplied
    const long at = (long)b * WA + i;
    const float df = pred[at] - target[at];
    const double c = (double)cf;
    const double e = unit ? (double)df * un : (double)df;
    const double t2 = c * (e * e), t1 = c * fabs(e);
    sq = sq + t2;
    ab = ab + t1;
    cn = cn + c;
  }
  return {wave_sum_f64(sq), wave_sum_f64(ab), wave_sum_f64(cn)};
}

__global__ __launch_bounds__(256) void action_error_kernel(ModeActionErrorDesc d) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6), WA = d.W * d.A;
  if (i >= WA) return;                                                       // (wave-uniform)
  const int w = i / d.A, a = i - w * d.A;
  const ErrorSums s = masked_error_sums(d.pred, d.target, d.mask, d.weight, d.unit, nullptr, 0, d.B, d.W, d.A, i, lane);
  if (lane == 0) {
    d.sq[i] = d.accumulate ? d.sq[i] + s.sq : s.sq;
    d.ab[i] = d.accumulate ? d.ab[i] + s.ab : s.ab;
    if (a == 0) d.cnt[w] = d.accumulate ? d.cnt[w] + s.cn : s.cn;
  }
}

// The noised input of a held-out window at its level of this draw (include/mode_hip.h: mode_val_noise_levels).  grid (B), 256 threads like the sweep:
// every thread forms the row's (uniform) level and reads its sigma - level < K by the modulus, so the table read is in bounds -, and the threads share
// the row's W * A elements.  The pragma keeps the product and the sum two roundings (see normalise_unfused).
__device__ __forceinline__ float noised_unfused(float a, float z, float sigma) {
#pragma clang fp contract(off)
  const float t = z * sigma;
  return a + t;
}

__global__ __launch_bounds__(256) void val_noise_levels_kernel(ModeValLevelsDesc d) {
  const int j = blockIdx.x, tid = threadIdx.x, WA = d.W * d.A;
  const uint32_t lv = ((uint32_t)d.window[j] + d.draw) % (uint32_t)d.K;
  const float sg = d.sigmas[lv];
  if (tid == 0) {
    d.level[j] = (int32_t)lv;
    d.sigma[j] = sg;
  }
  const float* a = d.actions + (long)j * WA;
  const float* z = d.noise + (long)j * WA;
  float* x = d.x + (long)j * WA;
  for (int i = tid; i < WA; i += 256) x[i] = noised_unfused(a[i], z[i], sg);
}

// mode_action_error binned by level (include/mode_hip.h: mode_level_error): the same 4 waves per workgroup, wave g of the grid owns the pair
// (k, i) = (g / (W * A), g % (W * A)) and runs the shared body over the rows of level k.  K * W * A waves, each reading level [B] once: at K = 16,
// W * A = 70, B = 128 that is 1120 waves over 72 KB - latency-bound like the kernel above.
__global__ __launch_bounds__(256) void level_error_kernel(ModeLevelErrorDesc d) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63, g = blockIdx.x * 4 + (threadIdx.x >> 6), WA = d.W * d.A;
  if (g >= d.K * WA) return;                                                 // (wave-uniform)
  const int k = g / WA, i = g - k * WA, w = i / d.A, a = i - w * d.A;
  const ErrorSums s = masked_error_sums(d.pred, d.target, d.mask, d.weight, nullptr, d.level, k, d.B, d.W, d.A, i, lane);
  if (lane == 0) {
    double* sq = d.sq + (long)k * WA + i;
    double* cn = d.cnt + (long)k * d.W + w;
    *sq = d.accumulate ? *sq + s.sq : s.sq;
    if (a == 0) *cn = d.accumulate ? *cn + s.cn : s.cn;
  }
}

}  // namespace mode

using namespace mode;

// The MODE_ERR_BAD_ARG refusals over the fields that ModeDataStreamDesc and ModeDataSweepDesc share: the required pointers, lo / scale given together,
// positive sizes, n_total <= S and E <= S.  An entry point tests what is its own after this and the limits last: every BAD_ARG before any UNSUPPORTED.
template <class Desc>
static bool window_desc_ok(const Desc* d) {
  return d && d->actions && d->ep_begin && d->starts && d->goals && d->out_actions && d->action_mask && d->latent_goal && d->index && d->episode &&
         (d->lo == nullptr) == (d->scale == nullptr) && d->S > 0 && d->E > 0 && d->A > 0 && d->G > 0 && d->W > 0 && d->B > 0 && d->n_total > 0 &&
         d->n_total <= d->S && d->E <= d->S;
}

// The kernels' limits (include/mode_hip.h), MODE_ERR_UNSUPPORTED beyond them; 0 for a size that an entry point does not have.
static bool within_limits(int B, long WA, int G, int K) { return B <= 65535 && WA <= 4096 && G <= 4096 && K <= 256; }

// The refusals of mode_data_sample_windows, shared with the ordered entry point (whose descriptor embeds the same struct).
static int check_stream_desc(const ModeDataStreamDesc* d) {
  if (!window_desc_ok(d)) return MODE_ERR_BAD_ARG;
  for (int q = 0; q < 2; ++q)
    if (d->shift_pad[q] < 0 || d->shift_pad[q] > 16384 || (d->shifts[q] && d->shift_pad[q] == 0)) return MODE_ERR_BAD_ARG;
  return within_limits(d->B, (long)d->W * d->A, d->G, 0) ? MODE_OK : MODE_ERR_UNSUPPORTED;
}

extern "C" int mode_data_sample_windows(const ModeDataStreamDesc* d, void* stream) {
  const int rc = check_stream_desc(d);
  if (rc != MODE_OK) return rc;
  hipLaunchKernelGGL(data_sample_windows_kernel, dim3(d->B), dim3(256), 0, (hipStream_t)stream, *d);
  MODE_LAUNCH_CHECK();
  return MODE_OK;
}

extern "C" int mode_data_sample_windows_ordered(const ModeDataOrderDesc* o, void* stream) {
  if (!o) return MODE_ERR_BAD_ARG;
  if (o->mode != MODE_ORDER_EPOCH && o->mode != MODE_ORDER_WEIGHTED) return MODE_ERR_BAD_ARG;
  if (o->mode == MODE_ORDER_EPOCH && (!o->epoch || !o->position)) return MODE_ERR_BAD_ARG;
  if (o->mode == MODE_ORDER_WEIGHTED && !o->cut) return MODE_ERR_BAD_ARG;
  const int rc = check_stream_desc(&o->s);
  if (rc != MODE_OK) return rc;
  hipLaunchKernelGGL(data_sample_windows_ordered_kernel, dim3(o->s.B), dim3(256), 0, (hipStream_t)stream, *o);
  MODE_LAUNCH_CHECK();
  return MODE_OK;
}

extern "C" int mode_data_sweep_windows(const ModeDataSweepDesc* d, void* stream) {
  if (!window_desc_ok(d) || !d->valid || !d->window || d->stride < 1 || d->first < 0 || d->first >= d->n_total) return MODE_ERR_BAD_ARG;
  if (!within_limits(d->B, (long)d->W * d->A, d->G, 0)) return MODE_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(data_sweep_windows_kernel, dim3(d->B), dim3(256), 0, (hipStream_t)stream, *d);
  MODE_LAUNCH_CHECK();
  return MODE_OK;
}

extern "C" int mode_data_relabel_goals(const ModeDataGoalDesc* d, void* stream) {
  if (!d || !d->step_goals || !d->ep_begin || !d->index || !d->episode || !d->latent_goal) return MODE_ERR_BAD_ARG;
  if (d->S <= 0 || d->E <= 0 || d->G <= 0 || d->B <= 0 || d->E > d->S) return MODE_ERR_BAD_ARG;
  if (d->lo < 0 || d->hi < d->lo || d->thresh > (1ull << 32)) return MODE_ERR_BAD_ARG;
  if (d->goal_dtype != MODE_F32 && d->goal_dtype != MODE_BF16) return MODE_ERR_BAD_ARG;
  if (!within_limits(d->B, 0, d->G, 0)) return MODE_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(data_relabel_goals_kernel, dim3(d->B), dim3(256), 0, (hipStream_t)stream, *d);
  MODE_LAUNCH_CHECK();
  return MODE_OK;
}

extern "C" int mode_action_error(const ModeActionErrorDesc* d, void* stream) {
  if (!d || !d->pred || !d->target || !d->sq || !d->ab || !d->cnt) return MODE_ERR_BAD_ARG;
  if (d->B <= 0 || d->W <= 0 || d->A <= 0) return MODE_ERR_BAD_ARG;
  if (!within_limits(d->B, (long)d->W * d->A, 0, 0)) return MODE_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(action_error_kernel, dim3((unsigned)((d->W * d->A + 3) / 4)), dim3(256), 0, (hipStream_t)stream, *d);
  MODE_LAUNCH_CHECK();
  return MODE_OK;
}

extern "C" int mode_val_noise_levels(const ModeValLevelsDesc* d, void* stream) {
  if (!d || !d->actions || !d->noise || !d->window || !d->sigmas || !d->level || !d->sigma || !d->x) return MODE_ERR_BAD_ARG;
  if (d->B <= 0 || d->W <= 0 || d->A <= 0 || d->K <= 0) return MODE_ERR_BAD_ARG;
  if (!within_limits(d->B, (long)d->W * d->A, 0, d->K)) return MODE_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(val_noise_levels_kernel, dim3(d->B), dim3(256), 0, (hipStream_t)stream, *d);
  MODE_LAUNCH_CHECK();
  return MODE_OK;
}

extern "C" int mode_level_error(const ModeLevelErrorDesc* d, void* stream) {
  if (!d || !d->pred || !d->target || !d->level || !d->sq || !d->cnt) return MODE_ERR_BAD_ARG;
  if (d->B <= 0 || d->W <= 0 || d->A <= 0 || d->K <= 0) return MODE_ERR_BAD_ARG;
  if (!within_limits(d->B, (long)d->W * d->A, 0, d->K)) return MODE_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(level_error_kernel, dim3((unsigned)((d->K * d->W * d->A + 3) / 4)), dim3(256), 0, (hipStream_t)stream, *d);
  MODE_LAUNCH_CHECK();
  return MODE_OK;
}
