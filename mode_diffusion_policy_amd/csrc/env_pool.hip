// Per-environment replanning of a vectorised rollout (include/mode_hip.h, ABI 13; rollout.VectorEnvPolicy): the gather of the replanning
// environments' observations with their initial noise - or, warm-started, their previous plan's tail noised to an intermediate level - into a
// chunk's input buffers, and the commit of the chunk's plans + the emission of one action per active environment - the newest plan's row, or with temporal ensembling the weighted mean of the rows that the environment's last K
// plans predict for the step (env_commit_emit_ens_kernel).  With candidate selection (rollout.VectorEnvPolicy(candidates=N)) the gathers fill N
// rows per environment and env_select_kernel picks, between the chain and the commit, the candidate closest to the previous plan's tail (staged in LDS).
// With forward contrast (candidates=N, contrast=M) the gathers fill N + M rows, the last M with a zero goal row, and env_select_bid_kernel adds to
// each strong candidate's score its distance to the best strong candidates minus that to the best weak ones.
// All move a few hundred KB at most: one launch each, plain coalesced loops, no LDS beside that tail.  The gather of the
// replanning environments' camera frames into the encoders' input (mode_env_gather_frames) moves ~1.2 MB per fp32 row at 224 x 224: HBM-bound,
// 16-byte loads and stores.
#include "mode_common.h"

#include <cfloat>

namespace mode {

// (env_normal, the Box-Muller sample of the environment noise stream, is defined in mode_common.h: the training batch stream draws from it too)

// Observation and goal rows of environment r -> row j of a chunk's inputs (256 threads; either pair may be absent)
__device__ __forceinline__ void env_gather_obs(const int r, const int j, const float* __restrict__ img, const long img_floats,
                                               const float* __restrict__ goals, const long goal_floats, float* __restrict__ img_out,
                                               float* __restrict__ goal_out, const bool zero_goal) {
  if (img && img_out) {
    const float* src = img + (long)r * img_floats;
    float* dst = img_out + (long)j * img_floats;
    for (long i = threadIdx.x; i < img_floats; i += 256) dst[i] = src[i];
  }
  if (goals && goal_out) {
    const float* src = goals + (long)r * goal_floats;
    float* dst = goal_out + (long)j * goal_floats;
    for (long i = threadIdx.x; i < goal_floats; i += 256) dst[i] = zero_goal ? 0.f : src[i];
  }
}

// Bit b of a little-endian bitmask of uint32 words (the active and has-previous-plan masks), given its word, words[b >> 5]
__device__ __forceinline__ bool env_bit(const uint32_t word, const int b) { return (word >> (b & 31)) & 1u; }

// Both gathers run on grid (m_b, N): block (j, c) fills chunk row j * N + c, candidate c of environment rows[j], from draw draws[r] * N + c of
// its stream (uint32 arithmetic).  N = 1 - a replan without candidate selection - is row j from draw draws[r].  The first `strong` candidates
// carry the environment's goal row, the others (forward contrast: the weak candidates of the _bid gathers) a zero goal row.
__global__ __launch_bounds__(256) void env_gather_noise_kernel(const int32_t* __restrict__ rows, int num_envs, const uint32_t* __restrict__ seeds,
                                                               const uint32_t* __restrict__ draws, const float* __restrict__ img, long img_floats,
                                                               const float* __restrict__ goals, long goal_floats, float* __restrict__ img_out,
                                                               float* __restrict__ goal_out, float* __restrict__ x0, int noise_floats, float sigma_max,
                                                               int strong) {
  const int r = rows[blockIdx.x];
  if (r < 0 || r >= num_envs) return;
  const int j = blockIdx.x * gridDim.y + blockIdx.y;
  env_gather_obs(r, j, img, img_floats, goals, goal_floats, img_out, goal_out, (int)blockIdx.y >= strong);
  const uint32_t k = mode_stream_seed(seeds[r], draws[r] * gridDim.y + blockIdx.y);
  float* dst = x0 + (long)j * noise_floats;
  for (int e = threadIdx.x; e < noise_floats; e += 256) dst[e] = sigma_max * env_normal(k, (uint32_t)e);
}

// The warm-started form of the gather above (rollout.VectorEnvPolicy(warm_start=k)): the same rows, the same stream element z, but the latent is
// the environment's previous plan advanced by `shift` rows - its last row held beyond the end - noised to sigma_start, one fused multiply-add per
// element.  plan is only read: the commit launch that wrote it is earlier in the stream.
__global__ __launch_bounds__(256) void env_gather_warm_kernel(const int32_t* __restrict__ rows, int num_envs, const uint32_t* __restrict__ seeds,
                                                              const uint32_t* __restrict__ draws, const float* __restrict__ img, long img_floats,
                                                              const float* __restrict__ goals, long goal_floats, float* __restrict__ img_out,
                                                              float* __restrict__ goal_out, float* __restrict__ x0, const float* __restrict__ plan, int W,
                                                              int A, int shift, float sigma_start, int strong) {
  const int r = rows[blockIdx.x];
  if (r < 0 || r >= num_envs) return;
  const int j = blockIdx.x * gridDim.y + blockIdx.y;
  env_gather_obs(r, j, img, img_floats, goals, goal_floats, img_out, goal_out, (int)blockIdx.y >= strong);
  const uint32_t k = mode_stream_seed(seeds[r], draws[r] * gridDim.y + blockIdx.y);
  const int WA = W * A;
  const float* old = plan + (long)r * WA;
  float* dst = x0 + (long)j * WA;
  for (int e = threadIdx.x; e < WA; e += 256) {
    const int w = e / A, a = e - w * A;
    dst[e] = fmaf(sigma_start, env_normal(k, (uint32_t)e), old[min(w + shift, W - 1) * A + a]);
  }
}

// Frames of the replanning environments -> the encoders' input [m_b * T, C, H, W].  grid (x blocks per row, m_b, 2 cameras), 256 threads; each
// thread moves 8 elements per iteration: fp32 -> fp32 two 16-byte loads + two stores, fp32 -> bf16 two loads + one store (RNE, the rounding the
// stem applies to an fp32 image), bf16 -> bf16 one load + one store.  A row whose source or destination is not 16-byte aligned (an odd row pitch,
// odd H * W) takes the element loop; so does the tail of a row that is not a multiple of 8 elements.
__device__ __forceinline__ void frames_copy_row(const ModeEnvFramesCam& c, const int r, const int j) {
  const long n = c.row_elems;
  const int so = c.src_dtype == MODE_F32 ? 4 : 2, dso = c.dst_dtype == MODE_F32 ? 4 : 2;
  const char* src = static_cast<const char*>(c.src) + (long)r * c.src_stride * so;
  char* dst = static_cast<char*>(c.dst) + (long)j * n * dso;
  const long nthr = (long)gridDim.x * 256, t = (long)blockIdx.x * 256 + threadIdx.x;
  long done = 0;
  if ((((uintptr_t)src | (uintptr_t)dst) & 15) == 0) {
    const long nv = n >> 3;                                    // 8-element groups
    if (c.src_dtype == MODE_BF16) {
      const uint4* s4 = reinterpret_cast<const uint4*>(src);
      uint4* d4 = reinterpret_cast<uint4*>(dst);
      for (long v = t; v < nv; v += nthr) d4[v] = s4[v];
    } else if (c.dst_dtype == MODE_F32) {
      const float4* s4 = reinterpret_cast<const float4*>(src);
      float4* d4 = reinterpret_cast<float4*>(dst);
      for (long v = t; v < nv; v += nthr) {
        const float4 a = s4[2 * v], b = s4[2 * v + 1];
        d4[2 * v] = a; d4[2 * v + 1] = b;
      }
    } else {
      const float4* s4 = reinterpret_cast<const float4*>(src);
      uint4* d4 = reinterpret_cast<uint4*>(dst);
      for (long v = t; v < nv; v += nthr) {
        const float4 a = s4[2 * v], b = s4[2 * v + 1];
        d4[v] = make_uint4(pack_bf16x2(a.x, a.y), pack_bf16x2(a.z, a.w), pack_bf16x2(b.x, b.y), pack_bf16x2(b.z, b.w));
      }
    }
    done = nv << 3;
  }
  for (long i = done + t; i < n; i += nthr) {
    if (c.src_dtype == MODE_BF16) {
      reinterpret_cast<uint16_t*>(dst)[i] = reinterpret_cast<const uint16_t*>(src)[i];
    } else {
      const float f = reinterpret_cast<const float*>(src)[i];
      if (c.dst_dtype == MODE_F32) reinterpret_cast<float*>(dst)[i] = f;
      else reinterpret_cast<uint16_t*>(dst)[i] = f32_to_bf16_bits(f);
    }
  }
}

__global__ __launch_bounds__(256) void env_gather_frames_kernel(ModeEnvFramesDesc d) {
  const int j = blockIdx.y;
  const int r = d.rows[j];
  if (r < 0 || r >= d.num_envs) return;
  const ModeEnvFramesCam c = blockIdx.z == 0 ? d.cam[0] : d.cam[1];   // (no dynamic index into the argument block)
  if (!c.src || !c.dst) return;
  frames_copy_row(c, r, j);
}

// Head of both commit kernels, one wave per environment b: the step's output and the word of its active mask that holds b's bit from the control block (d.ctrl) or, without
// one, from the descriptor (then no row replans), and the row j of b among the chunk's m real rows (-1: b does not replan), known to every lane
__device__ __forceinline__ int env_commit_head(const ModeEnvPoolDesc& d, const int b, const int lane, float*& out, uint32_t& act_word) {
  const int NW = (d.num_envs + 31) >> 5;
  const int32_t* ctrl = d.ctrl;
  int m = 0;
  if (ctrl) {
    m = min(max(ctrl[0], 0), d.num_envs);
    out = reinterpret_cast<float*>((uint64_t)(uint32_t)ctrl[2] | ((uint64_t)(uint32_t)ctrl[3] << 32));
    act_word = (uint32_t)ctrl[4 + (b >> 5)];
  } else {
    out = d.out;
    act_word = d.active[b >> 5];
  }
  const int32_t* rows = ctrl ? ctrl + 4 + NW : nullptr;
  int j = -1;
  for (int i = lane; i < m; i += 64)
    if (rows[i] == b) j = i;
  // every lane learns the (unique) row: the largest index found by any lane
  for (int o = 32; o > 0; o >>= 1) j = max(j, __shfl_xor(j, o, 64));
  return j;
}

// One wave per environment b: find b among the chunk's m real rows (rows are distinct), commit that row, then emit.  The emitted row of a
// just-committed plan is read from the chunk itself (counter 0), so no thread reads plan memory another thread of this launch wrote.
__global__ __launch_bounds__(64) void env_commit_emit_kernel(ModeEnvPoolDesc d) {
  const int b = blockIdx.x, lane = threadIdx.x;
  float* out;
  uint32_t act_word;
  const int j = env_commit_head(d, b, lane, out, act_word);
  const bool active = env_bit(act_word, b);
  const int WA = d.W * d.A;
  float* plan = d.plan + (long)b * WA;
  int c;
  if (j >= 0) {
    const float* src = d.chunk + (long)j * WA;
    for (int i = lane; i < WA; i += 64) plan[i] = src[i];
    c = 0;
  } else {
    c = min(max(d.counter[b], 0), d.W - 1);
  }
  if (lane < d.A) {
    float v = 0.f;
    if (active) v = j >= 0 ? d.chunk[(long)j * WA + lane] : plan[(long)c * d.A + lane];
    out[(long)b * d.A + lane] = v;
  }
  if (lane == 0) {
    if (j >= 0) d.draws[b] += 1u;
    if (active) d.counter[b] = (c + 1) % d.multistep;
    else if (j >= 0) d.counter[b] = 0;
  }
}

// The ensembled pool (ModeEnvEnsDesc): the same wave per environment b, the same search for b among the chunk's rows.  A committed chunk goes to
// ring slot (t / s) % K (and to plan[b], the newest plan); the emitted row is the weighted mean of the live plans' rows for step t, oldest first.
// Lane i < K tests the plan i strides older than the newest, so one ballot holds the live set, bit i = age i; the rows are then loaded eight at a
// time before the first multiply-add of the batch, so that a K-deep ring costs K / 8 load latencies and not K.  As above, the row of a plan
// committed by this launch is read from the chunk, and birth / t / counter are written by lane 0 after every lane's reads of them.
__global__ __launch_bounds__(64) void env_commit_emit_ens_kernel(ModeEnvEnsDesc e) {
  const ModeEnvPoolDesc& d = e.pool;
  const int b = blockIdx.x, lane = threadIdx.x;
  float* out;
  uint32_t act_word;
  const int j = env_commit_head(d, b, lane, out, act_word);
  const bool active = env_bit(act_word, b);
  const int s = d.multistep, K = e.K, W = d.W, A = d.A, WA = W * A;
  const int t = max(e.t[b], 0);
  const int q = (t / s) % K;                   // slot of the newest plan, born at tn
  const int tn = t - t % s;
  float* ring = e.ring + (long)b * K * WA;
  int32_t* birth = e.birth + (long)b * K;
  bool live = false;
  if (lane < K) {
    const int want = tn - lane * s;            // birth of the plan `lane` strides older than the newest
    if (lane == 0 && j >= 0) live = true;
    else live = want >= 0 && t - want < W && birth[(q + K - lane) % K] == want;
  }
  unsigned long long ages = __ballot(live);    // bit i: the plan of age i is live (wave-uniform)
  if (j >= 0) {
    const float* src = d.chunk + (long)j * WA;
    float* slot = ring + (long)q * WA;
    float* plan = d.plan + (long)b * WA;
    for (int i = lane; i < WA; i += 64) {
      const float v = src[i];
      slot[i] = v; plan[i] = v;
    }
  }
  float num = 0.f, den = 0.f;
  int rank = 0;
  const int col = lane < A ? lane : 0;
  while (active && ages) {
    float x[8], w[8];
    int cnt = 0;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      x[u] = 0.f; w[u] = 0.f;
      if (ages) {
        const int i = 63 - __clzll((long long)ages);          // the oldest plan not yet taken
        ages &= ~(1ull << i);
        const float* src = (i == 0 && j >= 0) ? d.chunk + (long)j * WA : ring + (long)((q + K - i) % K) * WA + (long)(t - tn + i * s) * A;
        x[u] = src[col];
        w[u] = e.weights[rank + u];
        cnt = u + 1;
      }
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      if (u < cnt) {
        if (rank + u == 0) { num = w[u] * x[u]; den = w[u]; }
        else { num = fmaf(w[u], x[u], num); den += w[u]; }
      }
    }
    rank += cnt;
  }
  if (lane < A) out[(long)b * A + lane] = den > 0.f ? num / den : 0.f;
  if (lane == 0) {
    if (j >= 0) { d.draws[b] += 1u; birth[q] = t; }
    const int c = j >= 0 ? 0 : min(max(d.counter[b], 0), W - 1);
    if (active) { d.counter[b] = (c + 1) % s; e.t[b] = t + 1; }
    else if (j >= 0) d.counter[b] = 0;
  }
}

// Candidate selection (ModeEnvSelectDesc; the formula and the rule: include/mode_hip.h).  One workgroup of four waves per replanning row j.  The
// previous plan's tail - the L * A floats from row `shift` on, at most 16 KB - is staged in LDS once; the waves take the N candidates round-robin,
// a wave's lanes run the L * A elements coalesced and add their partial sums by shuffles; thread 0 takes the argmin of the <= 64 scores; then
// every thread copies the winner's W * A floats.  At most N * 16 KB read per row: latency-bound, plain loops.
// The coherence scores of a row's first n candidates against the staged tail, by the four waves of the workgroup (both selection kernels)
__device__ __forceinline__ void env_coherence_scores(const float* __restrict__ cands, const int n, const int WA, const int LA, const int A,
                                                     const float* __restrict__ weights, const float* tail, const bool has_prev, float* score) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int c = wave; c < n; c += 4) {
    float acc = 0.f;
    if (has_prev) {
      const float* x = cands + (long)c * WA;
      for (int e = lane; e < LA; e += 64) {
        const float df = x[e] - tail[e];
        acc = fmaf(weights[e / A], df * df, acc);
      }
      for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    }
    if (lane == 0) score[c] = acc;
  }
}

// The rule on n scores (one thread): the smallest, strictly - the lowest index wins ties; a NaN only loses; all NaN -> 0
__device__ __forceinline__ int env_select_min(const float* score, const int n) {
  int best = 0;
  float bs = score[0];
  for (int c = 1; c < n; ++c) {
    const float v = score[c];
    if (v < bs || (bs != bs && v == v)) { best = c; bs = v; }
  }
  return best;
}

__global__ __launch_bounds__(256) void env_select_kernel(ModeEnvSelectDesc d) {
  __shared__ float tail[4096];
  __shared__ float score[64];
  __shared__ int winner;
  const int j = blockIdx.x, tid = threadIdx.x;
  const int r = d.rows[j];
  if (r < 0 || r >= d.num_envs || (d.count && j >= d.count[0])) return;          // (uniform over the workgroup)
  const int N = d.N, WA = d.W * d.A, LA = (d.W - d.shift) * d.A;
  const bool has_prev = env_bit(d.has_prev[r >> 5], r);
  const float* prev = d.plan + (long)r * WA + d.shift * d.A;
  for (int e = tid; e < LA; e += 256) tail[e] = prev[e];
  __syncthreads();
  env_coherence_scores(d.chunk + (long)j * N * WA, N, WA, LA, d.A, d.weights, tail, has_prev, score);
  __syncthreads();
  if (tid == 0) {
    const int best = env_select_min(score, N);
    winner = best;
    d.selected[r] = best;
  }
  if (tid < N) d.scores[(long)r * N + tid] = score[tid];
  __syncthreads();
  const float* src = d.chunk + ((long)j * N + winner) * WA;
  float* dst = d.chosen + (long)j * WA;
  for (int e = tid; e < WA; e += 256) dst[e] = src[e];
}

// Unweighted squared distance of two whole chunk rows by one wave (every lane returns the sum): the lane owns elements 64 apart, the partial
// sums are added in the order of the coherence score
__device__ __forceinline__ float env_row_distance(const float* __restrict__ x, const float* __restrict__ y, const int WA, const int lane) {
  float acc = 0.f;
  for (int e = lane; e < WA; e += 64) {
    const float df = x[e] - y[e];
    acc = fmaf(df, df, acc);
  }
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  return acc;
}

// Selection with forward contrast (ModeEnvBidDesc; the formulas and the rule: include/mode_hip.h).  The workgroup of env_select_kernel per
// replanning row j, in four steps with a barrier between them: the coherence scores bc of the N + M candidates (the function above, the tail in
// LDS); thread c ranks candidate c within its kind - <= 63 compares on the LDS scores - and the first Ks / Kw ranks enter S+ / S-; the waves
// take the N strong candidates round-robin and add, in rank order, the distances to S+ and to S- (Ks + Kw wave-wide passes over two rows read
// from global memory: a chunk is L2-resident, and no row is staged); thread 0 takes the argmin of total.  Nothing is added across waves and no
// atomic is used, so the bits depend on the shape alone.
__global__ __launch_bounds__(256) void env_select_bid_kernel(ModeEnvBidDesc d) {
  __shared__ float tail[4096];
  __shared__ float bc[64], total[64];
  __shared__ int sp[64], sn[64];
  __shared__ int winner;
  const int j = blockIdx.x, tid = threadIdx.x;
  const int r = d.rows[j];
  if (r < 0 || r >= d.num_envs || (d.count && j >= d.count[0])) return;          // (uniform over the workgroup)
  const int N = d.N, NT = d.N + d.M, WA = d.W * d.A, LA = (d.W - d.shift) * d.A;
  const int Ks = min(d.K, N), Kw = min(d.K, d.M);
  const bool has_prev = env_bit(d.has_prev[r >> 5], r);
  const float* prev = d.plan + (long)r * WA + d.shift * d.A;
  const float* cands = d.chunk + (long)j * NT * WA;
  for (int e = tid; e < LA; e += 256) tail[e] = prev[e];
  __syncthreads();
  env_coherence_scores(cands, NT, WA, LA, d.A, d.weights, tail, has_prev, bc);
  __syncthreads();
  if (tid < NT) {
    const bool strong = tid < N;
    const int lo = strong ? 0 : N, hi = strong ? N : NT;
    const float v = bc[tid];
    int rank = 0;
    for (int c = lo; c < hi; ++c) {
      const float u = bc[c];
      // u ranks before v: smaller; equal (or both NaN) and of the lower index; any number before a NaN
      const bool before = (u < v) || (c < tid && (u == v || (u != u && v != v))) || (u == u && v != v);
      rank += before ? 1 : 0;
    }
    if (strong) { if (rank < Ks) sp[rank] = tid; }
    else if (rank < Kw) sn[rank] = tid;
    d.bc[(long)r * NT + tid] = v;
  }
  __syncthreads();
  const float lambda = d.lambda[0];
  const int wave = tid >> 6, lane = tid & 63;
  for (int c = wave; c < N; c += 4) {
    const float* x = cands + (long)c * WA;
    float pos = 0.f, neg = 0.f;
    for (int k = 0; k < Ks; ++k) pos += env_row_distance(x, cands + (long)sp[k] * WA, WA, lane);
    for (int k = 0; k < Kw; ++k) neg += env_row_distance(x, cands + (long)sn[k] * WA, WA, lane);
    if (lane == 0) {
      const float f = __fdiv_rn(pos, (float)Ks) - __fdiv_rn(neg, (float)Kw);
      const float t = fmaf(lambda, f, bc[c]);
      total[c] = t;
      d.fc[(long)r * N + c] = f;
      d.scores[(long)r * N + c] = t;
    }
  }
  __syncthreads();
  if (tid == 0) {
    const int best = env_select_min(total, N);
    winner = best;
    d.selected[r] = best;
  }
  __syncthreads();
  const float* src = cands + (long)winner * WA;
  float* dst = d.chosen + (long)j * WA;
  for (int e = tid; e < WA; e += 256) dst[e] = src[e];
}

}  // namespace mode

using namespace mode;

// N strong + M weak candidates per environment (M = 0: the _cand gathers)
static int env_gather_noise_launch(const int32_t* rows, int m_b, int num_envs, const uint32_t* seeds, const uint32_t* draws, const float* state_images,
                                   int64_t img_floats, const float* goals, int64_t goal_floats, float* img_out, float* goal_out, float* x0,
                                   int noise_floats, float sigma_max, int N, int M, void* stream) {
  if (!rows || !seeds || !draws || !x0 || m_b <= 0 || num_envs <= 0 || noise_floats <= 0 || img_floats < 0 || goal_floats < 0) return MODE_ERR_BAD_ARG;
  if (N < 1 || N > 64 || M < 0 || M > 64 - N) return MODE_ERR_BAD_ARG;
  hipLaunchKernelGGL(env_gather_noise_kernel, dim3(m_b, N + M), dim3(256), 0, (hipStream_t)stream, rows, num_envs, seeds, draws, state_images,
                     (long)img_floats, goals, (long)goal_floats, img_out, goal_out, x0, noise_floats, sigma_max, N);
  MODE_LAUNCH_CHECK();
  return MODE_OK;
}

extern "C" int mode_env_gather_noise_cand(const int32_t* rows, int m_b, int num_envs, const uint32_t* seeds, const uint32_t* draws,
                                          const float* state_images, int64_t img_floats, const float* goals, int64_t goal_floats,
                                          float* img_out, float* goal_out, float* x0, int noise_floats, float sigma_max, int N, void* stream) {
  return env_gather_noise_launch(rows, m_b, num_envs, seeds, draws, state_images, img_floats, goals, goal_floats, img_out, goal_out, x0, noise_floats,
                                 sigma_max, N, 0, stream);
}

extern "C" int mode_env_gather_noise_bid(const int32_t* rows, int m_b, int num_envs, const uint32_t* seeds, const uint32_t* draws,
                                         const float* state_images, int64_t img_floats, const float* goals, int64_t goal_floats,
                                         float* img_out, float* goal_out, float* x0, int noise_floats, float sigma_max, int N, int M, void* stream) {
  if (M < 1) return MODE_ERR_BAD_ARG;
  return env_gather_noise_launch(rows, m_b, num_envs, seeds, draws, state_images, img_floats, goals, goal_floats, img_out, goal_out, x0, noise_floats,
                                 sigma_max, N, M, stream);
}

extern "C" int mode_env_gather_noise(const int32_t* rows, int m_b, int num_envs, const uint32_t* seeds, const uint32_t* draws,
                                     const float* state_images, int64_t img_floats, const float* goals, int64_t goal_floats,
                                     float* img_out, float* goal_out, float* x0, int noise_floats, float sigma_max, void* stream) {
  return mode_env_gather_noise_cand(rows, m_b, num_envs, seeds, draws, state_images, img_floats, goals, goal_floats, img_out, goal_out, x0, noise_floats,
                                    sigma_max, 1, stream);
}

static int env_gather_warm_launch(const int32_t* rows, int m_b, int num_envs, const uint32_t* seeds, const uint32_t* draws, const float* state_images,
                                  int64_t img_floats, const float* goals, int64_t goal_floats, float* img_out, float* goal_out, float* x0,
                                  const float* plan, int W, int A, int shift, float sigma_start, int N, int M, void* stream) {
  if (!rows || !seeds || !draws || !x0 || !plan || m_b <= 0 || num_envs <= 0 || img_floats < 0 || goal_floats < 0) return MODE_ERR_BAD_ARG;
  if (W <= 0 || A <= 0 || (long)W * A > 4096 || shift < 1 || shift >= W || !(sigma_start >= 0.f) || !(sigma_start <= FLT_MAX)) return MODE_ERR_BAD_ARG;
  if (N < 1 || N > 64 || M < 0 || M > 64 - N) return MODE_ERR_BAD_ARG;
  hipLaunchKernelGGL(env_gather_warm_kernel, dim3(m_b, N + M), dim3(256), 0, (hipStream_t)stream, rows, num_envs, seeds, draws, state_images,
                     (long)img_floats, goals, (long)goal_floats, img_out, goal_out, x0, plan, W, A, shift, sigma_start, N);
  MODE_LAUNCH_CHECK();
  return MODE_OK;
}

extern "C" int mode_env_gather_warm_cand(const int32_t* rows, int m_b, int num_envs, const uint32_t* seeds, const uint32_t* draws,
                                         const float* state_images, int64_t img_floats, const float* goals, int64_t goal_floats,
                                         float* img_out, float* goal_out, float* x0, const float* plan, int W, int A, int shift, float sigma_start,
                                         int N, void* stream) {
  return env_gather_warm_launch(rows, m_b, num_envs, seeds, draws, state_images, img_floats, goals, goal_floats, img_out, goal_out, x0, plan, W, A, shift,
                                sigma_start, N, 0, stream);
}

extern "C" int mode_env_gather_warm_bid(const int32_t* rows, int m_b, int num_envs, const uint32_t* seeds, const uint32_t* draws,
                                        const float* state_images, int64_t img_floats, const float* goals, int64_t goal_floats,
                                        float* img_out, float* goal_out, float* x0, const float* plan, int W, int A, int shift, float sigma_start,
                                        int N, int M, void* stream) {
  if (M < 1) return MODE_ERR_BAD_ARG;
  return env_gather_warm_launch(rows, m_b, num_envs, seeds, draws, state_images, img_floats, goals, goal_floats, img_out, goal_out, x0, plan, W, A, shift,
                                sigma_start, N, M, stream);
}

extern "C" int mode_env_gather_warm(const int32_t* rows, int m_b, int num_envs, const uint32_t* seeds, const uint32_t* draws,
                                    const float* state_images, int64_t img_floats, const float* goals, int64_t goal_floats,
                                    float* img_out, float* goal_out, float* x0, const float* plan, int W, int A, int shift, float sigma_start,
                                    void* stream) {
  return mode_env_gather_warm_cand(rows, m_b, num_envs, seeds, draws, state_images, img_floats, goals, goal_floats, img_out, goal_out, x0, plan, W, A,
                                   shift, sigma_start, 1, stream);
}

// What both selection descriptors (D) share: the pointers every selection needs and the geometry
template <class D>
static bool env_select_desc_ok(const D* d) {
  return d && d->rows && d->has_prev && d->chunk && d->plan && d->weights && d->chosen && d->selected && d->scores && d->N >= 1 && d->N <= 64 &&
         d->W > 0 && d->A > 0 && (long)d->W * d->A <= 4096 && d->shift >= 1 && d->shift < d->W && d->m_b > 0 && d->num_envs > 0;
}

extern "C" int mode_env_select(const ModeEnvSelectDesc* d, void* stream) {
  if (!env_select_desc_ok(d)) return MODE_ERR_BAD_ARG;
  hipLaunchKernelGGL(env_select_kernel, dim3(d->m_b), dim3(256), 0, (hipStream_t)stream, *d);
  MODE_LAUNCH_CHECK();
  return MODE_OK;
}

extern "C" int mode_env_select_bid(const ModeEnvBidDesc* d, void* stream) {
  if (!env_select_desc_ok(d) || !d->lambda || !d->bc || !d->fc || d->M < 1 || d->M > 64 - d->N || d->K < 1) return MODE_ERR_BAD_ARG;
  hipLaunchKernelGGL(env_select_bid_kernel, dim3(d->m_b), dim3(256), 0, (hipStream_t)stream, *d);
  MODE_LAUNCH_CHECK();
  return MODE_OK;
}

// The pool descriptor of both commit exports: geometry, state pointers, and the chunk (control-block form) or the output (descriptor form)
static bool env_pool_desc_ok(const ModeEnvPoolDesc* d) {
  return d->num_envs > 0 && d->num_envs <= MODE_ENV_MAX && d->W > 0 && d->A > 0 && d->A <= 64 && d->W * d->A <= 4096 && d->multistep > 0 &&
         d->multistep <= d->W && d->plan && d->counter && d->draws && (d->ctrl ? d->chunk != nullptr : d->out != nullptr);
}

extern "C" int mode_env_commit_emit(const ModeEnvPoolDesc* d, void* stream) {
  if (!d || !env_pool_desc_ok(d)) return MODE_ERR_BAD_ARG;
  hipLaunchKernelGGL(env_commit_emit_kernel, dim3(d->num_envs), dim3(64), 0, (hipStream_t)stream, *d);
  MODE_LAUNCH_CHECK();
  return MODE_OK;
}

extern "C" int mode_env_commit_emit_ens(const ModeEnvEnsDesc* e, void* stream) {
  if (!e || !env_pool_desc_ok(&e->pool)) return MODE_ERR_BAD_ARG;
  const ModeEnvPoolDesc* d = &e->pool;
  if (!e->ring || !e->birth || !e->t || !e->weights || e->K < 1 || e->K > 64 || e->K != (d->W + d->multistep - 1) / d->multistep) return MODE_ERR_BAD_ARG;
  hipLaunchKernelGGL(env_commit_emit_ens_kernel, dim3(d->num_envs), dim3(64), 0, (hipStream_t)stream, *e);
  MODE_LAUNCH_CHECK();
  return MODE_OK;
}

extern "C" int mode_env_gather_frames(const ModeEnvFramesDesc* d, void* stream) {
  if (!d || !d->rows || d->m_b <= 0 || d->m_b > 65535 || d->num_envs <= 0) return MODE_ERR_BAD_ARG;
  long most = 0;
  for (int k = 0; k < 2; ++k) {
    const ModeEnvFramesCam& c = d->cam[k];
    if (!c.src && !c.dst) continue;
    if (!c.src || !c.dst || c.row_elems <= 0 || c.src_stride < c.row_elems) return MODE_ERR_BAD_ARG;
    const bool ok = (c.src_dtype == MODE_F32 && (c.dst_dtype == MODE_F32 || c.dst_dtype == MODE_BF16)) ||
                    (c.src_dtype == MODE_BF16 && c.dst_dtype == MODE_BF16);
    if (!ok) return MODE_ERR_UNSUPPORTED;
    const int so = c.src_dtype == MODE_F32 ? 4 : 2, dso = c.dst_dtype == MODE_F32 ? 4 : 2;
    if (((uintptr_t)c.src % so) || ((uintptr_t)c.dst % dso)) return MODE_ERR_BAD_ARG;
    most = c.row_elems > most ? c.row_elems : most;
  }
  if (most == 0) return MODE_ERR_BAD_ARG;
  // up to 4 iterations of 8 elements per thread: ~74 workgroups per 224 x 224 fp32 frame row and camera
  const long bx = (most + 8L * 256 * 4 - 1) / (8L * 256 * 4);
  hipLaunchKernelGGL(env_gather_frames_kernel, dim3((unsigned)bx, d->m_b, 2), dim3(256), 0, (hipStream_t)stream, *d);
  MODE_LAUNCH_CHECK();
  return MODE_OK;
}
