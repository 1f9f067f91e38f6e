// Camera frames as the camera delivers them -> the perceptual encoders' input (include/mode_hip.h: mode_frames_preprocess; camera.CameraTransform,
// rollout.VectorEnvPolicy(camera_transforms=...)): uint8 HWC frames are resized with the antialiased triangle filter, quantised to uint8 levels,
// shifted by an integer crop of the edge-replicated image, scaled, normalised and stored as NCHW fp32 / bf16 - one launch for both cameras, and
// with `rows` also the gather of the replanning environments' rows that mode_env_gather_frames does for float frames.
//
// grid (row bands, m_b * T frames, 2 cameras), 256 threads.  A workgroup owns RB output rows of one frame: it computes the filter tables of the
// frame's columns and of its own rows (exact integer weights, one division each), copies the source rows of its vertical footprint - one contiguous
// byte span of the HWC frame - into LDS with 16-byte loads (element loads up to the first and after the last 16-byte boundary), filters them
// horizontally into an fp32 LDS image [rows][3][OW], then filters vertically, quantises, normalises and stores x-fastest per channel plane,
// 16 bytes per lane where the destination rows are 16-byte aligned.  Bandwidth- and latency-bound: no MFMA, no inline asm, <= 64 KiB of LDS.
#include <vector>

#include "mode_common.h"

namespace mode {

constexpr size_t kFramePrepLdsMax = 64 * 1024;      // the convention of rowops.hip's kWaveRowLdsMax: no large-LDS attribute
constexpr int kFramePrepMaxDim = 16384;             // keeps every integer of the filter tables below 2^31

// Taps [lo, hi) of output index o on an axis resized in -> out, the filter of include/mode_hip.h in exact integers: with S = max(in, out) and
// cn = in (2 o + 1) (= 2 out center), lo = max(0, floor((cn - 2 S + out) / (2 out))), hi = min(in, floor((cn + 2 S + out) / (2 out))).
__host__ __device__ inline void prep_taps(int in, int out, int o, int& lo, int& hi) {
  const long long S = in > out ? in : out, cn = (long long)in * (2 * o + 1), two_out = 2LL * out;
  const long long nlo = cn - 2 * S + out, nhi = (cn + 2 * S + out) / two_out;
  lo = nlo < 0 ? 0 : (int)(nlo / two_out);
  hi = nhi > in ? in : (int)nhi;
}
// The unnormalised weight of source index p for output index o, times 2 S: max(0, 2 S - |(2 p + 1) out - cn|), an integer.
__device__ __forceinline__ long long prep_weight_num(int in, int out, int o, int p) {
  const long long S = in > out ? in : out, cn = (long long)in * (2 * o + 1);
  long long d = (long long)(2 * p + 1) * out - cn;
  d = d < 0 ? -d : d;
  return 2 * S - d > 0 ? 2 * S - d : 0;
}

struct PrepCam {
  const unsigned char* src; long src_stride;
  char* dst;
  const int32_t* shifts;
  int T, H, W, OH, OW, pad, dst_dtype;
  float m0, m1, m2, s0, s1, s2;
  int RB, KX, KY, NSRC;      // rows per band; widest horizontal / vertical filter; most source rows under a band
};
struct PrepArgs {
  const int32_t* rows;
  int m_b, num_envs;
  PrepCam cam[2];
};

__host__ __device__ inline size_t prep_raw_bytes(const PrepCam& c) { return ((size_t)c.NSRC * c.W * 3 + 16 + 15) & ~(size_t)15; }
__host__ __device__ inline size_t prep_lds_bytes(const PrepCam& c) {
  return prep_raw_bytes(c) + 4 * ((size_t)c.NSRC * 3 * c.OW + (size_t)c.OW * (1 + c.KX) + (size_t)c.RB * (1 + c.KY));
}

// Filter table of outputs [o0, o0 + n) of one axis: first[i] = lo, w[k * n + i] = weight of tap lo + k (0 past the last tap).
__device__ __forceinline__ void prep_table(int in, int out, int o0, int n, int K, int* first, float* w) {
  for (int i = threadIdx.x; i < n; i += 256) {
    int lo, hi;
    prep_taps(in, out, o0 + i, lo, hi);
    long long sum = 0;
    for (int p = lo; p < hi; ++p) sum += prep_weight_num(in, out, o0 + i, p);
    const float fs = (float)sum;
    first[i] = lo;
    for (int k = 0; k < K; ++k) w[k * n + i] = lo + k < hi ? __fdiv_rn((float)prep_weight_num(in, out, o0 + i, lo + k), fs) : 0.f;
  }
}

__global__ __launch_bounds__(256) void frames_preprocess_kernel(PrepArgs a) {
  extern __shared__ __align__(16) unsigned char prep_smem[];
  const PrepCam c = blockIdx.z == 0 ? a.cam[0] : a.cam[1];          // (no dynamic index into the argument block)
  if (!c.src) return;
  const int fr = blockIdx.y;
  if (fr >= a.m_b * c.T) return;
  const int j = fr / c.T, t = fr - j * c.T;
  const int r = a.rows ? a.rows[j] : j;
  if (r < 0 || r >= a.num_envs) return;
  const int y0 = blockIdx.x * c.RB;
  if (y0 >= c.OH) return;
  const int ny = min(c.RB, c.OH - y0), OW = c.OW, OH = c.OH, W = c.W;
  // the frame's shift, clamped into [0, 2 pad] before it is used: out[y][x] = L[clamp(y + sy)][clamp(x + sx)] with sx, sy in [-pad, pad]
  int sx = 0, sy = 0;
  if (c.shifts) {
    sx = min(max(c.shifts[2 * fr], 0), 2 * c.pad) - c.pad;
    sy = min(max(c.shifts[2 * fr + 1], 0), 2 * c.pad) - c.pad;
  }
  // rows of the quantised image L this band reads: ly0 .. ly1 (at most RB), and their source rows fy0 .. fy1 - 1 (at most NSRC)
  const int ly0 = min(max(y0 + sy, 0), OH - 1), ly1 = min(max(y0 + ny - 1 + sy, 0), OH - 1), nl = ly1 - ly0 + 1;
  int fy0, fy1, tmp;
  prep_taps(c.H, OH, ly0, fy0, tmp);
  prep_taps(c.H, OH, ly1, tmp, fy1);
  const int nsrc = fy1 - fy0;

  unsigned char* raw_base = prep_smem;
  float* hf = reinterpret_cast<float*>(prep_smem + prep_raw_bytes(c));          // [nsrc][3][OW]
  int* xfirst = reinterpret_cast<int*>(hf + (size_t)c.NSRC * 3 * OW);           // [OW]
  float* wx = reinterpret_cast<float*>(xfirst + OW);                            // [KX][OW]
  int* yfirst = reinterpret_cast<int*>(wx + (size_t)c.KX * OW);                 // [nl]
  float* wy = reinterpret_cast<float*>(yfirst + c.RB);                          // [KY][nl]

  prep_table(W, OW, 0, OW, c.KX, xfirst, wx);
  prep_table(c.H, OH, ly0, nl, c.KY, yfirst, wy);

  // the footprint's bytes -> LDS at the same offset modulo 16, so that the 16-byte body is aligned on both sides
  const unsigned char* g = c.src + (long)r * c.src_stride + ((long)t * c.H + fy0) * W * 3;
  const int len = nsrc * W * 3, a_off = (int)((uintptr_t)g & 15);
  unsigned char* raw = raw_base + a_off;
  const int head = min((16 - a_off) & 15, len), body = (len - head) >> 4;
  for (int i = threadIdx.x; i < head; i += 256) raw[i] = g[i];
  {
    const uint4* g4 = reinterpret_cast<const uint4*>(g + head);
    uint4* l4 = reinterpret_cast<uint4*>(raw + head);
    for (int i = threadIdx.x; i < body; i += 256) l4[i] = g4[i];
  }
  for (int i = head + (body << 4) + threadIdx.x; i < len; i += 256) raw[i] = g[i];
  __syncthreads();

  // horizontal pass: every L column of every footprint row, the three channels of a pixel per thread
  for (int it = threadIdx.x; it < nsrc * OW; it += 256) {
    const int sr = it / OW, ox = it - sr * OW;
    const unsigned char* row = raw + (size_t)sr * W * 3;
    const int x0 = xfirst[ox];
    float r0 = 0.f, r1 = 0.f, r2 = 0.f;
    for (int k = 0; k < c.KX; ++k) {
      const float w = wx[k * OW + ox];
      const unsigned char* px = row + min(x0 + k, W - 1) * 3;       // (taps past the filter's last carry weight 0)
      r0 = __builtin_fmaf(w, (float)px[0], r0);
      r1 = __builtin_fmaf(w, (float)px[1], r1);
      r2 = __builtin_fmaf(w, (float)px[2], r2);
    }
    float* o = hf + (size_t)sr * 3 * OW + ox;
    o[0] = r0; o[OW] = r1; o[2 * OW] = r2;
  }
  __syncthreads();

  // vertical pass, quantisation, shift, normalisation, store
  const int esz = c.dst_dtype == MODE_F32 ? 4 : 2;
  char* dst = c.dst + (long)fr * 3 * OH * OW * esz;
  const int V = 16 / esz;                                            // elements of a 16-byte store
  const bool vec = (((uintptr_t)dst & 15) == 0) && (OW % V == 0);
  const int G = vec ? OW / V : OW, nv = vec ? V : 1;
  for (int it = threadIdx.x; it < ny * 3 * G; it += 256) {
    const int yc = it / G, gx = it - yc * G, yy = yc / 3, ch = yc - yy * 3;
    const int y = y0 + yy, li = min(max(y + sy, 0), OH - 1) - ly0;
    const int yb = yfirst[li] - fy0;
    const float mean = ch == 0 ? c.m0 : (ch == 1 ? c.m1 : c.m2), istd = ch == 0 ? c.s0 : (ch == 1 ? c.s1 : c.s2);
    const float* plane = hf + (size_t)ch * OW;
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = 0.f;
    for (int k = 0; k < c.KY; ++k) {
      const float w = wy[k * nl + li];
      const float* hrow = plane + (size_t)min(yb + k, nsrc - 1) * 3 * OW;
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (e < nv) v[e] = __builtin_fmaf(w, hrow[min(max(gx * nv + e + sx, 0), OW - 1)], v[e]);
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float lvl = fminf(fmaxf(rintf(v[e]), 0.f), 255.f);
      v[e] = __fmul_rn(__fsub_rn(__fmul_rn(lvl, 1.0f / 255.0f), mean), istd);
    }
    char* p = dst + ((long)(ch * OH + y) * OW + (long)gx * nv) * esz;
    if (vec) {
      if (esz == 4) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
      else *reinterpret_cast<uint4*>(p) = make_uint4(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]), pack_bf16x2(v[6], v[7]));
    } else if (esz == 4) {
      *reinterpret_cast<float*>(p) = v[0];
    } else {
      *reinterpret_cast<uint16_t*>(p) = f32_to_bf16_bits(v[0]);
    }
  }
}

// Host: the band height and the table sizes of one camera.  false = not even RB = 1 fits the LDS budget.
static bool prep_plan(PrepCam& c) {
  std::vector<int> ylo(c.OH), yhi(c.OH);
  int lo, hi;
  c.KX = c.KY = 1;
  for (int o = 0; o < c.OW; ++o) { prep_taps(c.W, c.OW, o, lo, hi); c.KX = hi - lo > c.KX ? hi - lo : c.KX; }
  for (int o = 0; o < c.OH; ++o) { prep_taps(c.H, c.OH, o, ylo[o], yhi[o]); c.KY = yhi[o] - ylo[o] > c.KY ? yhi[o] - ylo[o] : c.KY; }
  for (int rb = 8; rb >= 1; rb >>= 1) {
    c.RB = rb; c.NSRC = 1;
    for (int o = 0; o < c.OH; ++o) {
      const int last = o + rb - 1 < c.OH ? o + rb - 1 : c.OH - 1;
      c.NSRC = yhi[last] - ylo[o] > c.NSRC ? yhi[last] - ylo[o] : c.NSRC;
    }
    if (prep_lds_bytes(c) <= kFramePrepLdsMax) return true;
  }
  return false;
}

}  // namespace mode

using namespace mode;

extern "C" int mode_frames_preprocess(const ModeFramePrepDesc* d, void* stream) {
  if (!d || d->m_b <= 0 || d->m_b > 65535 || d->num_envs <= 0) return MODE_ERR_BAD_ARG;
  if (!d->rows && d->m_b > d->num_envs) return MODE_ERR_BAD_ARG;
  PrepArgs a;
  a.rows = d->rows; a.m_b = d->m_b; a.num_envs = d->num_envs;
  int cams = 0;
  for (int k = 0; k < 2; ++k) {
    const ModeFramePrepCam& s = d->cam[k];
    PrepCam& c = a.cam[k];
    c = PrepCam{};
    if (!s.src && !s.dst) continue;
    if (!s.src || !s.dst || s.T <= 0 || s.H <= 0 || s.W <= 0 || s.OH <= 0 || s.OW <= 0 || s.pad < 0) return MODE_ERR_BAD_ARG;
    if (s.src_stride < (int64_t)s.T * s.H * s.W * 3) return MODE_ERR_BAD_ARG;
    for (int i = 0; i < 3; ++i)
      if (!(s.inv_std[i] == s.inv_std[i]) || !(s.mean[i] == s.mean[i])) return MODE_ERR_BAD_ARG;
    ++cams;
  }
  if (!cams) return MODE_ERR_BAD_ARG;
  unsigned bands = 0, frames = 0;
  size_t lds = 0;
  for (int k = 0; k < 2; ++k) {
    const ModeFramePrepCam& s = d->cam[k];
    PrepCam& c = a.cam[k];
    if (!s.src) continue;
    if (s.dst_dtype != MODE_F32 && s.dst_dtype != MODE_BF16) return MODE_ERR_UNSUPPORTED;
    if ((uintptr_t)s.dst % (s.dst_dtype == MODE_F32 ? 4 : 2) || (s.shifts && (uintptr_t)s.shifts % 4)) return MODE_ERR_BAD_ARG;
    if (s.H > 8LL * s.OH || s.W > 8LL * s.OW) return MODE_ERR_UNSUPPORTED;
    if (s.H > kFramePrepMaxDim || s.W > kFramePrepMaxDim || s.OH > kFramePrepMaxDim || s.OW > kFramePrepMaxDim || s.pad > kFramePrepMaxDim ||
        (int64_t)d->m_b * s.T > 65535)
      return MODE_ERR_UNSUPPORTED;
    c.src = static_cast<const unsigned char*>(s.src); c.src_stride = (long)s.src_stride;
    c.dst = static_cast<char*>(s.dst); c.shifts = s.shifts;
    c.T = s.T; c.H = s.H; c.W = s.W; c.OH = s.OH; c.OW = s.OW; c.pad = s.pad; c.dst_dtype = s.dst_dtype;
    c.m0 = s.mean[0]; c.m1 = s.mean[1]; c.m2 = s.mean[2];
    c.s0 = s.inv_std[0]; c.s1 = s.inv_std[1]; c.s2 = s.inv_std[2];
    if (!prep_plan(c)) return MODE_ERR_UNSUPPORTED;
    const unsigned nb = (unsigned)((c.OH + c.RB - 1) / c.RB), nf = (unsigned)(d->m_b * c.T);
    bands = nb > bands ? nb : bands;
    frames = nf > frames ? nf : frames;
    lds = prep_lds_bytes(c) > lds ? prep_lds_bytes(c) : lds;
  }
  hipLaunchKernelGGL(frames_preprocess_kernel, dim3(bands, frames, 2), dim3(256), lds, (hipStream_t)stream, a);
  MODE_LAUNCH_CHECK();
  return MODE_OK;
}
