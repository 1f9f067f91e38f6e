#pragma once
#include "gemm_tile.h"

namespace mode {

// What only the two persistent ping-pong kernels share (gemm_bf16_pp.hip, gemm_bf16_pptr.hip; include it in nothing else: the PP_* macros at the
// end are not scoped).  A K-step's operand tile lives in LDS as four 16-KiB HALF-tiles (A halves 0 / 1, W halves 0 / 1), two K-steps
// resident: A[t][h] at (t*2+h) * 16 KiB, W[t][h] 64 KiB further.  Each kernel adds its own LDS_TOTAL (and gemm_bf16_pp.hip its bias / norm regions).
namespace ppc {
constexpr int BKK = 64;
constexpr int HALF_BYTES = 128 * BKK * 2;                  // one half-tile (128 rows x 64 k, or 64 k x 128 columns): 16 KiB
constexpr int LDS_A = 0;                                   // A[t][h] at (t*2+h) * 16 KiB
constexpr int LDS_B = 4 * HALF_BYTES;                      // W[t][h] at 64 KiB + (t*2+h) * 16 KiB
constexpr int GM = 8;                                      // m-tiles per rasterisation band
template <int V>
using IC = std::integral_constant<int, V>;

// banded tile order: linear tile l -> (m-tile, n-tile, K-slice); bands of GM m-tiles, slice-major inside a band, runs of RN n-tiles per m-tile
// (XCD-aware: an XCD's workgroups cover GM m-tiles x a few n-tiles, so its L2 sees each operand K-slice once)
__device__ __forceinline__ void band_tile(int l, int n_tiles, int S, int RN, int m_real, int& m, int& n, int& slice) {
  const int per_band = GM * n_tiles * S;
  const int band = l / per_band, first_m = band * GM;
  const int gsz = min(GM, m_real - first_m);
  const int rem = l - band * per_band;
  const int per_slice = gsz * n_tiles;
  slice = rem / per_slice;
  const int q = rem - slice * per_slice;
  const int run = gsz * RN;
  const int n_hi = q / run, r2 = q - n_hi * run;
  m = first_m + r2 / RN;
  n = n_hi * RN + r2 % RN;
}

// DMA of half-tile (operand OP, K-step buffer T, half H): 16 1-KiB pieces, wave w fills pieces 2w and 2w+1 from the uniform base g + this lane's offsets
template <int OP, int T, int H>
__device__ __forceinline__ void stage_half(char* smem, int wave, const char* g, uint32_t o0, uint32_t o1) {
  constexpr int base = (OP ? LDS_B : LDS_A) + (T * 2 + H) * HALF_BYTES;
  dma16(g + o0, smem + base + (wave * 2 + 0) * 1024);
  dma16(g + o1, smem + base + (wave * 2 + 1) * 1024);
}
}  // namespace ppc

}  // namespace mode

// One MFMA segment of a phase: A half AH x both W halves between two barriers.  Expands INSIDE the kernel and names three of its locals: the `mma`
// lambda and the IC<0> / IC<1> tags `_0`, `_1`.  Each kernel file #undefs the three macros at its end.
#define PP_SB() __builtin_amdgcn_sched_barrier(0)
#define PP_BAR() __builtin_amdgcn_s_barrier()
#define PP_COMPUTE2(AH)           \
  PP_BAR();                       \
  wait_lgkmcnt<0>();              \
  PP_SB();                        \
  __builtin_amdgcn_s_setprio(1);  \
  mma(AH, _0);                    \
  mma(AH, _1);                    \
  __builtin_amdgcn_s_setprio(0);  \
  PP_SB();                        \
  PP_BAR();                       \
  PP_SB();
