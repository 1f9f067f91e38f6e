// The hand-scheduled primitives of the GEMM family (ring, ping-pong, transpose-read, convolution, fused QKV kernels): LDS reads and waits the
// compiler does not track.  Its own scoreboard puts `s_waitcnt lgkmcnt(0)` in front of the first MFMA that uses a compiler-visible LDS read,
// and `s_waitcnt vmcnt(0)` - i.e. a wait for the just-issued LDS-DMA of the NEXT tile - in front of the read itself.  Hidden in `asm volatile`,
// the MFMA operands are requested with hand-counted lgkmcnt waits (+ sched_barriers at the call sites), so the second k32 half's LDS round trip
// stays in flight under the first half's MFMAs.  The "memory" clobber is what orders these reads and waits against the DMA, the barriers and
// each other: the counted schedules of every kernel that includes this header depend on these six lines.
#pragma once
#include "mode_common.h"

namespace mode {

typedef short s16x4 __attribute__((ext_vector_type(4)));

template <int N>
__device__ __forceinline__ void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
template <int N>
__device__ __forceinline__ void wait_lgkmcnt() { asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(N) : "memory"); }

template <int OFF>
__device__ __forceinline__ void lds_read128(bf16x8& dst, uint32_t addr) {
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(OFF) : "memory");
}
// dst[i] = 16 bytes at addr + BASE + i * STRIDE, i = 0 .. CNT-1 (unrolled: the offsets are immediates)
template <int STRIDE, int CNT, int BASE = 0, int I = 0>
__device__ __forceinline__ void lds_read_seq(bf16x8* dst, uint32_t addr) {
  if constexpr (I < CNT) {
    lds_read128<BASE + I * STRIDE>(dst[I], addr);
    lds_read_seq<STRIDE, CNT, BASE, I + 1>(dst, addr);
  }
}
// transpose read of a [k][n] image; join8(lo, hi) of two of them is one MFMA operand
template <int OFF>
__device__ __forceinline__ void lds_tr64(s16x4& dst, uint32_t addr) {
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(OFF) : "memory");
}
__device__ __forceinline__ bf16x8 join8(s16x4 lo, s16x4 hi) {
  typedef short s16x8 __attribute__((ext_vector_type(8)));
  const s16x8 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_bit_cast(bf16x8, v);
}

}  // namespace mode
