// Weight run-ahead: a kernel that is already running pulls the weight matrices of the kernels BEHIND it from HBM into the Infinity Cache with
// loads whose data nobody uses, so that the consumer's operand stream hits the cache instead of cold HBM (LABNOTES.md, "weight run-ahead";
// profiles/weight_runahead.txt).  No value changes: every output stays byte-identical.
//
// This header is the ONE place that decides which bytes are touched.  The mapping is plain integer arithmetic, compiles as host C++ without HIP
// (tests/test_runahead_plan.py runs it on the CPU) and is the same function the device half below calls.
//
// Plan.  A range of `bytes` bytes is cut into 128-byte lines (the cache-line size; offsets are relative to the range's base, which the callers
// keep 128-byte aligned so that they ARE cache lines).  `nwg` workgroups issue, each has `slots` touch slots, a slot is one wave instruction of 64
// lanes, one dword per lane:   line = (slot * nwg + wg) * 64 + lane,   offset = line * 128.
//   * a line is touched at most once (the map (slot, wg, lane) -> line is injective);
//   * every touched dword lies inside the range: offset + 4 <= bytes.  A trailing line that holds fewer than four bytes is therefore NOT a line of
//     the plan (a dword load there would read past the range) - ra_lines() counts the lines that hold a whole dword at their start;
//   * slots * 64 * nwg >= ra_lines(bytes)  =>  every line is touched exactly once; fewer slots touch a prefix of the range;
//   * bytes <= 0 (or a null base, refused by ra_range_ok) => nothing is touched.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MODE_RA_HD __host__ __device__ inline
#else
#define MODE_RA_HD inline
#endif

namespace mode {

constexpr int kRaLine = 128;        // bytes per touched line
constexpr int kRaLanes = 64;        // lanes of one touch instruction
constexpr int kRaMaxRanges = 2;     // ranges one launch can be handed
constexpr int kRaMaxSlots = 16;     // touch slots per workgroup and range the issuing kernels provide at most (two per wave of an 8-wave workgroup)

// The ranges one launch touches (kernel argument of an issuing kernel; all zero = no touch).
struct RaRanges {
  const char* ptr[kRaMaxRanges];
  long bytes[kRaMaxRanges];
};

// lines of the range that hold a whole dword at their start
MODE_RA_HD long ra_lines(long bytes) { return bytes >= 4 ? (bytes - 4) / kRaLine + 1 : 0; }

// first line of (workgroup wg of nwg, slot): the slot's 64 lanes touch lines [first, first + 64)
MODE_RA_HD long ra_slot_first_line(int nwg, int wg, int slot) { return ((long)slot * nwg + wg) * kRaLanes; }

// byte offset touched by (workgroup wg of nwg, slot of slots, lane), or -1 for "none"
MODE_RA_HD long ra_offset(long bytes, int nwg, int slots, int wg, int slot, int lane) {
  if (bytes < 4 || nwg <= 0 || slots <= 0 || wg < 0 || wg >= nwg || slot < 0 || slot >= slots || lane < 0 || lane >= kRaLanes) return -1;
  const long line = ra_slot_first_line(nwg, wg, slot) + lane;
  return line < ra_lines(bytes) ? line * kRaLine : -1;
}

// slots per workgroup that cover the range with nwg issuing workgroups, capped (a capped plan touches a prefix)
MODE_RA_HD int ra_slots(long bytes, int nwg, int max_slots) {
  if (nwg <= 0) return 0;
  const long per = (long)nwg * kRaLanes;
  const long s = (ra_lines(bytes) + per - 1) / per;
  return (int)(s < max_slots ? s : max_slots);
}

// host: a range an issuing launch accepts - non-null, dword-aligned, non-empty.  Anything else means "no touch" (never an error: a touch is a hint).
inline bool ra_range_ok(const void* p, long bytes) { return p != nullptr && bytes >= 4 && (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

// host: descriptor fields -> kernel argument (refused ranges become empty ones)
inline RaRanges ra_make(const void* p0, long b0, const void* p1, long b1) {
  RaRanges r;
  r.ptr[0] = ra_range_ok(p0, b0) ? static_cast<const char*>(p0) : nullptr; r.bytes[0] = r.ptr[0] ? b0 : 0;
  r.ptr[1] = ra_range_ok(p1, b1) ? static_cast<const char*>(p1) : nullptr; r.bytes[1] = r.ptr[1] ? b1 : 0;
  return r;
}

#if defined(__HIPCC__)
// Device half.  The load is a dword LDS-DMA into a landing strip nobody reads (256 bytes per wave: lane i lands at strip + 4 i).  A register
// destination that is never waited for is written whenever the data arrives, long after the compiler has reused the register
// (profiles/r05_pp_l2touch.txt: outputs differed); an LDS destination has no such hazard - the only obligation is that the workgroup does not end
// (and release its LDS) before the load has retired, which the issuing kernels' final `s_waitcnt vmcnt(0)` covers.  Counts in vmcnt like any load.
// The address is a wave-uniform base (the slot's first line: scalar registers) plus one 32-bit per-lane offset - ONE VGPR per touch.
__device__ __forceinline__ void ra_touch_dma(const char* slot_base, uint32_t lane_off, void* strip) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(slot_base + lane_off), (__attribute__((address_space(3))) void*)strip, 4, 0, 0);
}
// All ranges of `ra`, this wave's slots of the kRaMaxSlots-slot plan (a longer range is touched as a prefix): slot s of an even range is issued by
// wave s mod NWAVES, of an odd range by wave NWAVES - 1 - s mod NWAVES, so two short ranges load different waves.  wg / nwg: this workgroup's index
// among the nwg ISSUING workgroups of the launch (both wave-uniform).  strip: this wave's 256-byte landing strip.  Lane l of slot s issues exactly
// ra_offset(bytes, nwg, kRaMaxSlots, wg, s, l) = (ra_slot_first_line + l) * 128 when that line exists.  No division, scalars but for one VGPR, the lane
// index read off the hardware: the issuing kernels have no registers to spare.
template <int NWAVES>
__device__ __forceinline__ void ra_touch_ranges(const RaRanges& ra, int nwg, int wg, int wave, void* strip) {
  static_assert(kRaMaxSlots % NWAVES == 0, "every wave owns the same number of slots");
  const int lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
#pragma unroll
  for (int r = 0; r < kRaMaxRanges; ++r) {
    const long lines = ra_lines(ra.bytes[r]);
    const int w = (r & 1) ? NWAVES - 1 - wave : wave;
#pragma unroll
    for (int s = 0; s < kRaMaxSlots; s += NWAVES) {
      const long first = ra_slot_first_line(nwg, wg, s + w);
      if (first < lines) {                                                   // wave-uniform: the slot has at least one line
        if (lane < lines - first) ra_touch_dma(ra.ptr[r] + first * kRaLine, (uint32_t)lane * kRaLine, strip);
      }
    }
  }
}
#endif

}  // namespace mode
