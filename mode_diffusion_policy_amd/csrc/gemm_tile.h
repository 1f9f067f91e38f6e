// What the tiled bf16 GEMM kernels share of their tile geometry and LDS images: the 16-byte LDS DMA, the GROUP_M rasterisation, the expert-segment
// lookups, the chunk swizzles of the two operand images.  ONE definition each - a swizzle that differs by one bit between the DMA source address and
// the fragment read gives wrong numbers, not a crash.  Forceinline functions over values and references to locals; a piece lives here only where the
// kernels that call it keep their compiled code (scripts/isa_compare.py; LABNOTES.md, 2026-10-17, names what stayed written out where, and why).
#pragma once
#include "mode_common.h"
#include "lds_asm.h"
#include <type_traits>

namespace mode {

// ---- the 16-byte LDS DMA: `global_load_lds_dwordx4`, global / L2 -> LDS without VGPR staging.  The LDS destination of a wave is lane-linear
// (lane i writes bytes [16 i, 16 i + 16) from lds_dst), the SOURCE address is per lane: every LDS image below is "linear destination + swizzled source +
// swizzled read".
__device__ __forceinline__ void dma16(const void* src, void* lds_dst) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src, (__attribute__((address_space(3))) void*)lds_dst, 16, 0, 0);
}

// ---- expert segments (grouped / MoE products): rows are sorted by expert; expert e owns sorted rows [o[e], o[e+1]) and ceil(count / BM) m-tiles.
// m-tile `t` of the grouped tile space -> its rows [row0, row_end) and expert; outputs untouched for a tile past the last expert's.  Two forms:
//   segment_tile9      register scan over the nine offsets o[e] = offsets[min(e, E)] (E <= 8; the caller fetched them by independent loads - no
//                      dependent chain); also the expert's first row seg0
//   segment_tile_loop  any E, two dependent loads per expert; false = no such tile
template <int BM>
__device__ __forceinline__ void segment_tile9(const int (&o)[9], int E, int t, int& row0, int& row_end, int& expert, int& seg0) {
  bool found = false;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    if (!found && e < E) {
      const int nt_e = (o[e + 1] - o[e] + BM - 1) / BM;
      if (t < nt_e) { row0 = o[e] + t * BM; row_end = min(o[e + 1], row0 + BM); expert = e; seg0 = o[e]; found = true; }
      else t -= nt_e;
    }
  }
}
template <int BM>
__device__ __forceinline__ bool segment_tile_loop(const int* offsets, int E, int t, int& row0, int& row_end, int& expert) {
  bool found = false;
  for (int e = 0; e < E && !found; ++e) {
    const int o0 = offsets[e], o1 = offsets[e + 1];
    const int nt_e = (o1 - o0 + BM - 1) / BM;
    if (t < nt_e) { row0 = o0 + t * BM; row_end = min(o1, row0 + BM); expert = e; found = true; }
    else t -= nt_e;
  }
  return found;
}

// ---- GROUP_M rasterisation of the ring kernels: (XCD-remapped) block id -> (m-tile, n-tile), group_m m-tiles x all n-tiles per group, m fastest
__device__ __forceinline__ void group_m_tile(int sb, int m_tiles, int n_tiles, int group_m, int& mt, int& nt) {
  const int per_group = group_m * n_tiles;
  const int grp = sb / per_group, first_m = grp * group_m;
  const int gsz = min(m_tiles - first_m, group_m);
  const int rem = sb - grp * per_group;
  mt = first_m + rem % gsz; nt = rem / gsz;
}

// ---- operand image [rows][64 k] (a K-contiguous operand: 128-byte rows).  A 1-KiB DMA piece = 8 rows; lane i fills row i >> 3, PHYSICAL 16-byte chunk
// i & 7 of it with the LOGICAL chunk (i & 7) ^ (i >> 3) - the chunk index XOR (row & 7), pieces start at multiples of 8 rows.  A fragment read
// (ds_read_b128: lane -> row fr = lane & 15 of a 16-row fragment, k-chunk fq = lane >> 4; the second k32 half is 4 chunks on, i.e. the byte offset ^ 64)
// applies the same XOR: the 16 lanes of a read group hit 16 distinct 16-byte slots (measured SQ_LDS_BANK_CONFLICT = 0).
__device__ __forceinline__ int rk_dma_chunk(int lane) { return (lane & 7) ^ (lane >> 3); }         // logical chunk this lane's DMA fetches
__device__ __forceinline__ int rk_frag_byte(int fr, int fq) { return (fq ^ (fr & 7)) * 16; }      // byte offset in the fragment row, first k32 half

// ---- operand image [64 k][COLS] (an operand whose reduction index is its ROW index, DMA'd as it lies in memory; COLS = 128: 256-byte rows, 64: 128-byte
// rows).  32-byte column groups are XOR-swizzled by f(k) = kn_swz<COLS>(k), so the 32 lanes of one LDS cycle of a transpose read (2 groups x 4 rows x 32 B)
// cover all 64 banks once (COLS = 64: odd rows already sit on the other half of the banks).  A 1-KiB DMA piece = 1024 / (2 COLS) k-rows; a lane fills
// PHYSICAL 16-byte chunk pc of its row with the LOGICAL chunk pc ^ (f(k) << 1); the transpose reads of the kernels apply the same f to their row.
template <int COLS>
__device__ __forceinline__ int kn_swz(int row) {
  if constexpr (COLS == 128) return (row & 3) | (((row >> 3) & 1) << 2);
  else return ((row >> 1) & 1) | (((row >> 3) & 1) << 1);
}
template <int COLS>
__device__ __forceinline__ int kn_chunk_col(int piece_row, int pc) { return (pc ^ (kn_swz<COLS>(piece_row) << 1)) * 8; }   // logical column (elements) behind physical chunk pc of k-row piece_row

}  // namespace mode
