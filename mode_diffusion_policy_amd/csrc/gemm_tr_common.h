// Shared by the transpose-read backward GEMMs (gemm_bf16_tr.hip: ring kernels; gemm_bf16_trws.hip: the wave-specialised weight-gradient + AdamW kernel):
// the kernel argument block; the [k][n] tile image and its swizzle come from gemm_tile.h, the untracked LDS reads and waits from lds_asm.h.
#pragma once
#include "gemm_tile.h"

namespace mode {

struct TrParams {
  const uint16_t* A; long lda;
  const uint16_t* W; long ldw; long w_estride;
  void* C; long ldc;
  const int* offsets; int E;              // data gradient, grouped rows (MoE): expert e owns rows [offsets[e], offsets[e+1])
  const int* koffs; long c_gstride;       // weight gradient: blockIdx.z = group, K rows [koffs[z], koffs[z+1])
  const int* w_rows;                      // weight gradient: gather of W's K rows (dispatch permutation)
  int tap_cols; long tap_stride;          // w_rows in taps: output column n belongs to tap n / tap_cols, which reads W's columns n % tap_cols through w_rows + tap * tap_stride
  int M, N, K, m_tiles, n_tiles;
  int split_k; long split_stride;         // data gradient only: blockIdx.y = K-slice, partial sums to C + slice*split_stride (the consumer adds the slabs)
  // EPI = 1, data gradient dH = dY W2 fused with the SwishGLU (+ dropout) backward and the bias-gradient partial sums (train_ops.hip: swiglu_bwd_bias): C is not written
  const uint16_t* P; uint16_t* dP;        // pre-activations / their gradients [M, 2 N] (value | gate)
  uint32_t seed, thresh; float inv_keep;  // expert-dropout stream of this layer
  float* bsum;                            // [m-tile][2 N] column sums of the bf16-rounded dP over the tile's rows (a tile lies inside one expert's segment)
  int* tile_offs;                         // [E + 1] out: first m-tile of every expert (written by workgroup 0: the segment table of the bias-gradient column sum)
  // EPI = 2, weight gradient with the AdamW update in its epilogue (ModeAdamWFuse, include/mode_hip.h): C is not written; the pointers below are
  // already offset to this GEMM's output tensor (group z at + z * c_gstride elements, row pitch ldc)
  float* ad_p; float* ad_m; float* ad_v; uint16_t* ad_lp; float* ad_ema; float* ad_gsq;
  float ad_decay, ad_b1, ad_b2, ad_eps, ad_step_size, ad_inv_bc2_sqrt, ad_gscale, ad_ema_rate;
};

}  // namespace mode
