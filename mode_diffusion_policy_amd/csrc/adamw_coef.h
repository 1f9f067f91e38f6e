// The host half of mode::adamw_update_f (mode_common.h): the per-launch coefficients of one AdamW step.  ONE definition for the streaming pass
// (train_ops.hip: mode_adamw_step / _clipped / _lp) and the weight-gradient GEMM's fused epilogue (gemm_bf16_tr.hip) - the fused expert step equals the
// two-pass update bit for bit only while both round alike.  Plain host C++ without HIP (tests/test_adamw_coef.py runs it on the CPU): bias corrections,
// division and square root in double with one final cast each, the decay factor a float expression.
#pragma once
#include <math.h>

namespace mode {

struct AdamWCoef { float decay, step_size, inv_bc2_sqrt; };   // 1 - lr * wd;  lr / (1 - beta1^step);  1 / sqrt(1 - beta2^step)

inline AdamWCoef adamw_coef(float lr, float beta1, float beta2, float weight_decay, int step) {
  const double bc1 = 1.0 - pow((double)beta1, step), bc2 = 1.0 - pow((double)beta2, step);
  return {1.f - lr * weight_decay, (float)(lr / bc1), (float)(1.0 / sqrt(bc2))};
}

}  // namespace mode
