// Host program behind tests/test_adamw_coef.py: the host half of the AdamW step (csrc/adamw_coef.h) on the CPU.  One line per case - the step and the
// bit patterns of decay, step_size and inv_bc2_sqrt - for the hyper-parameters of the two optimizers' defaults x steps 1 ... 100000.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "adamw_coef.h"

static uint32_t bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}

int main() {
  const float hp[2][4] = {{1e-4f, 0.9f, 0.95f, 0.05f}, {1e-3f, 0.9f, 0.999f, 1e-2f}};   // lr, beta1, beta2, weight_decay
  const int steps[] = {1, 2, 10, 1000, 100000};
  for (const auto& h : hp)
    for (int step : steps) {
      const mode::AdamWCoef c = mode::adamw_coef(h[0], h[1], h[2], h[3], step);
      std::printf("%d %08x %08x %08x\n", step, bits(c.decay), bits(c.step_size), bits(c.inv_bc2_sqrt));
    }
  return 0;
}
