// The host form of the control-cost coefficients (humanoid_mppi-rl_amd/csrc/control_cost.h) as a stand-alone program,
// built host-only with AddressSanitizer + UndefinedBehaviorSanitizer by tests/test_control_cost.py.
// usage: control_cost_host <U.f32> <rows> <H> <gamma> <sigma> <rho>
// The file holds rows * H float32 values, the (b, u) rows of U; one line per row: lin[0..H) (hex floats, so the caller
// reads the exact fp32 values).
#include <hip/hip_runtime.h>  // (built as host-only HIP: the header's host + device qualifiers)

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "control_cost.h"

int main(int argc, char** argv) {
  if (argc != 7) return 2;
  const int rows = std::atoi(argv[2]), H = std::atoi(argv[3]);
  const float gamma = std::strtof(argv[4], nullptr), sigma = std::strtof(argv[5], nullptr),
              rho = std::strtof(argv[6], nullptr);
  if (rows < 1 || H < 1) return 2;
  std::vector<float> U((size_t)rows * H), lin((size_t)H);
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  const size_t got = std::fread(U.data(), sizeof(float), U.size(), f);
  std::fclose(f);
  if (got != U.size()) return 2;
  for (int r = 0; r < rows; ++r) {
    ctrl_lin_row(gamma, sigma, rho, U.data() + (size_t)r * H, lin.data(), H);
    for (int t = 0; t < H; ++t) std::printf("%a%c", lin[(size_t)t], t + 1 < H ? ' ' : '\n');
  }
  return 0;
}
