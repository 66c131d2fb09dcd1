// The host form of the ESS-targeting rule (humanoid_mppi-rl_amd/csrc/ess_target.h) as a stand-alone program, built
// host-only with AddressSanitizer + UndefinedBehaviorSanitizer by tests/test_ess_target.py.
// usage: ess_target_host <costs.f32> <rows> <K> <ess_frac> <lambda_min> <lambda_max> <cfg_lambda>
// The file holds rows * K float32 costs; one line per row: lambda of the 15-candidate search, lambda of plain
// bisection, and the passes each took (hex floats, so the caller reads the exact fp32 values).
#include <hip/hip_runtime.h>  // (built as host-only HIP: the header's host + device qualifiers)

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ess_target.h"

int main(int argc, char** argv) {
  if (argc != 8) return 2;
  const int rows = std::atoi(argv[2]), K = std::atoi(argv[3]);
  const EssTarget s{std::strtof(argv[4], nullptr), std::strtof(argv[5], nullptr), std::strtof(argv[6], nullptr)};
  const float cfg_lambda = std::strtof(argv[7], nullptr);
  if (rows < 1 || K < 1) return 2;
  std::vector<float> c((size_t)rows * K);
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  const size_t got = std::fread(c.data(), sizeof(float), c.size(), f);
  std::fclose(f);
  if (got != c.size()) return 2;
  for (int r = 0; r < rows; ++r) {
    int p15 = 0, p1 = 0;
    const float l15 = ess_lambda_host<15>(s, cfg_lambda, c.data() + (size_t)r * K, K, &p15);
    const float l1 = ess_lambda_host<1>(s, cfg_lambda, c.data() + (size_t)r * K, K, &p1);
    std::printf("%a %a %d %d\n", l15, l1, p15, p1);
  }
  return 0;
}
