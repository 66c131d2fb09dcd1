// The host form of the ensemble's combining rule (humanoid_mppi-rl_amd/csrc/ensemble.h) as a stand-alone program, built
// host-only with AddressSanitizer + UndefinedBehaviorSanitizer by tests/test_ensemble.py.
// usage: ensemble_host <in.bin> <n> <rows> <K> <mode> <kappa> <out.bin>
// The input holds the members' costs, float32 [n][rows][K]; the output the combined costs float32 [rows][K], then the
// spread float32 [rows][K]: the caller compares bits, not printed numbers.
#include <hip/hip_runtime.h>  // (built as host-only HIP: the header's host + device qualifiers)

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ensemble.h"

int main(int argc, char** argv) {
  if (argc != 8) return 2;
  const int n = std::atoi(argv[2]), rows = std::atoi(argv[3]), K = std::atoi(argv[4]), mode = std::atoi(argv[5]);
  const float kappa = (float)std::atof(argv[6]);
  if (n < 2 || n > MPPI_ENS_MAX || rows < 1 || K < 1 || !ensemble_mode_valid(mode) || !ensemble_kappa_valid(kappa)) return 2;
  const size_t row = (size_t)rows * K;
  std::vector<float> in((size_t)n * row), cost(row), sd(row);
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  const size_t got = std::fread(in.data(), 4, in.size(), f);
  std::fclose(f);
  if (got != in.size()) return 2;
  for (int r = 0; r < rows; ++r)  // member e's row r lies rows * K behind member e - 1's
    ensemble_row(in.data() + (size_t)r * K, (long)row, n, K, mode, kappa, cost.data() + (size_t)r * K,
                 sd.data() + (size_t)r * K);
  FILE* o = std::fopen(argv[7], "wb");
  if (!o) return 2;
  bool ok = std::fwrite(cost.data(), 4, cost.size(), o) == cost.size();
  ok = ok && std::fwrite(sd.data(), 4, sd.size(), o) == sd.size();
  return std::fclose(o) == 0 && ok ? 0 : 2;
}
