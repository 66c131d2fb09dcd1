// The host form of the control-rate cost term (humanoid_mppi-rl_amd/csrc/rate_cost.h) as a stand-alone program,
// built with g++ by tests/test_rate_cost.py.
// usage: rate_cost_host <in.f32> <nu> <H> <K> <anchor> <clamp>
// The file holds float32 values: U [nu][H], r [nu], u_prev [nu], eps [nu][H][K] (k fastest); one line per sample:
// its term (a hex float, so the caller reads the exact fp32 value).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rate_cost.h"  // (plain C++ here: MPPI_HD is `inline`)

int main(int argc, char** argv) {
  if (argc != 7) return 2;
  const int nu = std::atoi(argv[2]), H = std::atoi(argv[3]), K = std::atoi(argv[4]), anchor = std::atoi(argv[5]);
  const float clamp = std::strtof(argv[6], nullptr);
  if (nu < 1 || H < 1 || K < 1) return 2;
  const size_t R = (size_t)nu * H;
  std::vector<float> in(R + 2 * (size_t)nu + R * K);
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  const size_t got = std::fread(in.data(), sizeof(float), in.size(), f);
  std::fclose(f);
  if (got != in.size()) return 2;
  const float *U = in.data(), *r = U + R, *up = r + nu, *eps = up + nu;
  if (!rate_cost_valid(r, nu)) return 3;
  for (int k = 0; k < K; ++k) std::printf("%a\n", rate_cost_sample(U, eps + k, K, r, up, anchor, clamp, nu, H));
  return 0;
}
