// The host form of the best-sample tracking (humanoid_mppi-rl_amd/csrc/iter_best.h) as a stand-alone program, built
// host-only with AddressSanitizer + UndefinedBehaviorSanitizer by tests/test_iterations.py.
// usage: iter_best_host <in.bin> <B> <nu> <H> <K> <clamp> <reset> <it> <out.bin>
// The input holds, 4 bytes per element and in this order: U float32 [B][nu][H], noise float32 [B][nu][H][K], costs
// float32 [B][K], then the stored best carried in (read with reset == 0, present either way): v float32 [B][nu][H],
// cost float32 [B], k int32 [B], iter int32 [B].  The output holds the stored best behind the iteration in the same
// order and types: the caller compares bits, not printed numbers.
#include <hip/hip_runtime.h>  // (built as host-only HIP: the header's host + device qualifiers)

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "iter_best.h"

int main(int argc, char** argv) {
  if (argc != 10) return 2;
  const int B = std::atoi(argv[2]), nu = std::atoi(argv[3]), H = std::atoi(argv[4]), K = std::atoi(argv[5]);
  const float clamp = (float)std::atof(argv[6]);
  const int reset = std::atoi(argv[7]), it = std::atoi(argv[8]);
  if (B < 1 || nu < 1 || H < 1 || K < 1) return 2;
  const size_t nU = (size_t)B * nu * H, nN = nU * K, nC = (size_t)B * K, nB = (size_t)B;
  std::vector<uint32_t> in(2 * nU + nN + nC + 3 * nB);
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  const size_t got = std::fread(in.data(), 4, in.size(), f);
  std::fclose(f);
  if (got != in.size()) return 2;
  std::vector<float> U(nU), eps(nN), c(nC), v(nU), cost(nB);
  std::vector<int32_t> k(nB), iter(nB);
  const uint32_t* p = in.data();
  std::memcpy(U.data(), p, nU * 4);
  std::memcpy(eps.data(), p += nU, nN * 4);
  std::memcpy(c.data(), p += nN, nC * 4);
  std::memcpy(v.data(), p += nC, nU * 4);
  std::memcpy(cost.data(), p += nU, nB * 4);
  std::memcpy(k.data(), p += nB, nB * 4);
  std::memcpy(iter.data(), p += nB, nB * 4);
  for (int b = 0; b < B; ++b)
    iter_best_row(U.data() + (size_t)b * nu * H, eps.data() + (size_t)b * nu * H * K, c.data() + (size_t)b * K, nu, H, K,
                  clamp, reset, it, v.data() + (size_t)b * nu * H, &cost[(size_t)b], &k[(size_t)b], &iter[(size_t)b]);
  FILE* o = std::fopen(argv[9], "wb");
  if (!o) return 2;
  bool ok = std::fwrite(v.data(), 4, v.size(), o) == v.size();
  ok = ok && std::fwrite(cost.data(), 4, cost.size(), o) == cost.size();
  ok = ok && std::fwrite(k.data(), 4, k.size(), o) == k.size();
  ok = ok && std::fwrite(iter.data(), 4, iter.size(), o) == iter.size();
  return std::fclose(o) == 0 && ok ? 0 : 2;
}
