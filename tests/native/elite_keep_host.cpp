// The host form of keep / shift elites (humanoid_mppi-rl_amd/csrc/elite_keep.h) as a stand-alone program, built
// host-only with AddressSanitizer + UndefinedBehaviorSanitizer by tests/test_elite_keep.py.
// usage: elite_keep_host <in.f32> <B> <nu> <H> <K> <n_keep> <shift> <clamp> <out.bin>
// The input holds, float32 and in this order: U [B][nu][H], noise [B][nu][H][K], costs [B][K] (the storing solve), then
// U2 [B][nu][H], noise2 [B][nu][H][K] (the solve the set is injected into).  The output holds, raw and in this order:
// v float32 [B][nu][H][n_keep], kcost float32 [B][n_keep], idx int32 [B][n_keep], count int32 [B], steps int32 [B],
// noise2 after the injection float32 [B][nu][H][K]: the caller compares bits, not printed numbers.
#include <hip/hip_runtime.h>  // (built as host-only HIP: the header's host + device qualifiers)

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "elite_keep.h"

int main(int argc, char** argv) {
  if (argc != 10) return 2;
  const int B = std::atoi(argv[2]), nu = std::atoi(argv[3]), H = std::atoi(argv[4]), K = std::atoi(argv[5]);
  const int n_keep = std::atoi(argv[6]), shift = std::atoi(argv[7]);
  const float clamp = (float)std::atof(argv[8]);
  if (B < 1 || nu < 1 || H < 1 || K < 1 || n_keep < 1 || n_keep > K) return 2;
  const size_t nU = (size_t)B * nu * H, nN = nU * K, nC = (size_t)B * K, nV = nU * n_keep, nK = (size_t)B * n_keep;
  std::vector<float> in(2 * nU + 2 * nN + nC);
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  const size_t got = std::fread(in.data(), sizeof(float), in.size(), f);
  std::fclose(f);
  if (got != in.size()) return 2;
  const float *U = in.data(), *eps = U + nU, *c = eps + nN, *U2 = c + nC;
  float* eps2 = in.data() + 2 * nU + nN + nC;
  std::vector<float> v(nV), kcost(nK);
  std::vector<int32_t> idx(nK), count((size_t)B), steps((size_t)B);
  for (int b = 0; b < B; ++b) {
    int st = -1;
    count[(size_t)b] = keep_store_row(U + (size_t)b * nu * H, eps + (size_t)b * nu * H * K, c + (size_t)b * K, nu, H, K,
                                      n_keep, shift, clamp, v.data() + (size_t)b * nu * H * n_keep,
                                      kcost.data() + (size_t)b * n_keep, idx.data() + (size_t)b * n_keep, &st);
    steps[(size_t)b] = st;
    if (st != keep_steps(H, shift)) return 3;
    keep_inject_row(U2 + (size_t)b * nu * H, eps2 + (size_t)b * nu * H * K, v.data() + (size_t)b * nu * H * n_keep, nu, H,
                    K, n_keep, count[(size_t)b], st);
  }
  FILE* o = std::fopen(argv[9], "wb");
  if (!o) return 2;
  bool ok = std::fwrite(v.data(), 4, v.size(), o) == v.size();
  ok = ok && std::fwrite(kcost.data(), 4, kcost.size(), o) == kcost.size();
  ok = ok && std::fwrite(idx.data(), 4, idx.size(), o) == idx.size();
  ok = ok && std::fwrite(count.data(), 4, count.size(), o) == count.size();
  ok = ok && std::fwrite(steps.data(), 4, steps.size(), o) == steps.size();
  ok = ok && std::fwrite(eps2, 4, nN, o) == nN;
  return std::fclose(o) == 0 && ok ? 0 : 2;
}
