// The host form of elite truncation (humanoid_mppi-rl_amd/csrc/elite_select.h) as a stand-alone program, built
// host-only with AddressSanitizer + UndefinedBehaviorSanitizer by tests/test_elites.py.
// usage: elite_select_host <costs.f32> <rows> <K> <n_elite> <out.bin>
// The input holds rows * K float32 costs.  The output holds, raw and in this order: idx int32 [rows][n_elite],
// count int32 [rows], tau float32 [rows], ecost float32 [rows][K], key uint32 [rows][K] (elite_key of a finite cost,
// 0xFFFFFFFF otherwise): the caller compares bits, not printed numbers.
#include <hip/hip_runtime.h>  // (built as host-only HIP: the header's host + device qualifiers)

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "elite_select.h"

int main(int argc, char** argv) {
  if (argc != 6) return 2;
  const int rows = std::atoi(argv[2]), K = std::atoi(argv[3]), n_elite = std::atoi(argv[4]);
  if (rows < 1 || K < 1 || n_elite < 1 || n_elite > K) return 2;
  std::vector<float> c((size_t)rows * K);
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  const size_t got = std::fread(c.data(), sizeof(float), c.size(), f);
  std::fclose(f);
  if (got != c.size()) return 2;
  std::vector<int32_t> idx((size_t)rows * n_elite), count((size_t)rows);
  std::vector<float> tau((size_t)rows), ecost((size_t)rows * K);
  std::vector<uint32_t> key((size_t)rows * K);
  for (int r = 0; r < rows; ++r) {
    const float* row = c.data() + (size_t)r * K;
    count[(size_t)r] = elite_select_row(row, K, n_elite, idx.data() + (size_t)r * n_elite, &tau[(size_t)r],
                                        ecost.data() + (size_t)r * K);
    if (elite_select_row(row, K, n_elite, nullptr, nullptr, nullptr) != count[(size_t)r]) return 3;  // (all optional)
    for (int k = 0; k < K; ++k) {
      key[(size_t)r * K + k] = elite_key_or_none(row[k]);
      // the key stands for its cost: back through the inverse map and forth again
      if (ess_finite(row[k]) && elite_key(elite_key_cost(elite_key(row[k]))) != elite_key(row[k])) return 3;
    }
  }
  FILE* o = std::fopen(argv[5], "wb");
  if (!o) return 2;
  bool ok = std::fwrite(idx.data(), 4, idx.size(), o) == idx.size();
  ok = ok && std::fwrite(count.data(), 4, count.size(), o) == count.size();
  ok = ok && std::fwrite(tau.data(), 4, tau.size(), o) == tau.size();
  ok = ok && std::fwrite(ecost.data(), 4, ecost.size(), o) == ecost.size();
  ok = ok && std::fwrite(key.data(), 4, key.size(), o) == key.size();
  return std::fclose(o) == 0 && ok ? 0 : 2;
}
