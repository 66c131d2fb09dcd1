// Host form of the population-size decay rule (csrc/population.h), for tests/test_population.py: built host-only with
// AddressSanitizer + UndefinedBehaviorSanitizer.
//   population_host icem K n_iter gamma k_min [K n_iter gamma k_min ...]
//       -> per case one line "rc v0 v1 ..."  (rc != 0: the arguments were refused)
//   population_host validate K n_iter n_elite n_keep add_mean n v0 v1 ...   -> the PopError code
//   population_host off K n v0 v1 ...                      -> 1 if the table is the feature off
//   population_host pitch K_i                              -> Kp_i
//   population_host walk Kp Kp_next
//       the two-pitch pass of one wave over one row, restated as a plain loop over (tile q0, lane, j) with the kernel's
//       predicates (pop_walk / pop_reads / pop_writes), against today's one-pitch loop over the read row:
//       -> "wmin wmax rmin rmax order tiles": the fewest / most times a quad of the next row was written and a quad of
//          the read row consumed, 1 if every lane consumed its quads in exactly today's order, and the tiles walked
#include <hip/hip_runtime.h>  // (built as host-only HIP: the header's host + device qualifiers)

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "population.h"

static int usage() {
  std::fprintf(stderr, "usage: population_host icem|validate|off|pitch|walk ...\n");
  return 2;
}

int main(int argc, char** argv) {
  if (argc < 2) return usage();
  const char* mode = argv[1];
  if (!std::strcmp(mode, "icem")) {  // any number of cases, one line each
    if (argc < 6 || (argc - 2) % 4) return usage();
    for (int a = 2; a < argc; a += 4) {
      const int K = std::atoi(argv[a]), n = std::atoi(argv[a + 1]), k_min = std::atoi(argv[a + 3]);
      const double gamma = std::strtod(argv[a + 2], nullptr);
      std::vector<int32_t> tab(n > 0 && n <= kPopMaxIter ? n : 1, -1);  // exactly n entries
      const int rc = pop_icem(K, n, gamma, k_min, tab.data());
      std::printf("%d", rc);
      for (int i = 0; rc == 0 && i < n; ++i) std::printf(" %d", tab[i]);
      std::printf("\n");
    }
    return 0;
  }
  if (!std::strcmp(mode, "validate")) {
    if (argc < 8) return usage();
    const int K = std::atoi(argv[2]), n_iter = std::atoi(argv[3]), n_elite = std::atoi(argv[4]);
    const int n_keep = std::atoi(argv[5]), add_mean = std::atoi(argv[6]), n = std::atoi(argv[7]);
    if (argc != 8 + (n > 0 ? n : 0)) return usage();
    std::vector<int32_t> tab(n > 0 ? n : 0);  // exactly n entries: a read past them is the sanitizer's to find
    for (int i = 0; i < n; ++i) tab[i] = std::atoi(argv[8 + i]);
    std::printf("%d\n", pop_validate(tab.data(), n, K, n_iter, n_elite, n_keep, add_mean));
    return 0;
  }
  if (!std::strcmp(mode, "off")) {
    if (argc < 4) return usage();
    const int K = std::atoi(argv[2]), n = std::atoi(argv[3]);
    if (n < 0 || argc != 4 + n) return usage();
    std::vector<int32_t> tab(n);
    for (int i = 0; i < n; ++i) tab[i] = std::atoi(argv[4 + i]);
    std::printf("%d\n", pop_is_off(tab.data(), n, K) ? 1 : 0);
    return 0;
  }
  if (!std::strcmp(mode, "pitch")) {
    if (argc != 3) return usage();
    std::printf("%d\n", pop_pitch(std::atoi(argv[2])));
    return 0;
  }
  if (!std::strcmp(mode, "walk")) {
    if (argc != 4) return usage();
    const int Kp = std::atoi(argv[2]), Kp_next = std::atoi(argv[3]);
    if (Kp < kPopAlign || Kp_next < kPopAlign || Kp % kPopAlign || Kp_next % kPopAlign) return usage();
    const PopWalk w = pop_walk(Kp, Kp_next);
    std::vector<int> written(w.nq_next, 0), consumed(w.nq, 0);
    std::vector<std::vector<int>> order(kPopWave), today(kPopWave);
    int tiles = 0;
    const int stride = kPopWave * kPopTileQuads;
    for (int base = 0; base < w.nq_walk; base += stride) {  // the wave's tiles; lane l walks q0 = base + l
      bool any = false;
      for (int lane = 0; lane < kPopWave; ++lane) {
        const int q0 = base + lane;
        if (q0 >= w.nq_walk) continue;  // the kernel's loop condition, per lane
        any = true;
        for (int j = 0; j < kPopTileQuads; ++j) {  // generate(r, q0): the next row's quads
          const int q = q0 + kPopWave * j;
          if (pop_writes(w, q)) written.at(q) += 1;
        }
        for (int j = 0; j < kPopTileQuads; ++j) {  // the fmas: the read row's quads
          const int q = q0 + kPopWave * j;
          if (pop_reads(w, q)) {
            consumed.at(q) += 1;
            order[lane].push_back(q);
          }
        }
      }
      tiles += any ? 1 : 0;
    }
    for (int lane = 0; lane < kPopWave; ++lane)  // today's one-pitch loop over the read row
      for (int q0 = lane; q0 < w.nq; q0 += stride)
        for (int j = 0; j < kPopTileQuads; ++j)
          if (q0 + kPopWave * j < w.nq) today[lane].push_back(q0 + kPopWave * j);
    int wmin = 1 << 30, wmax = -1, rmin = 1 << 30, rmax = -1;
    for (int v : written) wmin = v < wmin ? v : wmin, wmax = v > wmax ? v : wmax;
    for (int v : consumed) rmin = v < rmin ? v : rmin, rmax = v > rmax ? v : rmax;
    std::printf("%d %d %d %d %d %d\n", wmin, wmax, rmin, rmax, order == today ? 1 : 0, tiles);
    return 0;
  }
  return usage();
}
