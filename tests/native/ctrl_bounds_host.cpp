// The host form of the control-bounds rule (humanoid_mppi-rl_amd/csrc/ctrl_bounds.h) as a stand-alone program, built
// host-only with AddressSanitizer + UndefinedBehaviorSanitizer by tests/test_control_bounds.py.
// usage: ctrl_bounds_host <U.f32> <eps.f32> <box.f32> <out.f32> <rows> <H> <K>
// U holds rows * H float32 values (the (b, u) rows of the nominal), eps rows * H * K (their noise), box rows * 2 (lo, hi
// of each row).  The projected noise is written to out (raw float32, so the caller compares bits); one line per row on
// stdout: the row's count.  Exit 3: a box with lo > hi or a NaN (ctrl_bounds_valid).
#include <hip/hip_runtime.h>  // (built as host-only HIP: the header's host + device qualifiers)

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ctrl_bounds.h"

static bool read_all(const char* path, std::vector<float>& v) {
  FILE* f = std::fopen(path, "rb");
  if (!f) return false;
  const size_t got = std::fread(v.data(), sizeof(float), v.size(), f);
  std::fclose(f);
  return got == v.size();
}

int main(int argc, char** argv) {
  if (argc != 8) return 2;
  const int rows = std::atoi(argv[5]), H = std::atoi(argv[6]), K = std::atoi(argv[7]);
  if (rows < 1 || H < 1 || K < 1) return 2;
  std::vector<float> U((size_t)rows * H), eps((size_t)rows * H * K), box((size_t)rows * 2);
  if (!read_all(argv[1], U) || !read_all(argv[2], eps) || !read_all(argv[3], box)) return 2;
  for (int r = 0; r < rows; ++r)
    if (!ctrl_bounds_valid(&box[(size_t)2 * r], &box[(size_t)2 * r + 1], 1)) return 3;
  for (int r = 0; r < rows; ++r) {
    const unsigned n = ctrl_bounds_project_row(U.data() + (size_t)r * H, eps.data() + (size_t)r * H * K,
                                               box[(size_t)2 * r], box[(size_t)2 * r + 1], H, K);
    std::printf("%u\n", n);
  }
  FILE* f = std::fopen(argv[4], "wb");
  if (!f) return 2;
  const size_t put = std::fwrite(eps.data(), sizeof(float), eps.size(), f);
  std::fclose(f);
  return put == eps.size() ? 0 : 2;
}
