// The arithmetic of the rule that routes a chained solve's next noise beside its rollout
// (humanoid_mppi-rl_amd/csrc/gen_overlap.h) and the row-uniform form of the Philox rounds its generator runs
// (philox.h philox4x32_10_row) as a stand-alone program, built host-only with AddressSanitizer +
// UndefinedBehaviorSanitizer by tests/test_gen_overlap.py.
// usage: gen_overlap_host            prints one line per check, "ok <name>" or "FAIL <name>"; exit 0 iff all hold
#include <hip/hip_runtime.h>  // (built as host-only HIP: the headers' host + device qualifiers)

#include <cstdio>

#include "gen_overlap.h"
#include "philox.h"

static int failures = 0;
static void check(bool ok, const char* name) {
  std::printf("%s %s\n", ok ? "ok" : "FAIL", name);
  if (!ok) ++failures;
}

int main() {
  // rounding to the allocation granule
  check(gen_alloc(248) == 248 && gen_alloc(249) == 256 && gen_alloc(252) == 256 && gen_alloc(12) == 16 &&
            gen_alloc(16) == 16 && gen_alloc(17) == 24 && gen_alloc(20) == 24 && gen_alloc(1) == 8,
        "alloc rounds up to 8");
  // the fit: two rollout waves and one generator wave in a SIMD's 512 registers
  check(gen_fits(248, 16), "248 + 248 + 16 fits");
  check(!gen_fits(252, 16), "252 + 252 + 16 does not");
  check(!gen_fits(248, 20), "248 + 248 + 20 does not");
  check(gen_fits(248, 12) && gen_fits(241, 9) && !gen_fits(249, 8), "the fit is on allocations, not counts");
  check(gen_fits(236, 16) && gen_fits(230, 32) && !gen_fits(236, 41), "smaller rollouts leave more");
  check(!gen_fits(0, 16) && !gen_fits(248, 0) && !gen_fits(-1, -1), "an unknown count never fits");
  // the size threshold, both sides (strictly past 128 MiB, as the reduce's own nontemporal test)
  check(!gen_size_ok(kGenMinNoiseBytes) && gen_size_ok(kGenMinNoiseBytes + 1) && !gen_size_ok(kGenMinNoiseBytes - 1) &&
            !gen_size_ok(0),
        "size threshold: both sides");
  check(kGenMinNoiseBytes == 128ull * 1024 * 1024, "size threshold = 128 MiB");
  // in shapes: 64 solves of the humanoid (nu 21, H 64, Kp 1024) are 352 MB, 16 solves 88 MB
  check(gen_noise_bytes(64, 21, 64, 1024) == 352321536ull, "noise bytes of 64 solves");
  check(gen_noise_bytes(4096, 64, 512, 4096) == 4096ull * 64 * 512 * 4096 * 4, "noise bytes past 2^32");
  check(gen_overlap_rule(64, 21, 64, 1024, 248, 16), "rule: 64 solves, 248 + 16");
  check(gen_overlap_rule(32, 21, 64, 1024, 248, 12), "rule: 32 solves");
  check(!gen_overlap_rule(16, 21, 64, 1024, 248, 16), "rule: 16 solves are below the size");
  check(!gen_overlap_rule(64, 21, 2, 1024, 248, 16), "rule: a two-step horizon is below the size");
  check(!gen_overlap_rule(64, 21, 64, 1024, 252, 16), "rule: size alone is not enough");
  check(gen_overlap_rule(25, 21, 64, 1024, 248, 16) && !gen_overlap_rule(24, 21, 64, 1024, 248, 16),
        "rule: the threshold between 24 and 25 solves");
  // the row-uniform Philox form against the reference form, bit for bit
  {
    bool same = true;
    const uint32_t qs[] = {0u, 1u, 63u, 64u, 255u, 271u, 0x7fffffffu, 0xffffffffu};
    const uint32_t ts[] = {0u, 1u, 63u, 511u}, us[] = {0u, 20u, 63u}, bs[] = {0u, 1u, 63u, 4095u};
    const uint64_t keys[] = {0ull, 1ull, 0x5EEDC0DEull, 0xFFFFFFFFFFFFFFFFull, 0x123456789ABCDEF0ull};
    for (uint64_t key : keys)
      for (uint32_t q : qs)
        for (uint32_t t : ts)
          for (uint32_t u : us)
            for (uint32_t b : bs) {
              const uint32_t k0 = (uint32_t)key, k1 = (uint32_t)(key >> 32);
              const mppi_u4 a = philox4x32_10(mppi_u4{q, t, u, b}, k0, k1);
              const mppi_u4 r = philox4x32_10_row(q, t, u, b, k0, k1);
              same = same && a.x == r.x && a.y == r.y && a.z == r.z && a.w == r.w;
            }
    check(same, "philox4x32_10_row == philox4x32_10");
    // Random123's known answer for Philox4x32-10: counter and key all ones
    const mppi_u4 kat = philox4x32_10_row(0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu);
    check(kat.x == 0x408f276du && kat.y == 0x41c83b0eu && kat.z == 0xa20bc7c6u && kat.w == 0x6d5451fdu,
          "philox4x32_10_row known answer");
  }
  return failures == 0 ? 0 : 1;
}
