// The arithmetic of the rule by which the read-only reduce regenerates part of the noise it sums
// (humanoid_mppi-rl_amd/csrc/reduce_regen.h) as a stand-alone program, built host-only with AddressSanitizer +
// UndefinedBehaviorSanitizer by tests/test_reduce_regen.py.
// usage: reduce_regen_host            prints one line per check, "ok <name>" or "FAIL <name>"; exit 0 iff all hold
#include <hip/hip_runtime.h>  // (built as host-only HIP: the headers' host + device qualifiers)

#include <cstdio>
#include <vector>

#include "reduce_regen.h"

static int failures = 0;
static void check(bool ok, const char* name) {
  std::printf("%s %s\n", ok ? "ok" : "FAIL", name);
  if (!ok) ++failures;
}

// One wave's walk over a row of Kp floats as reduce_kernel makes it (64 lanes, kRegenTileQuads quads per lane and tile,
// quad j of a lane at q0 + 64 j, the loads clamped to the row but only quads < nq summed): every quad of the row must be
// summed exactly once, as a load or as a regenerated quad, and the regenerated ones must number what the share says
static bool walk_covers(int Kp, int arg, int alt, long* n_regen) {
  const int nq = Kp / 4;
  std::vector<int> loaded(nq, 0), regen(nq, 0);
  const int n = regen_row_quads(arg, alt);
  for (int lane = 0; lane < 64; ++lane)
    for (int q0 = lane; q0 < nq; q0 += 64 * kRegenTileQuads)
      for (int j = 0; j < kRegenTileQuads; ++j) {
        const int q = q0 + 64 * j;
        if (q >= nq) continue;  // (the fma is skipped; a clamped load's value is never used)
        if (regen_slot(n, j))
          ++regen[q];
        else
          ++loaded[q];
      }
  bool ok = true;
  for (int q = 0; q < nq; ++q) {
    ok = ok && loaded[q] + regen[q] == 1;
    *n_regen += regen[q];
  }
  return ok;
}

int main() {
  // the size threshold, both sides (strictly past 128 MiB, as the reduce's own nontemporal test)
  check(!regen_size_ok(kRegenMinNoiseBytes) && regen_size_ok(kRegenMinNoiseBytes + 1) &&
            !regen_size_ok(kRegenMinNoiseBytes - 1) && !regen_size_ok(0),
        "size threshold is strict");
  check(kRegenMinNoiseBytes == 128ull * 1024 * 1024, "size threshold = 128 MiB");
  check(regen_noise_bytes(64, 21, 64, 1024) == 352321536ull, "noise bytes of 64 solves");
  check(regen_noise_bytes(4096, 64, 512, 4096) == 4096ull * 64 * 512 * 4096 * 4, "noise bytes past 2^32");
  // eighths -> rows: of any 8 consecutive places, `eighths` rows are computed entirely and the others read
  {
    bool ok = true;
    for (int e = 0; e <= kRegenMaxEighths; ++e)
      for (int start = 0; start < 24; ++start) {
        int whole = 0;
        for (int alt = start; alt < start + 8; ++alt) {
          const int n = regen_row_quads(e, alt);
          ok = ok && (n == 0 || n == kRegenTileQuads);
          whole += n == kRegenTileQuads ? 1 : 0;
        }
        ok = ok && whole == e;
      }
    check(ok, "whole rows: eighths of any 8 consecutive rows");
    check(regen_row_quads(0, 0) == 0 && regen_row_quads(0, 1) == 0 && regen_row_quads(0, 7) == 0,
          "share 0 regenerates nothing");
  }
  // the slots: the last n of the tile
  {
    bool ok = true;
    for (int n = 0; n <= kRegenTileQuads; ++n) {
      int cnt = 0;
      for (int j = 0; j < kRegenTileQuads; ++j) {
        cnt += regen_slot(n, j) ? 1 : 0;
        ok = ok && regen_slot(n, j) == (j >= kRegenTileQuads - n);
      }
      ok = ok && cnt == n;
    }
    check(ok, "a row regenerates its tile's last slots");
  }
  // every quad exactly once, loaded or regenerated: fewer quads than lanes, exactly one tile, a second partial tile
  for (int Kp : {96, 1024, 1536}) {
    bool ok = true;
    for (int e = 0; e <= kRegenMaxEighths; ++e)
      for (int alt = 0; alt < 8; ++alt) {
        long n = 0;
        ok = ok && walk_covers(Kp, e, alt, &n);
        if (e == 0) ok = ok && n == 0;
      }
    char name[64];
    std::snprintf(name, sizeof name, "Kp %d: every quad once", Kp);
    check(ok, name);
  }
  // where whole tiles are walked the regenerated share is exact: Kp = 1024, 8 rows
  {
    bool ok = true;
    for (int e = 0; e <= kRegenMaxEighths; ++e) {
      long n = 0;
      for (int alt = 0; alt < 8; ++alt) ok = ok && walk_covers(1024, e, alt, &n);
      ok = ok && n * 8 == (long)e * 8 * 256;
    }
    check(ok, "Kp 1024: the share is eighths / 8");
  }
  // the knob and the rule
  check(regen_knob(nullptr) == -1 && regen_knob("") == -1 && regen_knob("8") == -1 && regen_knob("12") == -1 &&
            regen_knob("x") == -1 && regen_knob("0") == 0 && regen_knob("3") == 3 && regen_knob("7") == 7,
        "knob: one digit 0..7");
  const uint64_t big = regen_noise_bytes(64, 21, 64, 1024), small = regen_noise_bytes(8, 21, 64, 1024);
  check(regen_share(true, big, -1) == kRegenDefaultEighths && regen_share(true, small, -1) == 0 &&
            regen_share(true, kRegenMinNoiseBytes, -1) == 0,
        "rule: the default share past the size only");
  check(regen_share(true, big, 0) == 0 && regen_share(true, small, 0) == 0, "rule: 0 turns it off");
  check(regen_share(true, small, 1) == 1 && regen_share(true, small, 7) == 7 && regen_share(true, big, 5) == 5,
        "rule: a forced share ignores the size");
  check(regen_share(false, big, -1) == 0 && regen_share(false, big, 7) == 0 && regen_share(false, small, 3) == 0,
        "rule: content is never overridden");
  check(kRegenDefaultEighths >= 0 && kRegenDefaultEighths <= kRegenMaxEighths && kRegenMaxEighths == 7,
        "rule: the default is a share");
  return failures == 0 ? 0 : 1;
}
