// Population-size decay (mppi_set_population): a sample count per inner iteration of a control step, iCEM's shrinking
// budget N_i = max(N / gamma^i, k_min).  This header is the only statement of the rule: the ABI (mppi_api.hip) validates
// and shapes every iteration by it, reduce_kernel's two-pitch form (kernels_common.hip) takes its loop extents from it,
// tests/native/population_host.cpp runs all of it on the host, and mppi_hip.stats.icem_population is the numpy
// restatement of the helper.
//
// The table.  K_it[i], i < n, is the number of samples iteration i of every control step draws, rolls out and weighs.
// With a table on, iteration i is bit for bit the solve of a handle created with cfg.K = K_it[i]: every buffer was
// sized for cfg.K and is re-read densely at the iteration's own shape (K_i, Kp_i = pop_pitch(K_i)), so no kernel's
// addressing changes.  Philox counters are (k / 4, t, u, b) and do not depend on the pitch: iteration i sees the first
// K_i columns of its key's noise.
//   valid:  n == n_iter;  K_it[0] == K;  1 <= K_it[i] <= K;  n_elite, n_keep and, with add_mean, n_keep + 1 <= K_it[i]
//   off:    every entry == K (the same branches, arguments and launches as a handle that never set a table)
//
// The helper.  d = 1.0; for i: K_it[i] = max(k_min, (int)(K / d)); d *= gamma -- in double, a division, a truncation
// and a product per entry, all correctly rounded: no pow, so any host computes the same table.
//
// The two-pitch pass.  reduce_kernel<GEN> reads this iteration's noise rows at Kp and writes the same (b, u, t) rows of
// the next iteration's at Kp_next.  A wave walks a row in tiles: lane l of the wave owns the quads q0 + 64 j, j <
// kPopTileQuads, of tile q0 = l, l + 256, ...; the walk runs to max(nq, nq_next) quads, reads and accumulates where
// q < nq (today's order over those) and generates where q < nq_next.
#pragma once
#include <stdint.h>

#include "philox.h"  // MPPI_HD

constexpr int kPopMaxIter = 16;   // mppi_set_iterations' bound on n_iter
constexpr int kPopAlign = 64;     // the K axis' device pitch granule (mppi::kKpAlign)
constexpr int kPopWave = 64;      // lanes of a wave
constexpr int kPopTileQuads = 4;  // quads per lane in flight per tile (reduce_kernel's kRU)

// Kp_i: the device pitch of an iteration of K_i samples
MPPI_HD int pop_pitch(int K_i) { return (K_i + kPopAlign - 1) / kPopAlign * kPopAlign; }

// why a table is refused (0: it is valid)
enum PopError : int {
  kPopOk = 0,
  kPopCount = 1,   // n != n_iter (or n outside [1, kPopMaxIter])
  kPopFirst = 2,   // K_it[0] != K
  kPopRange = 3,   // some K_it[i] outside [1, K]
  kPopElite = 4,   // n_elite > some K_it[i]
  kPopKeep = 5,    // n_keep > some K_it[i]
  kPopMean = 6,    // add_mean and n_keep + 1 > some K_it[i]
};

inline int pop_validate(const int32_t* K_it, int n, int K, int n_iter, int n_elite, int n_keep, int add_mean) {
  if (n < 1 || n > kPopMaxIter || n != n_iter) return kPopCount;
  if (K_it[0] != K) return kPopFirst;
  for (int i = 0; i < n; ++i)
    if (K_it[i] < 1 || K_it[i] > K) return kPopRange;
  for (int i = 0; i < n; ++i) {
    if (n_elite > K_it[i]) return kPopElite;
    if (n_keep > K_it[i]) return kPopKeep;
    if (add_mean && n_keep + 1 > K_it[i]) return kPopMean;
  }
  return kPopOk;
}

inline const char* pop_error_text(int e) {
  switch (e) {
    case kPopOk: return "valid";
    case kPopCount: return "the table has one entry per iteration (n == n_iter of mppi_set_iterations)";
    case kPopFirst: return "K_it[0] must equal cfg.K";
    case kPopRange: return "every K_it[i] must be in [1, cfg.K]";
    case kPopElite: return "n_elite of mppi_set_elites exceeds some K_it[i]";
    case kPopKeep: return "n_keep of mppi_set_elite_keep exceeds some K_it[i]";
    default: return "add_mean of mppi_set_iterations needs n_keep + 1 <= every K_it[i]";
  }
}

// whether a valid table is the feature off
inline bool pop_is_off(const int32_t* K_it, int n, int K) {
  for (int i = 0; i < n; ++i)
    if (K_it[i] != K) return false;
  return true;
}

// iCEM's schedule; 0: written, nonzero: an argument out of range (gamma >= 1, 1 <= k_min <= K, 1 <= n_iter <= 16)
inline int pop_icem(int K, int n_iter, double gamma, int k_min, int32_t* K_it) {
  if (!(gamma >= 1.0) || K < 1 || k_min < 1 || k_min > K || n_iter < 1 || n_iter > kPopMaxIter)
    return 1;
  double d = 1.0;
  for (int i = 0; i < n_iter; ++i) {
    const double q = (double)K / d;  // in [0, K]: the conversion below is exact truncation
    const int v = (int)q;
    K_it[i] = v > k_min ? v : k_min;
    d *= gamma;
  }
  return 0;
}

// The two-pitch pass' extents for one row: quads read, quads written, quads walked.
struct PopWalk {
  int nq, nq_next, nq_walk;
};
MPPI_HD PopWalk pop_walk(int Kp, int Kp_next) {
  const int a = Kp >> 2, b = Kp_next >> 2;
  return PopWalk{a, b, a > b ? a : b};
}
// the walk's predicates for quad q = q0 + 64 j of a tile
MPPI_HD bool pop_reads(const PopWalk& w, int q) { return q < w.nq; }
MPPI_HD bool pop_writes(const PopWalk& w, int q) { return q < w.nq_next; }
