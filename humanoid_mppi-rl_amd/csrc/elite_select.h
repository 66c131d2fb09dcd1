// Elite truncation (mppi_set_elites): the softmin weighs only the n_elite best samples of a solve.  This header is the
// only statement of the rule: elite_select_kernel (kernels_elite.hip) runs it with one block per solve,
// tests/native/elite_select_host.cpp runs elite_select_row on the host, and mppi_hip.stats.elite_select_ref is the
// numpy restatement (a stable argsort over the finite costs).
//
// For solve b with c[0..K) the costs the softmin would otherwise weigh (costs [+ control-cost term] [+ rate term]; pad
// lanes K..Kp never counted):
//   F = {k : ess_finite(c_k)},  n = |F|            (NaN, +inf and -inf are not finite)
//   m = min(n_elite, n)
//   F is ordered by the pair (elite_key(c_k), k): cost first, the lower index on equal cost.  elite_key adds 0.0f
//   (so -0.0f and +0.0f share a key) and maps the float's bits to a uint32 whose unsigned order is the floats' order;
//   denormals keep their value (nothing is flushed).
//   E     = the first m samples of that order: exactly m members, ties at the threshold admitted by ascending k
//   tau   = the m-th smallest cost as elite_key orders it (a zero reads +0.0f), +inf when n == 0
//   ecost[k] = c[k] bit for bit on E, +inf elsewhere (non-finite inputs and the pads K..Kp included)
//   idx[0..m) = the members of E in ascending k, idx[m..n_elite) = -1;  count = m
// Consequences: the lowest k attaining the minimum (the statistics' k_best) is always elite; with n_elite >= n the
// set of weighted samples is F, what it is without the feature; n == 0 leaves every ecost +inf, so the solve reports
// MPPI_E_NONFINITE as before.
// Everything is integer work on the keys: the device and the host agree exactly, and runs repeat bitwise.
#pragma once
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "ess_target.h"  // MPPI_HD, ess_finite

constexpr uint32_t kEliteNoKey = 0xFFFFFFFFu;  // above every finite cost's key (FLT_MAX: 0xFF7FFFFF): never selected

// finite c -> uint32, ascending with c; -0.0f and +0.0f alike
MPPI_HD uint32_t elite_key(float c) {
  const float z = c + 0.0f;  // -0.0f + 0.0f = +0.0f; every other value unchanged, denormals included
  uint32_t u;
  __builtin_memcpy(&u, &z, 4);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// the key of a sample as the selection sees it: non-finite costs sort behind every finite one and are never elite
MPPI_HD uint32_t elite_key_or_none(float c) { return ess_finite(c) ? elite_key(c) : kEliteNoKey; }

// the cost a key stands for (the canonical one: +0.0f for either zero)
MPPI_HD float elite_key_cost(uint32_t key) {
  const uint32_t u = (key & 0x80000000u) ? (key & 0x7FFFFFFFu) : ~key;
  float c;
  __builtin_memcpy(&c, &u, 4);
  return c;
}

// The host form of one solve: costs c[0..K) -> m.  idx [n_elite], tau [1] and ecost [K] may each be nullptr.
inline int elite_select_row(const float* c, int K, int n_elite, int32_t* idx, float* tau, float* ecost) {
  std::vector<uint64_t> order;  // (key, k) packed: one integer sort gives the pair order
  order.reserve((size_t)K);
  for (int k = 0; k < K; ++k)
    if (ess_finite(c[k])) order.push_back(((uint64_t)elite_key(c[k]) << 32) | (uint32_t)k);
  std::sort(order.begin(), order.end());
  const int n = (int)order.size();
  const int m = n_elite < n ? n_elite : n;
  if (tau) *tau = m > 0 ? elite_key_cost((uint32_t)(order[(size_t)m - 1] >> 32)) : INFINITY;
  std::vector<int32_t> members((size_t)m);
  for (int i = 0; i < m; ++i) members[(size_t)i] = (int32_t)(order[(size_t)i] & 0xFFFFFFFFu);
  std::sort(members.begin(), members.end());
  if (ecost) {
    for (int k = 0; k < K; ++k) ecost[k] = INFINITY;
    for (int i = 0; i < m; ++i) ecost[members[(size_t)i]] = c[members[(size_t)i]];
  }
  if (idx)
    for (int i = 0; i < n_elite; ++i) idx[i] = i < m ? members[(size_t)i] : -1;
  return m;
}
