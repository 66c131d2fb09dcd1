// Best sample of a control step (mppi_set_iterations): while a step runs its inner iterations, the best SAMPLED control
// sequence seen so far is tracked on the device -- what iCEM executes (return_best) and the planned-trajectory read-out
// (mppi_get_best).  This header is the only statement of the rule: iter_best_kernel (kernels_iter.hip) runs it on the
// device with one block per solve, tests/native/iter_best_host.cpp runs iter_best_row on the host, and
// mppi_hip.stats.iter_best_ref is the numpy restatement.  The rule is integer work on the cost keys, one strict fp32
// comparison and, per stored element, one add (rate_cost_v: the control the rollout applied, with its clamp),
// contraction off: all three agree bitwise.
//
// In iteration `it` of a step, behind the cost terms and the elite / keep selection, ahead of the lambda search and
// the reduce (U is still the nominal the rollout perturbed).  For solve b, with c[0..K) the costs the softmin would
// weigh ahead of any elite masking (costs [+ control-cost term] [+ rate term]; the keep store's input; the pad lanes
// K..Kp never counted) and eps' the noise as the rollout saw it (injected, then projected):
//   k*  = the first sample by (elite_key(c_k), k) over the finite costs: elite_select.h's order with n = 1 (-0 equals
//         +0, the lowest k wins a tie); no finite cost: no candidate
//   reset (the step's first iteration), ahead of the candidate: bcost = +inf, bk = -1, biter = -1, bv = +0.0
//   the candidate is accepted iff c[k*] < bcost, strict in fp32: a carried elite that reproduces its cost keeps the
//   earlier iteration.  On acceptance
//     bcost = c[k*] bit for bit,  bk = k*,  biter = it
//     bv[u][t] = rate_cost_v(U[u][t], eps'[u][t][k*], ctrl_clamp)      the control the rollout applied
//   otherwise the stored best stays, bit for bit.
#pragma once
#include <math.h>
#include <stdint.h>

#include "elite_select.h"  // elite_key: the order of the costs
#include "rate_cost.h"     // rate_cost_v: the control the rollout applied

constexpr uint64_t kIterNoCand = 0xFFFFFFFFFFFFFFFFull;  // above every candidate: no finite cost

// (key, k) of one sample as a single integer: its unsigned order is the pair order; a non-finite cost is no candidate
MPPI_HD uint64_t iter_best_pack(float c, int k) {
  return ess_finite(c) ? (((uint64_t)elite_key(c) << 32) | (uint32_t)k) : kIterNoCand;
}

// the sample a packed minimum stands for (-1: no candidate)
MPPI_HD int iter_best_k(uint64_t packed) { return packed == kIterNoCand ? -1 : (int)(uint32_t)(packed & 0xFFFFFFFFull); }

// whether a candidate of cost c replaces a stored best of cost bcost
MPPI_HD bool iter_best_accept(float c, float bcost) { return c < bcost; }

// The host form of one solve: U [nu][H], eps [nu][H][K] (k fastest), c [K]; v [nu][H], cost, k, iter in/out (read only
// with reset == 0).  Returns 1 if the candidate was accepted.
inline int iter_best_row(const float* U, const float* eps, const float* c, int nu, int H, int K, float clamp, int reset,
                         int it, float* v, float* cost, int32_t* k, int32_t* iter) {
  if (reset) {
    *cost = INFINITY;
    *k = -1;
    *iter = -1;
    for (int r = 0; r < nu * H; ++r) v[r] = 0.0f;
  }
  uint64_t best = kIterNoCand;
  for (int j = 0; j < K; ++j) {
    const uint64_t p = iter_best_pack(c[j], j);
    best = p < best ? p : best;
  }
  const int ks = iter_best_k(best);
  if (ks < 0 || !iter_best_accept(c[ks], *cost)) return 0;
  *cost = c[ks];
  *k = ks;
  *iter = it;
  for (int r = 0; r < nu * H; ++r) v[r] = rate_cost_v(U[r], eps[(long)r * K + ks], clamp);
  return 1;
}
