// Dynamics-model ensembles (mppi_set_ensemble): every sample of a solve is rolled under each of n members -- n learned
// nets of one kind, or n parameter sets of the analytic cartpole -- and the members' costs are combined, per sample,
// into the one cost everything behind the rollout reads.  This header is the only statement of the combining rule:
// ensemble_kernel (kernels_ensemble.hip) runs it on the device, four samples per lane, tests/native/ensemble_host.cpp
// runs ensemble_row on the host, and mppi_hip.stats.ensemble_combine_f32 is the numpy restatement.  The rule is fp32,
// every sum, product and fmaf its own statement, contraction off: all three agree bit for bit.
//
// Per sample, with c_0 .. c_{n-1} the members' costs (2 <= n <= MPPI_ENS_MAX) and r = 1.0f / (float)n, computed once
// on the host and passed in:
//   any c_e not finite (NaN, +inf, -inf):  cost = +inf, sd = +inf
//   s = c_0;  s = s + c_e         e = 1 .. n-1 ascending;    m = s * r
//   every c_e bit for bit c_0:  m = c_0                      the mean of n equal numbers is that number
//   q = +0;   q = fmaf(c_e - m, c_e - m, q)   e = 0 .. n-1;  sd = sqrtf(q * r)       the population std
//   MPPI_ENS_MEAN      cost = m
//   MPPI_ENS_MEAN_STD  cost = fmaf(kappa, sd, m)             kappa < 0: an optimism bonus
//   MPPI_ENS_WORST     cost = max(.. max(c_0, c_1) .., c_{n-1})
//   a non-finite cost (a sum that overflowed) becomes +inf; a non-finite sd becomes +inf
// The maximum is fmaxf on finite operands with the one case C leaves open decided here: +0 is above -0 (IEEE 754-2019
// maximum), so host and device return the same zero.
// The line for equal members is what makes an ensemble of n identical models the single model: the sequential sum is
// exact for n in {2, 4} only (3 c is not always a float: fl(fl(3 c) r) != c for a third of the costs a rollout gives, and
// the spread about such an m is an ulp of c, not 0), and n c overflows where c does not.  With it n identical members
// give cost = c bit for bit and sd = +0 in every mode and for every n (MPPI_ENS_MEAN_STD: fmaf(kappa, +0, c), which is
// c but for c = -0, which comes out +0); where some member differs by a bit the line does not apply and the rule is the
// sums as written.  For n in {2, 4} it changes nothing but the overflow.
// The pad lanes K..Kp of a cost row go through the same rule and are never counted downstream.
#pragma once
#include <math.h>

#include "ess_target.h"  // MPPI_HD, ess_finite

#ifndef MPPI_ENS_MAX  // (include/mppi.h states them for the ABI)
#define MPPI_ENS_MAX 8
#define MPPI_ENS_MEAN 0
#define MPPI_ENS_MEAN_STD 1
#define MPPI_ENS_WORST 2
#endif

// 1 / n as the rule takes it: one fp32 division, on the host
inline float ensemble_rcp(int n) { return 1.0f / (float)n; }

// what mppi_set_ensemble and mppi_ensemble_eval accept
inline bool ensemble_mode_valid(int mode) { return mode == MPPI_ENS_MEAN || mode == MPPI_ENS_MEAN_STD || mode == MPPI_ENS_WORST; }
inline bool ensemble_kappa_valid(float kappa) { return ess_finite(kappa); }

// the larger of two finite costs; of two zeros, +0
MPPI_HD float ensemble_max(float a, float b) {
  return a < b ? b : (b < a ? a : (__builtin_signbitf(a) ? b : a));
}

MPPI_HD unsigned ensemble_bits(float x) {
  unsigned u;
  __builtin_memcpy(&u, &x, 4);
  return u;
}

// One sample: c[e * stride], e < n.  Returns the combined cost; *sd the members' spread.
MPPI_HD float ensemble_combine(const float* c, long stride, int n, float r, int mode, float kappa, float* sd) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  bool fin = true;
  for (int e = 0; e < n; ++e) fin = fin && ess_finite(c[e * stride]);
  if (!fin) {
    *sd = INFINITY;
    return INFINITY;
  }
  float s = c[0], mx = c[0];
  for (int e = 1; e < n; ++e) {
    s = s + c[e * stride];
    mx = ensemble_max(mx, c[e * stride]);
  }
  bool same = true;
  for (int e = 1; e < n; ++e) same = same && ensemble_bits(c[e * stride]) == ensemble_bits(c[0]);
  const float m = same ? c[0] : s * r;
  float q = 0.0f;
  for (int e = 0; e < n; ++e) {
    const float d = c[e * stride] - m;
    q = fmaf(d, d, q);
  }
  const float v = q * r;
  const float dev = sqrtf(v);
  float cost = m;
  if (mode == MPPI_ENS_MEAN_STD) cost = fmaf(kappa, dev, m);
  if (mode == MPPI_ENS_WORST) cost = mx;
  *sd = ess_finite(dev) ? dev : INFINITY;
  return ess_finite(cost) ? cost : INFINITY;
}

// The host form of one row of samples: members [n][stride] (stride >= K), cost and sd [K].
inline void ensemble_row(const float* members, long stride, int n, int K, int mode, float kappa, float* cost, float* sd) {
  const float r = ensemble_rcp(n);
  for (int k = 0; k < K; ++k) cost[k] = ensemble_combine(members + k, stride, n, r, mode, kappa, &sd[k]);
}
