// The control-rate (smoothness) cost term (mppi_set_rate_cost): a penalty on how fast the SAMPLED control sequence
// changes, added to the costs the softmin weighs,
//   v[u][t]  = U[u][t] + eps'[u][t]            the control the rollout applied: fp32, one rounding, then the rollouts'
//                                              own clamp to +-ctrl_clamp when ctrl_clamp > 0
//   v[u][-1] = u_prev[u]                       the control applied the step before (anchor on; used as stored)
//   rate     = sum_u r[u] sum_{t = t0..H-1} (v[u][t] - v[u][t-1])^2            t0 = 0 with the anchor, 1 without
// with r[u] >= 0 per actuator.  This header is the only statement of the fp32 rule per element: the term kernels
// (kernels_rate_cost.hip) run it on the device, tests/native/rate_cost_host.cpp on the host,
// mppi_hip.stats.rate_term_ref is the float64 restatement.
//
// EVERY row enters the sum as one fmaf, a row with r[u] == 0 included, and so does the first row of an actuator without
// the anchor, whose difference is taken against itself: it adds an exact 0 when v is finite (so H == 1 without the
// anchor gives exactly 0) and a NaN when it is not.  A non-finite eps' on ANY row therefore makes its sample's term
// non-finite.  With a clamp an infinite sum would clamp to a finite control, as in the rollouts; rate_cost_v adds
// s - s (an exact 0 for every finite s, NaN otherwise) so that such a sample is non-finite here too.
//
// Roundings (u = 2^-24) per summand r d^2: one for d, one for q = r d, one for the fmaf that adds q d; v itself is
// the value the rollout used, not an approximation of one.  All summands are >= 0, so n of them summed in any order
// stay within (n + 4) u / (1 - (n + 4) u) of the exact sum of r (v_t - v_t-1)^2: the tests' bound.
// Every product and sum is its own statement or an explicit fmaf, contraction off: host and device agree bit for bit.
#pragma once
#include <math.h>

#include "philox.h"  // MPPI_HD

// the sampled control of one element: U + eps, clamped as the rollouts clamp it (clamp <= 0: none)
MPPI_HD float rate_cost_v(float U, float eps, float clamp) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float s = U + eps;
  if (!(clamp > 0.0f)) return s;
  const float c = fminf(clamp, fmaxf(-clamp, s));
  const float z = s - s;  // 0, or NaN for a non-finite s
  return c + z;
}

// one summand: acc + r (v - prev)^2
MPPI_HD float rate_cost_add(float r, float v, float prev, float acc) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float d = v - prev;
  const float q = r * d;
  return fmaf(q, d, acc);
}

// the term of one sample in plain row order (the CPU form; the kernels sum the same summands cell by cell):
// U [nu][H], eps [nu][H] with element (u, t) at eps[(u * H + t) * stride], r [nu], u_prev [nu] (read with anchor only)
MPPI_HD float rate_cost_sample(const float* U, const float* eps, long stride, const float* r, const float* u_prev,
                               int anchor, float clamp, int nu, int H) {
  float acc = 0.0f;
  for (int u = 0; u < nu; ++u) {
    float prev = 0.0f;
    for (int t = 0; t < H; ++t) {
      const float v = rate_cost_v(U[u * H + t], eps[((long)u * H + t) * stride], clamp);
      if (t == 0) prev = anchor ? u_prev[u] : v;
      acc = rate_cost_add(r[u], v, prev, acc);
      prev = v;
    }
  }
  return acc;
}

// r as mppi_set_rate_cost accepts it: finite, every entry >= 0, at least one > 0
MPPI_HD bool rate_cost_valid(const float* r, int nu) {
  bool any = false;
  for (int u = 0; u < nu; ++u) {
    if (!(r[u] >= 0.0f) || isinf(r[u])) return false;
    any = any || r[u] > 0.0f;
  }
  return any;
}
