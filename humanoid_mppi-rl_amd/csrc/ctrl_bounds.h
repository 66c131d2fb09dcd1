// Per-actuator control bounds (mppi_set_control_bounds): the box [lo[u], hi[u]] every sampled control U + eps and the
// nominal U itself stay inside.  The rollouts compute U + eps themselves, so the solve's noise is PROJECTED ahead of
// them (pytorch_mppi's rule): the buffer holds eps' = clip(U + eps, lo, hi) - U, and the reduce, the control-cost term,
// the statistics and the noise adaptation describe the controls that were evaluated.  For one element, in fp32:
//   s = U + eps                     (one add)
//   s <  lo : eps' = lo - U         (one subtract)   counted
//   s >  hi : eps' = hi - U                          counted
//   else    : eps' = eps            (untouched, bit for bit; a NaN s lands here: both comparisons are false)
// An element inside the box is never rewritten, so a solve whose box never binds is bit for bit the solve without bounds.
// Consequently U + eps' is WITHIN ONE ROUNDING of the bound, not always equal to it: fl(U + fl(lo - U)) can miss lo by
// one ulp of the larger operand.  The nominal is held to the box exactly by ctrl_bounds_clip behind the update.
// +inf noise projects to hi - U; lo = -inf / hi = +inf leave that side unbounded (no s is beyond them); lo == hi pins
// the actuator (s == lo is inside).  A U outside the box projects every finite element of its row.
// This header is the only statement of the rule: bounds_project_kernel / bounds_clip_kernel (kernels_bounds.hip) run it
// on the device, tests/native/ctrl_bounds_host.cpp on the host, mppi_hip.stats.project_noise_ref is its numpy
// restatement.  The rule is a select and one subtract (no product: nothing to contract), so all three agree bitwise.
#pragma once
#include <math.h>

#include "philox.h"  // MPPI_HD

// eps' of one element; *hit = 1 when it was projected (counted), else 0
MPPI_HD float ctrl_bounds_project(float U, float eps, float lo, float hi, int* hit) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float s = U + eps;
  if (s < lo) {
    *hit = 1;
    return lo - U;
  }
  if (s > hi) {
    *hit = 1;
    return hi - U;
  }
  *hit = 0;
  return eps;
}

// the nominal's clip (U, u0 behind the update): exact, NaN stays NaN
MPPI_HD float ctrl_bounds_clip(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }

// lo[u] <= hi[u] and neither a NaN, for all u (what mppi_set_control_bounds accepts)
MPPI_HD int ctrl_bounds_valid(const float* lo, const float* hi, int nu) {
  for (int u = 0; u < nu; ++u)
    if (!(lo[u] <= hi[u])) return 0;
  return 1;
}

// a whole (b, u) row on the host: eps [H][K] in place against U [H]; returns the count
inline unsigned ctrl_bounds_project_row(const float* U, float* eps, float lo, float hi, int H, int K) {
  unsigned n = 0;
  for (int t = 0; t < H; ++t)
    for (int k = 0; k < K; ++k) {
      int hit;
      eps[(long)t * K + k] = ctrl_bounds_project(U[t], eps[(long)t * K + k], lo, hi, &hit);
      n += (unsigned)hit;
    }
  return n;
}
