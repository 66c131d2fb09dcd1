// The refit of the per-step sampling scale on the device (mppi_set_noise_steps_adapt): CEM's rule for the table
// S[b][u][t] of mppi_set_noise_steps, the fp32 restatement of mppi_hip.stats.adapt_noise_steps.
//
// Per solve b -- no batch mean: every solve owns its table -- with m1, m2 [nu][H] its per-step moments
// (step_moments.h) and S its row of the table:
//   n_finite[b] == 0: no cell of the solve is refit (the shift below still applies)
//   v  = centred ? fmaf(-m1, m1, m2) : m2          the weighted variance about the weighted mean, or about zero
//   a non-finite v leaves the cell as it was;   v = v > 0 ? v : 0   (the difference can round below zero)
//   S' = na_sigma({rate, sigma_min, sigma_max}, S, v)
//      = clamp(sqrtf(fmaf(rate, v, (1 - rate) * (S * S))), sigma_min, sigma_max)           (noise_adapt.h)
// and, if the solve carries MPPI_FLAG_SHIFT, the refitted row moves with the nominal:
//   S[t] <- S'[t + 1]  for t < H - 1;   S[H - 1] <- fill = sigma_u[u]   (H == 1: the one cell becomes the fill)
// Cell t of the new row reads cells t or t + 1 of the old one, never a lower one: a serial walk in ascending t may
// run in place, and a wave that reads a tile of 64 cells before it stores them may too (step_adapt_kernel).
//
// This header is the only statement of the rule: step_adapt_kernel (kernels_step_moments.hip) runs sl_cell with one
// wave per (b, u) row, tests/test_noise_steps.py runs step_law_row through g++, and
// mppi_hip.stats.adapt_noise_steps_f32 is its numpy restatement.
#pragma once
#include <math.h>

#include "noise_adapt.h"  // NoiseAdapt, na_sigma, na_finite

// the settings of mppi_set_noise_steps_adapt, a kernel argument by value
struct StepAdapt {
  float rate, sigma_min, sigma_max;
  int centred;
};

// one cell's refit from its own moments (live: the solve had a finite cost)
MPPI_HD float sl_refit(const StepAdapt& a, float s, float m1, float m2, bool live) {
  if (!live) return s;
  float v = m2;
  if (a.centred) {
    const float neg = -m1;
    v = fmaf(neg, m1, m2);
  }
  if (!na_finite(v)) return s;
  v = v > 0.0f ? v : 0.0f;
  const NoiseAdapt na = {a.rate, a.sigma_min, a.sigma_max, 0.0f};
  return na_sigma(na, s, v);
}

// cell t of the new row of one (b, u): S, m1, m2 the row's H cells as they stand
MPPI_HD float sl_cell(const StepAdapt& a, const float* S, const float* m1, const float* m2, int H, int t, bool shift,
                      float fill, bool live) {
  if (!shift) return sl_refit(a, S[t], m1[t], m2[t], live);
  if (t + 1 >= H) return fill;
  return sl_refit(a, S[t + 1], m1[t + 1], m2[t + 1], live);
}

// one row in place, ascending t (the CPU form of step_adapt_kernel's wave)
MPPI_HD void step_law_row(const StepAdapt& a, float* S, const float* m1, const float* m2, int H, bool shift, float fill,
                          bool live) {
  for (int t = 0; t < H; ++t) S[t] = sl_cell(a, S, m1, m2, H, t, shift, fill, live);
}
