// The adaptation of the sampling law on the device (mppi_set_noise_adapt): one step of (sigma_u[nu], rho) towards the
// weighted noise moments of one batch of solves, the fp32 restatement of mppi_hip.stats.adapt_noise_model.
//
// With m2[b][u], m11[b][u] the moments of the batch's B solves (include/mppi.h eps_m2, eps_m11):
//   if any n_finite[b] == 0: the law is unchanged (the host controller skips a solve that reports MPPI_E_NONFINITE)
//   m2bar[u]  = (m2[0][u] + m2[1][u] + ...) / (float)B          sequential fp32 sums, b ascending; m11bar alike
//   var       = fmaf(rate, m2bar[u], (1 - rate) * (s * s))      s = sigma_u[u]
//   sigma_u[u] = min(max(sqrtf(var), sigma_min), sigma_max)     (a frozen actuator, s = 0, is clipped up to sigma_min,
//                                                                as the host rule does; sigma_min = 0 keeps it frozen)
//   den = m2bar[0] + m2bar[1] + ...,  num = m11bar[0] + ...     u ascending
//   rho_hat   = den > 0 ? clamp(num / den, 0, rho_max) : 0
//   rho       = fmaf(rate, rho_hat, (1 - rate) * rho);   c = ar1_innovation_scale(rho)
//   a non-finite var or rho leaves that entry as it was
// Every product, sum and difference is its own statement or an explicit fmaf (as in noise_model.h), so no compiler
// contracts them differently on the two sides.  This header is the only statement of the rule: noise_adapt_kernel
// (kernels_noise.hip) runs it with lane u owning actuator u, tests/test_noise_adapt.py runs it through g++, and
// mppi_hip.stats.adapt_noise_model_f32 is its numpy restatement.
#pragma once
#include <math.h>

#include "noise_model.h"  // MPPI_HD, ar1_innovation_scale

// the settings of mppi_set_noise_adapt, a kernel argument by value
struct NoiseAdapt {
  float rate, sigma_min, sigma_max, rho_max;
};

MPPI_HD bool na_finite(float x) { return fabsf(x) <= 3.402823466e+38f; }  // false for NaN and +-inf

// sum of v[0], v[stride], ..., n terms in ascending order.  The terms are read sixteen at a time ahead of the ordered
// chain of additions: the reads do not depend on one another, so on the device their latencies overlap (one lane
// adding 64 solves' moments pays 4 round trips to memory, not 64); the additions are the same, in the same order.
MPPI_HD float na_sum(const float* v, int n, int stride) {
  constexpr int kAhead = 16;
  float acc = 0.0f;
  int i = 0;
  for (; i + kAhead <= n; i += kAhead) {
    float x[kAhead];
    for (int j = 0; j < kAhead; ++j) x[j] = v[(long)(i + j) * stride];
    for (int j = 0; j < kAhead; ++j) acc = acc + x[j];
  }
  for (; i < n; ++i) acc = acc + v[(long)i * stride];
  return acc;
}

// mean over the batch of column u of m[B][nu]
MPPI_HD float na_mean(const float* m, int B, int nu, int u) {
  const float sum = na_sum(m + u, B, nu);
  return sum / (float)B;
}

MPPI_HD float na_sigma(const NoiseAdapt& a, float s, float m2bar) {
  const float keep = 1.0f - a.rate;
  const float s2 = s * s;
  const float old_part = keep * s2;
  const float var = fmaf(a.rate, m2bar, old_part);
  if (!na_finite(var)) return s;
  float r = sqrtf(var);
  if (!na_finite(r)) return s;  // (var < 0: moments about zero are never negative, a corrupted one leaves s)
  r = r < a.sigma_min ? a.sigma_min : r;
  r = r > a.sigma_max ? a.sigma_max : r;
  return r;
}

MPPI_HD float na_rho(const NoiseAdapt& a, float rho, float num, float den) {
  float rho_hat = 0.0f;
  if (den > 0.0f) {
    rho_hat = num / den;
    rho_hat = rho_hat < 0.0f ? 0.0f : rho_hat;
    rho_hat = rho_hat > a.rho_max ? a.rho_max : rho_hat;
  }
  const float keep = 1.0f - a.rate;
  const float old_part = keep * rho;
  const float r = fmaf(a.rate, rho_hat, old_part);
  return na_finite(r) ? r : rho;
}

// The whole step for one batch, in place (the CPU form of noise_adapt_kernel): sigma_u[nu], *rho, *c updated from
// m2 / m11 [B][nu] and n_finite[B] (element stride nf_stride: the device reads it out of mppi_solve_stats records).
// nu <= 32.  Returns 0 if the law was left unchanged for a solve without a finite cost, else 1.
MPPI_HD int noise_adapt_step(const NoiseAdapt& a, float* sigma_u, float* rho, float* c, const float* m2,
                             const float* m11, const int* n_finite, int nf_stride, int B, int nu) {
  for (int b = 0; b < B; ++b)
    if (n_finite[(long)b * nf_stride] == 0) return 0;
  float m2bar[32], m11bar[32];
  for (int u = 0; u < nu; ++u) {
    m2bar[u] = na_mean(m2, B, nu, u);
    m11bar[u] = na_mean(m11, B, nu, u);
    sigma_u[u] = na_sigma(a, sigma_u[u], m2bar[u]);
  }
  const float den = na_sum(m2bar, nu, 1);
  const float num = na_sum(m11bar, nu, 1);
  *rho = na_rho(a, *rho, num, den);
  *c = ar1_innovation_scale(*rho);
  return 1;
}
