// ESS targeting (mppi_set_ess_target): per solve, the softmin temperature lambda_b in [lambda_min, lambda_max] at which
// the solve's own costs give a requested effective sample size.  This header is the only statement of the rule:
// lambda_search_kernel (kernels_lambda.hip) runs it with one block per solve, tests/native/ess_target_host.cpp runs it
// on the host, and mppi_hip.stats.ess_lambda_ref is its float64 restatement (the true root, same end rules).
//
// For solve b with costs c[0..K) (pad lanes never counted):
//   F = {k : isfinite(c_k)},  n = |F|,  beta = min_F c
//   wt_k(lambda) = expf(-(1 / lambda) * (c_k - beta)) on F, 0 elsewhere     (reduce_kernel's own weight expression)
//   ESS(lambda)  = (sum wt)^2 / sum wt^2                                    fp32, summed in a fixed order
//   T            = max(1, ess_frac * n)
//   n == 0:                     lambda_b = cfg.lambda  (the solve reports MPPI_E_NONFINITE as before)
//   ESS(lambda_min) >= T:       lambda_b = lambda_min  (ties at the minimum, n == 1, all costs equal)
//   ESS(lambda_max) <  T:       lambda_b = lambda_max
//   otherwise a bracketing search that keeps ESS(lo) < T <= ESS(hi) on the fp32 evaluations it actually made, ends with
//   hi <= lo * (1 + 2^-19) (hi / lo <= 1 + 2e-6) and returns hi.
// The search evaluates NC candidates inside (lo, hi) per pass -- geometric while hi / lo > 2, arithmetic below, where
// the two spacings agree and the arithmetic one still separates candidates one ulp apart -- and keeps the first
// candidate pair that brackets T.  NC = 1 is plain bisection (~24 passes for lambda_max / lambda_min = 1e8), NC = 15 cuts the
// bracket's log-width 16x per pass (~6 passes): a pass costs one block-wide reduction whatever NC is.
// The search is stateless: lambda_b depends on nothing but that solve's costs and the three settings.
#pragma once
#include <math.h>

#include "noise_model.h"  // MPPI_HD

// the settings of mppi_set_ess_target, a kernel argument by value (ess_frac == 0: targeting is off)
struct EssTarget {
  float ess_frac, lambda_min, lambda_max;
};

constexpr float kEssBracket = 1.0f + 0x1p-19f;  // the final hi / lo (16 ulps: 1 + 1.9e-6)
constexpr int kEssMaxPasses = 64;               // (every pass at least halves the bracket: never reached)

MPPI_HD bool ess_finite(float x) { return fabsf(x) <= 3.402823466e+38f; }  // false for NaN and +-inf

MPPI_HD float ess_target_count(float ess_frac, int n) {
  const float t = ess_frac * (float)n;
  return t > 1.0f ? t : 1.0f;
}

// Candidate j of NC inside (lo, hi), ascending in j, for hi > lo * kEssBracket; a closed form in j, so lane j of a wave
// computes its own.  ends: the first pass, which evaluates the two ends instead (j == 0: lo, every other j: hi).
template <int NC>
MPPI_HD float ess_candidate(float lo, float hi, int j, bool ends) {
  if (ends) return j == 0 ? lo : hi;
  const float frac = (float)(j + 1) / (float)(NC + 1);
  float v;
  if (hi > 2.0f * lo) {
    v = lo * exp2f(log2f(hi / lo) * frac);  // steps of >= 2^(1/16): far above the rounding of exp2f / log2f
  } else {
    const float w = hi - lo;  // exact (hi <= 2 lo), >= 16 ulps of lo
    v = lo + w * frac;
  }
  v = v > lo ? v : lo;  // (a candidate rounded onto an end re-evaluates that end: the same value, the same decision)
  return v < hi ? v : hi;
}

// mask bit j: ESS(candidate j) >= T.  The first candidate at or above the target becomes hi, the one below it lo.
template <int NC>
MPPI_HD void ess_narrow(unsigned mask, float& lo, float& hi) {
  int first = NC;
  for (int j = NC - 1; j >= 0; --j)
    if (mask & (1u << j)) first = j;
  const float new_hi = first < NC ? ess_candidate<NC>(lo, hi, first, false) : hi;
  const float new_lo = first > 0 ? ess_candidate<NC>(lo, hi, first - 1, false) : lo;
  lo = new_lo;
  hi = new_hi;
}

// eval(lo, hi, ends) -> mask over the NC candidates ess_candidate<NC>(lo, hi, j, ends) (bit j: ESS(candidate j) >= T),
// every candidate evaluated with the same arithmetic.  On the device eval is block-collective and every thread gets
// the same mask, so the control flow is uniform.
template <int NC, class Eval>
MPPI_HD float ess_search(const EssTarget& s, Eval&& eval) {
  unsigned at_min, at_max;
  if constexpr (NC >= 2) {  // both ends in one pass
    const unsigned m = eval(s.lambda_min, s.lambda_max, true);
    at_min = m & 1u;
    at_max = m & 2u;
  } else {
    at_min = eval(s.lambda_min, s.lambda_min, true) & 1u;
    at_max = eval(s.lambda_max, s.lambda_max, true) & 1u;
  }
  if (at_min) return s.lambda_min;
  if (!at_max) return s.lambda_max;
  float lo = s.lambda_min, hi = s.lambda_max;
  for (int pass = 0; pass < kEssMaxPasses && hi > lo * kEssBracket; ++pass) {
    const unsigned m = eval(lo, hi, false);
    ess_narrow<NC>(m, lo, hi);
  }
  return hi;
}

// ESS(lambda) >= T for one solve on the host: fixed-order fp32 sums, expf where the device has __expf
inline bool ess_reaches_host(const float* c, int K, float beta, float lambda, float T) {
  const float inv_lam = 1.0f / lambda;
  float S = 0.0f, S2 = 0.0f;
  for (int k = 0; k < K; ++k) {
    const float wt = ess_finite(c[k]) ? expf(-inv_lam * (c[k] - beta)) : 0.0f;
    S = S + wt;
    S2 = fmaf(wt, wt, S2);
  }
  const float sq = S * S;
  return sq / S2 >= T;
}

// The host form of one solve: costs c[0..K).  passes (or nullptr): the evaluations (block-wide reductions) it took.
template <int NC>
inline float ess_lambda_host(const EssTarget& s, float cfg_lambda, const float* c, int K, int* passes = nullptr) {
  if (passes) *passes = 0;
  int n = 0;
  float beta = INFINITY;
  for (int k = 0; k < K; ++k)
    if (ess_finite(c[k])) {
      n += 1;
      beta = c[k] < beta ? c[k] : beta;
    }
  if (n == 0) return cfg_lambda;
  const float T = ess_target_count(s.ess_frac, n);
  return ess_search<NC>(s, [&](float lo, float hi, bool ends) {
    if (passes) *passes += 1;
    unsigned mask = 0;
    for (int j = 0; j < NC; ++j)
      if (ess_reaches_host(c, K, beta, ess_candidate<NC>(lo, hi, j, ends), T)) mask |= 1u << j;
    return mask;
  });
}
