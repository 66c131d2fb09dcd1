// The adaptation of the full sampling covariance on the device (mppi_set_noise_cov_adapt): one step of Sigma [nu][nu]
// towards the weighted cross moments of one batch of solves (cross_moments.h), the clamp of its standard deviations,
// and the factors the generator and the control-cost term read (L, Sigma^-1), by the arithmetic of cov_factor
// (noise_cov.h).
//
// With S the law's Sigma (fp32, symmetric bit for bit) and mx[b][u][v] the cross moments of the batch's B solves:
//   any n_finite[b] == 0: nothing changes (the host controller skips a solve that reports MPPI_E_NONFINITE)
//   Mbar[u][v] = (mx[0][u][v] + mx[1][u][v] + ...) / (float)B             v <= u; na_sum's order (noise_adapt.h)
//   S1[u][v]   = fmaf(rate, Mbar[u][v], (1 - rate) * S[u][v])             v <= u, mirrored
//   s_u = sqrtf(S1[u][u]);  c_u = min(max(s_u, sigma_min), sigma_max);  g_u = c_u / s_u
//   S2[u][v]   = (S1[u][v] * g_u) * g_v   for v < u, mirrored;   S2[u][u] = (c_u == s_u) ? S1[u][u] : c_u * c_u
// The clamp scales row and column u together (a congruence): it clips the standard deviations and keeps the
// correlations and the positive definiteness.  S2 is then factored as cov_factor factors it -- in double, every
// product and difference its own statement, each element's chain in the same j order, L and Sinv rounded to fp32
// once, sigma_u = (float)sqrt((double)S2[u][u]) -- so the setter's host factor and this one agree bit for bit.
// The step is REJECTED whole (S, L, Sinv, sigma_u as they were; the caller counts it) when some s_u is not finite or
// not > 0, some pivot is not > 0 and finite, or some entry of Sigma^-1 leaves fp32.  rho is not adapted.
//
// The element functions below are the only statement of the rule: noise_cov_adapt_kernel (kernels_noise.hip) runs them
// with lane u owning row u (the factor column by column, Ld^-1 one column per lane, Sigma^-1 one row per lane),
// noise_cov_adapt_step runs them serially on the host (tests/native/cross_adapt_host.cpp, through g++), and
// mppi_hip.stats.adapt_noise_cov_f32 is the numpy restatement.
#pragma once
#include <math.h>

#include "noise_adapt.h"  // MPPI_HD, na_sum, na_finite

#if defined(__GNUC__) && !defined(__clang__)
#define NCA_FN __attribute__((optimize("fp-contract=off"))) MPPI_HD
#else
#define NCA_FN MPPI_HD
#endif
#if defined(__clang__)
#define NCA_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define NCA_NO_CONTRACT
#endif

// the settings of mppi_set_noise_cov_adapt, a kernel argument by value
struct NoiseCovAdapt {
  float rate, sigma_min, sigma_max;
};

// the batch mean of element idx of mx [B][nn]
NCA_FN float nca_mean(const float* mx, int B, int nn, int idx) {
  const float sum = na_sum(mx + idx, B, nn);
  return sum / (float)B;
}

NCA_FN float nca_blend(const NoiseCovAdapt& a, float s, float mbar) {
  NCA_NO_CONTRACT
  const float keep = 1.0f - a.rate;
  const float old_part = keep * s;
  return fmaf(a.rate, mbar, old_part);
}

NCA_FN bool nca_scale_ok(float s) { return na_finite(s) && s > 0.0f; }

NCA_FN float nca_clamp(const NoiseCovAdapt& a, float s) {
  float c = s < a.sigma_min ? a.sigma_min : s;
  c = c > a.sigma_max ? a.sigma_max : c;
  return c;
}

NCA_FN float nca_gain(float c, float s) { return c / s; }

NCA_FN float nca_offdiag(float s1, float gu, float gv) {
  NCA_NO_CONTRACT
  const float t = s1 * gu;
  return t * gv;
}

NCA_FN float nca_diag(float s1, float s, float c) {
  NCA_NO_CONTRACT
  return c == s ? s1 : c * c;
}

// cov_factor's chain of element (u, v <= u): a = S[u][v] - sum_{j < v} Ld[u][j] Ld[v][j], j ascending.  Lu / Lv: rows
// u and v of Ld.  The diagonal takes sqrt(a) (nca_pivot_ok first), the others a / Ld[v][v]
NCA_FN double nca_chol_chain(const double* Lu, const double* Lv, int v, float s) {
  NCA_NO_CONTRACT
  double a = (double)s;
  for (int j = 0; j < v; ++j) {
    const double p = Lu[j] * Lv[j];
    a = a - p;
  }
  return a;
}

NCA_FN bool nca_pivot_ok(double a) { return a > 0.0 && fabs(a) <= 1.7976931348623157e308; }

// cov_factor's forward substitution: element (r, c <= r) of Wd = Ld^-1, given its column's entries c .. r - 1
NCA_FN double nca_winv_elem(const double* Ld, const double* Wd, int ld, int r, int c) {
  NCA_NO_CONTRACT
  double a = r == c ? 1.0 : 0.0;
  for (int j = c; j < r; ++j) {
    const double p = Ld[r * ld + j] * Wd[j * ld + c];
    a = a - p;
  }
  return a / Ld[r * ld + r];
}

// cov_factor's element (u, v <= u) of Sigma^-1 = Wd^T Wd
NCA_FN double nca_sinv_elem(const double* Wd, int ld, int nu, int u, int v) {
  NCA_NO_CONTRACT
  double a = 0.0;
  for (int j = u; j < nu; ++j) {
    const double p = Wd[j * ld + u] * Wd[j * ld + v];
    a = a + p;
  }
  return a;
}

NCA_FN bool nca_sinv_ok(double a) { return na_finite((float)a); }

NCA_FN float nca_sigma(float s2_diag) { return (float)sqrt((double)s2_diag); }

// The whole step for one batch, in place (the CPU form of noise_cov_adapt_kernel): S, L, Sinv [nu][nu] and sigma_u [nu]
// updated from mx [B][nu][nu] and n_finite[B] (element stride nf_stride).  nu <= 32; scratch: 2 nu nu doubles.
// Returns 0 if the law was left unchanged for a solve without a finite cost, 1 if it moved, -1 if the step was
// rejected (nothing written).
inline int noise_cov_adapt_step(const NoiseCovAdapt& a, float* S, float* L, float* Sinv, float* sigma_u,
                                const float* mx, const int* n_finite, int nf_stride, int B, int nu, double* scratch) {
  for (int b = 0; b < B; ++b)
    if (n_finite[(long)b * nf_stride] == 0) return 0;
  float S1[32 * 32], S2[32 * 32], Si[32 * 32], s[32], c[32], g[32];
  const int nn = nu * nu;
  for (int u = 0; u < nu; ++u)
    for (int v = 0; v <= u; ++v) S1[u * nu + v] = nca_blend(a, S[u * nu + v], nca_mean(mx, B, nn, u * nu + v));
  for (int u = 0; u < nu; ++u) {
    s[u] = sqrtf(S1[u * nu + u]);
    if (!nca_scale_ok(s[u])) return -1;
    c[u] = nca_clamp(a, s[u]);
    g[u] = nca_gain(c[u], s[u]);
  }
  for (int u = 0; u < nu; ++u) {
    for (int v = 0; v < u; ++v) S2[u * nu + v] = S2[v * nu + u] = nca_offdiag(S1[u * nu + v], g[u], g[v]);
    S2[u * nu + u] = nca_diag(S1[u * nu + u], s[u], c[u]);
  }
  double* Ld = scratch;
  double* Wd = scratch + nn;
  for (int i = 0; i < nn; ++i) Ld[i] = Wd[i] = 0.0;
  for (int v = 0; v < nu; ++v)  // column by column, as the device runs it: each element's chain is cov_factor's
    for (int u = v; u < nu; ++u) {
      const double x = nca_chol_chain(Ld + u * nu, Ld + v * nu, v, S2[u * nu + v]);
      if (u == v) {
        if (!nca_pivot_ok(x)) return -1;
        Ld[v * nu + v] = sqrt(x);
      } else {
        Ld[u * nu + v] = x / Ld[v * nu + v];
      }
    }
  for (int col = 0; col < nu; ++col)
    for (int r = col; r < nu; ++r) Wd[r * nu + col] = nca_winv_elem(Ld, Wd, nu, r, col);
  for (int u = 0; u < nu; ++u)
    for (int v = 0; v <= u; ++v) {
      const double x = nca_sinv_elem(Wd, nu, nu, u, v);
      if (!nca_sinv_ok(x)) return -1;
      Si[u * nu + v] = Si[v * nu + u] = (float)x;
    }
  for (int u = 0; u < nu; ++u) {
    for (int v = 0; v < nu; ++v) {
      S[u * nu + v] = S2[u * nu + v];
      L[u * nu + v] = v <= u ? (float)Ld[u * nu + v] : 0.0f;
      Sinv[u * nu + v] = Si[u * nu + v];
    }
    sigma_u[u] = nca_sigma(S2[u * nu + u]);
  }
  return 1;
}
