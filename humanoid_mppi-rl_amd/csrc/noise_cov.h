// Cross-actuator sampling covariance (mppi_set_noise_cov): the perturbations of one (b, t, k) are drawn with a full
// nu x nu covariance Sigma across the actuators (the Sigma of information-theoretic MPPI; pytorch_mppi's noise_sigma)
// instead of one independent scale per actuator.
//
// The factor.  The caller passes Sigma [nu][nu] in fp32: finite, symmetric bit for bit, and positive definite in the
// sense that every pivot below is > 0 and finite.  It is factored once on the host, in double, row by row
// (Cholesky-Banachiewicz), every product and difference its own statement:
//   for u in 0..nu-1: for v in 0..u:
//     a = (double)Sigma[u][v];   for j in 0..v-1:  p = Ld[u][j] * Ld[v][j];  a = a - p
//     u == v:  require a > 0 and finite,  Ld[u][u] = sqrt(a)         else:  Ld[u][v] = a / Ld[v][v]
//   L[u][v] = (float)Ld[u][v]  (rounded once, after the whole factorisation);   L[u][v] = 0 for v > u
// Sinv = Sigma^-1 comes from Ld in double (Ld^-1 by forward substitution, then Ld^-T Ld^-1) and is rounded to fp32 once;
// it is symmetric bit for bit.  sigma_u[u] = (float)sqrt((double)Sigma[u][u]) is the per-actuator scale the model
// reports (mppi_get_noise_model) and continues with when the covariance is disabled.
//
// The noise.  e_v[t] is the handle's unit-variance AR(1) row of actuator v (noise_model.h, unchanged: the normals at
// Philox counter (k/4, t, v, b), rho = 0: the normals themselves).  The mix is fp32, in this fixed order:
//   acc = L[u][0] * e_0[t];    acc = fmaf(L[u][v], e_v[t], acc)   v = 1..u;    eps[b][u][t][k] = acc
// sigma_u does not enter again.  Sigma = I gives eps == e (a signed zero aside); nu == 1 gives L[0][0] * e_0.
// cov(eps[:, t], eps[:, s]) = Sigma * rho^|t-s|.
//
// Host + device (the MPPI_HD style of noise_model.h / noise_knots.h): tests/test_noise_cov.py runs the factor and the
// mix through g++; noise_cov_kernel (kernels_noise.hip) runs the chain of cov_mix on quads of k.
#pragma once
#include <math.h>

#include "noise_model.h"  // MPPI_HD

// Sigma [nu][nu] -> L [nu][nu] (lower, the strict upper triangle 0), Sinv [nu][nu], sigma_u [nu] (each may be null);
// scratch: Ld [nu][nu], Wd [2][nu][nu] doubles.  false (nothing written but the scratch) when Sigma is not finite, not
// symmetric bit for bit or a pivot is not > 0 and finite.  Host only; no operation of it may be contracted into an fma
#if defined(__GNUC__) && !defined(__clang__)
__attribute__((optimize("fp-contract=off")))
#endif
inline bool cov_factor(const float* Sigma, int nu, float* L, float* Sinv, float* sigma_u, double* Ld, double* Wd) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  for (int u = 0; u < nu; ++u)
    for (int v = 0; v < nu; ++v) {
      if (!isfinite(Sigma[u * nu + v])) return false;
      if (!(Sigma[u * nu + v] == Sigma[v * nu + u])) return false;
    }
  for (int i = 0; i < nu * nu; ++i) Ld[i] = 0.0;
  for (int u = 0; u < nu; ++u)
    for (int v = 0; v <= u; ++v) {
      double a = (double)Sigma[u * nu + v];
      for (int j = 0; j < v; ++j) {
        const double p = Ld[u * nu + j] * Ld[v * nu + j];
        a = a - p;
      }
      if (u == v) {
        if (!(a > 0.0) || !isfinite(a)) return false;
        Ld[u * nu + u] = sqrt(a);
      } else {
        Ld[u * nu + v] = a / Ld[v * nu + v];
      }
    }
  // Wd = Ld^-1 (lower), column by column by forward substitution
  for (int i = 0; i < nu * nu; ++i) Wd[i] = 0.0;
  for (int c = 0; c < nu; ++c)
    for (int r = c; r < nu; ++r) {
      double a = r == c ? 1.0 : 0.0;
      for (int j = c; j < r; ++j) {
        const double p = Ld[r * nu + j] * Wd[j * nu + c];
        a = a - p;
      }
      Wd[r * nu + c] = a / Ld[r * nu + r];
    }
  double* Sd = Wd + nu * nu;  // Sigma^-1 = Wd^T Wd, in double
  for (int u = 0; u < nu; ++u)
    for (int v = 0; v <= u; ++v) {
      double a = 0.0;
      for (int j = u; j < nu; ++j) {
        const double p = Wd[j * nu + u] * Wd[j * nu + v];
        a = a + p;
      }
      if (!isfinite((float)a)) return false;  // (an inverse that leaves fp32: no usable control-cost coefficients)
      Sd[u * nu + v] = a;
      Sd[v * nu + u] = a;
    }
  for (int u = 0; u < nu; ++u)
    for (int v = 0; v < nu; ++v) {
      if (L) L[u * nu + v] = v <= u ? (float)Ld[u * nu + v] : 0.0f;
      if (Sinv) Sinv[u * nu + v] = (float)Sd[u * nu + v];
    }
  if (sigma_u)
    for (int u = 0; u < nu; ++u) sigma_u[u] = (float)sqrt((double)Sigma[u * nu + u]);
  return true;
}

// one element of the mix: row u of L (its entries 0..u) over e[v * stride], v = 0..u
MPPI_HD float cov_mix(const float* Lrow, int u, const float* e, int stride) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  float acc = Lrow[0] * e[0];
  for (int v = 1; v <= u; ++v) acc = fmaf(Lrow[v], e[(long)v * stride], acc);
  return acc;
}

// a whole column eps[0..nu) of one (b, t, k) from e[0..nu) (the CPU form of noise_cov_kernel's walk over v)
MPPI_HD void cov_mix_column(const float* L, int nu, const float* e, int e_stride, float* eps, int eps_stride) {
  for (int u = 0; u < nu; ++u) eps[(long)u * eps_stride] = cov_mix(L + u * nu, u, e, e_stride);
}
