// The control-cost term of information-theoretic MPPI (mppi_set_control_cost): the importance-sampling correction for
// sampling around a non-zero nominal U.  The softmin weighs
//   S~_k = S_k + gamma * sum_{u,t} U[u][t] * (Sigma^-1 eps_k)[u][t]
// with Sigma the covariance of the law that drew eps: per actuator sigma_u[u]^2 times the unit-variance AR(1) row
// covariance C[t][s] = rho^|t-s| (noise_model.h).  Its inverse P = C^-1 is tridiagonal:
//   H >= 2:  P = 1/(1 - rho^2) * tridiag(-rho; [1, 1 + rho^2, ..., 1 + rho^2, 1]; -rho)        H == 1:  P = [1]
// so the term is linear in eps with the coefficients
//   lin[u][t] = gamma / sigma_u[u]^2 * (P U[u][:])[t]                  (sigma_u[u] == 0, a frozen actuator: lin = 0)
// This header is the only statement of the fp32 rule for lin: ctrl_lin_kernel (kernels_ctrl_cost.hip) runs it on the
// device, tests/native/control_cost_host.cpp on the host, mppi_hip.stats.control_term_ref is its float64 restatement.
//
// Roundings (u = 2^-24), which the tests' bound 8u * A on |lin_f32 - lin_f64| rests on, A the absolute-value majorant
// gamma / sigma^2 / (1 - rho^2) * (d |U_t| + rho (|U_t-1| + |U_t+1|)):
//   scale = gamma / (sigma^2 * (1 - rho^2)): 1 - rho^2 as ONE fmaf (1 u: no cancellation of a rounded square), the
//           square, the product, the quotient: 4 u
//   v     = (P U)[t] (1 - rho^2): d = fmaf(rho, rho, 1) (1 u), the neighbours' sum and its product with -rho (2 u on
//           that part), one fmaf (1 u of a value the majorant bounds): 3 u of the majorant; the end rows are one fmaf
//   lin   = scale * v: 1 u more.
// Every product and sum is its own statement or an explicit fmaf, contraction off: host and device agree bit for bit.
#pragma once
#include <math.h>

#include "philox.h"  // MPPI_HD

// gamma / (sigma^2 (1 - rho^2)) (H == 1: gamma / sigma^2); 0 for a frozen actuator (and for a sigma whose square
// underflows: no finite coefficient exists there)
MPPI_HD float ctrl_lin_scale(float gamma, float sigma, float rho, int H) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float s2 = sigma * sigma;
  const float om = H > 1 ? fmaf(-rho, rho, 1.0f) : 1.0f;
  const float den = s2 * om;
  if (!(den > 0.0f)) return 0.0f;
  return gamma / den;
}

// lin[t] of one (b, u) row U[0..H) from the row's scale
MPPI_HD float ctrl_lin_entry(float scale, float rho, const float* U, int t, int H) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (scale == 0.0f) return 0.0f;
  float v;
  if (H == 1) {
    v = U[0];
  } else if (t == 0) {
    v = fmaf(-rho, U[1], U[0]);
  } else if (t == H - 1) {
    v = fmaf(-rho, U[H - 2], U[H - 1]);
  } else {
    const float d = fmaf(rho, rho, 1.0f);
    const float nb = U[t - 1] + U[t + 1];
    const float w = -rho * nb;
    v = fmaf(d, U[t], w);
  }
  return scale * v;
}

// a whole row (the CPU form of ctrl_lin_kernel's one thread per entry)
MPPI_HD void ctrl_lin_row(float gamma, float sigma, float rho, const float* U, float* lin, int H) {
  const float scale = ctrl_lin_scale(gamma, sigma, rho, H);
  for (int t = 0; t < H; ++t) lin[t] = ctrl_lin_entry(scale, rho, U, t, H);
}

// Under a cross-actuator covariance (mppi_set_noise_cov; noise_cov.h) the law's covariance is Sigma (x) C, so
//   lin[u][t] = gamma * sum_v Sinv[u][v] * (P U[v][:])[t]
// in fp32 and in this fixed order, with pv_v[t] = ctrl_lin_entry(1.0f, rho, U[v][:], t, H) = (P U_v)[t] (1 - rho^2):
//   om = H > 1 ? fmaf(-rho, rho, 1) : 1;    scale0 = gamma / om
//   acc = Sinv[u][0] * pv_0[t];    acc = fmaf(Sinv[u][v], pv_v[t], acc)   v = 1..nu-1;    lin[u][t] = scale0 * acc
// Roundings: 3 u of its majorant A_v on each pv_v, one per product / fmaf of the sum, 2 u on scale0, 1 u on the last
// product: |lin_f32 - lin_f64| <= (nu + 8) u * scale0 * sum_v |Sinv[u][v]| A_v.
// Ub: the solve's U [nu][H]; Sinv_row: row u of Sinv [nu][nu]
MPPI_HD float ctrl_lin_cov_entry(float gamma, float rho, const float* Sinv_row, int nu, const float* Ub, int t, int H) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float om = H > 1 ? fmaf(-rho, rho, 1.0f) : 1.0f;
  const float scale0 = gamma / om;
  float acc = Sinv_row[0] * ctrl_lin_entry(1.0f, rho, Ub, t, H);
  for (int v = 1; v < nu; ++v) acc = fmaf(Sinv_row[v], ctrl_lin_entry(1.0f, rho, Ub + (long)v * H, t, H), acc);
  return scale0 * acc;
}
