// Knot-parameterised sampling noise (mppi_set_noise_knots): the perturbation of one (b, u, k) is drawn at P knots
// along the horizon and interpolated to its H steps (MuJoCo MPC's spline points, STORM's / cuRobo's control knots).
//
// A knot law is (n_knots = P, order) with 1 <= P <= H and order in {0, 1, 3}; it sits in the handle's sampling law
// next to sigma_u and rho (noise_model.h).
//
// The table, four taps per horizon step: idx[t][4] (int32, each in 0..P-1) and w[t][4] (fp32).  Built once on the host,
// in double, in exactly the order of operations written below, rounded to fp32 once:
//   order 0 (hold):    idx[t][0..3] = (t * P) / H  (integer arithmetic),  w = (1, 0, 0, 0)
//   H == 1 or P == 1, orders 1 and 3:  idx = 0,  w = (1, 0, 0, 0)
//   otherwise          s = (double)(t * (P - 1)) / (double)(H - 1),  j = min((int)floor(s), P - 2),  a = s - (double)j
//   order 1 (linear):  idx = (j, j + 1, j, j),  w = (1 - a, a, 0, 0)
//   order 3 (uniform Catmull-Rom, clamped ends):  idx = (j - 1, j, j + 1, j + 2), each clamped to [0, P - 1] (a
//                      duplicated index keeps its own tap), and with a2 = a * a, a3 = a2 * a:
//                        w0 = ((-a3 + 2 a2) - a) * 0.5          w1 = ((3 a3 - 5 a2) + 2) * 0.5
//                        w2 = ((-3 a3 + 4 a2) + a) * 0.5        w3 = (a3 - a2) * 0.5
// idx[t][0] is the smallest index of its row and non-decreasing in t, and a row spans at most 4 consecutive knots: a
// generator walking t needs a window of four knots (noise_knot_kernel).
//
// The knot values: z[j], j < P, are the standard normals of philox.h at counter (k/4, j, u, b) -- the white law's
// counter with t replaced by the knot index, under the key the solve would draw anyway -- and the knot row is the
// handle's AR(1) row of length P:  kn[0..P) = ar1_row(rho, c, z)  (rho = 0: independent knots).
//
// The interpolation, fp32, in this fixed order (zero-weight taps enter the sum: the normals are finite, each adds an
// exact 0):
//   e[t] = w[t][0] * kn[idx[t][0]]
//   e[t] = fmaf(w[t][i], kn[idx[t][i]], e[t])      i = 1, 2, 3
//   eps  = sigma_u[u] * e[t]
//
// Identities: P == H with order 0 or 1 gives e[t] = kn[t] bit for bit (the AR(1) / white noise of the handle, value
// for value); P == 1 gives a row constant in t.
// Variance: at a knot e[t] has unit variance; between knots it is sum_i w_i^2 < 1 for independent knots (0.5 halfway
// between two knots of order 1).  MuJoCo MPC and STORM sample this way and so does the engine: sigma_u is the scale at
// the knots.  eps_m2 of MPPI_FLAG_STATS reports what was actually drawn.
//
// Host + device (the MPPI_HD style of noise_model.h): tests/test_noise_knots.py runs the table and the rows through g++.
#pragma once
#include <math.h>
#include <stdint.h>

#include "noise_model.h"  // MPPI_HD, ar1_row

// 1 <= P <= H and order in {0, 1, 3}
MPPI_HD bool knot_law_valid(int H, int P, int order) {
  return P >= 1 && P <= H && (order == 0 || order == 1 || order == 3);
}

// the table of one (H, P, order): idx [H][4], w [H][4].  Host only; no operation of it may be contracted into an fma
#if defined(__GNUC__) && !defined(__clang__)
__attribute__((optimize("fp-contract=off")))
#endif
inline void knot_table(int H, int P, int order, int32_t* idx, float* w) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  for (int t = 0; t < H; ++t) {
    int32_t* ix = idx + 4 * t;
    float* wt = w + 4 * t;
    if (order == 0 || H == 1 || P == 1) {
      const int32_t j = order == 0 ? (int32_t)(((long)t * P) / H) : 0;
      ix[0] = ix[1] = ix[2] = ix[3] = j;
      wt[0] = 1.0f;
      wt[1] = wt[2] = wt[3] = 0.0f;
      continue;
    }
    const double s = (double)((long)t * (P - 1)) / (double)(H - 1);
    int j = (int)floor(s);
    if (j > P - 2) j = P - 2;
    const double a = s - (double)j;
    if (order == 1) {
      ix[0] = j, ix[1] = j + 1, ix[2] = j, ix[3] = j;
      wt[0] = (float)(1.0 - a);
      wt[1] = (float)a;
      wt[2] = wt[3] = 0.0f;
      continue;
    }
    for (int i = 0; i < 4; ++i) {
      const int n = j - 1 + i;
      ix[i] = n < 0 ? 0 : (n > P - 1 ? P - 1 : n);
    }
    const double a2 = a * a;
    const double a3 = a2 * a;
    const double m2a2 = 2.0 * a2, m3a3 = 3.0 * a3, m5a2 = 5.0 * a2, m4a2 = 4.0 * a2;
    wt[0] = (float)(((-a3 + m2a2) - a) * 0.5);
    wt[1] = (float)(((m3a3 - m5a2) + 2.0) * 0.5);
    wt[2] = (float)(((-m3a3 + m4a2) + a) * 0.5);
    wt[3] = (float)((a3 - a2) * 0.5);
  }
}

// one step of the interpolation from the four knots its taps name (before the scale)
MPPI_HD float knot_interp(const float w[4], float k0, float k1, float k2, float k3) {
  float e = w[0] * k0;
  e = fmaf(w[1], k1, e);
  e = fmaf(w[2], k2, e);
  e = fmaf(w[3], k3, e);
  return e;
}

// a whole row eps[0..H) from the normals z[0..P) (the CPU form of noise_knot_kernel's walk over t); kn: scratch [P]
MPPI_HD void knot_row(float rho, float c, float sigma, const float* z, int P, const int32_t* idx, const float* w,
                      float* kn, float* eps, int H) {
  ar1_row(rho, c, z, kn, P);
  for (int t = 0; t < H; ++t) {
    const int32_t* ix = idx + 4 * t;
    eps[t] = sigma * knot_interp(w + 4 * t, kn[ix[0]], kn[ix[1]], kn[ix[2]], kn[ix[3]]);
  }
}
