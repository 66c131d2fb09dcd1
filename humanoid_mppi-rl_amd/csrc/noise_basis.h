// Horizon-basis sampling noise (mppi_set_noise_basis): the perturbation of one (b, u, k) is a dense matrix M [H][R]
// applied along the horizon to R independent standard normals -- iCEM's coloured (power-law) noise, a squared-exponential
// temporal kernel, a B-spline or a truncated cosine basis are all this object.
//
// A basis law is (n_basis = R, M) with 1 <= R <= min(H, kMaxBasis) and every entry of M finite, M fp32 row-major; it
// sits in the handle's sampling law next to sigma_u (noise_model.h) as the third horizon law, beside AR(1) and the knot
// table (noise_knots.h).  rho is 0 under it: the basis is the horizon correlation.
//
// The normals: z[r], r < R, are the standard normals of philox.h at counter (k/4, r, u, b) -- the white law's counter
// with t replaced by the basis index, under the key the solve would draw anyway.  They are white: no AR(1) over them.
//
// The mix, fp32, in this fixed order (no partial sums over chunks of r):
//   e[t] = M[t][0] * z[0]
//   e[t] = fmaf(M[t][r], z[r], e[t])      r = 1 .. R-1, ascending
//   eps  = sigma_u[u] * e[t]
//
// The covariance along the horizon is sigma_u^2 M M^T.  M = I (R = H) gives eps[t] = sigma_u z[t] bit for bit (every
// other product is an exact signed zero, and z[t] = 0 has probability 0 under Box-Muller's open interval): the handle's
// rho = 0 model, value for value.
//
// Host + device (the MPPI_HD style of noise_model.h): tests/test_noise_basis.py runs the rows through g++.
#pragma once
#include <math.h>

#include "noise_model.h"  // MPPI_HD

// the largest R: config #5's horizon, the largest the presets use; it bounds noise_basis_kernel's LDS (R floats per k)
// and, with H <= 128, noise_basis_mfma_kernel's accumulators (H registers per lane)
constexpr int kMaxBasis = 128;

// 1 <= R <= H (the setter answers R > kMaxBasis on its own: unsupported, not invalid)
MPPI_HD bool basis_law_valid(int H, int R) { return R >= 1 && R <= H; }

// every entry finite
inline bool basis_table_finite(const float* M, int H, int R) {
  for (long i = 0; i < (long)H * R; ++i)
    if (!isfinite(M[i])) return false;
  return true;
}

// one step of the mix from its row m[0..R) of M and the normals z[0..R), z strided by zs (before the scale)
MPPI_HD float basis_mix(const float* m, const float* z, int zs, int R) {
  float e = m[0] * z[0];
  for (int r = 1; r < R; ++r) e = fmaf(m[r], z[(long)r * zs], e);
  return e;
}

// a whole row eps[0..H) from the normals z[0..R) (the CPU form of noise_basis_kernel's walk over t)
MPPI_HD void basis_row(float sigma, const float* z, int R, const float* M, float* eps, int H) {
  for (int t = 0; t < H; ++t) eps[t] = sigma * basis_mix(M + (long)t * R, z, 1, R);
}
