// The sampling law of the device noise: per-actuator scale and AR(1) correlation along the horizon
// (mppi_set_noise_model).
//
// With z[t] the standard normals of philox.h (counter (k/4, t, u, b), unchanged):
//   e[0] = z[0]
//   e[t] = fmaf(rho, e[t-1], c * z[t])      c = sqrtf(1 - rho*rho), computed once on the host in fp32
//   eps  = sigma_u[u] * e[t]
// Every e[t] has unit variance and corr(e[t], e[s]) = rho^|t-s|.  rho = 0 gives c = 1 and e[t] = z[t] exactly, so
// sigma_u == sigma reproduces the white noise of noise_kernel value for value.
//
// Host + device (the MPPI_HD style of philox.h): tests/test_noise_model.py runs the recursion through g++.
#pragma once
#include <math.h>

#include "philox.h"  // MPPI_HD

// c of the recursion; the square and the difference are separate statements, so no compiler contracts them into an fma
MPPI_HD float ar1_innovation_scale(float rho) {
#if defined(__clang__)  // ... also where the default is to contract across statements (device code: noise_adapt_kernel)
#pragma clang fp contract(off)
#endif
  const float r2 = rho * rho;
  return sqrtf(1.0f - r2);
}

// one step of the recursion in its two parts: the innovation c * z (no dependence on e_prev: drawn ahead, in any
// order) and the advance, the only serial operation of a row (one fma)
MPPI_HD float ar1_innovation(float c, float z) { return c * z; }
MPPI_HD float ar1_advance(float rho, float e_prev, float innovation) { return fmaf(rho, e_prev, innovation); }
MPPI_HD float ar1_step(float rho, float c, float e_prev, float z) {
  return ar1_advance(rho, e_prev, ar1_innovation(c, z));
}

// a whole row e[0..H) from z[0..H) (the CPU form of noise_ar1_kernel's walk over t)
MPPI_HD void ar1_row(float rho, float c, const float* z, float* e, int H) {
  float prev = 0.0f;
  for (int t = 0; t < H; ++t) {
    prev = t == 0 ? z[0] : ar1_step(rho, c, prev, z[t]);
    e[t] = prev;
  }
}
