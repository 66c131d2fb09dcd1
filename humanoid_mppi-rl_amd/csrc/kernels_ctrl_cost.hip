// The control-cost term of information-theoretic MPPI (mppi_set_control_cost; the rule for lin is control_cost.h):
//   lin  [b][u][t] = gamma / sigma_u[u]^2 * (P U[b][u][:])[t]          ctrl_lin_kernel (B nu H values: tiny)
//                    under mppi_set_noise_cov: gamma * sum_v Sinv[u][v] (P U[b][v][:])[t]
//   term [b][k]    = sum_{u,t} lin[b][u][t] * eps[b][u][t][k]          ctrl_term_*_kernel (the whole noise once: the hot part)
//   wcost[b][k]    = costs[b][k] + term[b][k]                          (pads K..Kp: costs copied through, term 0)
// Two launches (three in the split form) between the rollout and everything that weighs the solve's costs; read-only
// on U, the noise and the costs.
#include <hip/hip_runtime.h>

#include "control_cost.h"
#include "mppi_internal.h"
#include "term_cells.h"

namespace mppi {

// one thread per entry of lin; the law by value, or (d_law: an adapting handle) read from the device law on the stream
__global__ __launch_bounds__(256) void ctrl_lin_kernel(CtrlArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.B * a.nu * a.H) return;
  const int bu = i / a.H, t = i - bu * a.H, u = bu % a.nu;
  if (a.sinv) {  // a cross-actuator covariance: the row of Sigma^-1 over every actuator's P U (never with d_law)
    // (Sinv is written by the setter and, on a handle that adapts its covariance, by noise_cov_adapt_kernel: a launch of
    // its own behind this solve's statistics on the same stream, so never while this kernel runs)
    a.lin[i] = ctrl_lin_cov_entry(a.law.gamma, a.law.rho, a.sinv + u * a.nu, a.nu, a.U + (long)(bu - u) * a.H, t, a.H);
    return;
  }
  const float sigma = a.d_law ? a.d_law[u] : (a.law.per_u ? a.law.sigma_u[u] : a.law.sigma);
  const float rho = a.d_law ? a.d_law[kLawRho] : a.law.rho;
  a.lin[i] = ctrl_lin_entry(ctrl_lin_scale(a.law.gamma, sigma, rho, a.H), rho, a.U + (long)bu * a.H, t, a.H);
}

// The term, by the cell scheme of term_cells.h.  The sum of one cell, rows [r0, r1) of the solve whose row r is
// src + r * nq (this lane's quad) and lin[r]: fmaf(lin, eps, acc) in row order, lin wave-uniform (scalar loads)
template <bool NT>
__device__ __forceinline__ f4 ctrl_cell(const f4* src, const float* __restrict__ lin, int r0, int r1, int nq) {
  f4 cur[kTermTile], nxt[kTermTile];
  auto load = [&](f4* dst, int t0) {
#pragma unroll
    for (int j = 0; j < kTermTile; ++j) dst[j] = term_ld<NT>(src + (long)min(t0 + j, r1 - 1) * nq);
  };
  load(cur, r0);
  f4 acc = f4{0.0f, 0.0f, 0.0f, 0.0f};
  for (int t0 = r0; t0 < r1; t0 += kTermTile) {
    const bool more = t0 + kTermTile < r1;
    if (more) load(nxt, t0 + kTermTile);
#pragma unroll
    for (int j = 0; j < kTermTile; ++j) {
      if (t0 + j < r1) {  // (uniform)
        const float l = lin[t0 + j];
        acc.x = fmaf(l, cur[j].x, acc.x);
        acc.y = fmaf(l, cur[j].y, acc.y);
        acc.z = fmaf(l, cur[j].z, acc.z);
        acc.w = fmaf(l, cur[j].w, acc.w);
      }
    }
    if (more) {
#pragma unroll
      for (int j = 0; j < kTermTile; ++j) cur[j] = nxt[j];
    }
  }
  return acc;
}

template <bool NT>
__global__ __launch_bounds__(kTermCells * 64) void ctrl_term_block_kernel(CtrlArgs a, int Lc, int ncell) {
  term_block_body(a, Lc, ncell, [&](const f4* src, int b, int r0, int r1, int nq) {
    return ctrl_cell<NT>(src, a.lin + (long)b * (a.nu * a.H), r0, r1, nq);
  });
}

template <bool NT>
__global__ __launch_bounds__(64) void ctrl_term_split_kernel(CtrlArgs a, int Lc, int ncell) {
  term_split_body(a, Lc, ncell, [&](const f4* src, int b, int r0, int r1, int nq) {
    return ctrl_cell<NT>(src, a.lin + (long)b * (a.nu * a.H), r0, r1, nq);
  });
}

__global__ __launch_bounds__(256) void ctrl_finish_kernel(CtrlArgs a, int ncell) { term_finish_body(a, ncell); }

hipError_t launch_ctrl_cost(const CtrlArgs& a, hipStream_t stream) {
  if (a.B < 1 || a.B > 65535) return hipErrorInvalidValue;  // (b is a grid's y / z index)
  const int n = a.B * a.nu * a.H;
  hipLaunchKernelGGL(ctrl_lin_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const int nchunk = ((a.Kp >> 2) + 63) / 64;
  const TermForm f = term_form("MPPI_CTRL_COST_FORM", "MPPI_CTRL_COST_NT", a.B, nchunk, (double)n * a.Kp * 4.0);
  return term_launch(a, f.block, f.nt ? ctrl_term_block_kernel<true> : ctrl_term_block_kernel<false>,
                     f.nt ? ctrl_term_split_kernel<true> : ctrl_term_split_kernel<false>, ctrl_finish_kernel, stream);
}

}  // namespace mppi
