// Keep / shift elites (mppi_set_elite_keep): the n_keep best SAMPLED control sequences of a solve are gathered on the
// device, held per handle (per batch slot b, as u_prev is), and injected into the first columns of the next solve's
// noise, where they compete again (iCEM's "keep elites" and "shift elites").  This header is the only statement of the
// rule: keep_gather_kernel / keep_inject_kernel (kernels_elite_keep.hip) run it on the device,
// tests/native/elite_keep_host.cpp on the host, mppi_hip.stats.keep_store_ref / keep_inject_ref are its numpy
// restatements.  The rule is one add (rate_cost_v: the control the rollout applied, with its clamp) and one subtract,
// contraction off: all three agree bitwise.
//
// STORE, in solve i, behind the cost terms and the selection, ahead of the lambda search and the reduce (U is still the
// nominal the rollout perturbed).  For solve b, with c[0..K) the costs the softmin would weigh ahead of any elite
// masking (costs [+ control-cost term] [+ rate term]) and eps' the noise as the rollout saw it (projected with bounds):
//   the kept set = elite_select.h's rule with n = n_keep: m = min(n_keep, |finite c|), the first m by (c_k, k),
//                  idx[0..m) in ascending k, idx[m..n_keep) = -1
//   shift = 1 when the solve carries MPPI_FLAG_SHIFT, else 0;  steps = H - shift
//   v[u][t][j]  = rate_cost_v(U[u][t + shift], eps'[u][t + shift][idx[j]], ctrl_clamp)     t < steps, j < m
//               = +0.0 everywhere else
//   kcost[j]    = c[idx[j]] bit for bit for j < m, +inf for j >= m;  count = m
// steps == 0 (H == 1 with shift) stores nothing: v is all +0.0, and the injection below then writes nothing.
//
// INJECT, at the start of solve i + 1, behind whatever filled its noise and ahead of the bounds projection and the
// rollout, with U that solve's nominal:
//   eps[u][t][j] = v[u][t][j] - U[u][t]          one fp32 subtract, for j < count and t < steps
//   every other element (columns count.., the pads K..Kp, rows t >= steps) is untouched, bit for bit: after a shift the
//   last step of a carried sample keeps its freshly drawn noise, which is iCEM's rule.
// U + eps is then v within one rounding of the larger operand, not always v itself (fl(U + fl(v - U))).  The
// perturbation is always taken against the nominal in effect, so mppi_set_U between solves needs no special case.
//
// Everything behind the injection sees the injected eps: the projection, the costs, the terms, the statistics' moments
// and so the noise adaptation, and the reduce.  In particular the control-cost term treats a carried column like any
// other, although those samples were not drawn from the law; iCEM makes the same simplification.
#pragma once
#include <math.h>
#include <stdint.h>

#include "elite_select.h"  // elite_select_row: the kept set's rule
#include "rate_cost.h"     // rate_cost_v: the control the rollout applied

// the horizon steps a stored sequence covers
MPPI_HD int keep_steps(int H, int shift) { return H - (shift ? 1 : 0); }

// one stored element: the control sample k applied at step t + shift (U, eps already taken there)
MPPI_HD float keep_store_v(float U, float eps, float clamp) { return rate_cost_v(U, eps, clamp); }

// one injected element: the perturbation that brings the nominal U to the stored control v
MPPI_HD float keep_inject_eps(float v, float U) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return v - U;
}

// The host form of one solve's store: U [nu][H], eps [nu][H][K] (k fastest), c [K] -> v [nu][H][n_keep] (j fastest),
// kcost [n_keep], idx [n_keep]; returns count, *steps_out = steps.
inline int keep_store_row(const float* U, const float* eps, const float* c, int nu, int H, int K, int n_keep, int shift,
                          float clamp, float* v, float* kcost, int32_t* idx, int* steps_out) {
  const int m = elite_select_row(c, K, n_keep, idx, nullptr, nullptr);
  const int sh = shift ? 1 : 0, steps = keep_steps(H, shift);
  for (int u = 0; u < nu; ++u)
    for (int t = 0; t < H; ++t)
      for (int j = 0; j < n_keep; ++j) {
        float o = 0.0f;
        if (t < steps && j < m) {
          const long r = (long)u * H + t + sh;
          o = keep_store_v(U[r], eps[r * K + idx[j]], clamp);
        }
        v[((long)u * H + t) * n_keep + j] = o;
      }
  for (int j = 0; j < n_keep; ++j) kcost[j] = j < m ? c[idx[j]] : INFINITY;
  *steps_out = steps;
  return m;
}

// The host form of one solve's injection: eps [nu][H][K] in place against U [nu][H] from v [nu][H][n_keep].
inline void keep_inject_row(const float* U, float* eps, const float* v, int nu, int H, int K, int n_keep, int count,
                            int steps) {
  for (int u = 0; u < nu; ++u)
    for (int t = 0; t < steps; ++t)
      for (int j = 0; j < count; ++j) {
        const long r = (long)u * H + t;
        eps[r * K + j] = keep_inject_eps(v[r * n_keep + j], U[r]);
      }
}
