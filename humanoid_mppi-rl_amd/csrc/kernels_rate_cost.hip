// The control-rate cost term (mppi_set_rate_cost; the rule per element is rate_cost.h):
//   v    [b][u][t][k] = clamp(U[b][u][t] + eps'[b][u][t][k])           the control the rollout applied
//   term [b][k]       = sum_u r[u] sum_t (v[u][t] - v[u][t-1])^2       v[u][-1] = u_prev[b][u] with the anchor
//   wcost[b][k]       = costs[b][k] + term[b][k]                       (pads K..Kp: costs copied through, term 0)
// One launch (two in the split form) between the rollout (and the control-cost term, whose wcost is then this one's
// `costs`) and everything that weighs the solve's costs; read-only on U, the noise, u_prev and the costs.
#include <hip/hip_runtime.h>

#include "mppi_internal.h"
#include "rate_cost.h"
#include "term_cells.h"

namespace mppi {

// The term, by the cell scheme of term_cells.h.  A cell walks its rows in row order with the row before it held in
// registers, U, r[u] and u_prev wave-uniform (scalar loads).  A cell that begins inside an actuator's row (t > 0) reads
// row t - 1 once more to difference against (config #4: 16 rows of 1344, 1.2 %); a cell, or a row inside a cell, that
// begins an actuator's row takes u_prev (or, without the anchor, itself) instead, so nothing is ever differenced
// across actuators.  The kernels are templated on the anchor: with it, `prev` becomes u_prev where an actuator's row
// ENDS, so the row body carries no select (the small grids are bound by instruction issue).
__device__ __forceinline__ f4 rate_v(float U, const f4& e, float cl) {
  return f4{rate_cost_v(U, e.x, cl), rate_cost_v(U, e.y, cl), rate_cost_v(U, e.z, cl), rate_cost_v(U, e.w, cl)};
}

// the sum of one cell, rows [r0, r1) of solve b whose row r is src + r * nq (this lane's quad), U[r] and up[u]
template <bool NT, bool CLAMP, bool ANCHOR>
__device__ __forceinline__ f4 rate_cell(const RateArgs& a, const f4* src, const float* __restrict__ U,
                                        const float* __restrict__ up, int r0, int r1, int nq) {
  const float cl = CLAMP ? a.clamp : 0.0f;
  if constexpr (CLAMP) __builtin_assume(cl > 0.0f);
  // the wave-uniform operands travel with the tiles, so no row waits for a scalar load of its own: a tile's U values
  // are loaded with its rows, and the weight and anchor of the NEXT actuator are fetched when an actuator's row begins.
  // With the anchor the row before an actuator's first IS u_prev: it replaces `prev` where the actuator's row ends (a
  // rare uniform branch), so the row body has no select; without it the first row is differenced against itself
  f4 cur[kTermTile], nxt[kTermTile];
  float Uc[kTermTile], Un[kTermTile];
  auto load = [&](f4* dst, float* Ud, int t0) {
#pragma unroll
    for (int j = 0; j < kTermTile; ++j) {
      const int row = min(t0 + j, r1 - 1);
      dst[j] = term_ld<NT>(src + (long)row * nq);
      Ud[j] = U[row];
    }
  };
  int u = r0 / a.H, t = r0 - u * a.H;  // (uniform)
  float rw = a.r[u], pu = up[u];
  int un = min(u + 1, a.nu - 1);
  float rwn = a.r[un], pun = up[un];
  f4 prev = f4{pu, pu, pu, pu};
  if (t > 0) prev = term_ld<NT>(src + (long)(r0 - 1) * nq);  // the cell begins inside an actuator's row
  load(cur, Uc, r0);
  if (t > 0) prev = rate_v(U[r0 - 1], prev, cl);
  f4 acc = f4{0.0f, 0.0f, 0.0f, 0.0f};
  for (int t0 = r0; t0 < r1; t0 += kTermTile) {
    const bool more = t0 + kTermTile < r1;
    if (more) load(nxt, Un, t0 + kTermTile);
#pragma unroll
    for (int j = 0; j < kTermTile; ++j) {
      if (t0 + j < r1) {  // (uniform)
        const f4 v = rate_v(Uc[j], cur[j], cl);
        if constexpr (!ANCHOR) {
          if (t == 0) prev = v;  // an actuator's row begins: the row itself (an exact 0, NaN if non-finite)
        }
        acc.x = rate_cost_add(rw, v.x, prev.x, acc.x);
        acc.y = rate_cost_add(rw, v.y, prev.y, acc.y);
        acc.z = rate_cost_add(rw, v.z, prev.z, acc.z);
        acc.w = rate_cost_add(rw, v.w, prev.w, acc.w);
        prev = v;
        if (++t == a.H) {
          t = 0;
          rw = rwn;
          pu = pun;
          un = min(un + 1, a.nu - 1);
          rwn = a.r[un];
          pun = up[un];
          if constexpr (ANCHOR) prev = f4{pu, pu, pu, pu};  // the next actuator's row begins at its anchor
        }
      }
    }
    if (more) {
#pragma unroll
      for (int j = 0; j < kTermTile; ++j) {
        cur[j] = nxt[j];
        Uc[j] = Un[j];
      }
    }
  }
  return acc;
}

template <bool NT, bool CLAMP, bool ANCHOR>
__global__ __launch_bounds__(kTermCells * 64) void rate_term_block_kernel(RateArgs a, int Lc, int ncell) {
  term_block_body(a, Lc, ncell, [&](const f4* src, int b, int r0, int r1, int nq) {
    return rate_cell<NT, CLAMP, ANCHOR>(a, src, a.U + (long)b * (a.nu * a.H), a.u_prev + (long)b * a.nu, r0, r1, nq);
  });
}

template <bool NT, bool CLAMP, bool ANCHOR>
__global__ __launch_bounds__(64) void rate_term_split_kernel(RateArgs a, int Lc, int ncell) {
  term_split_body(a, Lc, ncell, [&](const f4* src, int b, int r0, int r1, int nq) {
    return rate_cell<NT, CLAMP, ANCHOR>(a, src, a.U + (long)b * (a.nu * a.H), a.u_prev + (long)b * a.nu, r0, r1, nq);
  });
}

__global__ __launch_bounds__(256) void rate_finish_kernel(RateArgs a, int ncell) { term_finish_body(a, ncell); }

// u_prev <- the u0 the solve returns (MPPI_FLAG_SHIFT with the anchor on), behind the update and the bounds' clip
__global__ __launch_bounds__(256) void rate_store_prev_kernel(const float* __restrict__ u0, float* __restrict__ u_prev,
                                                              int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) u_prev[i] = u0[i];
}

template <bool NT, bool CLAMP, bool ANCHOR>
static hipError_t rate_launch(const RateArgs& a, bool block, hipStream_t stream) {
  return term_launch(a, block, rate_term_block_kernel<NT, CLAMP, ANCHOR>, rate_term_split_kernel<NT, CLAMP, ANCHOR>,
                     rate_finish_kernel, stream);
}

hipError_t launch_rate_cost(const RateArgs& a, hipStream_t stream) {
  if (a.B < 1 || a.B > 65535 || a.nu < 1 || a.nu > kMaxNu || a.H < 1) return hipErrorInvalidValue;  // (b: a grid's y / z)
  const int nchunk = ((a.Kp >> 2) + 63) / 64;
  const TermForm f = term_form("MPPI_RATE_COST_FORM", "MPPI_RATE_COST_NT", a.B, nchunk,
                               (double)a.B * a.nu * a.H * a.Kp * 4.0);
  using Launch = hipError_t (*)(const RateArgs&, bool, hipStream_t);
  static const Launch table[2][2][2] = {  // [nt][clamp][anchor]
      {{rate_launch<false, false, false>, rate_launch<false, false, true>},
       {rate_launch<false, true, false>, rate_launch<false, true, true>}},
      {{rate_launch<true, false, false>, rate_launch<true, false, true>},
       {rate_launch<true, true, false>, rate_launch<true, true, true>}}};
  return table[f.nt][a.clamp > 0.0f][a.anchor != 0](a, f.block, stream);
}

hipError_t launch_rate_store_prev(const float* u0, float* u_prev, int n, hipStream_t stream) {
  hipLaunchKernelGGL(rate_store_prev_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, u0, u_prev, n);
  return hipGetLastError();
}

}  // namespace mppi
