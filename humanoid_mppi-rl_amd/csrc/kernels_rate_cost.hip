// The control-rate cost term (mppi_set_rate_cost; the rule per element is rate_cost.h):
//   v    [b][u][t][k] = clamp(U[b][u][t] + eps'[b][u][t][k])           the control the rollout applied
//   term [b][k]       = sum_u r[u] sum_t (v[u][t] - v[u][t-1])^2       v[u][-1] = u_prev[b][u] with the anchor
//   wcost[b][k]       = costs[b][k] + term[b][k]                       (pads K..Kp: costs copied through, term 0)
// One launch (two in the split form) between the rollout (and the control-cost term, whose wcost is then this one's
// `costs`) and everything that weighs the solve's costs; read-only on U, the noise, u_prev and the costs.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>

#include "mppi_internal.h"
#include "rate_cost.h"

namespace mppi {

// ------------------------------------------------------------------------------------------------
// The access scheme is ctrl_term_*_kernel's (kernels_ctrl_cost.hip): every noise element read once, [B][nu][H][Kp]
// with k fastest.  The R = nu H rows of a solve are cut into CELLS of Lc consecutive rows in (u, t) order (rate_cells:
// at most kRateCells of them, at least kRateMinRows rows each); a wave owns a chunk of 256 consecutive k (each lane one
// k-quad, 16-B loads) of one cell and walks the cell's rows in row order with the row before it held in registers, U,
// r[u] and u_prev wave-uniform (scalar loads), kRateTile rows per load tile with the next tile issued before the
// current one is consumed, nontemporal above launch_reduce's 128 MB cut.  A cell that begins inside an actuator's row
// (t > 0) reads row t - 1 once more to difference against (config #4: 16 rows of 1344, 1.2 %); a cell, or a row inside
// a cell, that begins an actuator's row takes u_prev (or, without the anchor, itself) instead, so nothing is ever
// differenced across actuators.  The kernels are templated on the anchor: with it, `prev` becomes u_prev where an
// actuator's row ENDS, so the row body carries no select (the small grids are bound by instruction issue).  The cells' sums are then added in cell order.  The order per k is fixed by the shape
// alone, so runs repeat bitwise and the two forms agree bit for bit:
//   block  a block owns (b, chunk), wave w walks cell w, the sums meet in LDS (16 KiB) and wave 0 adds them and
//          forms wcost: no partial buffer, one launch.  For batches whose (b, chunk) blocks fill the chip (config #4).
//   split  one single-wave block per (chunk, cell, b) stores its sum as a partial [B][cells][Kp]; rate_finish_kernel
//          adds them and forms wcost.  For grids that would leave most CUs idle (config #2, config #5, the shards).
// No atomics; inactive lanes (quads beyond Kp) read a clamped, in-bounds quad and store nothing.
// ------------------------------------------------------------------------------------------------
constexpr int kRateCells = 16;    // cells per solve (at most) = waves per block of the block form
constexpr int kRateMinRows = 16;  // rows per cell (at least, while the solve has them)
constexpr int kRateTile = 8;      // rows per load tile
typedef float f4 __attribute__((ext_vector_type(4)));

template <bool NT>
__device__ __forceinline__ f4 rate_ld(const f4* p) {
  if constexpr (NT) return __builtin_nontemporal_load(p);
  else return *p;
}

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
  f4 cur[kRateTile], nxt[kRateTile];
  float Uc[kRateTile], Un[kRateTile];
  auto load = [&](f4* dst, float* Ud, int t0) {
#pragma unroll
    for (int j = 0; j < kRateTile; ++j) {
      const int row = min(t0 + j, r1 - 1);
      dst[j] = rate_ld<NT>(src + (long)row * nq);
      Ud[j] = U[row];
    }
  };
  int u = r0 / a.H, t = r0 - u * a.H;  // (uniform)
  float rw = a.r[u], pu = up[u];
  int un = min(u + 1, a.nu - 1);
  float rwn = a.r[un], pun = up[un];
  f4 prev = f4{pu, pu, pu, pu};
  if (t > 0) prev = rate_ld<NT>(src + (long)(r0 - 1) * nq);  // the cell begins inside an actuator's row
  load(cur, Uc, r0);
  if (t > 0) prev = rate_v(U[r0 - 1], prev, cl);
  f4 acc = f4{0.0f, 0.0f, 0.0f, 0.0f};
  for (int t0 = r0; t0 < r1; t0 += kRateTile) {
    const bool more = t0 + kRateTile < r1;
    if (more) load(nxt, Un, t0 + kRateTile);
#pragma unroll
    for (int j = 0; j < kRateTile; ++j) {
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
      for (int j = 0; j < kRateTile; ++j) {
        cur[j] = nxt[j];
        Uc[j] = Un[j];
      }
    }
  }
  return acc;
}

// quad q of solve b: term and wcost from the summed cells (pads K..Kp: term 0, the cost copied through)
__device__ __forceinline__ void rate_store(const RateArgs& a, int b, int q, const f4& s) {
  const long o = (long)b * (a.Kp >> 2) + q;
  const f4 c = reinterpret_cast<const f4*>(a.costs)[o];
  const int k = 4 * q;
  const f4 t = f4{k + 0 < a.K ? s.x : 0.0f, k + 1 < a.K ? s.y : 0.0f, k + 2 < a.K ? s.z : 0.0f,
                  k + 3 < a.K ? s.w : 0.0f};
  reinterpret_cast<f4*>(a.term)[o] = t;
  reinterpret_cast<f4*>(a.wcost)[o] = f4{k + 0 < a.K ? c.x + t.x : c.x, k + 1 < a.K ? c.y + t.y : c.y,
                                         k + 2 < a.K ? c.z + t.z : c.z, k + 3 < a.K ? c.w + t.w : c.w};
}

template <bool NT, bool CLAMP, bool ANCHOR>
__global__ __launch_bounds__(kRateCells * 64) void rate_term_block_kernel(RateArgs a, int Lc, int ncell) {
  __shared__ f4 sp[kRateCells][64];
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const int cell = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // (blockDim.x = 64 ncell)
  const int R = a.nu * a.H, nq = a.Kp >> 2;
  const int q = blockIdx.x * 64 + lane;
  const bool act = q < nq;
  const f4* src = reinterpret_cast<const f4*>(a.noise + (long)b * R * a.Kp) + (act ? q : nq - 1);
  sp[cell][lane] = rate_cell<NT, CLAMP, ANCHOR>(a, src, a.U + (long)b * R, a.u_prev + (long)b * a.nu, cell * Lc,
                                        min(R, (cell + 1) * Lc), nq);
  __syncthreads();
  if (cell == 0 && act) {
    f4 s = sp[0][lane];
    for (int c = 1; c < ncell; ++c) s = s + sp[c][lane];  // cell order
    rate_store(a, b, q, s);
  }
}

template <bool NT, bool CLAMP, bool ANCHOR>
__global__ __launch_bounds__(64) void rate_term_split_kernel(RateArgs a, int Lc, int ncell) {
  const int b = blockIdx.z, cell = blockIdx.y, lane = threadIdx.x;
  const int R = a.nu * a.H, nq = a.Kp >> 2;
  const int q = blockIdx.x * 64 + lane;
  const bool act = q < nq;
  const f4* src = reinterpret_cast<const f4*>(a.noise + (long)b * R * a.Kp) + (act ? q : nq - 1);
  const f4 s = rate_cell<NT, CLAMP, ANCHOR>(a, src, a.U + (long)b * R, a.u_prev + (long)b * a.nu, cell * Lc,
                                    min(R, (cell + 1) * Lc), nq);
  if (act) reinterpret_cast<f4*>(a.part)[((long)b * ncell + cell) * nq + q] = s;
}

__global__ __launch_bounds__(256) void rate_finish_kernel(RateArgs a, int ncell) {
  const int b = blockIdx.y, nq = a.Kp >> 2;
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= nq) return;
  const f4* p = reinterpret_cast<const f4*>(a.part) + (long)b * ncell * nq + q;
  f4 s = p[0];
  for (int c = 1; c < ncell; ++c) s = s + p[(long)c * nq];  // cell order
  rate_store(a, b, q, s);
}

// u_prev <- the u0 the solve returns (MPPI_FLAG_SHIFT with the anchor on), behind the update and the bounds' clip
__global__ __launch_bounds__(256) void rate_store_prev_kernel(const float* __restrict__ u0, float* __restrict__ u_prev,
                                                              int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) u_prev[i] = u0[i];
}

// the cells of one solve: fixed by nu H alone (so by the handle)
static void rate_cells(int R, int* Lc, int* ncell) {
  int l = (R + kRateCells - 1) / kRateCells;
  l = l < kRateMinRows ? kRateMinRows : l;
  *Lc = l;
  *ncell = (R + l - 1) / l;
}

size_t rate_part_floats(int B, int nu, int H, int Kp) {
  int Lc, ncell;
  rate_cells(nu * H, &Lc, &ncell);
  return (size_t)B * ncell * Kp;
}

// MPPI_RATE_COST_FORM=block|split and MPPI_RATE_COST_NT=0|1 (read per launch; A/B and test knobs): force one form of
// the term kernel / the nontemporal loads; default: block when its (b, chunk) grid has at least as many blocks as the
// device has CUs, nontemporal above launch_reduce's cut
static int rate_form_knob() {
  const char* e = std::getenv("MPPI_RATE_COST_FORM");
  if (!e) return 0;
  return std::strcmp(e, "block") == 0 ? 1 : (std::strcmp(e, "split") == 0 ? 2 : 0);
}

static int rate_nt_knob() {
  const char* e = std::getenv("MPPI_RATE_COST_NT");
  if (!e || (e[0] != '0' && e[0] != '1') || e[1] != '\0') return -1;
  return e[0] - '0';
}

template <bool NT, bool CLAMP, bool ANCHOR>
static hipError_t rate_launch(const RateArgs& a, bool block, int Lc, int ncell, hipStream_t stream) {
  const int nq = a.Kp >> 2, nchunk = (nq + 63) / 64;
  if (block) {
    hipLaunchKernelGGL((rate_term_block_kernel<NT, CLAMP, ANCHOR>), dim3(nchunk, a.B), dim3(64 * ncell), 0, stream, a, Lc,
                       ncell);
    return hipGetLastError();
  }
  hipLaunchKernelGGL((rate_term_split_kernel<NT, CLAMP, ANCHOR>), dim3(nchunk, ncell, a.B), dim3(64), 0, stream, a, Lc, ncell);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(rate_finish_kernel, dim3((nq + 255) / 256, a.B), dim3(256), 0, stream, a, ncell);
  return hipGetLastError();
}

hipError_t launch_rate_cost(const RateArgs& a, hipStream_t stream) {
  if (a.B < 1 || a.B > 65535 || a.nu < 1 || a.nu > kMaxNu || a.H < 1) return hipErrorInvalidValue;  // (b: a grid's y / z)
  int Lc, ncell;
  rate_cells(a.nu * a.H, &Lc, &ncell);
  const int nq = a.Kp >> 2, nchunk = (nq + 63) / 64;
  const int form = rate_form_knob(), ntk = rate_nt_knob();
  const bool block = form == 1 || (form == 0 && (long)a.B * nchunk >= current_device_cus());
  const bool nt = ntk >= 0 ? ntk == 1 : (double)a.B * a.nu * a.H * a.Kp * 4.0 > 128.0 * 1024 * 1024;  // launch_reduce's cut
  const bool clamp = a.clamp > 0.0f;
  using Launch = hipError_t (*)(const RateArgs&, bool, int, int, hipStream_t);
  static const Launch table[2][2][2] = {  // [nt][clamp][anchor]
      {{rate_launch<false, false, false>, rate_launch<false, false, true>},
       {rate_launch<false, true, false>, rate_launch<false, true, true>}},
      {{rate_launch<true, false, false>, rate_launch<true, false, true>},
       {rate_launch<true, true, false>, rate_launch<true, true, true>}}};
  return table[nt][clamp][a.anchor != 0](a, block, Lc, ncell, stream);
}

hipError_t launch_rate_store_prev(const float* u0, float* u_prev, int n, hipStream_t stream) {
  hipLaunchKernelGGL(rate_store_prev_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, u0, u_prev, n);
  return hipGetLastError();
}

}  // namespace mppi
