// The control-cost term of information-theoretic MPPI (mppi_set_control_cost; the rule for lin is control_cost.h):
//   lin  [b][u][t] = gamma / sigma_u[u]^2 * (P U[b][u][:])[t]          ctrl_lin_kernel (B nu H values: tiny)
//   term [b][k]    = sum_{u,t} lin[b][u][t] * eps[b][u][t][k]          ctrl_term_*_kernel (the whole noise once: the hot part)
//   wcost[b][k]    = costs[b][k] + term[b][k]                          (pads K..Kp: costs copied through, term 0)
// Two launches (three in the split form) between the rollout and everything that weighs the solve's costs; read-only
// on U, the noise and the costs.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>

#include "control_cost.h"
#include "mppi_internal.h"

namespace mppi {

// one thread per entry of lin; the law by value, or (d_law: an adapting handle) read from the device law on the stream
__global__ __launch_bounds__(256) void ctrl_lin_kernel(CtrlArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.B * a.nu * a.H) return;
  const int bu = i / a.H, t = i - bu * a.H, u = bu % a.nu;
  const float sigma = a.d_law ? a.d_law[u] : (a.law.per_u ? a.law.sigma_u[u] : a.law.sigma);
  const float rho = a.d_law ? a.d_law[kLawRho] : a.law.rho;
  a.lin[i] = ctrl_lin_entry(ctrl_lin_scale(a.law.gamma, sigma, rho, a.H), rho, a.U + (long)bu * a.H, t, a.H);
}

// ------------------------------------------------------------------------------------------------
// The term: every noise element read once, [B][nu][H][Kp] with k fastest (config #4: 352 MB, reduce_kernel's stream).
// The R = nu H rows of a solve are cut into CELLS of Lc consecutive rows in (u, t) order (ctrl_cells: at most
// kCtrlCells of them, at least kCtrlMinRows rows each, so the split form's partials are <= 1/16 of the noise and
// 1.2 % at config #4); a wave owns a chunk of 256 consecutive k (each lane one k-quad, 16-B loads) of one cell and
// accumulates fmaf(lin, eps, acc) over the cell's rows in row order, lin wave-uniform (scalar loads), kCtrlTile rows
// per load tile with the next tile issued before the current one is consumed (16 loads per lane in flight),
// nontemporal above launch_reduce's 128 MB cut.  The cells' sums are then added in cell order.  The order per k is
// fixed by the shape alone, so runs repeat bitwise and the two forms agree bit for bit:
//   block  a block owns (b, chunk), wave w walks cell w, the sums meet in LDS (16 KiB) and wave 0 adds them and
//          forms wcost: no partial buffer, one launch.  For batches whose (b, chunk) blocks fill the chip (config #4).
//   split  one single-wave block per (chunk, cell, b) stores its sum as a partial [B][cells][Kp]; ctrl_finish_kernel
//          adds them and forms wcost.  For grids that would leave most CUs idle (config #2, config #5, the shards).
// No atomics; inactive lanes (quads beyond Kp) read a clamped, in-bounds quad and store nothing.
// ------------------------------------------------------------------------------------------------
constexpr int kCtrlCells = 16;    // cells per solve (at most) = waves per block of the block form
constexpr int kCtrlMinRows = 16;  // rows per cell (at least, while the solve has them)
constexpr int kCtrlTile = 8;      // rows per load tile
typedef float f4 __attribute__((ext_vector_type(4)));

template <bool NT>
__device__ __forceinline__ f4 ctrl_ld(const f4* p) {
  if constexpr (NT) return __builtin_nontemporal_load(p);
  else return *p;
}

// the sum of one cell, rows [r0, r1) of the solve whose row r is src + r * nq (this lane's quad) and lin[r]
template <bool NT>
__device__ __forceinline__ f4 ctrl_cell(const f4* src, const float* __restrict__ lin, int r0, int r1, int nq) {
  f4 cur[kCtrlTile], nxt[kCtrlTile];
  auto load = [&](f4* dst, int t0) {
#pragma unroll
    for (int j = 0; j < kCtrlTile; ++j) dst[j] = ctrl_ld<NT>(src + (long)min(t0 + j, r1 - 1) * nq);
  };
  load(cur, r0);
  f4 acc = f4{0.0f, 0.0f, 0.0f, 0.0f};
  for (int t0 = r0; t0 < r1; t0 += kCtrlTile) {
    const bool more = t0 + kCtrlTile < r1;
    if (more) load(nxt, t0 + kCtrlTile);
#pragma unroll
    for (int j = 0; j < kCtrlTile; ++j) {
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
      for (int j = 0; j < kCtrlTile; ++j) cur[j] = nxt[j];
    }
  }
  return acc;
}

// quad q of solve b: term and wcost from the summed cells (pads K..Kp: term 0, the cost copied through)
__device__ __forceinline__ void ctrl_store(const CtrlArgs& a, int b, int q, const f4& s) {
  const long o = (long)b * (a.Kp >> 2) + q;
  const f4 c = reinterpret_cast<const f4*>(a.costs)[o];
  const int k = 4 * q;
  const f4 t = f4{k + 0 < a.K ? s.x : 0.0f, k + 1 < a.K ? s.y : 0.0f, k + 2 < a.K ? s.z : 0.0f,
                  k + 3 < a.K ? s.w : 0.0f};
  reinterpret_cast<f4*>(a.term)[o] = t;
  reinterpret_cast<f4*>(a.wcost)[o] = f4{k + 0 < a.K ? c.x + t.x : c.x, k + 1 < a.K ? c.y + t.y : c.y,
                                         k + 2 < a.K ? c.z + t.z : c.z, k + 3 < a.K ? c.w + t.w : c.w};
}

template <bool NT>
__global__ __launch_bounds__(kCtrlCells * 64) void ctrl_term_block_kernel(CtrlArgs a, int Lc, int ncell) {
  __shared__ f4 sp[kCtrlCells][64];
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const int cell = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // (blockDim.x = 64 ncell)
  const int R = a.nu * a.H, nq = a.Kp >> 2;
  const int q = blockIdx.x * 64 + lane;
  const bool act = q < nq;
  const f4* src = reinterpret_cast<const f4*>(a.noise + (long)b * R * a.Kp) + (act ? q : nq - 1);
  sp[cell][lane] = ctrl_cell<NT>(src, a.lin + (long)b * R, cell * Lc, min(R, (cell + 1) * Lc), nq);
  __syncthreads();
  if (cell == 0 && act) {
    f4 s = sp[0][lane];
    for (int c = 1; c < ncell; ++c) s = s + sp[c][lane];  // cell order
    ctrl_store(a, b, q, s);
  }
}

template <bool NT>
__global__ __launch_bounds__(64) void ctrl_term_split_kernel(CtrlArgs a, int Lc, int ncell) {
  const int b = blockIdx.z, cell = blockIdx.y, lane = threadIdx.x;
  const int R = a.nu * a.H, nq = a.Kp >> 2;
  const int q = blockIdx.x * 64 + lane;
  const bool act = q < nq;
  const f4* src = reinterpret_cast<const f4*>(a.noise + (long)b * R * a.Kp) + (act ? q : nq - 1);
  const f4 s = ctrl_cell<NT>(src, a.lin + (long)b * R, cell * Lc, min(R, (cell + 1) * Lc), nq);
  if (act) reinterpret_cast<f4*>(a.part)[((long)b * ncell + cell) * nq + q] = s;
}

__global__ __launch_bounds__(256) void ctrl_finish_kernel(CtrlArgs a, int ncell) {
  const int b = blockIdx.y, nq = a.Kp >> 2;
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= nq) return;
  const f4* p = reinterpret_cast<const f4*>(a.part) + (long)b * ncell * nq + q;
  f4 s = p[0];
  for (int c = 1; c < ncell; ++c) s = s + p[(long)c * nq];  // cell order
  ctrl_store(a, b, q, s);
}

// the cells of one solve: fixed by nu H alone (so by the handle)
static void ctrl_cells(int R, int* Lc, int* ncell) {
  int l = (R + kCtrlCells - 1) / kCtrlCells;
  l = l < kCtrlMinRows ? kCtrlMinRows : l;
  *Lc = l;
  *ncell = (R + l - 1) / l;
}

size_t ctrl_part_floats(int B, int nu, int H, int Kp) {
  int Lc, ncell;
  ctrl_cells(nu * H, &Lc, &ncell);
  return (size_t)B * ncell * Kp;
}

// MPPI_CTRL_COST_FORM=block|split and MPPI_CTRL_COST_NT=0|1 (read per launch; A/B and test knobs): force one form of
// the term kernel / the nontemporal loads; default: block when its (b, chunk) grid has at least as many blocks as the
// device has CUs, nontemporal above launch_reduce's cut
static int ctrl_form_knob() {
  const char* e = std::getenv("MPPI_CTRL_COST_FORM");
  if (!e) return 0;
  return std::strcmp(e, "block") == 0 ? 1 : (std::strcmp(e, "split") == 0 ? 2 : 0);
}

static int ctrl_nt_knob() {
  const char* e = std::getenv("MPPI_CTRL_COST_NT");
  if (!e || (e[0] != '0' && e[0] != '1') || e[1] != '\0') return -1;
  return e[0] - '0';
}

hipError_t launch_ctrl_cost(const CtrlArgs& a, hipStream_t stream) {
  if (a.B < 1 || a.B > 65535) return hipErrorInvalidValue;  // (b is a grid's y / z index)
  const int n = a.B * a.nu * a.H;
  hipLaunchKernelGGL(ctrl_lin_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  int Lc, ncell;
  ctrl_cells(a.nu * a.H, &Lc, &ncell);
  const int nq = a.Kp >> 2, nchunk = (nq + 63) / 64;
  const int form = ctrl_form_knob(), ntk = ctrl_nt_knob();
  const bool block = form == 1 || (form == 0 && (long)a.B * nchunk >= current_device_cus());
  const bool nt = ntk >= 0 ? ntk == 1 : (double)n * a.Kp * 4.0 > 128.0 * 1024 * 1024;  // launch_reduce's cut
  if (block) {
    hipLaunchKernelGGL(nt ? ctrl_term_block_kernel<true> : ctrl_term_block_kernel<false>, dim3(nchunk, a.B),
                       dim3(64 * ncell), 0, stream, a, Lc, ncell);
    return hipGetLastError();
  }
  hipLaunchKernelGGL(nt ? ctrl_term_split_kernel<true> : ctrl_term_split_kernel<false>, dim3(nchunk, ncell, a.B),
                     dim3(64), 0, stream, a, Lc, ncell);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(ctrl_finish_kernel, dim3((nq + 255) / 256, a.B), dim3(256), 0, stream, a, ncell);
  return hipGetLastError();
}

}  // namespace mppi
