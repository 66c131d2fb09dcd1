// The cell scheme of the cost-term kernels (kernels_ctrl_cost.hip, kernels_rate_cost.hip): a term [b][k] that is a sum
// over the solve's noise rows, and wcost = costs + term.
// ------------------------------------------------------------------------------------------------
// Every noise element is read once, [B][nu][H][Kp] with k fastest (config #4: 352 MB, reduce_kernel's stream).  The
// R = nu H rows of a solve are cut into CELLS of Lc consecutive rows in (u, t) order (term_cells: at most kTermCells of
// them, at least kTermMinRows rows each, so the split form's partials are <= 1/16 of the noise and 1.2 % at config
// #4); a wave owns a chunk of 256 consecutive k (each lane one k-quad, 16-B loads) of one cell and walks the cell's
// rows in row order -- the term's own cell_sum(src, b, r0, r1, nq), its operands wave-uniform (scalar loads) --
// kTermTile rows per load tile with the next tile issued before the current one is consumed (16 loads per lane in
// flight), nontemporal above launch_reduce's 128 MB cut.  The cells' sums are then added in cell order.  The order per
// k is fixed by the shape alone, so runs repeat bitwise and the two forms agree bit for bit:
//   block  a block owns (b, chunk), wave w walks cell w, the sums meet in LDS (16 KiB) and wave 0 adds them and
//          forms wcost: no partial buffer, one launch.  For batches whose (b, chunk) blocks fill the chip (config #4).
//   split  one single-wave block per (chunk, cell, b) stores its sum as a partial [B][cells][Kp]; the finish kernel
//          adds them and forms wcost.  For grids that would leave most CUs idle (config #2, config #5, the shards).
// No atomics; inactive lanes (quads beyond Kp) read a clamped, in-bounds quad and store nothing.
// The bodies read only the members every term's args struct has: B nu H K Kp noise costs term wcost part.
// ------------------------------------------------------------------------------------------------
#pragma once
#include <hip/hip_runtime.h>

#include "mppi_internal.h"

namespace mppi {

constexpr int kTermCells = 16;    // cells per solve (at most) = waves per block of the block form
constexpr int kTermMinRows = 16;  // rows per cell (at least, while the solve has them)
constexpr int kTermTile = 8;      // rows per load tile
typedef float f4 __attribute__((ext_vector_type(4)));

template <bool NT>
__device__ __forceinline__ f4 term_ld(const f4* p) {
  if constexpr (NT) return __builtin_nontemporal_load(p);
  else return *p;
}

// quad q of solve b: term and wcost from the summed cells (pads K..Kp: term 0, the cost copied through)
template <class Args>
__device__ __forceinline__ void term_store(const Args& a, int b, int q, const f4& s) {
  const long o = (long)b * (a.Kp >> 2) + q;
  const f4 c = reinterpret_cast<const f4*>(a.costs)[o];
  const int k = 4 * q;
  const f4 t = f4{k + 0 < a.K ? s.x : 0.0f, k + 1 < a.K ? s.y : 0.0f, k + 2 < a.K ? s.z : 0.0f,
                  k + 3 < a.K ? s.w : 0.0f};
  reinterpret_cast<f4*>(a.term)[o] = t;
  reinterpret_cast<f4*>(a.wcost)[o] = f4{k + 0 < a.K ? c.x + t.x : c.x, k + 1 < a.K ? c.y + t.y : c.y,
                                         k + 2 < a.K ? c.z + t.z : c.z, k + 3 < a.K ? c.w + t.w : c.w};
}

// The three kernel bodies.  cell_sum(src, b, r0, r1, nq): the sum of rows [r0, r1) of solve b, whose row r is
// src + r * nq (this lane's quad).  Grids: block (nchunk, B) x 64 ncell threads; split (nchunk, ncell, B) x 64;
// finish (ceil(nq / 256), B) x 256.
template <class Args, class CellSum>
__device__ __forceinline__ void term_block_body(const Args& a, int Lc, int ncell, CellSum&& cell_sum) {
  __shared__ f4 sp[kTermCells][64];
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const int cell = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // (blockDim.x = 64 ncell)
  const int R = a.nu * a.H, nq = a.Kp >> 2;
  const int q = blockIdx.x * 64 + lane;
  const bool act = q < nq;
  const f4* src = reinterpret_cast<const f4*>(a.noise + (long)b * R * a.Kp) + (act ? q : nq - 1);
  sp[cell][lane] = cell_sum(src, b, cell * Lc, min(R, (cell + 1) * Lc), nq);
  __syncthreads();
  if (cell == 0 && act) {
    f4 s = sp[0][lane];
    for (int c = 1; c < ncell; ++c) s = s + sp[c][lane];  // cell order
    term_store(a, b, q, s);
  }
}

template <class Args, class CellSum>
__device__ __forceinline__ void term_split_body(const Args& a, int Lc, int ncell, CellSum&& cell_sum) {
  const int b = blockIdx.z, cell = blockIdx.y, lane = threadIdx.x;
  const int R = a.nu * a.H, nq = a.Kp >> 2;
  const int q = blockIdx.x * 64 + lane;
  const bool act = q < nq;
  const f4* src = reinterpret_cast<const f4*>(a.noise + (long)b * R * a.Kp) + (act ? q : nq - 1);
  const f4 s = cell_sum(src, b, cell * Lc, min(R, (cell + 1) * Lc), nq);
  if (act) reinterpret_cast<f4*>(a.part)[((long)b * ncell + cell) * nq + q] = s;
}

template <class Args>
__device__ __forceinline__ void term_finish_body(const Args& a, int ncell) {
  const int b = blockIdx.y, nq = a.Kp >> 2;
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= nq) return;
  const f4* p = reinterpret_cast<const f4*>(a.part) + (long)b * ncell * nq + q;
  f4 s = p[0];
  for (int c = 1; c < ncell; ++c) s = s + p[(long)c * nq];  // cell order
  term_store(a, b, q, s);
}

// the cells of one solve: fixed by R = nu H alone (so by the handle)
inline void term_cells(int R, int* Lc, int* ncell) {
  int l = (R + kTermCells - 1) / kTermCells;
  l = l < kTermMinRows ? kTermMinRows : l;
  *Lc = l;
  *ncell = (R + l - 1) / l;
}

// the split form's partials [B][cells][Kp]
inline size_t term_part_floats(int B, int nu, int H, int Kp) {
  int Lc, ncell;
  term_cells(nu * H, &Lc, &ncell);
  return (size_t)B * ncell * Kp;
}

// The form and the loads of one launch.  form_env = block|split and nt_env = 0|1 (read per launch; A/B and test
// knobs) force one form of the term kernel / the nontemporal loads; default: block when its (b, chunk) grid has at
// least as many blocks as the device has CUs, nontemporal when the noise read (`bytes`) is above launch_reduce's cut
struct TermForm {
  bool block, nt;
};
inline TermForm term_form(const char* form_env, const char* nt_env, int B, int nchunk, double bytes) {
  const int form = env_choice(form_env, "block", "split"), ntk = env_flag(nt_env);
  return TermForm{form == 1 || (form == 0 && (long)B * nchunk >= current_device_cus()),
                  ntk >= 0 ? ntk == 1 : bytes > 128.0 * 1024 * 1024};
}

// the block form (one launch), or the split form and its finish (two); B <= 65535: b is a grid's y / z index
template <class Args, class TermKernel, class FinishKernel>
hipError_t term_launch(const Args& a, bool block_form, TermKernel block, TermKernel split, FinishKernel finish,
                       hipStream_t stream) {
  int Lc, ncell;
  term_cells(a.nu * a.H, &Lc, &ncell);
  const int nq = a.Kp >> 2, nchunk = (nq + 63) / 64;
  if (block_form) {
    hipLaunchKernelGGL(block, dim3(nchunk, a.B), dim3(64 * ncell), 0, stream, a, Lc, ncell);
    return hipGetLastError();
  }
  hipLaunchKernelGGL(split, dim3(nchunk, ncell, a.B), dim3(64), 0, stream, a, Lc, ncell);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(finish, dim3((nq + 255) / 256, a.B), dim3(256), 0, stream, a, ncell);
  return hipGetLastError();
}

}  // namespace mppi
