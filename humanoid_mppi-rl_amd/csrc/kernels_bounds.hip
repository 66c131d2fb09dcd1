// Per-actuator control bounds (mppi_set_control_bounds; the rule is ctrl_bounds.h):
//   eps'[b][u][t][k] = clip(U[b][u][t] + eps, lo[u], hi[u]) - U[b][u][t]   bounds_project_kernel, in place over the
//                      solve's noise ahead of the rollout (the whole noise once: the hot part); part[row][chunk] = the
//                      (k < K) elements each wave projected in each row
//   U, Umirror, u0   = clip(., lo[u], hi[u]);  counts[b][u] = sum part      bounds_clip_kernel, behind the update
// Both sit beside the rollout and reduce kernels, never inside them: a bounded solve is routed exactly as without bounds.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>

#include "ctrl_bounds.h"
#include "mppi_internal.h"

namespace mppi {

typedef float f4 __attribute__((ext_vector_type(4)));

template <bool NT>
__device__ __forceinline__ f4 bounds_ld(const f4* p) {
  if constexpr (NT) return __builtin_nontemporal_load(p);
  else return *p;
}

// ------------------------------------------------------------------------------------------------
// The projection.  The noise is rows = B nu H rows of Kp floats (k fastest; row r's nominal is U[r], its actuator
// u = (r / H) % nu).  A wave owns one CHUNK of 256 consecutive k (each lane one k-quad, 16-B loads) of T consecutive
// rows: all T loads are issued before the first is consumed, and U / lo / hi are wave-uniform (scalar loads).
// Stores (ST): a quad is dirty when one of its four elements changed;
//   quad  a lane stores its quad only if it is dirty
//   line  the eight lanes of a 128-B line store all eight quads if one of them is dirty (clean quads are written back
//         bit for bit as they were read), so no line is written in part -- and no line that is wholly clean is written
//         at all: the write traffic follows the share of dirty lines either way
// Elements K..Kp (the pads; the fused generators leave non-zero values there) are passed through and never counted;
// lanes whose quad lies beyond Kp read a clamped, in-bounds quad and store nothing (Kp is a multiple of 64, so a line's
// eight lanes are all inside or all beyond).  The wave's count of a row is the popcount of four ballots (scalar) and
// goes to part[row][chunk], every entry written on every launch: no atomics, nothing to zero, and bounds_clip_kernel
// sums a (b, u)'s entries as integers (exactly repeatable).  Waves are numbered chunk-fastest (the waves of a block
// walk one row tile side by side); T is chosen by the launcher so that small solves still spread over the chip.
// ------------------------------------------------------------------------------------------------
enum BoundsStore : int { kStoreQuad = 0, kStoreLine = 1 };

template <int T, bool NT, int ST>
__global__ __launch_bounds__(256) void bounds_project_kernel(BoundsArgs a, int rows, int nchunk, int nwave) {
  // (rows, waves and so every index below but the element offsets fit 32 bits: the launcher checks)
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) + (int)blockIdx.x * 4;
  if (w >= nwave) return;  // (wave-uniform)
  const int lane = threadIdx.x & 63;
  const int nq = a.Kp >> 2;
  const int tile = (int)((unsigned)w / (unsigned)nchunk);
  const int chunk = w - tile * nchunk;
  const int r0 = tile * T;
  const int q = chunk * 64 + lane;
  const bool act = q < nq;
  f4* base = reinterpret_cast<f4*>(a.noise) + (act ? q : nq - 1);
  f4 v[T];
  float Ur[T];  // (read ahead of the first store: the compiler keeps them scalar loads)
#pragma unroll
  for (int j = 0; j < T; ++j) {
    const int r = r0 + j < rows ? r0 + j : rows - 1;
    v[j] = bounds_ld<NT>(base + (long)r * nq);
    Ur[j] = a.U[r];
  }
  const int k = 4 * q;
  const bool in0 = act && k + 0 < a.K, in1 = act && k + 1 < a.K, in2 = act && k + 2 < a.K, in3 = act && k + 3 < a.K;
  // row r0 is step t of actuator u; the rows behind it step t, then u (one division each per wave, none per row)
  const int bu0 = (int)((unsigned)r0 / (unsigned)a.H);
  int t = r0 - bu0 * a.H, u = (int)((unsigned)bu0 % (unsigned)a.nu);
#pragma unroll
  for (int j = 0; j < T; ++j) {
    const int r = r0 + j;
    if (r < rows) {  // (uniform)
      const float U = Ur[j], lo = a.lo[u], hi = a.hi[u];
      int h0, h1, h2, h3;
      f4 o;
      o.x = ctrl_bounds_project(U, v[j].x, lo, hi, &h0);
      o.y = ctrl_bounds_project(U, v[j].y, lo, hi, &h1);
      o.z = ctrl_bounds_project(U, v[j].z, lo, hi, &h2);
      o.w = ctrl_bounds_project(U, v[j].w, lo, hi, &h3);
      const bool c0 = in0 && h0, c1 = in1 && h1, c2 = in2 && h2, c3 = in3 && h3;
      const bool dirty = c0 || c1 || c2 || c3;
      bool store = dirty;
      if constexpr (ST == kStoreLine) store = act && ((__ballot(dirty) >> (lane & 56)) & 0xffull) != 0ull;
      if (store) base[(long)r * nq] = f4{c0 ? o.x : v[j].x, c1 ? o.y : v[j].y, c2 ? o.z : v[j].z, c3 ? o.w : v[j].w};
      const unsigned n = (unsigned)(__popcll(__ballot(c0)) + __popcll(__ballot(c1)) + __popcll(__ballot(c2)) +
                                    __popcll(__ballot(c3)));
      if (lane == 0) a.part[(long)r * nchunk + chunk] = n;
      if (++t == a.H) {
        t = 0;
        u = u + 1 == a.nu ? 0 : u + 1;
      }
    }
  }
}

// One block per (b, u), behind the update: counts[b][u] = the sum of the row's H nchunk partial counts, and (U given: a
// solve; mppi_bounds_eval passes none) the H entries of U, their mirror and u0 clipped, storing only what changes.
__global__ __launch_bounds__(256) void bounds_clip_kernel(BoundsArgs a, float* U, float* Umirror, float* u0,
                                                          int nchunk) {
  __shared__ unsigned total;
  const int bu = blockIdx.x, u = bu % a.nu;
  if (threadIdx.x == 0) total = 0u;
  __syncthreads();
  const unsigned* p = a.part + (long)bu * a.H * nchunk;
  unsigned n = 0u;
  for (int i = threadIdx.x; i < a.H * nchunk; i += 256) n += p[i];
  if (n) atomicAdd(&total, n);  // (LDS, integers: any order gives the same sum)
  if (U) {
    const float lo = a.lo[u], hi = a.hi[u];
    for (int j = threadIdx.x; j < a.H; j += 256) {
      const long o = (long)bu * a.H + j;
      const float v = U[o], c = ctrl_bounds_clip(v, lo, hi);
      if (c != v) {
        U[o] = c;
        if (Umirror) Umirror[o] = c;
      }
    }
    if (threadIdx.x == 0 && u0) {
      const float v = u0[bu], c = ctrl_bounds_clip(v, lo, hi);
      if (c != v) u0[bu] = c;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) a.counts[bu] = total;
}

// MPPI_BOUNDS_NT=0|1 (read per launch; an A/B and test knob): force the cached / the nontemporal loads of the
// projection; default: nontemporal above launch_reduce's 128 MB cut (below it the rollout behind finds the noise cached)
static int bounds_nt_knob() { return env_flag("MPPI_BOUNDS_NT"); }

// MPPI_BOUNDS_STORE=quad|line (read per launch; an A/B and test knob): force one store form of the projection
static int bounds_store_knob() {
  const char* e = std::getenv("MPPI_BOUNDS_STORE");
  if (!e) return -1;
  return std::strcmp(e, "quad") == 0 ? kStoreQuad : (std::strcmp(e, "line") == 0 ? kStoreLine : -1);
}

// MPPI_BOUNDS_ROWS=1|2|4|8 (read per launch; a test knob): force the rows a wave of the projection takes
static int bounds_rows_knob() {
  const char* e = std::getenv("MPPI_BOUNDS_ROWS");
  const int v = e ? std::atoi(e) : 0;
  return (v == 1 || v == 2 || v == 4 || v == 8) ? v : 0;
}

int bounds_chunks(int Kp) { return ((Kp >> 2) + 63) / 64; }

template <int T>
static void bounds_project_launch(const BoundsArgs& a, bool nt, int st, int rows, int nchunk, hipStream_t stream) {
  const int nwave = (rows + T - 1) / T * nchunk;
  const dim3 grid((unsigned)((nwave + 3) / 4));
  void (*kern)(BoundsArgs, int, int, int);
  if (st == kStoreLine) kern = nt ? bounds_project_kernel<T, true, kStoreLine> : bounds_project_kernel<T, false, kStoreLine>;
  else kern = nt ? bounds_project_kernel<T, true, kStoreQuad> : bounds_project_kernel<T, false, kStoreQuad>;
  hipLaunchKernelGGL(kern, grid, dim3(256), 0, stream, a, rows, nchunk, nwave);
}

hipError_t launch_bounds_project(const BoundsArgs& a, hipStream_t stream) {
  const long lrows = (long)a.B * a.nu * a.H;
  const int nchunk = bounds_chunks(a.Kp);
  // (rows and waves are 32-bit indices in the kernel: 2^30 waves are a noise buffer of a terabyte)
  if (a.B < 1 || lrows * nchunk >= (1L << 30)) return hipErrorInvalidValue;
  const int rows = (int)lrows;
  const int ntk = bounds_nt_knob(), stk = bounds_store_knob();
  const bool nt = ntk >= 0 ? ntk == 1 : (double)lrows * a.Kp * 4.0 > 128.0 * 1024 * 1024;  // launch_reduce's cut
  const int st = stk >= 0 ? stk : kStoreLine;
  // rows per wave: 8 while that leaves every CU at least 8 waves (config #4: 43,008 waves; config #5: 10,752), else
  // fewer (config #2: 1 row, 800 waves)
  const long want = 8L * current_device_cus();  // (long: rows / T * nchunk below stays exact)
  int T = bounds_rows_knob();
  if (T == 0)
    for (T = 8; T > 1 && lrows / T * nchunk < want; T >>= 1) {
    }
  if (T == 8) bounds_project_launch<8>(a, nt, st, rows, nchunk, stream);
  else if (T == 4) bounds_project_launch<4>(a, nt, st, rows, nchunk, stream);
  else if (T == 2) bounds_project_launch<2>(a, nt, st, rows, nchunk, stream);
  else bounds_project_launch<1>(a, nt, st, rows, nchunk, stream);
  return hipGetLastError();
}

hipError_t launch_bounds_clip(const BoundsArgs& a, float* U, float* Umirror, float* u0, hipStream_t stream) {
  if (a.B < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(bounds_clip_kernel, dim3((unsigned)(a.B * a.nu)), dim3(256), 0, stream, a, U, Umirror, u0,
                     bounds_chunks(a.Kp));
  return hipGetLastError();
}

}  // namespace mppi
