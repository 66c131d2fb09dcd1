// Weighted cross moments of a solve's noise (MPPI_FLAG_CROSS, mppi_cross_moments_eval; the definition and its cell
// scheme: cross_moments.h).  Two launches on the solve's stream behind the statistics, whose normalised weights they
// read: cross_moment_kernel (the noise stream, the hot part) and cross_finish_kernel (the fixed-order sum of its
// partials).  Read-only on everything a solve owns.
#include <hip/hip_runtime.h>

#include "cross_moments.h"
#include "mppi_internal.h"
#include "wave_reduce.h"

namespace mppi {

// ------------------------------------------------------------------------------------------------
// The triangle of pairs (u, v <= u) is cut into tiles of kCrossTile x kCrossTile pairs: row block I against row block
// J <= I.  One WAVE owns one tile of one cell walk: its lanes own the k-quads of a wave-chunk (the weights in registers
// for the whole walk, as in stats_moment_kernel) and hold the tile's 64 accumulators (a diagonal tile: the 36 of
// v <= u).  The waves of a block are the tiles of ONE (solve, chunk, segment walk): they read the same nu rows at
// about the same time, each row block as often as it has tiles (nu = 21: 3 times, nu = 32: 4-5 times), so the buffer
// comes from HBM once and the re-reads from the block's L1 / the L2.  More than 8 tiles (nu > 24) are spread over two
// blocks, which keeps a wave at 256 registers.  16-B loads, one step's rows (8 or 16 per lane) issued ahead of the step
// being consumed.  The loads are NOT nontemporal, unlike stats_moment_kernel's above launch_reduce's 128 MB cut: a row
// is wanted again by the block's other waves, and the hint measured 20-30 % slower on config #4 (DESIGN.md §4;
// MPPI_CROSS_NT=1 keeps the arm).  No barrier, no atomics, no LDS; inactive lanes carry weight 0 and read a clamped,
// in-bounds quad; rows beyond nu are clamped to nu - 1 and their sums dropped.
//   direct  one wave walks all segments of its chunk
//   seg     one wave per segment: for grids too small to give every SIMD several waves (config #4: 64 solves x 4 chunks
//           x 6 tiles are 1.5 waves per SIMD in the direct form)
// At the end of a cell the 64 accumulators are summed over the wave together: wave_sum's butterfly (offsets 32 .. 1)
// with every step exchanging half of the values still held, so lane l ends with the sum of accumulator l, the bits of
// wave_sum of it, for 63 exchanges instead of 384; the 64 lanes then store their partials side by side.
// ------------------------------------------------------------------------------------------------
constexpr int kCrossTile = 8;
typedef float x4 __attribute__((ext_vector_type(4)));

template <bool NT>
__device__ __forceinline__ x4 cross_ld(const x4* p) {
  if constexpr (NT) return __builtin_nontemporal_load(p);
  else return *p;
}

// N sums over the wave at once: lane l returns the wave_sum of v[l] (N = 64), bit for bit -- at offset O the lane
// whose bit O is clear keeps the lower half of the values and sends the upper, its partner the reverse (the addition
// commutes, so both orders of a pair give wave_sum's bits); v is consumed
template <int N, int O = 32>
__device__ __forceinline__ float cross_wave_sums(float (&v)[N], int lane) {
  if constexpr (N > 1) {
    const bool up = (lane & O) != 0;
    float h[N / 2];
#pragma unroll
    for (int i = 0; i < N / 2; ++i) {
      const float keep = up ? v[N / 2 + i] : v[i];
      const float send = up ? v[i] : v[N / 2 + i];
      h[i] = keep + __shfl_xor(send, O);
    }
    return cross_wave_sums<N / 2, O / 2>(h, lane);
  } else {
    return v[0];
  }
}

struct CrossWalk {
  int b, I, J, wc, s_begin, s_end, L, nseg, ncell;
};

template <bool NT, bool DIAG>
__device__ __forceinline__ void cross_walk(const CrossArgs& a, const CrossWalk& k) {
  constexpr int T = kCrossTile;
  const int lane = threadIdx.x & 63;
  const int nq = a.Kp >> 2;
  const int q = k.wc * 64 + lane;
  const bool act = q < nq;
  const int qc = act ? q : nq - 1;
  x4 w = reinterpret_cast<const x4*>(a.w + (long)k.b * a.Kp)[qc];
  if (!act) w = x4{0.0f, 0.0f, 0.0f, 0.0f};
  // row (u, t) of this solve: src + ((long)u * H + t) * nq
  const x4* src = reinterpret_cast<const x4*>(a.noise + (long)k.b * a.nu * a.H * a.Kp) + qc;
  long ru[T], rv[T];  // (wave-uniform: scalar registers)
#pragma unroll
  for (int i = 0; i < T; ++i) {
    ru[i] = (long)min(k.I * T + i, a.nu - 1) * a.H * nq;
    rv[i] = (long)min(k.J * T + i, a.nu - 1) * a.H * nq;
  }
  const int t_begin = k.s_begin * k.L, t_end = min(a.H, k.s_end * k.L);
  x4 cu[T], cv[T], nu_[T], nv[T];
  auto load = [&](x4* du, x4* dv, int t) {
#pragma unroll
    for (int i = 0; i < T; ++i) du[i] = cross_ld<NT>(src + ru[i] + (long)t * nq);
    if constexpr (!DIAG) {
#pragma unroll
      for (int i = 0; i < T; ++i) dv[i] = cross_ld<NT>(src + rv[i] + (long)t * nq);
    }
  };
  float acc[T * T];
#pragma unroll
  for (int i = 0; i < T * T; ++i) acc[i] = 0.0f;
  int seg = k.s_begin, seg_end = t_begin + k.L;
  auto flush = [&]() {
    const float s = cross_wave_sums<T * T>(acc, lane);  // lane l: accumulator l = pair (l / T, l % T) of the tile
    const int u = k.I * T + lane / T, v = k.J * T + lane % T;
    if (u < a.nu && v <= u)
      a.part[((long)k.b * cross_pairs(a.nu) + cross_pair(u, v)) * k.ncell + k.wc * k.nseg + seg] = s;
  };
  load(cu, cv, t_begin);
  for (int t = t_begin; t < t_end; ++t) {
    if (t + 1 < t_end) load(nu_, nv, t + 1);
    if (t == seg_end) {  // (direct form: the next segment's cell starts)
      flush();
      seg += 1;
      seg_end += k.L;
#pragma unroll
      for (int i = 0; i < T * T; ++i) acc[i] = 0.0f;
    }
#pragma unroll
    for (int i = 0; i < T; ++i) {
      const float p0 = cross_weigh(w.x, cu[i].x), p1 = cross_weigh(w.y, cu[i].y), p2 = cross_weigh(w.z, cu[i].z),
                  p3 = cross_weigh(w.w, cu[i].w);
#pragma unroll
      for (int j = 0; j < T; ++j) {
        if (DIAG && j > i) continue;
        const x4 e = DIAG ? cu[j] : cv[j];
        float s = acc[i * T + j];
        s = cross_fma(p0, e.x, s);
        s = cross_fma(p1, e.y, s);
        s = cross_fma(p2, e.z, s);
        s = cross_fma(p3, e.w, s);
        acc[i * T + j] = s;
      }
    }
    if (t + 1 < t_end) {
#pragma unroll
      for (int i = 0; i < T; ++i) {
        cu[i] = nu_[i];
        if constexpr (!DIAG) cv[i] = nv[i];
      }
    }
  }
  flush();
}

template <bool NT>
__global__ __launch_bounds__(512) void cross_moment_kernel(CrossArgs a, int nwc, int L, int nseg, int split, int ngrp,
                                                           int wpb) {
  const int b = blockIdx.z * 65535 + blockIdx.y;
  const int wave = threadIdx.x >> 6;
  const int grp = blockIdx.x % ngrp, cx = blockIdx.x / ngrp;
  const int nrb = (a.nu + kCrossTile - 1) / kCrossTile;
  const int tile = grp * wpb + wave;
  // direct: block = chunk, all segments; seg: block = (chunk, segment)
  const int wc = split ? cx / nseg : cx;
  if (b >= a.B || wc >= nwc || tile >= nrb * (nrb + 1) / 2) return;  // (uniform per wave; the kernel has no barrier)
  int I = 0;
  while ((I + 1) * (I + 2) / 2 <= tile) ++I;
  CrossWalk k;
  k.b = b;
  k.I = I;
  k.J = tile - I * (I + 1) / 2;
  k.wc = wc;
  k.s_begin = split ? cx - wc * nseg : 0;
  k.s_end = split ? k.s_begin + 1 : nseg;
  k.L = L;
  k.nseg = nseg;
  k.ncell = nwc * nseg;
  if (k.I == k.J) cross_walk<NT, true>(a, k);
  else cross_walk<NT, false>(a, k);
}

// one wave per (b, pair): stats_finish_kernel's order -- lane l adds its cells l, l + 64, ... ((chunk, segment) order),
// then the wave's fixed butterfly -- and the division by (float)H; the value is stored at [u][v] and [v][u]
__global__ __launch_bounds__(256) void cross_finish_kernel(CrossArgs a, int npair, int ncell) {
  const long bp = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (bp >= (long)a.B * npair) return;  // (uniform per wave; no barrier)
  const int b = (int)(bp / npair), p = (int)(bp - (long)b * npair);
  int u = 0;
  while ((u + 1) * (u + 2) / 2 <= p) ++u;
  const int v = p - u * (u + 1) / 2;
  const float* part = a.part + bp * ncell;
  float s = 0.0f;
  for (int i = lane; i < ncell; i += 64) s += part[i];
  s = wave_sum(s);
  if (lane == 0) {
    const float m = s / (float)a.H;
    a.mx[((long)b * a.nu + u) * a.nu + v] = m;
    a.mx[((long)b * a.nu + v) * a.nu + u] = m;
  }
}

size_t cross_part_floats(int B, int nu, int H, int Kp) {
  int nwc, L, nseg;
  moment_cells(H, Kp, &nwc, &L, &nseg);
  return (size_t)B * cross_pairs(nu) * nwc * nseg;
}

// MPPI_CROSS_FORM=direct|seg (read per launch; an A/B and test knob): force one form of cross_moment_kernel; default:
// seg while the direct form's grid gives a SIMD fewer than 8 waves.  MPPI_CROSS_NT=1 (A/B): nontemporal loads
hipError_t launch_cross(const CrossArgs& a, hipStream_t stream) {
  if (a.nu < 1 || a.nu > kMaxNu) return hipErrorInvalidValue;
  int nwc, L, nseg;
  moment_cells(a.H, a.Kp, &nwc, &L, &nseg);
  const int nrb = (a.nu + kCrossTile - 1) / kCrossTile, ntile = nrb * (nrb + 1) / 2;
  const int ngrp = (ntile + 7) / 8, wpb = (ntile + ngrp - 1) / ngrp;
  const int knob = env_choice("MPPI_CROSS_FORM", "direct", "seg");
  const bool split = knob == 2 || (knob == 0 && (long)a.B * nwc * ntile < 32L * current_device_cus());
  const bool nt = env_flag("MPPI_CROSS_NT") == 1;
  const int y = a.B < 65535 ? a.B : 65535, z = (a.B + 65534) / 65535;
  const dim3 grid((split ? nwc * nseg : nwc) * ngrp, y, z), block(wpb * kWave);
  hipLaunchKernelGGL(nt ? cross_moment_kernel<true> : cross_moment_kernel<false>, grid, block, 0, stream, a, nwc, L,
                     nseg, split ? 1 : 0, ngrp, wpb);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const int npair = cross_pairs(a.nu);
  const long nbp = (long)a.B * npair;
  hipLaunchKernelGGL(cross_finish_kernel, dim3((unsigned)((nbp + 3) / 4)), dim3(256), 0, stream, a, npair, nwc * nseg);
  return hipGetLastError();
}

}  // namespace mppi
