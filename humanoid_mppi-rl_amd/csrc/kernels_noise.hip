// The configurable sampling law (mppi_set_noise_model): per-actuator scale and AR(1) correlation along the horizon.
// The law itself is noise_model.h; the default law (white noise of one sigma) stays noise_kernel and the fused
// generators of kernels_common.hip / kernels_cartpole.hip.
// Two laws build on it: knots along the horizon (mppi_set_noise_knots; noise_knots.h, noise_knot_kernel) and a full
// covariance across the actuators (mppi_set_noise_cov; noise_cov.h, noise_cov_kernel).
// A third horizon law stands beside AR(1) and the knots: a dense basis (mppi_set_noise_basis; noise_basis.h,
// noise_basis_mfma_kernel on the matrix cores up to H = 128, noise_basis_kernel beyond).
// The AR(1) generators also run under a table of per-step scales (mppi_set_noise_steps; StepLaw,
// noise_ar1_steps_kernel / noise_ar1_lds_steps_kernel).
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>

#include "mppi_internal.h"
#include "noise_adapt.h"
#include "noise_basis.h"
#include "noise_cov.h"
#include "noise_cov_adapt.h"
#include "noise_knots.h"
#include "noise_model.h"
#include "philox.h"

namespace mppi {

// ------------------------------------------------------------------------------------------------
// a1 with the model active: eps[b][u][t][k] = sigma_u[u] * e[t][k], e the AR(1) recursion of noise_model.h over
// the same normals noise_kernel draws (Philox counter (k/4, t, u, b), key = seed + *seed_ctr).
// One thread = 4 consecutive k of one (b, u), walking t = 0..H-1: one 16-B nontemporal store per step into row
// (b*nu + u)*H + t, so a wave's stores stay contiguous in k (1 KiB per wave and step).  The pad lanes K..Kp are
// written like every other lane, as noise_kernel does.
// The draws of different t are independent: a tile of kAr1Tile steps is drawn first (Philox + Box-Muller of the tile
// overlap in the pipeline) and only the one-fma chain e[t] = fma(rho, e[t-1], c z[t]) is serial.
// grid = (k-quad chunks, b*nu folded over y and z): no 64-bit div/mod per element, u and b are uniform per block.
// ------------------------------------------------------------------------------------------------
constexpr int kAr1Tile = 4;

// The law as the generators read it: the by-value kernel argument (NoiseModel), or the device law of a handle that
// adapts it on the stream (mppi_set_noise_adapt; DeviceLaw: sigma_u[kMaxNu], rho, c in device memory, written by
// noise_law_set_kernel / noise_adapt_kernel).  Both forms of a generator share one body: the same operations per
// element in the same order, so equal law values give value-for-value the same noise.
struct DeviceLaw {
  const float* p;
};
__device__ __forceinline__ void law_read(const NoiseModel& m, int u, float& su, float& rho, float& c) {
  su = m.sigma_u[u];
  rho = m.rho;
  c = m.c;
}
__device__ __forceinline__ void law_read(const DeviceLaw& m, int u, float& su, float& rho, float& c) {
  su = m.p[u];
  rho = m.p[kLawRho];
  c = m.p[kLawC];
}
// A third form: the table of per-step scales of mppi_set_noise_steps, S [B][nu][H] in device memory (written by the
// setter and, on a handle that refits it, by step_adapt_kernel: a launch of its own ahead of the generator on the same
// stream, never during it), rho and c by value.  The scale of step t is S[(b*nu + u)*H + t]: b, u and t are uniform per
// block, so it arrives as one scalar load through the constant address space.  For the two laws above law_scale is the
// per-actuator su itself: their instantiations are instruction for instruction what they were.
struct StepLaw {
  const float* S;
  float rho, c;
};
typedef const __attribute__((address_space(4))) float* step_scales;
__device__ __forceinline__ void law_read(const StepLaw& m, int, float& su, float& rho, float& c) {
  su = 0.0f;  // (not read: law_scale)
  rho = m.rho;
  c = m.c;
}
template <class Law>
__device__ __forceinline__ float law_scale(const Law&, float su, int, int, int) {
  return su;
}
__device__ __forceinline__ float law_scale(const StepLaw& m, float, int bu, int H, int t) {
  return ((step_scales)m.S)[(long)bu * H + t];
}

template <class Law>
__device__ __forceinline__ void noise_ar1_body(float* __restrict__ noise, int nbu, int nu, int H, int Kp,
                                               uint64_t seed, const unsigned long long* seed_ctr, const Law& m) {
  const int bu = blockIdx.z * 65535 + blockIdx.y;  // b*nu + u
  const int kq = blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t key = seed + (seed_ctr ? *seed_ctr : 0ull);
  if (bu >= nbu || 4 * kq >= Kp) return;
  const uint32_t k0 = (uint32_t)key, k1 = (uint32_t)(key >> 32);
  const int u = bu % nu;
  const int b = bu / nu;
  float su, rho, c;
  law_read(m, u, su, rho, c);
  typedef float f4 __attribute__((ext_vector_type(4)));
  const int nq = Kp >> 2;
  f4* dst = reinterpret_cast<f4*>(noise + (long)bu * H * Kp) + kq;  // row t: dst + t * nq
  float e[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  for (int t0 = 0; t0 < H; t0 += kAr1Tile) {
    float z[kAr1Tile][4];
#pragma unroll
    for (int j = 0; j < kAr1Tile; ++j)
      if (t0 + j < H) philox_normal4((uint32_t)kq, (uint32_t)(t0 + j), (uint32_t)u, (uint32_t)b, k0, k1, z[j]);
#pragma unroll
    for (int j = 0; j < kAr1Tile; ++j) {
      const int t = t0 + j;
      if (t < H) {
#pragma unroll
        for (int i = 0; i < 4; ++i) e[i] = t == 0 ? z[j][i] : ar1_step(rho, c, e[i], z[j][i]);
        const float st = law_scale(m, su, bu, H, t);
        const f4 v = {st * e[0], st * e[1], st * e[2], st * e[3]};
        __builtin_nontemporal_store(v, dst + (long)t * nq);
      }
    }
  }
}

__global__ __launch_bounds__(256) void noise_ar1_kernel(float* __restrict__ noise, int nbu, int nu, int H, int Kp,
                                                        uint64_t seed, const unsigned long long* seed_ctr,
                                                        NoiseModel m) {
  noise_ar1_body(noise, nbu, nu, H, Kp, seed, seed_ctr, m);
}
__global__ __launch_bounds__(256) void noise_ar1_dev_kernel(float* __restrict__ noise, int nbu, int nu, int H, int Kp,
                                                            uint64_t seed, const unsigned long long* seed_ctr,
                                                            DeviceLaw m) {
  noise_ar1_body(noise, nbu, nu, H, Kp, seed, seed_ctr, m);
}
__global__ __launch_bounds__(256) void noise_ar1_steps_kernel(float* __restrict__ noise, int nbu, int nu, int H, int Kp,
                                                              uint64_t seed, const unsigned long long* seed_ctr,
                                                              StepLaw m) {
  noise_ar1_body(noise, nbu, nu, H, Kp, seed, seed_ctr, m);
}

// ------------------------------------------------------------------------------------------------
// The same values for grids too small to fill the chip (config #2: one (b, u) row of 16 k-quads, where the kernel
// above is 16 lanes drawing H = 100 steps one after the other).  One block = kAr1LdsK = 64 consecutive k of one
// (b, u): its 256 threads first draw all H x 16 (t, k-quad) innovations side by side into LDS ([H][64] floats; row 0
// holds z[0] itself), then the first wave walks t with one lane per k: an LDS read, the fma, a 4-B nontemporal store
// per lane (256 contiguous bytes per wave and step).  Same operations in the same order per element as the kernel
// above, so the two agree bit for bit.  Kp is a multiple of 64 (kKpAlign): every block's 16 quads exist.
// ------------------------------------------------------------------------------------------------
constexpr int kAr1LdsK = 64;
constexpr int kAr1LdsMaxH = 256;  // [H][64] floats <= 64 KiB
static_assert(kKpAlign % kAr1LdsK == 0, "every block of noise_ar1_lds_kernel owns 64 existing k");

template <class Law>
__device__ __forceinline__ void noise_ar1_lds_body(float* inno, float* __restrict__ noise, int nbu, int nu, int H,
                                                   int Kp, uint64_t seed, const unsigned long long* seed_ctr,
                                                   const Law& m) {
  const int bu = blockIdx.z * 65535 + blockIdx.y;  // b*nu + u
  const int k_base = blockIdx.x * kAr1LdsK;
  const uint64_t key = seed + (seed_ctr ? *seed_ctr : 0ull);
  if (bu >= nbu || k_base >= Kp) return;  // (uniform per block: before the barrier)
  const uint32_t k0 = (uint32_t)key, k1 = (uint32_t)(key >> 32);
  const int u = bu % nu;
  const int b = bu / nu;
  float su, rho, c;
  law_read(m, u, su, rho, c);
  typedef float f4 __attribute__((ext_vector_type(4)));
  constexpr int kQ = kAr1LdsK / 4;  // k-quads per block
  for (int i = threadIdx.x; i < H * kQ; i += blockDim.x) {
    const int t = i / kQ, q = i - t * kQ;
    float z[4];
    philox_normal4((uint32_t)(k_base / 4 + q), (uint32_t)t, (uint32_t)u, (uint32_t)b, k0, k1, z);
    f4 v;
    if (t == 0) v = f4{z[0], z[1], z[2], z[3]};
    else v = f4{ar1_innovation(c, z[0]), ar1_innovation(c, z[1]), ar1_innovation(c, z[2]), ar1_innovation(c, z[3])};
    reinterpret_cast<f4*>(inno)[i] = v;  // [t][4 q .. 4 q + 3]
  }
  __syncthreads();
  if (threadIdx.x >= kAr1LdsK) return;
  float* dst = noise + (long)bu * H * Kp + k_base + threadIdx.x;
  float e = 0.0f;
#pragma unroll 4
  for (int t = 0; t < H; ++t) {
    const float v = inno[t * kAr1LdsK + threadIdx.x];
    e = t == 0 ? v : ar1_advance(rho, e, v);
    __builtin_nontemporal_store(law_scale(m, su, bu, H, t) * e, dst + (long)t * Kp);
  }
}

__global__ __launch_bounds__(256) void noise_ar1_lds_kernel(float* __restrict__ noise, int nbu, int nu, int H,
                                                            int Kp, uint64_t seed,
                                                            const unsigned long long* seed_ctr, NoiseModel m) {
  extern __shared__ __attribute__((aligned(16))) float inno[];  // [H][kAr1LdsK]
  noise_ar1_lds_body(inno, noise, nbu, nu, H, Kp, seed, seed_ctr, m);
}
__global__ __launch_bounds__(256) void noise_ar1_lds_dev_kernel(float* __restrict__ noise, int nbu, int nu, int H,
                                                                int Kp, uint64_t seed,
                                                                const unsigned long long* seed_ctr, DeviceLaw m) {
  extern __shared__ __attribute__((aligned(16))) float inno[];  // [H][kAr1LdsK]
  noise_ar1_lds_body(inno, noise, nbu, nu, H, Kp, seed, seed_ctr, m);
}
__global__ __launch_bounds__(256) void noise_ar1_lds_steps_kernel(float* __restrict__ noise, int nbu, int nu, int H,
                                                                  int Kp, uint64_t seed,
                                                                  const unsigned long long* seed_ctr, StepLaw m) {
  extern __shared__ __attribute__((aligned(16))) float inno[];  // [H][kAr1LdsK]
  noise_ar1_lds_body(inno, noise, nbu, nu, H, Kp, seed, seed_ctr, m);
}

// ------------------------------------------------------------------------------------------------
// a1 under a knot law (mppi_set_noise_knots; the rule is noise_knots.h): eps[b][u][t][k] = sigma_u[u] * e[t][k], e the
// interpolation through the table (kidx, kw: [H][4] taps) of the knot row kn[0..P) = AR(1)(rho) over the normals at
// counter (k/4, j, u, b), j the knot index.
// The thread layout of noise_ar1_kernel: one thread = 4 consecutive k of one (b, u), walking t; one 16-B nontemporal
// store per step into row (b*nu + u)*H + t; the pad lanes K..Kp are written like every other lane.
// The taps of a step are four consecutive knots around its segment j (noise_knots.h), and j never falls as t grows, so
// the thread keeps the window W = kn[clamp(jw - 1 .. jw + 2)] of four knot quads in registers and slides it when the
// table's j passes jw: three moves, and one Philox draw + AR(1) advance while a knot jw + 2 <= P - 1 is left -- P
// draws per thread instead of H, no array of P knots.  Which window entries a step's taps are is fixed per order:
// order 3 (W0, W1, W2, W3), order 1 (W1, W2, W1, W1) = (j, j + 1, j, j), order 0 and the one-knot / one-step laws
// (W1, W1, W1, W1) -- the template parameter, so no select sits in the loop.  t, j and jw are the same in every lane
// of a block (no divergence); the table is read through the constant address space (scalar loads), one row ahead.
// What bounds it: the 16 B per thread and step of stores, as for noise_ar1_kernel.
// No LDS form: noise_ar1_lds_kernel exists because one lane draws H normals one after the other on a grid too small
// to fill the chip; here a lane draws P <= H, and the H steps behind them are 4 fma and one store each.
// ------------------------------------------------------------------------------------------------
typedef float knot_f4 __attribute__((ext_vector_type(4)));
typedef int knot_i4 __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(4))) knot_i4* knot_idx_rows;
typedef const __attribute__((address_space(4))) knot_f4* knot_w_rows;

// kOrder: 3, 1, or 0 (order 0, and every law whose table is idx = one knot, w = (1, 0, 0, 0): P == 1 or H == 1)
template <int kOrder>
__global__ __launch_bounds__(256) void noise_knot_kernel(float* __restrict__ noise, int nbu, int nu, int H, int Kp,
                                                         uint64_t seed, const unsigned long long* seed_ctr,
                                                         NoiseModel m) {
  const int bu = blockIdx.z * 65535 + blockIdx.y;  // b*nu + u
  const int kq = blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t key = seed + (seed_ctr ? *seed_ctr : 0ull);
  if (bu >= nbu || 4 * kq >= Kp) return;
  const uint32_t k0 = (uint32_t)key, k1 = (uint32_t)(key >> 32);
  const int u = bu % nu;
  const int b = bu / nu;
  const float su = m.sigma_u[u], rho = m.rho, c = m.c;
  const int last = m.n_knots - 1;
  const knot_idx_rows kidx = (knot_idx_rows)m.kidx;  // the table is written by the setter only, never during a launch
  const knot_w_rows kw = (knot_w_rows)m.kw;
  const int nq = Kp >> 2;
  knot_f4* dst = reinterpret_cast<knot_f4*>(noise + (long)bu * H * Kp) + kq;  // row t: dst + t * nq
  int drawn = 0;  // knots 0..drawn-1 exist; `top` is knot drawn - 1
  knot_f4 top = {0.0f, 0.0f, 0.0f, 0.0f};
  auto draw = [&]() {  // the next knot of the AR(1) row
    float z[4];
    philox_normal4((uint32_t)kq, (uint32_t)drawn, (uint32_t)u, (uint32_t)b, k0, k1, z);
#pragma unroll
    for (int i = 0; i < 4; ++i) top[i] = drawn == 0 ? z[i] : ar1_step(rho, c, top[i], z[i]);
    ++drawn;
  };
  // the window at jw = 0: kn[clamp(-1, 0, 1, 2)]
  draw();
  knot_f4 w0 = top, w1 = top;
  if (last >= 1) draw();
  knot_f4 w2 = top;
  if (last >= 2) draw();
  knot_f4 w3 = top;
  int jw = 0;
  knot_i4 ix = kidx[0];
  knot_f4 wt = kw[0];
  for (int t = 0; t < H; ++t) {
    const int tn = min(t + 1, H - 1);
    const knot_i4 ix_next = kidx[tn];  // one row ahead of its use
    const knot_f4 wt_next = kw[tn];
    const int j = min(kOrder == 3 ? ix.y : ix.x, last);  // (the table's indices are < n_knots: the draws stay P)
    while (jw < j) {  // slide: W <- kn[clamp(jw .. jw + 3)]
      ++jw;
      w0 = w1, w1 = w2, w2 = w3;
      if (jw + 2 <= last) {
        draw();
        w3 = top;
      }
    }
    const float w[4] = {wt.x, wt.y, wt.z, wt.w};
    knot_f4 v;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float e = kOrder == 3   ? knot_interp(w, w0[i], w1[i], w2[i], w3[i])
                      : kOrder == 1 ? knot_interp(w, w1[i], w2[i], w1[i], w1[i])
                                    : knot_interp(w, w1[i], w1[i], w1[i], w1[i]);
      v[i] = su * e;
    }
    __builtin_nontemporal_store(v, dst + (long)t * nq);
    ix = ix_next, wt = wt_next;
  }
}

// ------------------------------------------------------------------------------------------------
// a1 under a cross-actuator covariance (mppi_set_noise_cov; the rule is noise_cov.h): eps[b][u][t][k] =
// sum_{v <= u} L[u][v] e_v[t][k], e_v the unit-variance AR(1) row of actuator v over the normals at counter
// (k/4, t, v, b) -- what noise_ar1_kernel draws for (b, v) before its scale.  One pass over the noise buffer: the
// rows e_v never leave the CU.
// A block owns one b and 64 k-quads (256 k); lane = k-quad, as in noise_ar1_kernel, so every store is the same 16-B
// nontemporal store, 1 KiB contiguous per wave and (u, t).  Its waves are drawers and mixers, one step apart:
//   drawers (nd = min(nu, 8) waves): wave d advances the rows v = d, d + nd, ... (at most kCovRows = 4, unrolled: the
//          chain state stays in registers, no indexed register array) to step s and writes e[v][lane] as 16-B quads
//          into LDS buffer s & 1 (consecutive lanes hold consecutive 16 B: ds_write_b128 / ds_read_b128 without bank
//          conflicts);
//   mixers (nm = min(ceil(nu / 2), 8) waves): in the same pass of the loop a mixer forms, for step s - 1 out of buffer
//          (s - 1) & 1, the output rows of its pairs (2p, 2p + 1), walking v = 0..2p: two rows per LDS read (half the
//          LDS traffic of the triangle), 8 fmaf per read, L through the constant address space (scalar loads: the wave
//          index and p are wave-uniform).  The pairs go to the mixers longest first in serpentine order.
// One barrier per step: behind it the drawers overwrite the buffer the mixers have just left.  The Philox / Box-Muller
// work of step s (VALU) and the LDS and scalar-load latencies of the mix of step s - 1 overlap on every SIMD (a CU
// holds one such block at config #4: 256 blocks), which a block whose waves all draw, then all mix, cannot do.
// LDS: 2 nu KiB (42 KiB at nu = 21, 64 KiB at the limit nu = 32: at least two blocks per CU).  L's rows are padded to
// kMaxNu floats: every row starts 128-B aligned.
// The operations per element are cov_mix's in cov_mix's order: host and device agree bit for bit.
// Lanes past Kp (the last block along k when Kp / 4 is no multiple of 64) draw and store nothing but meet every barrier.
// ------------------------------------------------------------------------------------------------
constexpr int kCovWaves = 8;                  // drawers at most, and mixers at most
constexpr int kCovRows = kMaxNu / kCovWaves;  // AR(1) rows a drawer advances at most
typedef const __attribute__((address_space(4))) float* cov_factor_rows;

__global__ __launch_bounds__(2 * kCovWaves * kWave) void noise_cov_kernel(float* __restrict__ noise, int B, int nu,
                                                                           int H, int Kp, uint64_t seed,
                                                                           const unsigned long long* seed_ctr,
                                                                           NoiseModel m) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  extern __shared__ __attribute__((aligned(16))) float cov_lds[];  // [2][nu][kWave] quads
  const int b = blockIdx.z * 65535 + blockIdx.y;
  if (b >= B) return;  // (uniform per block: before any barrier)
  const int lane = threadIdx.x & (kWave - 1);
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int nd = nu < kCovWaves ? nu : kCovWaves;  // drawers: waves 0..nd-1
  const int nm = blockDim.x / kWave - nd;          // mixers: waves nd..nd+nm-1
  const int kq = blockIdx.x * kWave + lane;
  const bool live = 4 * kq < Kp;
  knot_f4* lds = reinterpret_cast<knot_f4*>(cov_lds) + lane;  // e_v of step s: lds[((s & 1) * nu + v) * kWave]
  if (w < nd) {
    const uint64_t key = seed + (seed_ctr ? *seed_ctr : 0ull);
    const uint32_t k0 = (uint32_t)key, k1 = (uint32_t)(key >> 32);
    const float rho = m.rho, c = m.c;
    knot_f4 e[kCovRows];
#pragma unroll
    for (int r = 0; r < kCovRows; ++r) e[r] = knot_f4{0.0f, 0.0f, 0.0f, 0.0f};
    for (int s = 0; s <= H; ++s) {
      if (live && s < H) {
        knot_f4* buf = lds + (s & 1) * nu * kWave;
#pragma unroll
        for (int r = 0; r < kCovRows; ++r) {
          const int v = w + r * nd;
          if (v < nu) {
            float z[4];
            philox_normal4((uint32_t)kq, (uint32_t)s, (uint32_t)v, (uint32_t)b, k0, k1, z);
#pragma unroll
            for (int i = 0; i < 4; ++i) e[r][i] = s == 0 ? z[i] : ar1_step(rho, c, e[r][i], z[i]);
            buf[v * kWave] = e[r];
          }
        }
      }
      __syncthreads();
    }
    return;
  }
  const int wm = w - nd;
  // [nu][kMaxNu]; written by the setter and, on a handle that adapts its covariance, by noise_cov_adapt_kernel: a launch
  // of its own ahead of this one on the same stream (the generator never runs beside it), so never during this launch
  const cov_factor_rows L = (cov_factor_rows)m.cov_L;
  const int nq = Kp >> 2;
  const long row_q = (long)H * nq;  // quads per (b, u)
  knot_f4* dst = reinterpret_cast<knot_f4*>(noise) + (long)b * nu * row_q + kq;  // (u, t): dst + u * row_q + t * nq
  const int np = (nu + 1) >> 1;     // pairs of output rows
  for (int s = 0; s <= H; ++s) {
    if (live && s > 0) {
      const int t = s - 1;
      const knot_f4* buf = lds + (t & 1) * nu * kWave;
      for (int g = 0; g * nm < np; ++g) {
        const int p = np - 1 - (g * nm + ((g & 1) ? nm - 1 - wm : wm));
        if (p < 0) break;
        const int ua = 2 * p, ub = ua + 1;
        const bool two = ub < nu;
        const cov_factor_rows La = L + ua * kMaxNu, Lb = L + (two ? ub : ua) * kMaxNu;
        knot_f4 ev = buf[0];
        knot_f4 acc_a, acc_b;
        {
          const float la = La[0], lb = Lb[0];
#pragma unroll
          for (int i = 0; i < 4; ++i) acc_a[i] = la * ev[i], acc_b[i] = lb * ev[i];
        }
#pragma unroll 4
        for (int v = 1; v <= ua; ++v) {
          ev = buf[v * kWave];
          const float la = La[v], lb = Lb[v];
#pragma unroll
          for (int i = 0; i < 4; ++i) acc_a[i] = fmaf(la, ev[i], acc_a[i]), acc_b[i] = fmaf(lb, ev[i], acc_b[i]);
        }
        __builtin_nontemporal_store(acc_a, dst + ua * row_q + (long)t * nq);
        if (two) {
          ev = buf[ub * kWave];
          const float lb = Lb[ub];
#pragma unroll
          for (int i = 0; i < 4; ++i) acc_b[i] = fmaf(lb, ev[i], acc_b[i]);
          __builtin_nontemporal_store(acc_b, dst + ub * row_q + (long)t * nq);
        }
      }
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------
// a1 under a horizon basis (mppi_set_noise_basis; the rule is noise_basis.h): eps[b][u][t][k] = sigma_u[u] * e[t][k],
// e[t] = sum_r M[t][r] z[r] as ONE fmaf chain over r ascending, z[r] the white normals at counter (k/4, r, u, b).
// H * R multiply-adds per (b, u, k) behind R draws: the first generator whose arithmetic weighs as much as its stores.
// This is the VALU form: horizons past the MFMA form below (H > 128) run it, and MPPI_NOISE_BASIS=valu forces it (the
// tests run both at every shape; at config #4's shape with R = 64 it takes 1.9x the MFMA form's time).
// A block owns one (b, u) and kb = blockDim.x consecutive k (256, or 128 where R > 64: [R][kb] floats of LDS, 64 KiB at
// most).  Its threads first draw the R x kb / 4 (r, k-quad) normals side by side into LDS (16-B writes, a row of the
// block contiguous); behind one barrier the lane is ONE k and walks the horizon in tiles of kBasisTile = 16 steps: per r
// one 4-B LDS read of z[r][k] (consecutive lanes, consecutive banks) feeds 16 fmaf into 16 accumulators, so the LDS
// moves 1/16 of a float per multiply-add and the chain of every e[t] still runs over r in order.  The 16 coefficients
// M[t0 .. t0 + 15][r] are uniform over the block: the setter stores M transposed ([R][basis_pitch(H)], pad zero) and they
// arrive as one scalar load through the constant address space into SGPRs, which the fmaf reads directly.
// One 4-B nontemporal store per lane and step, as in noise_ar1_lds_kernel: 256 contiguous bytes per wave, 1 KiB per
// block and step.  The pad lanes K..Kp are written like every other lane; waves past Kp (Kp is a multiple of 64: whole
// waves) draw and store nothing but meet the barrier.  Steps H..pitch of the last tile are mixed (zeros) and not stored.
// The operations per element are basis_mix's in basis_mix's order: host and device agree bit for bit.
// ------------------------------------------------------------------------------------------------
typedef float basis_f16 __attribute__((ext_vector_type(16)));
typedef const __attribute__((address_space(4))) basis_f16* basis_rows;
static_assert(sizeof(basis_f16) == kBasisTile * sizeof(float), "one scalar load per tile and r");
constexpr int kBasisWideR = 64;  // up to here a block owns 256 k (R KiB of LDS), beyond 128 k (R / 2 KiB)

__global__ __launch_bounds__(256) void noise_basis_kernel(float* __restrict__ noise, int nbu, int nu, int H, int Kp,
                                                          uint64_t seed, const unsigned long long* seed_ctr,
                                                          NoiseModel m) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  extern __shared__ __attribute__((aligned(16))) float basis_z[];  // [R][kb]
  const int bu = blockIdx.z * 65535 + blockIdx.y;  // b*nu + u
  const int kb = blockDim.x;
  const int k_base = blockIdx.x * kb;
  if (bu >= nbu || k_base >= Kp) return;  // (uniform per block: before the barrier)
  const uint64_t key = seed + (seed_ctr ? *seed_ctr : 0ull);
  const uint32_t k0 = (uint32_t)key, k1 = (uint32_t)(key >> 32);
  const int u = bu % nu;
  const int b = bu / nu;
  const int R = m.n_basis;
  const int nq = kb >> 2;  // k-quads per row of the block
  for (int i = threadIdx.x; i < R * nq; i += kb) {
    const int r = i / nq, q = i - r * nq;
    if (k_base + 4 * q < Kp) {
      float z[4];
      philox_normal4((uint32_t)(k_base / 4 + q), (uint32_t)r, (uint32_t)u, (uint32_t)b, k0, k1, z);
      reinterpret_cast<knot_f4*>(basis_z)[i] = knot_f4{z[0], z[1], z[2], z[3]};  // [r][4 q .. 4 q + 3]
    }
  }
  __syncthreads();
  const int k = k_base + threadIdx.x;
  if (k >= Kp) return;
  const float su = m.sigma_u[u];
  const float* zk = basis_z + threadIdx.x;  // z[r] of this k: zk[r * kb]
  const int tiles = basis_pitch(H) / kBasisTile;
  const basis_rows MT = (basis_rows)m.basis_T;  // the table is written by the setter only, never during a launch
  float* dst = noise + (long)bu * H * Kp + k;   // row t: dst + t * Kp
  for (int tt = 0; tt < tiles; ++tt) {
    float e[kBasisTile];
    {
      const basis_f16 c = MT[tt];
      const float z = zk[0];
#pragma unroll
      for (int i = 0; i < kBasisTile; ++i) e[i] = c[i] * z;
    }
#pragma unroll 4
    for (int r = 1; r < R; ++r) {
      const basis_f16 c = MT[r * tiles + tt];
      const float z = zk[r * kb];
#pragma unroll
      for (int i = 0; i < kBasisTile; ++i) e[i] = fmaf(c[i], z, e[i]);
    }
#pragma unroll
    for (int i = 0; i < kBasisTile; ++i) {
      const int t = tt * kBasisTile + i;
      if (t < H) __builtin_nontemporal_store(su * e[i], dst + (long)t * Kp);
    }
  }
}

// ------------------------------------------------------------------------------------------------
// The same law on the matrix cores, for H <= 16 kNT (noise_basis_mfma_kernel<kNT>): v_mfma_f32_16x16x4_f32 is exact
// fp32 and accumulates its four k in ascending order, one rounding per product -- an fmaf chain -- so with rows = steps,
// columns = samples and the MFMA's k = the basis index r, a chain of R / 4 instructions IS basis_mix's chain.  Two
// details make it so to the bit: the accumulators start at -0.0f (fmaf(a, b, -0) = a * b for every finite a b, signed
// zeros included: the rule's first operation is a product, not an fmaf onto +0), and R is padded to a multiple of 4
// with coefficients -0.0f against normals +0: each pad adds -0, which leaves every value, -0 included, as it is.
// One wave owns 64 consecutive k of one (b, u) and ALL H steps: 4 kNT accumulator quads.  Per group of four r, lane l
// draws ONE Philox quad -- r = r0 + (l >> 4), k-quad (l & 15) -- and its four normals are, as they stand, the B operands
// of four MFMAs whose column j = l & 15 is sample 4 j + c of accumulator set c: no LDS, no transposition, and every
// normal is drawn once.  The A operand of step tile n is M[16 n + (l & 15)][r0 + (l >> 4)], one 4-B load per lane from
// the transposed table (four 64-B rows per wave; the table is 32 KiB at most and stays in cache).  At the end register i
// of the four sets of tile n is steps 16 n + 4 (l >> 4) + i of samples 4 j .. 4 j + 3: one 16-B nontemporal store, 256
// contiguous bytes per row.  No barrier; 4 kNT + ~40 VGPRs.
// ------------------------------------------------------------------------------------------------
constexpr int kBasisMfmaMaxNT = 8;  // H <= 128: beyond, noise_basis_kernel
static_assert(kBasisTile == 16, "a tile of steps is the 16 rows of one MFMA");

template <int kNT>
__global__ __launch_bounds__(256) void noise_basis_mfma_kernel(float* __restrict__ noise, int nbu, int nu, int H, int Kp,
                                                               uint64_t seed, const unsigned long long* seed_ctr,
                                                               NoiseModel m) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const int bu = blockIdx.z * 65535 + blockIdx.y;  // b*nu + u
  const int lane = threadIdx.x & (kWave - 1);
  const int k_base = (blockIdx.x * (blockDim.x / kWave) + threadIdx.x / kWave) * kWave;  // of this wave
  if (bu >= nbu || k_base >= Kp) return;  // (whole waves: Kp is a multiple of 64)
  const uint64_t key = seed + (seed_ctr ? *seed_ctr : 0ull);
  const uint32_t k0 = (uint32_t)key, k1 = (uint32_t)(key >> 32);
  const int u = bu % nu;
  const int b = bu / nu;
  const int R = m.n_basis;
  const int j = lane & 15, rr = lane >> 4;
  const int pitch = basis_pitch(H);
  const float* mt = m.basis_T + j;  // A of (tile n, r): mt[r * pitch + 16 n]; rows R .. round_up(R, 4) hold -0.0f
  knot_f4 acc[kNT][4];
#pragma unroll
  for (int n = 0; n < kNT; ++n)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[n][c] = knot_f4{-0.0f, -0.0f, -0.0f, -0.0f};
  // (The MFMAs of one group and the draw of the next dealt out between them in one basic block measured the same: the
  // f32 MFMA and the VALU do not run side by side on a SIMD)
  for (int r0 = 0; r0 < R; r0 += 4) {
    const int r = r0 + rr;
    float z[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (r < R) philox_normal4((uint32_t)(k_base / 4 + j), (uint32_t)r, (uint32_t)u, (uint32_t)b, k0, k1, z);
    const float* row = mt + (long)r * pitch;
#pragma unroll
    for (int n = 0; n < kNT; ++n) {
      const float a = row[16 * n];
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[n][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, z[c], acc[n][c], 0, 0, 0);
    }
  }
  const float su = m.sigma_u[u];
  float* dst = noise + (long)bu * H * Kp + k_base + 4 * j;  // row t: dst + t * Kp
#pragma unroll
  for (int n = 0; n < kNT; ++n)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int t = 16 * n + 4 * rr + i;
      if (t < H) {
        const knot_f4 v = {su * acc[n][0][i], su * acc[n][1][i], su * acc[n][2][i], su * acc[n][3][i]};
        __builtin_nontemporal_store(v, reinterpret_cast<knot_f4*>(dst + (long)t * Kp));
      }
    }
}

template <int kNT>
static void launch_basis_mfma(int nt, float* noise, int nbu, int nu, int H, int Kp, uint64_t seed,
                              const unsigned long long* seed_ctr, const NoiseModel& model, hipStream_t stream) {
  if constexpr (kNT > 1) {
    if (nt < kNT) return launch_basis_mfma<kNT - 1>(nt, noise, nbu, nu, H, Kp, seed, seed_ctr, model, stream);
  }
  const int threads = Kp >= 256 ? 256 : Kp;  // (Kp is a multiple of 64)
  const dim3 grid((Kp + threads - 1) / threads, nbu < 65535 ? nbu : 65535, (nbu + 65534) / 65535);
  hipLaunchKernelGGL(noise_basis_mfma_kernel<kNT>, grid, dim3(threads), 0, stream, noise, nbu, nu, H, Kp, seed,
                     seed_ctr, model);
}

// MPPI_NOISE_AR1=direct|lds (read per launch; an A/B and test knob): force one of the two kernels (lds: where its
// LDS row fits, H <= 256); default: noise_ar1_lds_kernel when noise_ar1_kernel would have fewer waves than SIMDs
static int ar1_knob() {
  const char* e = std::getenv("MPPI_NOISE_AR1");
  if (!e) return 0;
  return std::strcmp(e, "direct") == 0 ? 1 : (std::strcmp(e, "lds") == 0 ? 2 : 0);
}

hipError_t launch_noise_model(float* noise, int B, int nu, int H, int Kp, uint64_t seed,
                              const unsigned long long* seed_ctr, float sigma, const NoiseModel& model,
                              hipStream_t stream, const float* d_law, const float* d_steps,
                              unsigned long long* key_out) {
  if (!model.active) return launch_noise(noise, B, nu, H, Kp, seed, seed_ctr, sigma, stream, key_out);
  if (nu > kMaxNu) return hipErrorInvalidValue;  // (mppi_set_noise_model refuses such a handle)
  const int nbu = B * nu, nq = Kp / 4;
  // a table of per-step scales (mppi_set_noise_steps refuses it beside every law below but sigma_u and rho)
  if (d_steps && (d_law || model.n_basis > 0 || model.cov_L || model.n_knots > 0)) return hipErrorInvalidValue;
  if (model.n_basis > 0) {  // a horizon basis (mppi_set_noise_basis refuses it beside every other law but sigma_u)
    if (d_law || model.cov_L || model.n_knots > 0 || !model.basis_T || model.n_basis > H || model.n_basis > kMaxBasis)
      return hipErrorInvalidValue;
    // MPPI_NOISE_BASIS=valu (read per launch; an A/B and test knob) forces noise_basis_kernel where the MFMA form fits
    const char* knob = std::getenv("MPPI_NOISE_BASIS");
    const int nt = basis_pitch(H) / kBasisTile;
    if (nt <= kBasisMfmaMaxNT && !(knob && std::strcmp(knob, "valu") == 0)) {
      launch_basis_mfma<kBasisMfmaMaxNT>(nt, noise, nbu, nu, H, Kp, seed, seed_ctr, model, stream);
      return hipGetLastError();
    }
    const int kb = model.n_basis <= kBasisWideR ? 256 : 128;
    const dim3 grid((Kp + kb - 1) / kb, nbu < 65535 ? nbu : 65535, (nbu + 65534) / 65535);
    hipLaunchKernelGGL(noise_basis_kernel, grid, dim3(kb), (size_t)model.n_basis * kb * sizeof(float), stream, noise,
                       nbu, nu, H, Kp, seed, seed_ctr, model);
    return hipGetLastError();
  }
  if (model.cov_L) {  // a cross-actuator covariance (mppi_set_noise_cov refuses it beside a knot law or an adapted one)
    if (d_law || model.n_knots > 0) return hipErrorInvalidValue;
    const int nd = nu < kCovWaves ? nu : kCovWaves, np = (nu + 1) / 2;  // drawers and mixers (noise_cov_kernel)
    const int nm = np < kCovWaves ? np : kCovWaves;
    const dim3 grid((nq + kWave - 1) / kWave, B < 65535 ? B : 65535, (B + 65534) / 65535);
    hipLaunchKernelGGL(noise_cov_kernel, grid, dim3((nd + nm) * kWave), (size_t)2 * nu * kWave * 4 * sizeof(float),
                       stream, noise, B, nu, H, Kp, seed, seed_ctr, model);
    return hipGetLastError();
  }
  if (model.n_knots > 0) {  // a knot law (mppi_set_noise_knots refuses it on an adapting handle: no device-law form)
    if (d_law || !model.kidx || !model.kw || model.n_knots > H) return hipErrorInvalidValue;
    const int threads = nq >= 256 ? 256 : (nq + kWave - 1) / kWave * kWave;
    const dim3 grid((nq + threads - 1) / threads, nbu < 65535 ? nbu : 65535, (nbu + 65534) / 65535);
    // (one knot or one step: the table is one knot with weight 1 whatever the order)
    const int order = model.n_knots == 1 || H == 1 ? 0 : model.order;
    auto* kernel = order == 3 ? noise_knot_kernel<3> : (order == 1 ? noise_knot_kernel<1> : noise_knot_kernel<0>);
    hipLaunchKernelGGL(kernel, grid, dim3(threads), 0, stream, noise, nbu, nu, H, Kp, seed, seed_ctr, model);
    return hipGetLastError();
  }
  const int knob = ar1_knob();
  const long waves = ((long)nbu * nq + kWave - 1) / kWave;
  const bool lds = H <= kAr1LdsMaxH && (knob == 2 || (knob == 0 && waves < 4L * current_device_cus()));
  if (lds) {
    const dim3 grid(Kp / kAr1LdsK, nbu < 65535 ? nbu : 65535, (nbu + 65534) / 65535);
    if (d_steps)
      hipLaunchKernelGGL(noise_ar1_lds_steps_kernel, grid, dim3(256), (size_t)H * kAr1LdsK * sizeof(float), stream,
                         noise, nbu, nu, H, Kp, seed, seed_ctr, StepLaw{d_steps, model.rho, model.c});
    else if (d_law)
      hipLaunchKernelGGL(noise_ar1_lds_dev_kernel, grid, dim3(256), (size_t)H * kAr1LdsK * sizeof(float), stream,
                         noise, nbu, nu, H, Kp, seed, seed_ctr, DeviceLaw{d_law});
    else
      hipLaunchKernelGGL(noise_ar1_lds_kernel, grid, dim3(256), (size_t)H * kAr1LdsK * sizeof(float), stream, noise,
                         nbu, nu, H, Kp, seed, seed_ctr, model);
    return hipGetLastError();
  }
  const int threads = nq >= 256 ? 256 : (nq + kWave - 1) / kWave * kWave;
  const dim3 grid((nq + threads - 1) / threads, nbu < 65535 ? nbu : 65535, (nbu + 65534) / 65535);
  if (d_steps)
    hipLaunchKernelGGL(noise_ar1_steps_kernel, grid, dim3(threads), 0, stream, noise, nbu, nu, H, Kp, seed, seed_ctr,
                       StepLaw{d_steps, model.rho, model.c});
  else if (d_law)
    hipLaunchKernelGGL(noise_ar1_dev_kernel, grid, dim3(threads), 0, stream, noise, nbu, nu, H, Kp, seed, seed_ctr,
                       DeviceLaw{d_law});
  else
    hipLaunchKernelGGL(noise_ar1_kernel, grid, dim3(threads), 0, stream, noise, nbu, nu, H, Kp, seed, seed_ctr, model);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// The device law (mppi_set_noise_adapt): [kLawFloats] = sigma_u[kMaxNu], rho, c.
// noise_law_set_kernel: the by-value model into the device law, on the stream (no host buffer to keep alive).
// noise_adapt_kernel: one wave behind a solve's statistics.  It records the law the solve drew its noise from into
// hist[0..nu] (sigma_u, then rho) and moves the law by the rule of noise_adapt.h from slot-local statistics
// (st [B], m2 / m11 [B][nu]).  Lane u owns actuator u (the batch mean of its m2, its sigma), lane 32 + u adds the
// batch mean of its m11 beside it; lane 0 then adds the means in ascending u and updates rho and c: a fixed order,
// bitwise repeatable.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void noise_law_set_kernel(float* __restrict__ law, NoiseModel m) {
  const int i = threadIdx.x;
  if (i < kMaxNu) law[i] = m.sigma_u[i];
  if (i == kLawRho) law[i] = m.rho;
  if (i == kLawC) law[i] = m.c;
}

__global__ __launch_bounds__(64) void noise_adapt_kernel(float* __restrict__ law, float* __restrict__ hist,
                                                         const mppi_solve_stats* __restrict__ st,
                                                         const float* __restrict__ m2, const float* __restrict__ m11,
                                                         int B, int nu, NoiseAdapt a) {
  static_assert(kWave == 2 * kMaxNu, "one half of the wave per moment");
  __shared__ float s_bar[2][kMaxNu];  // [0]: the batch means of m2, [1]: of m11
  const int lane = threadIdx.x;
  const int u = lane & (kMaxNu - 1), half = lane / kMaxNu;  // lane u and lane kMaxNu + u work for actuator u
  const float rho = law[kLawRho];
  float s = 0.0f;
  if (lane < nu) {
    s = law[lane];
    hist[lane] = s;
  }
  if (lane == 0) hist[nu] = rho;
  int dead = 0;  // a solve without a finite cost: the law stays
  for (int b = lane; b < B; b += kWave) dead |= st[b].n_finite == 0;
  if (__any(dead)) return;  // (uniform over the wave)
  if (u < nu) s_bar[half][u] = na_mean(half ? m11 : m2, B, nu, u);  // the two means side by side
  __syncthreads();
  if (lane < nu) law[lane] = na_sigma(a, s, s_bar[0][lane]);
  if (lane == 0) {
    const float den = na_sum(s_bar[0], nu, 1);
    const float num = na_sum(s_bar[1], nu, 1);
    const float r = na_rho(a, rho, num, den);
    law[kLawRho] = r;
    law[kLawC] = ar1_innovation_scale(r);
  }
}

// ------------------------------------------------------------------------------------------------
// The adapted covariance (mppi_set_noise_cov_adapt; the rule: noise_cov_adapt.h).  One block behind a solve's cross
// moments.  It records the Sigma the solve drew its noise from into hist [nu][nu], then all of its threads form the
// batch means of the cross moments and the blended S1 (one pair (u, v <= u) per thread and trip: the reads of a pair's
// B moments are na_sum's, sixteen ahead of the ordered additions), and ONE wave runs the rest with lane u owning row
// u: the clamp, cov_factor's chains column by column (the pivot travels by a shuffle, every lane takes its root),
// Ld^-1 one column per lane, Sigma^-1 one row per lane -- each element by the header's function, so the result is the
// host's bit for bit.  Nothing is written until the step is known to stand; a rejected step counts one in *rejects.
// The other waves leave behind the one block barrier; the wave's own exchanges through LDS are ordered by wave_lds_sync.
// Ordinary stores: L, Sinv and Sigma are visible to the next launch on the stream.
// ------------------------------------------------------------------------------------------------
constexpr int kCovAdaptThreads = 256;

__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ __launch_bounds__(kCovAdaptThreads) void noise_cov_adapt_kernel(CovLaw law, float* __restrict__ hist,
                                                                           const mppi_solve_stats* __restrict__ st,
                                                                           const float* __restrict__ mx, int B, int nu,
                                                                           NoiseCovAdapt a) {
  __shared__ float s_s[kMaxNu][kMaxNu + 1];   // S1, then S2 in place (the lower triangle)
  __shared__ float s_si[kMaxNu][kMaxNu + 1];  // Sigma^-1 in fp32 (the lower triangle)
  __shared__ float s_g[kMaxNu];
  __shared__ double s_L[kMaxNu * kMaxNu], s_W[kMaxNu * kMaxNu];  // Ld, Wd = Ld^-1 (row pitch kMaxNu)
  const int tid = threadIdx.x, lane = tid & (kWave - 1);
  const int nn = nu * nu;
  for (int i = tid; i < nn; i += kCovAdaptThreads) hist[i] = law.S[i];
  int dead = 0;  // a solve without a finite cost: the law stays (every wave looks at every solve: uniform over the block)
  for (int b = lane; b < B; b += kWave) dead |= st[b].n_finite == 0;
  if (__any(dead)) return;
  for (int p = tid; p < nu * (nu + 1) / 2; p += kCovAdaptThreads) {
    int u = 0;
    while ((u + 1) * (u + 2) / 2 <= p) ++u;
    const int v = p - u * (u + 1) / 2;
    s_s[u][v] = nca_blend(a, law.S[u * nu + v], nca_mean(mx, B, nn, u * nu + v));
  }
  __syncthreads();
  if (tid >= kWave) return;
  auto reject = [&]() {
    if (lane == 0) *law.rejects = *law.rejects + 1ull;
  };
  const bool on = lane < nu;
  float s = 1.0f, c = 1.0f, g = 1.0f;
  bool ok = true;
  if (on) {
    s = sqrtf(s_s[lane][lane]);
    ok = nca_scale_ok(s);
    c = nca_clamp(a, s);
    g = nca_gain(c, s);
    s_g[lane] = g;
  }
  if (__any(!ok)) return reject();
  wave_lds_sync();
  if (on) {
    for (int v = 0; v < lane; ++v) s_s[lane][v] = nca_offdiag(s_s[lane][v], g, s_g[v]);
    s_s[lane][lane] = nca_diag(s_s[lane][lane], s, c);
  }
  for (int v = 0; v < nu; ++v) {
    double x = 0.0;
    if (on && lane >= v) x = nca_chol_chain(s_L + lane * kMaxNu, s_L + v * kMaxNu, v, s_s[lane][v]);
    const double piv = __shfl(x, v);
    if (!nca_pivot_ok(piv)) return reject();  // (uniform over the wave)
    const double d = sqrt(piv);
    if (on && lane >= v) s_L[lane * kMaxNu + v] = lane == v ? d : x / d;
    wave_lds_sync();
  }
  if (on)
    for (int r = lane; r < nu; ++r) s_W[r * kMaxNu + lane] = nca_winv_elem(s_L, s_W, kMaxNu, r, lane);
  wave_lds_sync();
  bool bad = false;
  if (on)
    for (int v = 0; v <= lane; ++v) {
      const double x = nca_sinv_elem(s_W, kMaxNu, nu, lane, v);
      bad |= !nca_sinv_ok(x);
      s_si[lane][v] = (float)x;
    }
  if (__any(bad)) return reject();
  wave_lds_sync();
  if (on) {
    for (int v = 0; v < nu; ++v) {
      const bool lo = v <= lane;
      law.S[lane * nu + v] = lo ? s_s[lane][v] : s_s[v][lane];
      law.L[lane * kMaxNu + v] = lo ? (float)s_L[lane * kMaxNu + v] : 0.0f;
      law.Sinv[lane * nu + v] = lo ? s_si[lane][v] : s_si[v][lane];
    }
    law.sigma_u[lane] = nca_sigma(s_s[lane][lane]);
  }
}

hipError_t launch_noise_cov_adapt(const CovLaw& law, float* hist, const mppi_solve_stats* stats, const float* mx,
                                  int B, int nu, const NoiseCovAdapt& a, hipStream_t stream) {
  if (nu > kMaxNu) return hipErrorInvalidValue;  // (mppi_set_noise_cov refuses such a handle)
  hipLaunchKernelGGL(noise_cov_adapt_kernel, dim3(1), dim3(kCovAdaptThreads), 0, stream, law, hist, stats, mx, B, nu, a);
  return hipGetLastError();
}

hipError_t launch_noise_law_set(float* d_law, const NoiseModel& model, hipStream_t stream) {
  hipLaunchKernelGGL(noise_law_set_kernel, dim3(1), dim3(kWave), 0, stream, d_law, model);
  return hipGetLastError();
}

hipError_t launch_noise_adapt(float* d_law, float* hist, const mppi_solve_stats* stats, const float* m2,
                              const float* m11, int B, int nu, const NoiseAdapt& a, hipStream_t stream) {
  if (nu > kMaxNu) return hipErrorInvalidValue;  // (mppi_set_noise_adapt refuses such a handle)
  hipLaunchKernelGGL(noise_adapt_kernel, dim3(1), dim3(kWave), 0, stream, d_law, hist, stats, m2, m11, B, nu, a);
  return hipGetLastError();
}

}  // namespace mppi
