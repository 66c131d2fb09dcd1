// Solve diagnostics (MPPI_FLAG_STATS, mppi_stats_eval; include/mppi.h states the definitions): the softmin statistics
// of a solve's K costs and the weighted second moments of the noise it used.  Three launches on the solve's stream,
// behind the reduce: stats_cost_kernel (the struct and the normalised weights), stats_moment_kernel (the noise stream,
// the hot part) and stats_finish_kernel (the fixed-order sum of its partials).  Read-only on everything a solve owns.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdlib>
#include <cstring>

#include "cross_moments.h"
#include "mppi_internal.h"
#include "wave_reduce.h"

namespace mppi {

// ------------------------------------------------------------------------------------------------
// Cost part: one block of 256 threads per solve over its K costs (<= 128 KiB, L2-resident behind the rollout), 16-B
// loads.  Three passes:
// (1) beta, max, mean, |F|; (2) the softmin sums with reduce_kernel's own weight expression; (3) the normalised
// weights w_k = wt_k / (S + norm_eps) into the [B][Kp] scratch the moment part reads (pads K..Kp: 0).  The sums run in
// fp64 (one block per solve: nothing to save), combined in a fixed order; the handful of final expressions too, so
// uniform weights give ess == n and entropy == ln n to the last bit of fp32.
// ------------------------------------------------------------------------------------------------
enum StatsOp { kOpSum, kOpMin, kOpMax };

template <StatsOp OP>
__device__ __forceinline__ double stats_combine(double a, double b) {
  if constexpr (OP == kOpSum) return a + b;
  if constexpr (OP == kOpMin) return a < b ? a : b;
  return a > b ? a : b;
}

__device__ __forceinline__ double stats_combine(int op, double a, double b) {
  return op == kOpSum ? stats_combine<kOpSum>(a, b) : (op == kOpMin ? stats_combine<kOpMin>(a, b)
                                                                      : stats_combine<kOpMax>(a, b));
}

// N values at once, v[i] combined with ops[i]; every thread gets the block's results.  red: [waves][N] doubles of LDS;
// one barrier pair for the lot
template <int N>
__device__ __forceinline__ void stats_block(double (&v)[N], const int (&ops)[N], double* red) {
#pragma unroll
  for (int i = 0; i < N; ++i) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[i] = stats_combine(ops[i], v[i], __shfl_xor(v[i], o));
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int i = 0; i < N; ++i) red[(threadIdx.x >> 6) * N + i] = v[i];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < N; ++i) {
    double r = red[i];
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w) r = stats_combine(ops[i], r, red[w * N + i]);  // fixed order
    v[i] = r;
  }
  __syncthreads();
}

constexpr int kStatsCostThreads = 256;  // (4 waves: the ten block-wide fp64 reductions cost more than the passes)
constexpr int kStatsCostPre = 4;        // quads per thread held in registers: K <= 4096 is read exactly once

__global__ __launch_bounds__(kStatsCostThreads) void stats_cost_kernel(StatsArgs a) {
  __shared__ double red[(kStatsCostThreads / 64) * 6];
  typedef float c4 __attribute__((ext_vector_type(4)));
  const int b = blockIdx.x, tid = threadIdx.x;
  constexpr int nt = kStatsCostThreads;
  const int nq = a.Kp >> 2;  // (Kp is a multiple of 64: whole, 16-B aligned quads)
  const c4* c = reinterpret_cast<const c4*>(a.costs + (long)b * a.Kp);
  // each thread owns the quads tid, tid + nt, ...; the first kStatsCostPre of them are loaded side by side and stay in
  // registers for all three passes, so up to K = 4096 no pass waits on a chain of dependent loop trips
  static_assert(kStatsCostPre == 4, "the register-held quads are spelled out below");
  const c4 p0 = c[min(tid, nq - 1)], p1 = c[min(tid + nt, nq - 1)], p2 = c[min(tid + 2 * nt, nq - 1)],
           p3 = c[min(tid + 3 * nt, nq - 1)];
  auto ldq = [&](int q) {
    const int j = (q - tid) / nt;
    return j == 0 ? p0 : (j == 1 ? p1 : (j == 2 ? p2 : (j == 3 ? p3 : c[q])));
  };
  auto quad = [&](int q, auto&& fn) {  // fn(k, c_k) for the k < K of quad q
    const c4 v = ldq(q);
    if (4 * q + 0 < a.K) fn(4 * q + 0, v.x);
    if (4 * q + 1 < a.K) fn(4 * q + 1, v.y);
    if (4 * q + 2 < a.K) fn(4 * q + 2, v.z);
    if (4 * q + 3 < a.K) fn(4 * q + 3, v.w);
  };
  auto each = [&](auto&& fn) {
    for (int q = tid; q < nq; q += nt) quad(q, fn);
  };
  double mn = INFINITY, mx = -INFINITY, sum = 0.0, cnt = 0.0;
  each([&](int, float ck) {
    if (isfinite(ck)) {
      mn = fmin(mn, (double)ck);
      mx = fmax(mx, (double)ck);
      sum += (double)ck;
      cnt += 1.0;
    }
  });
  {
    double v[4] = {mn, mx, sum, cnt};
    stats_block<4>(v, {kOpMin, kOpMax, kOpSum, kOpSum}, red);
    mn = v[0], mx = v[1], sum = v[2], cnt = v[3];
  }
  const int n = (int)cnt;
  const float beta = (float)mn;  // (exact: the minimum of floats)
  const double mean = n > 0 ? sum / cnt : (double)INFINITY;
  const float lambda = a.lambda_dev ? a.lambda_dev[b] : a.lambda;  // (ESS targeting: the solve's own)
  const float inv_lam = 1.0f / lambda;
  double S = 0.0, S2 = 0.0, SC = 0.0, SX = 0.0, V = 0.0, kb = (double)INT_MAX;
  each([&](int k, float ck) {
    if (isfinite(ck)) {  // (n > 0 here, so beta is finite)
      const float x = inv_lam * (ck - beta);
      const double wt = (double)__expf(-inv_lam * (ck - beta));  // reduce_kernel's expression
      S += wt;
      S2 += wt * wt;
      SC += wt * (double)ck;
      SX += wt * (double)x;  // -wt ln wt
      const double d = (double)ck - mean;
      V += d * d;
      if (ck == beta) kb = fmin(kb, (double)k);
    }
  });
  {
    double v[6] = {S, S2, SC, SX, V, kb};
    stats_block<6>(v, {kOpSum, kOpSum, kOpSum, kOpSum, kOpSum, kOpMin}, red);
    S = v[0], S2 = v[1], SC = v[2], SX = v[3], V = v[4], kb = v[5];
  }
  const float inv_S = 1.0f / ((float)S + a.norm_eps);
  for (int q = tid; q < nq; q += nt) {
    const c4 v = ldq(q);
    auto wk = [&](int i, float ck) {  // (pads K..Kp and non-finite costs: 0)
      return (4 * q + i < a.K && n > 0 && isfinite(ck)) ? __expf(-inv_lam * (ck - beta)) * inv_S : 0.0f;
    };
    reinterpret_cast<c4*>(a.w + (long)b * a.Kp)[q] = c4{wk(0, v.x), wk(1, v.y), wk(2, v.z), wk(3, v.w)};
  }
  if (tid == 0) {
    mppi_solve_stats st;
    if (n > 0) {
      st.cost_min = beta;
      st.cost_max = (float)mx;
      st.cost_mean = (float)mean;
      st.cost_std = (float)sqrt(V / cnt);
      st.cost_weighted = (float)(SC * (double)inv_S);
      st.ess = (float)(S * S / S2);
      st.entropy = (float)fmax(log(S) + SX / S, 0.0);
      st.free_energy = (float)((double)beta - (double)lambda * log(S / cnt));
      st.n_finite = n;
      st.k_best = (int)kb;
    } else {
      st.cost_min = st.cost_max = st.cost_mean = st.free_energy = INFINITY;
      st.cost_std = st.cost_weighted = st.ess = st.entropy = 0.0f;
      st.n_finite = 0;
      st.k_best = -1;
    }
    a.stats[b] = st;
  }
}

// ------------------------------------------------------------------------------------------------
// Moment part: every noise element read once (config #4: 352 MB, reduce_kernel's stream).
//   eps_m2 [b][u] = 1/H     sum_t      sum_k w_k eps[t][k]^2
//   eps_m11[b][u] = 1/(H-1) sum_{t>=1} sum_k w_k eps[t][k] eps[t-1][k]
// The work of one (b, u) row is cut into cells: a WAVE-CHUNK of 256 consecutive k (each lane owns one k-quad: its four
// weights sit in registers for the whole walk) times a horizon SEGMENT of L = ceil(H / 16) steps.  A cell's two sums are
// accumulated by its lanes in t order (fp32 fma chains), wave-reduced, and stored as one partial; stats_finish_kernel
// adds the partials of a row in an order fixed by the cell indices.  The value therefore does not depend on which wave ran which
// cell, and the two forms below agree bit for bit:
//   direct  one wave walks all segments of its chunk, the previous row's quad kept in registers for the lag product;
//           4 waves (1024 k) per block.  16-B loads, kStatsTile rows per tile, the next tile issued before the current
//           one is consumed (2 x 8 loads per lane in flight); nontemporal above launch_reduce's 128 MB cut.
//   seg     one wave per segment, 16 waves per block, each reading its predecessor's last row once more: for grids
//           with fewer blocks than CUs, where one lane walking H rows serially is latency-bound (config #2: one row,
//           Kp = 64, H = 100; the 8-solve shard of config #4: 168 rows).
// No barrier, no atomics, no LDS; inactive lanes (quads beyond Kp) carry weight 0 and read a clamped, in-bounds quad.
// ------------------------------------------------------------------------------------------------
constexpr int kStatsSegs = 16;   // horizon segments per row (at most)
constexpr int kStatsTile = 8;    // rows per load tile
typedef float f4 __attribute__((ext_vector_type(4)));

template <bool NT>
__device__ __forceinline__ f4 stats_ld(const f4* p) {
  if constexpr (NT) return __builtin_nontemporal_load(p);
  else return *p;
}

// one row of one lane: explicit fma chains (no mul + add pair the compiler could contract differently per call site)
__device__ __forceinline__ void stats_row(const f4& w, const f4& e, const f4& p, bool lag, float& m2, float& m11) {
  const float w0 = w.x * e.x, w1 = w.y * e.y, w2 = w.z * e.z, w3 = w.w * e.w;
  m2 = fmaf(w0, e.x, m2);
  m2 = fmaf(w1, e.y, m2);
  m2 = fmaf(w2, e.z, m2);
  m2 = fmaf(w3, e.w, m2);
  if (lag) {
    m11 = fmaf(w0, p.x, m11);
    m11 = fmaf(w1, p.y, m11);
    m11 = fmaf(w2, p.z, m11);
    m11 = fmaf(w3, p.w, m11);
  }
}

template <bool NT>
__global__ __launch_bounds__(1024) void stats_moment_kernel(StatsArgs a, int nbu, int nwc, int L, int nseg,
                                                            int split) {
  const int bu = blockIdx.z * 65535 + blockIdx.y;  // b*nu + u
  const int lane = threadIdx.x & 63;
  const int gw = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  // direct: wave = chunk, all segments; seg: wave = (chunk, segment)
  const int wc = split ? gw / nseg : gw;
  const int s_begin = split ? gw - wc * nseg : 0, s_end = split ? s_begin + 1 : nseg;
  if (bu >= nbu || wc >= nwc) return;  // (uniform per wave; the kernel has no barrier)
  const int b = bu / a.nu;
  const int nq = a.Kp >> 2;
  const int q = wc * 64 + lane;
  const bool act = q < nq;
  const int qc = act ? q : nq - 1;
  f4 w = reinterpret_cast<const f4*>(a.w + (long)b * a.Kp)[qc];
  if (!act) w = f4{0.0f, 0.0f, 0.0f, 0.0f};
  const f4* src = reinterpret_cast<const f4*>(a.noise + (long)bu * a.H * a.Kp) + qc;  // row t: src + t * nq
  float* part = a.part + ((long)bu * nwc + wc) * nseg * 2;
  const int t_begin = s_begin * L, t_end = min(a.H, s_end * L);
  f4 cur[kStatsTile], nxt[kStatsTile];
  auto load = [&](f4* dst, int t0) {
#pragma unroll
    for (int j = 0; j < kStatsTile; ++j) dst[j] = stats_ld<NT>(src + (long)min(t0 + j, t_end - 1) * nq);
  };
  load(cur, t_begin);
  f4 prev = f4{0.0f, 0.0f, 0.0f, 0.0f};
  if (t_begin > 0) prev = stats_ld<NT>(src + (long)(t_begin - 1) * nq);
  float m2 = 0.0f, m11 = 0.0f;
  int seg = s_begin, seg_end = t_begin + L;
  auto flush = [&]() {
    const float s2 = wave_sum(m2), s11 = wave_sum(m11);
    if (lane == 0) {
      part[2 * seg] = s2;
      part[2 * seg + 1] = s11;
    }
  };
  for (int t0 = t_begin; t0 < t_end; t0 += kStatsTile) {
    if (t0 + kStatsTile < t_end) load(nxt, t0 + kStatsTile);
#pragma unroll
    for (int j = 0; j < kStatsTile; ++j) {
      const int t = t0 + j;
      if (t < t_end) {
        if (t == seg_end) {  // (direct form: the next segment's cell starts)
          flush();
          seg += 1;
          seg_end += L;
          m2 = 0.0f;
          m11 = 0.0f;
        }
        stats_row(w, cur[j], prev, t > 0, m2, m11);
        prev = cur[j];
      }
    }
    if (t0 + kStatsTile < t_end) {
#pragma unroll
      for (int j = 0; j < kStatsTile; ++j) cur[j] = nxt[j];
    }
  }
  flush();
}

// one wave per (b, u) row: lane l adds its cells l, l + 64, ... ((chunk, segment) order, one coalesced 8-B load each),
// then the wave's fixed butterfly: an order that depends on nothing but the cell index
__global__ __launch_bounds__(256) void stats_finish_kernel(StatsArgs a, int nbu, int ncell) {
  const int bu = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (bu >= nbu) return;  // (uniform per wave; no barrier)
  const float2* part = reinterpret_cast<const float2*>(a.part) + (long)bu * ncell;
  float s2 = 0.0f, s11 = 0.0f;
  for (int i = lane; i < ncell; i += 64) {
    const float2 p = part[i];
    s2 += p.x;
    s11 += p.y;
  }
  s2 = wave_sum(s2);
  s11 = wave_sum(s11);
  if (lane == 0) {
    a.m2[bu] = s2 / (float)a.H;
    a.m11[bu] = a.H > 1 ? s11 / (float)(a.H - 1) : 0.0f;
  }
}

// the cells of one (b, u) row: wave-chunks x segments (fixed by H and Kp, so by the handle)
// (moment_cells of cross_moments.h: the one statement of the split, shared with the cross moments)
static_assert(kStatsSegs == kMomentSegs && kWave == kMomentLanes, "stats_moment_kernel's cells are moment_cells'");
static void stats_cells(int H, int Kp, int* nwc, int* L, int* nseg) { moment_cells(H, Kp, nwc, L, nseg); }

size_t stats_part_floats(int B, int nu, int H, int Kp) {
  int nwc, L, nseg;
  stats_cells(H, Kp, &nwc, &L, &nseg);
  return (size_t)B * nu * nwc * nseg * 2;
}

// MPPI_STATS_FORM=direct|seg (read per launch; an A/B and test knob): force one form of stats_moment_kernel; default:
// seg when the direct form's grid has fewer blocks than the device has CUs
static int stats_knob() { return env_choice("MPPI_STATS_FORM", "direct", "seg"); }

hipError_t launch_stats(const StatsArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL(stats_cost_kernel, dim3(a.B), dim3(kStatsCostThreads), 0, stream, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || !a.noise) return e;
  int nwc, L, nseg;
  stats_cells(a.H, a.Kp, &nwc, &L, &nseg);
  const int nbu = a.B * a.nu;
  const int knob = stats_knob();
  const bool split = knob == 2 || (knob == 0 && (long)nbu * ((nwc + 3) / 4) < current_device_cus());
  const bool nt = (double)nbu * a.H * a.Kp * 4.0 > 128.0 * 1024 * 1024;  // launch_reduce's cut
  const int y = nbu < 65535 ? nbu : 65535, z = (nbu + 65534) / 65535;
  const dim3 grid(split ? nwc : (nwc + 3) / 4, y, z), block(split ? nseg * kWave : 4 * kWave);
  hipLaunchKernelGGL(nt ? stats_moment_kernel<true> : stats_moment_kernel<false>, grid, block, 0, stream, a, nbu, nwc,
                     L, nseg, split ? 1 : 0);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(stats_finish_kernel, dim3((nbu + 3) / 4), dim3(256), 0, stream, a, nbu, nwc * nseg);
  return hipGetLastError();
}

}  // namespace mppi
