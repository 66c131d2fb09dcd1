// The per-step moments of a solve's noise (MPPI_FLAG_STEP_MOMENTS, mppi_step_moments_eval; the definition and its cell
// scheme: step_moments.h) and the refit of the per-step sampling scale from them (mppi_set_noise_steps_adapt; the rule:
// step_law.h).  step_moment_kernel is one more pass over the noise buffer behind the statistics, whose normalised
// weights it reads; step_adapt_kernel is one small launch behind it.  Read-only on everything a solve owns.
#include <hip/hip_runtime.h>

#include "mppi_internal.h"
#include "step_law.h"
#include "step_moments.h"
#include "wave_reduce.h"

namespace mppi {

// ------------------------------------------------------------------------------------------------
// A row reduction over k, one row per (b, u, t): the shape of reduce_kernel's weighted sum, not of stats_moment_kernel,
// which accumulates along t in the lanes.  The rows of one solve are contiguous ([nu H][Kp]); a WAVE owns a tile of
// kStepRows = 8 consecutive rows and walks their wave-chunks: per chunk the lane's weight quad and eight 16-B loads (one
// per row, 1 KiB contiguous per wave and row; the next chunk's issued before this one's are consumed), the sixteen lane
// values of step_lane (m1 and m2 of the eight rows), and ONE butterfly over all sixteen -- every step exchanges half of
// the values still held, then the last two offsets are plain sums: 8 + 4 + 2 + 1 + 2 = 17 exchanges per chunk instead of
// 96, the last two DPP quad permutes.  Lanes 4 s .. 4 s + 3 end with slot s, the bits of wave_sum of it, and add it to
// their running total in chunk order.  No barrier, no atomics, no LDS; inactive lanes (quads beyond Kp) carry weight 0
// and read a clamped, in-bounds quad; rows beyond the solve's last are clamped to it and their sums dropped.
// Loads are nontemporal above launch_reduce's 128 MB cut, as the other passes' are.
// What bounds it: the bytes of the noise buffer, read once.
// ------------------------------------------------------------------------------------------------
constexpr int kStepRows = 8;
typedef float s4 __attribute__((ext_vector_type(4)));

template <bool NT>
__device__ __forceinline__ s4 step_ld(const s4* p) {
  if constexpr (NT) return __builtin_nontemporal_load(p);
  else return *p;
}

// the offsets O, O / 2, ..., 1 of the butterfly on one value
template <int O>
__device__ __forceinline__ float step_wave_tail(float r) {
  if constexpr (O >= 1) {
    r = r + lane_xor<O>(r);
    return step_wave_tail<O / 2>(r);
  } else {
    return r;
  }
}

// N sums over the wave at once (N a power of two <= 64): every lane returns the wave_sum of one v[s], bit for bit -- at
// offset O the lane whose bit O is clear keeps the lower half of the values and sends the upper, its partner the reverse
// (the addition commutes, so both orders of a pair give wave_sum's bits).  Lane l ends with slot (l * N) >> 6; v is
// consumed
template <int N, int O = 32>
__device__ __forceinline__ float step_wave_sums(float (&v)[N], int lane) {
  if constexpr (N > 1) {
    const bool up = (lane & O) != 0;
    float h[N / 2];
#pragma unroll
    for (int i = 0; i < N / 2; ++i) {
      const float keep = up ? v[N / 2 + i] : v[i];
      const float send = up ? v[i] : v[N / 2 + i];
      h[i] = keep + lane_xor<O>(send);
    }
    return step_wave_sums<N / 2, O / 2>(h, lane);
  } else {
    return step_wave_tail<O>(v[0]);
  }
}

template <bool NT>
__global__ __launch_bounds__(256) void step_moment_kernel(StepMomArgs a, int ntile, int nwc) {
  const int b = blockIdx.z * 65535 + blockIdx.y;
  const int lane = threadIdx.x & 63;
  const int tile = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= a.B || tile >= ntile) return;  // (uniform per wave; the kernel has no barrier)
  const int nrow = a.nu * a.H;            // rows of one solve
  const int nq = a.Kp >> 2;
  const int r0 = tile * kStepRows;
  const s4* wq = reinterpret_cast<const s4*>(a.w + (long)b * a.Kp);
  const s4* src = reinterpret_cast<const s4*>(a.noise + (long)b * nrow * a.Kp);
  long ro[kStepRows];  // (wave-uniform: scalar registers)
#pragma unroll
  for (int i = 0; i < kStepRows; ++i) ro[i] = (long)min(r0 + i, nrow - 1) * nq;
  s4 wc_cur, wc_nxt, cur[kStepRows], nxt[kStepRows];
  auto load = [&](s4& wd, s4* ed, int wc) {
    const int q = wc * kStepLanes + lane;
    const bool act = q < nq;
    const int qc = act ? q : nq - 1;
    wd = wq[qc];
    if (!act) wd = s4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int i = 0; i < kStepRows; ++i) ed[i] = step_ld<NT>(src + ro[i] + qc);
  };
  load(wc_cur, cur, 0);
  float total = 0.0f;  // of this lane's slot
  for (int wc = 0; wc < nwc; ++wc) {
    if (wc + 1 < nwc) load(wc_nxt, nxt, wc + 1);
    float v[2 * kStepRows];  // m1 of the eight rows, then m2
    const float w[4] = {wc_cur.x, wc_cur.y, wc_cur.z, wc_cur.w};
#pragma unroll
    for (int i = 0; i < kStepRows; ++i) {
      const float e[4] = {cur[i].x, cur[i].y, cur[i].z, cur[i].w};
      step_lane(w, e, &v[i], &v[kStepRows + i]);
    }
    const float s = step_wave_sums<2 * kStepRows>(v, lane);
    total = total + s;
    if (wc + 1 < nwc) {
      wc_cur = wc_nxt;
#pragma unroll
      for (int i = 0; i < kStepRows; ++i) cur[i] = nxt[i];
    }
  }
  static_assert(kWave / (2 * kStepRows) == 4, "lanes 4 s .. 4 s + 3 hold slot s");
  const int slot = lane >> 2, row = r0 + (slot & (kStepRows - 1));
  if ((lane & 3) == 0 && row < nrow) (slot < kStepRows ? a.m1 : a.m2)[(long)b * nrow + row] = total;
}

hipError_t launch_step_moments(const StepMomArgs& a, hipStream_t stream) {
  if (a.B < 1 || a.nu < 1 || a.H < 1 || a.Kp < 4) return hipErrorInvalidValue;
  const int nrow = a.nu * a.H, ntile = (nrow + kStepRows - 1) / kStepRows, nwc = step_chunks(a.Kp);
  const bool nt = (double)a.B * nrow * a.Kp * 4.0 > 128.0 * 1024 * 1024;  // launch_reduce's cut
  const dim3 grid((ntile + 3) / 4, a.B < 65535 ? a.B : 65535, (a.B + 65534) / 65535);
  hipLaunchKernelGGL(nt ? step_moment_kernel<true> : step_moment_kernel<false>, grid, dim3(256), 0, stream, a, ntile,
                     nwc);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// The refit (step_law.h): one wave per (b, u) row of the table, 64 cells per trip in ascending t.  Cell t of the new row
// reads cell t (or, with the shift, t + 1) of the old one, which another lane of the same wave overwrites: every lane's
// reads of a trip are one load instruction each, complete before the trip's one store instruction issues (the stored
// value depends on them), and a later trip reads only cells no earlier trip wrote -- no cell is read after it was
// overwritten.  Slots >= B of the table are not touched.  The fill travels by value (sigma_u of the handle's model).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void step_adapt_kernel(float* __restrict__ S, const float* __restrict__ m1,
                                                         const float* __restrict__ m2,
                                                         const mppi_solve_stats* __restrict__ st, int nbu, int nu, int H,
                                                         int shift, StepAdapt a, StepFill f) {
  const int bu = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (bu >= nbu) return;  // (uniform per wave; no barrier)
  const int b = bu / nu, u = bu - b * nu;
  const bool live = st[b].n_finite != 0;
  const float fill = f.sigma_u[u];
  float* row = S + (long)bu * H;
  const float* r1 = m1 + (long)bu * H;
  const float* r2 = m2 + (long)bu * H;
  for (int t0 = 0; t0 < H; t0 += kWave) {
    const int t = t0 + lane;
    float v = 0.0f;
    if (t < H) v = sl_cell(a, row, r1, r2, H, t, shift != 0, fill, live);
    __builtin_amdgcn_wave_barrier();  // (the trip's reads above, its stores below)
    if (t < H) row[t] = v;
  }
}

hipError_t launch_step_adapt(float* S, const float* m1, const float* m2, const mppi_solve_stats* stats, int B, int nu,
                             int H, int shift, const StepAdapt& a, const StepFill& fill, hipStream_t stream) {
  if (nu > kMaxNu) return hipErrorInvalidValue;  // (mppi_set_noise_steps refuses such a handle)
  const int nbu = B * nu;
  hipLaunchKernelGGL(step_adapt_kernel, dim3((nbu + 3) / 4), dim3(256), 0, stream, S, m1, m2, stats, nbu, nu, H, shift,
                     a, fill);
  return hipGetLastError();
}

}  // namespace mppi
