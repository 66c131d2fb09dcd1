// Weighted cross moments of the noise a solve used (MPPI_FLAG_CROSS, mppi_cross_moments_eval):
//   eps_mx[b][u][v] = 1/H  sum_t sum_k  w_k  eps[b][u][t][k]  eps[b][v][t][k]        0 <= v <= u < nu, mirrored to v > u
// with w the normalised softmin weights [B][Kp] (pads 0) that stats_cost_kernel writes.  The value is defined by the
// cell scheme of the per-actuator moments (kernels_stats.hip), not by how a kernel is tiled:
//   a CELL is a wave-chunk of 256 consecutive k (lane l of 64 owns the k-quad 64 chunk + l) times a horizon segment of
//   L = ceil(H / 16) steps (moment_cells below: the split both moment kernels use);
//   in a cell every lane runs ONE fp32 chain per pair, in t order and within a step in the order x, y, z, w of its quad:
//       p = w_i * e_u_i;   acc = fmaf(p, e_v_i, acc)            (cross_weigh, cross_fma: stats_row's expression with
//                                                                e_v as the second factor, so u == v is eps_m2's chain)
//   then the wave's butterfly sum over the 64 lanes (offsets 32, 16, ..., 1), one partial per (pair, cell);
//   a finish pass adds a pair's partials -- lane l the cells l, l + 64, ... in (chunk, segment) order, then the same
//   butterfly -- and divides by (float)H.
// eps_mx[b][u][u] therefore equals eps_m2[b][u] bit for bit, and the result depends on nothing but the data: not on the
// form of the kernel, the grid, or which wave ran which cell.  Lanes beyond the row's last quad carry weight 0 and
// read the row's last quad (in bounds).
//
// Host + device (the MPPI_HD style of noise_model.h): cross_moment_kernel (kernels_cross.hip) runs cross_weigh /
// cross_fma on its register tiles, tests/native/cross_adapt_host.cpp runs cross_moments_host through g++, and
// mppi_hip.stats.cross_moments_f32 is the numpy restatement.
#pragma once
#include <math.h>

#include "noise_model.h"  // MPPI_HD

constexpr int kMomentSegs = 16;    // horizon segments per row (at most)
constexpr int kMomentLanes = 64;   // k-quads per wave-chunk

// the cells of one noise row: nwc wave-chunks x nseg segments of L steps (fixed by H and Kp, so by the handle)
MPPI_HD void moment_cells(int H, int Kp, int* nwc, int* L, int* nseg) {
  *nwc = (Kp / 4 + kMomentLanes - 1) / kMomentLanes;
  const int smax = H < kMomentSegs ? H : kMomentSegs;
  *L = (H + smax - 1) / smax;
  *nseg = (H + *L - 1) / *L;
}

MPPI_HD int cross_pairs(int nu) { return nu * (nu + 1) / 2; }
MPPI_HD int cross_pair(int u, int v) { return u * (u + 1) / 2 + v; }  // v <= u

// the chain's two operations, each its own statement (no mul + add pair a compiler could contract differently)
MPPI_HD float cross_weigh(float w, float eu) { return w * eu; }
MPPI_HD float cross_fma(float p, float ev, float acc) { return fmaf(p, ev, acc); }

// one lane's chain over one cell for the pair (u, v): w[4] its quad's weights, eu / ev its quad of row u / v at step
// t_begin (row pitch `pitch` floats), steps t_begin .. t_end - 1
MPPI_HD float cross_lane_cell(const float* w, const float* eu, const float* ev, long pitch, int t_begin, int t_end) {
  float acc = 0.0f;
  for (int t = t_begin; t < t_end; ++t)
    for (int i = 0; i < 4; ++i) {
      const float p = cross_weigh(w[i], eu[(long)t * pitch + i]);
      acc = cross_fma(p, ev[(long)t * pitch + i], acc);
    }
  return acc;
}

// the wave's butterfly sum of 64 lanes' values (wave_sum of wave_reduce.h on the host): offsets 32, 16, ..., 1
inline float cross_wave_sum_host(const float* lanes) {
  float v[kMomentLanes], n[kMomentLanes];
  for (int l = 0; l < kMomentLanes; ++l) v[l] = lanes[l];
  for (int o = 32; o > 0; o >>= 1) {
    for (int l = 0; l < kMomentLanes; ++l) n[l] = v[l] + v[l ^ o];
    for (int l = 0; l < kMomentLanes; ++l) v[l] = n[l];
  }
  return v[0];
}

// the finish pass of one pair on the host: part[0 .. ncell) its cell partials in (chunk, segment) order
inline float cross_finish_host(const float* part, int ncell, int H) {
  float lanes[kMomentLanes];
  for (int l = 0; l < kMomentLanes; ++l) {
    float s = 0.0f;
    for (int i = l; i < ncell; i += kMomentLanes) s += part[i];
    lanes[l] = s;
  }
  return cross_wave_sum_host(lanes) / (float)H;
}

// The whole definition on the host (the CPU form of cross_moment_kernel + cross_finish_kernel): w [B][Kp], noise
// [B][nu][H][Kp] (Kp a multiple of 4), mx [B][nu][nu] out; part: scratch of nwc * nseg floats
inline void cross_moments_host(const float* w, const float* noise, int B, int nu, int H, int Kp, float* mx,
                               float* part) {
  int nwc, L, nseg;
  moment_cells(H, Kp, &nwc, &L, &nseg);
  const int nq = Kp / 4;
  for (int b = 0; b < B; ++b)
    for (int u = 0; u < nu; ++u)
      for (int v = 0; v <= u; ++v) {
        const float* ru = noise + ((long)b * nu + u) * H * Kp;
        const float* rv = noise + ((long)b * nu + v) * H * Kp;
        for (int wc = 0; wc < nwc; ++wc)
          for (int s = 0; s < nseg; ++s) {
            float lanes[kMomentLanes];
            const int t_end = (s + 1) * L < H ? (s + 1) * L : H;
            for (int l = 0; l < kMomentLanes; ++l) {
              const int q = wc * kMomentLanes + l;
              const int qc = q < nq ? q : nq - 1;
              float wq[4] = {0.0f, 0.0f, 0.0f, 0.0f};
              if (q < nq)
                for (int i = 0; i < 4; ++i) wq[i] = w[(long)b * Kp + 4 * qc + i];
              lanes[l] = cross_lane_cell(wq, ru + 4 * qc, rv + 4 * qc, Kp, s * L, t_end);
            }
            part[wc * nseg + s] = cross_wave_sum_host(lanes);
          }
        const float m = cross_finish_host(part, nwc * nseg, H);
        mx[((long)b * nu + u) * nu + v] = m;
        mx[((long)b * nu + v) * nu + u] = m;
      }
}
