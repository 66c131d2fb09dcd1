// Weighted per-step moments of the noise a solve used (MPPI_FLAG_STEP_MOMENTS, mppi_step_moments_eval):
//   m1[b][u][t] = sum_k w_k eps[b][u][t][k]          m2[b][u][t] = sum_k w_k eps[b][u][t][k]^2
// with w the normalised softmin weights [B][Kp] (pads 0) that stats_cost_kernel writes: about the elite set of
// mppi_set_elites m1 is the elite mean and m2 - m1^2 the elite variance, per actuator AND per horizon step -- what a
// CEM-style refit of a per-step sampling scale is driven by (step_law.h).
// The value is defined by a cell scheme fixed by (H, Kp) alone, not by how a kernel is tiled:
//   a row (b, u, t) is cut into WAVE-CHUNKS of 256 consecutive k (lane l of 64 owns the k-quad 64 chunk + l);
//   per lane, one explicit fp32 chain per moment over its own four k in ascending order (x, y, z, w), from 0:
//       a1 = fmaf(w_i, e_i, a1)            p = w_i * e_i;  a2 = fmaf(p, e_i, a2)       (step_lane below; a2 is
//                                                                                         stats_row's expression)
//   across the 64 lanes of a chunk the wave's butterfly sum (offsets 32, 16, ..., 1: wave_sum of wave_reduce.h);
//   across the chunks of a row, ascending: tot = 0; tot = tot + chunk_sum.
// No division: the weights are normalised.  Lanes beyond the row's last quad carry weight 0 and read the row's last
// quad (in bounds).  The result depends on nothing but the data: not on the grid, nor on how many rows a wave reduces at
// once (step_moment_kernel sums eight rows' sixteen values through one butterfly; every sum has wave_sum's bits).
//
// Host + device (the MPPI_HD style of noise_model.h): step_moment_kernel (kernels_step_moments.hip) runs step_lane on
// its register tiles, tests/test_noise_steps.py runs step_moments_host through g++, and
// mppi_hip.stats.step_moments_f32 is the numpy restatement.
#pragma once
#include <math.h>

#include "noise_model.h"  // MPPI_HD

constexpr int kStepLanes = 64;  // k-quads per wave-chunk

MPPI_HD int step_chunks(int Kp) { return (Kp / 4 + kStepLanes - 1) / kStepLanes; }

// one lane's two chains over its quad of one row: every product and sum its own statement or an explicit fmaf (no
// mul + add pair a compiler could contract differently on the two sides)
MPPI_HD void step_lane(const float* w, const float* e, float* m1, float* m2) {
  float a1 = 0.0f, a2 = 0.0f;
  for (int i = 0; i < 4; ++i) {
    a1 = fmaf(w[i], e[i], a1);
    const float p = w[i] * e[i];
    a2 = fmaf(p, e[i], a2);
  }
  *m1 = a1;
  *m2 = a2;
}

// the wave's butterfly sum of 64 lanes' values on the host: offsets 32, 16, ..., 1
inline float step_wave_sum_host(const float* lanes) {
  float v[kStepLanes], n[kStepLanes];
  for (int l = 0; l < kStepLanes; ++l) v[l] = lanes[l];
  for (int o = 32; o > 0; o >>= 1) {
    for (int l = 0; l < kStepLanes; ++l) n[l] = v[l] + v[l ^ o];
    for (int l = 0; l < kStepLanes; ++l) v[l] = n[l];
  }
  return v[0];
}

// The whole definition on the host (the CPU form of step_moment_kernel): w [B][Kp], noise [B][nu][H][Kp] (Kp a multiple
// of 4), m1 / m2 [B][nu][H] out
inline void step_moments_host(const float* w, const float* noise, int B, int nu, int H, int Kp, float* m1, float* m2) {
  const int nq = Kp / 4, nwc = step_chunks(Kp);
  for (int b = 0; b < B; ++b)
    for (long r = 0; r < (long)nu * H; ++r) {
      const float* row = noise + ((long)b * nu * H + r) * Kp;
      float t1 = 0.0f, t2 = 0.0f;
      for (int wc = 0; wc < nwc; ++wc) {
        float l1[kStepLanes], l2[kStepLanes];
        for (int l = 0; l < kStepLanes; ++l) {
          const int q = wc * kStepLanes + l;
          const int qc = q < nq ? q : nq - 1;
          float wq[4] = {0.0f, 0.0f, 0.0f, 0.0f};
          if (q < nq)
            for (int i = 0; i < 4; ++i) wq[i] = w[(long)b * Kp + 4 * qc + i];
          step_lane(wq, row + 4 * qc, &l1[l], &l2[l]);
        }
        t1 = t1 + step_wave_sum_host(l1);
        t2 = t2 + step_wave_sum_host(l2);
      }
      m1[(long)b * nu * H + r] = t1;
      m2[(long)b * nu * H + r] = t2;
    }
}
