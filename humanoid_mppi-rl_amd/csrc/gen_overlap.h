// The rule that routes a chained solve's next-noise generation BESIDE its rollout (mppi_api.hip chain_iter): on a second,
// low-priority stream noise_beside_kernel (kernels_common.hip) draws solve i + 1's noise while solve i's rollout runs,
// and the reduce becomes the read-only pass -- instead of reduce_kernel<GEN>, which draws it behind the rollout.  This
// header is the only statement of the rule's arithmetic: the engine calls it on the host with the register counts
// hipFuncGetAttributes reports, and tests/native/gen_overlap_host.cpp runs it stand-alone.
//
// The overlap pays only where both hold:
//   size  the noise of one solve batch is past what the caches keep between the rollout's read and the reduce's
//         (reduce_kernel's own nontemporal threshold): below it the reduce is latency-bound, the fused generation hides
//         under it for free and the second stream's event waits cost more than they save;
//   fit   the generator can be resident while the rollout runs.  The rollout kernels this is for hold every SIMD at
//         kGenRolloutWaves waves of `rollout` registers; a wave's allocation is its count rounded up to the granule, a
//         SIMD's file has kGenSimdRegs, and one generator wave must fit into what is left:
//             kGenRolloutWaves * alloc(rollout) + alloc(generator) <= kGenSimdRegs
//         (fc_wave32_x3p_kernel at 248 + noise_beside_kernel at 16: 2 * 248 + 16 = 512.)  The file then also holds the
//         generator to one wave per SIMD, the youngest, which loses issue arbitration to the rollout's.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MPPI_GEN_HD __host__ __device__ inline
#else
#define MPPI_GEN_HD inline
#endif

constexpr int kGenWave = 64;          // noise_beside_kernel: one wave per block
constexpr int kGenVgprs = 16;         // ... compiled to at most this many registers
constexpr int kGenRows = 4;           // ... drawing this many whole noise rows per block
constexpr int kGenRegGranule = 8;     // the allocation granule of a wave's registers (512-entry unified file)
constexpr int kGenSimdRegs = 512;     // registers per lane of one SIMD
constexpr int kGenRolloutWaves = 2;   // the rollout's waves per SIMD
constexpr uint64_t kGenMinNoiseBytes = 128ull * 1024 * 1024;  // = reduce_kernel's nontemporal threshold

// the route a chained solve took (mppi_gen_route)
constexpr int kGenRouteNone = 0;     // no chained solve yet, or the last solve was not a chained one
constexpr int kGenRouteFused = 1;    // reduce_kernel<GEN> behind the rollout
constexpr int kGenRouteOverlap = 2;  // noise_beside_kernel beside the rollout, read-only reduce

// registers a wave of `regs` registers allocates
MPPI_GEN_HD int gen_alloc(int regs) { return (regs + kGenRegGranule - 1) / kGenRegGranule * kGenRegGranule; }

// whether one generator wave fits beside the rollout's waves on a SIMD (a count <= 0 is unknown: no fit)
MPPI_GEN_HD bool gen_fits(int rollout_regs, int gen_regs) {
  if (rollout_regs <= 0 || gen_regs <= 0) return false;
  return kGenRolloutWaves * gen_alloc(rollout_regs) + gen_alloc(gen_regs) <= kGenSimdRegs;
}

// bytes of one batch's noise [B][nu][H][Kp] fp32
MPPI_GEN_HD uint64_t gen_noise_bytes(int B, int nu, int H, int Kp) {
  return (uint64_t)B * (uint64_t)nu * (uint64_t)H * (uint64_t)Kp * 4ull;
}

// whether the noise is past the size where the reduce stops being latency-bound (strictly, as the reduce's own test)
MPPI_GEN_HD bool gen_size_ok(uint64_t noise_bytes) { return noise_bytes > kGenMinNoiseBytes; }

// the rule
MPPI_GEN_HD bool gen_overlap_rule(int B, int nu, int H, int Kp, int rollout_regs, int gen_regs) {
  return gen_size_ok(gen_noise_bytes(B, nu, H, Kp)) && gen_fits(rollout_regs, gen_regs);
}
