// Dynamics-model ensembles (mppi_set_ensemble; the rule is ensemble.h):
//   ensemble_kernel   the members' costs [n][B][Kp] combined, per sample, into the solve's costs [B][Kp] and the members'
//                     spread [B][Kp] -- one launch behind the n rollouts of a solve and ahead of everything that reads
//                     its costs (the cost terms, the selections, the lambda search, the reduce, the statistics)
// It works beside the rollout kernels, never inside them: every member is rolled by the kernel a handle that loaded it
// alone would be routed to.
#include <hip/hip_runtime.h>

#include "ensemble.h"
#include "mppi_internal.h"

namespace mppi {

// ------------------------------------------------------------------------------------------------
// ensemble_kernel<N>.  One lane per four consecutive samples: N 16-byte loads, one per member, all issued before the
// first is consumed (N is a template parameter, so the loop over the members unrolls and the loads sit in 4 N registers),
// then the rule of ensemble.h on each of the four samples from registers, and two 16-byte stores.  The rows of one member
// are dense ([B][Kp], Kp a multiple of 64), so lane i owns floats 4 i .. 4 i + 3 of every member's B Kp and of both
// outputs: a wave reads 1 KiB contiguous per member and writes 1 KiB per output.  The pad lanes K..Kp go through the
// rule like every other lane (whatever the rollouts left there; nothing downstream counts them).  At the sizes of a
// solve ((2 + N) x 256 KiB at 64 solves of 1024 samples) the launch, not the bytes, is the floor.
// No LDS, no atomics; 4 i + 3 < B Kp for every lane that passes the guard: no address outside the rows is formed.
// ------------------------------------------------------------------------------------------------
template <int N>
__global__ __launch_bounds__(256) void ensemble_kernel(EnsembleArgs a) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n4) return;
  float4 cv[N];
#pragma unroll
  for (int e = 0; e < N; ++e) cv[e] = *reinterpret_cast<const float4*>(a.members + e * a.stride + 4 * i);
  float c[4][N];
#pragma unroll
  for (int e = 0; e < N; ++e) {
    c[0][e] = cv[e].x;
    c[1][e] = cv[e].y;
    c[2][e] = cv[e].z;
    c[3][e] = cv[e].w;
  }
  float cost[4], sd[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) cost[j] = ensemble_combine(c[j], 1, N, a.r, a.mode, a.kappa, &sd[j]);
  *reinterpret_cast<float4*>(a.costs + 4 * i) = make_float4(cost[0], cost[1], cost[2], cost[3]);
  *reinterpret_cast<float4*>(a.sd + 4 * i) = make_float4(sd[0], sd[1], sd[2], sd[3]);
}

hipError_t launch_ensemble(const EnsembleArgs& a, hipStream_t stream) {
  if (a.n < 2 || a.n > MPPI_ENS_MAX || a.n4 < 1 || a.n4 >= (1L << 30) || a.stride < 4 * a.n4 || (a.stride & 3) ||
      !ensemble_mode_valid(a.mode) || !a.members || !a.costs || !a.sd)
    return hipErrorInvalidValue;
  void (*kern)(EnsembleArgs) = nullptr;
  switch (a.n) {
    case 2: kern = ensemble_kernel<2>; break;
    case 3: kern = ensemble_kernel<3>; break;
    case 4: kern = ensemble_kernel<4>; break;
    case 5: kern = ensemble_kernel<5>; break;
    case 6: kern = ensemble_kernel<6>; break;
    case 7: kern = ensemble_kernel<7>; break;
    default: kern = ensemble_kernel<8>; break;
  }
  hipLaunchKernelGGL(kern, dim3((unsigned)((a.n4 + 255) / 256)), dim3(256), 0, stream, a);
  return hipGetLastError();
}

}  // namespace mppi
