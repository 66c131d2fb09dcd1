// Learned-dynamics MPPI rollout, bf16 with two 16-sample tiles per wave (fc_rollout_kernel_wide, fc_rollout.h): the
// instantiations for the folded humanoid CA and MLP(128 x 2) nets and their launch.  Own translation unit so it takes
// its own codegen flags (build.py PER_FILE_FLAGS: accumulators in VGPRs, -amdgpu-mfma-vgpr-form).
#include "fc_rollout.h"

namespace mppi {

template <int ARCH, int COST>
static hipError_t launch_wide_t(const SolveArgs& a, const FcArgs& fa, hipStream_t stream) {
  using L = Lay<ARCH, MPPI_PREC_BF16, COST>;
  if ((a.Kp >> 4) % 2 != 0) return hipErrorInvalidValue;  // both tiles of a block in one solve
  return fc_launch(fc_rollout_kernel_wide<ARCH, COST>, a.B * (a.Kp >> 4) / 2, 64 * kSplit,
                   (size_t)fa.lds_bytes + 2 * (size_t)L::BYTES, stream, a, fa);
}

hipError_t launch_fc_wide(int arch, const SolveArgs& a, const FcArgs& fa, const FcRoute&, hipStream_t stream) {
  if (arch == kArchCA)  // the CA kernel is built for the humanoid (qpos 28) with its two costs
    return by_humanoid_cost(a.cost_kind, [&](auto cost) {
      return launch_wide_t<kArchCA, decltype(cost)::value>(a, fa, stream);
    });
  if (arch == kArchMLP)
    return by_cost(a.cost_kind, [&](auto cost) { return launch_wide_t<kArchMLP, decltype(cost)::value>(a, fa, stream); });
  return hipErrorInvalidValue;
}

}  // namespace mppi
