// Learned-dynamics MPPI rollout, fc-stack nets: the MLP instantiations of fc_rollout_kernel (fc_rollout.h) and the
// dispatcher (the CA instantiation lives in kernels_fc_ca.hip).
#include "fc_rollout.h"

#include <atomic>

namespace mppi {

thread_local const char* g_rollout_kernel = "";
thread_local const void* g_rollout_func = nullptr;

int current_device_cus() {
  constexpr int kMaxDev = 64;
  static std::atomic<int> cache[kMaxDev];
  int dev = 0, n = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 256;
  if (dev >= 0 && dev < kMaxDev) {
    const int c = cache[dev].load(std::memory_order_relaxed);
    if (c > 0) return c;
  }
  if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
  if (dev >= 0 && dev < kMaxDev) cache[dev].store(n, std::memory_order_relaxed);
  return n;
}

hipError_t launch_fc_msplit_mlp(const SolveArgs& a, const FcArgs& fa, const FcRoute& r, hipStream_t stream) {
  return by_cost(a.cost_kind, [&](auto cost) {
    return launch_msplit_t<kArchMLP, decltype(cost)::value>(a, fa, r, stream);
  });
}

hipError_t launch_fc_rollout(const SolveArgs& a, const FcNet& n, hipStream_t stream) {
  if (n.arch != kArchCA && n.arch != kArchMLP && n.arch != kArchGeneric) return hipErrorInvalidValue;
  const FcRoute r = fc_route(n.arch, n.precision, a, n.fa, n.x3_l1, n.x3_f16, current_device_cus(), fc_knobs_from_env());
  return launch_fc_route(a, n, r, stream);
}

hipError_t launch_fc_route(const SolveArgs& a, const FcNet& n, const FcRoute& r, hipStream_t stream) {
  note_kernel(fc_route_name(r));
  if (r.kernel == FcKernel::generic) return n.arch == kArchGeneric ? launch_fc_generic(a, n, stream) : hipErrorInvalidValue;
  const bool ca = n.arch == kArchCA, mlp = n.arch == kArchMLP;
  // the CA kernels are built for the humanoid (qpos 28) with its two costs
  if (ca && a.cost_kind != MPPI_COST_HUMANOID_V3 && a.cost_kind != MPPI_COST_HUMANOID_V1) return hipErrorInvalidValue;
  const FcArgs& fa = n.fa;
  if ((!ca && !mlp) || !fc_route_can_run(r.kernel, a, fa)) return hipErrorInvalidValue;
  switch (r.kernel) {
    case FcKernel::msplit:
    case FcKernel::msplit_f32:
    case FcKernel::msplit_x3:
    case FcKernel::msplit_x3w: return ca ? launch_fc_msplit_ca(a, fa, r, stream) : launch_fc_msplit_mlp(a, fa, r, stream);
    case FcKernel::wave:
    case FcKernel::wave32: return ca ? launch_fc_wave(a, fa, r, stream) : hipErrorInvalidValue;
    case FcKernel::wave_mlp: return mlp ? launch_fc_wave_mlp(a, fa, r, stream) : hipErrorInvalidValue;
    case FcKernel::x3_wave32: return ca ? launch_fc_wave_x3(a, fa, r, stream) : hipErrorInvalidValue;
    case FcKernel::x3p: return ca ? launch_fc_wave_x3p(a, fa, r, stream) : hipErrorInvalidValue;
    case FcKernel::x3d: return ca ? launch_fc_x3d(a, fa, r, stream) : hipErrorInvalidValue;
    case FcKernel::x3h: return ca ? launch_fc_x3h(a, fa, r, stream) : hipErrorInvalidValue;
    case FcKernel::x3m: return mlp ? launch_fc_wave_mlp_x3(a, fa, r, stream) : hipErrorInvalidValue;
    case FcKernel::x3mp: return mlp ? launch_fc_wave32_mlp_x3(a, fa, r, stream) : hipErrorInvalidValue;
#ifdef MPPI_AB_ARMS
    case FcKernel::pipe: return ca ? launch_fc_pipe(a, fa, r, stream) : hipErrorInvalidValue;
    case FcKernel::wide: return launch_fc_wide(n.arch, a, fa, r, stream);
#endif
    default: return hipErrorInvalidValue;
  }
}

#ifdef MPPI_STAMPS
extern "C" int mppi_debug_stamps(unsigned long long* out, int reset) {  // both fc translation units' sums
  unsigned long long s[kNumStamps];
  if (fc_ca_stamps(s, reset) != 0) return -2;
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_stamps), sizeof(unsigned long long) * kNumStamps) != hipSuccess) return -2;
  for (int i = 0; i < kNumStamps; ++i) out[i] += s[i];
  if (reset) {
    unsigned long long z[kNumStamps] = {0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_stamps), z, sizeof(z)) != hipSuccess) return -2;
  }
  return 0;
}
#endif

}  // namespace mppi
