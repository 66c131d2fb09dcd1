// Wave reductions shared by the reduce (kernels_common.hip) and the analytic cartpole (kernels_cartpole.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace mppi {

// ------------------------------------------------------------------------------------------------
// Wave / block reductions (fixed order -> bitwise deterministic).
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o));
  return v;
}

// lane l's value of lane l ^ O: within a quad (O = 1, 2) a DPP operand of the add itself, no LDS-pipe round trip
template <int O>
__device__ __forceinline__ float lane_xor(float x) {
  if constexpr (O == 1)
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0xB1, 0xF, 0xF, false));  // quad_perm [1,0,3,2]
  else if constexpr (O == 2)
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x4E, 0xF, 0xF, false));  // quad_perm [2,3,0,1]
  else
    return __shfl_xor(x, O);
}

// N sums over the wave at once (N a power of two <= 32): lane l < N returns the sum of v[wave_sum_slot<N>(l)] over
// the 64 lanes.  A butterfly over offsets 1, 2, ..., 32 whose first log2 N steps exchange HALF of the values each (the
// lane whose offset bit is clear keeps the lower half and sends the upper, its partner the reverse), so N sums cost
// N + 5 - log2 N exchanges rather than 6 N, and the steps that move the most values (offsets 1 and 2: 3/4 of them)
// are DPP quad permutes.  Every sum adds its 64 terms in one fixed order: bitwise repeatable.  v is consumed.
template <int N>
__device__ __forceinline__ int wave_sum_slot(int lane) {  // the slot lane `lane` < N ends up with: its bits reversed
  static_assert(N >= 1 && N <= 32 && (N & (N - 1)) == 0, "N: a power of two <= 32");
  int slot = 0;
#pragma unroll
  for (int n = N, bit = 1; n > 1; n >>= 1, bit <<= 1) slot |= (lane & bit) ? (n >> 1) : 0;
  return slot;
}
template <int N, int O = 1>
__device__ __forceinline__ float wave_sum_slots(float (&v)[N], int lane) {
  static_assert(N >= 1 && N <= 32 && (N & (N - 1)) == 0, "N: a power of two <= 32");
  if constexpr (N > 1) {
    const bool up = (lane & O) != 0;
    float h[N / 2];
#pragma unroll
    for (int i = 0; i < N / 2; ++i) {
      const float keep = up ? v[N / 2 + i] : v[i];
      const float send = up ? v[i] : v[N / 2 + i];
      h[i] = keep + lane_xor<O>(send);
    }
    return wave_sum_slots<N / 2, O * 2>(h, lane);
  } else {
    float r = v[0];
    if constexpr (O <= 1) r += lane_xor<1>(r);
    if constexpr (O <= 2) r += lane_xor<2>(r);
    if constexpr (O <= 4) r += lane_xor<4>(r);
    if constexpr (O <= 8) r += lane_xor<8>(r);
    if constexpr (O <= 16) r += lane_xor<16>(r);
    if constexpr (O <= 32) r += lane_xor<32>(r);
    return r;
  }
}

}  // namespace mppi
