// ESS targeting (mppi_set_ess_target; the rule is ess_target.h): lambda_search_kernel chooses, per solve, the softmin
// temperature at which the solve's own costs give the requested effective sample size, and writes it where the reduce
// and the statistics read it.  One launch between the rollout and the reduce; read-only on the costs.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>

#include "ess_target.h"
#include "mppi_internal.h"
#include "wave_reduce.h"

namespace mppi {

// ------------------------------------------------------------------------------------------------
// One block per solve, grid B.  Thread tid owns the costs k = tid, tid + nt, ... (coalesced; up to kLamPer = 32 of
// them at kMaxK and 1024 threads) and keeps d_k = c_k - beta in registers for the whole search: +inf for a non-finite
// cost and for the pads, so their weight __expf(-inf) is 0 with no test in the loop.
// A pass evaluates ESS at NC candidates (lane j forms candidate j and its reciprocal, read back wave-uniform): per
// thread NC exponentials per owned cost into 2 NC running sums (sum wt, sum wt^2), ONE transposed wave butterfly for
// all of them (wave_sum_slots: 32 sums in 32 exchanges, 24 of them DPP), one LDS store per slot-owning lane, one
// barrier, then lanes 0..NC-1 of EVERY wave add the waves' partials in wave order and a ballot gives each wave the
// pass's mask -- so all threads take the search's branches alike with a single barrier per pass (the partials are
// double-buffered by pass parity: a pass's buffer is rewritten two barriers later).
// Every sum has a fixed order (thread's costs ascending, the butterfly, waves ascending): runs repeat bitwise.
// Sizing: about four costs per thread, whole waves (K <= 4096: the PER = 4 form, 54 VGPRs); above that 1024 threads of
// up to 32 costs (PER = 32: 32 d + 32 sums and the loop's temporaries, 81 VGPRs, within the 128 that 16 waves per CU
// leave; the candidates are evaluated one after the other so only two running sums are live in the loop; no
// scratch).  4 KiB of LDS.  B blocks on 256 CUs and ~7 dependent passes: the kernel is bound by the instructions each
// wave issues per pass, not by throughput (DESIGN.md section 4 has the forms tried and their figures).
// ------------------------------------------------------------------------------------------------
constexpr int kLamPer = kMaxK / 1024;  // costs per thread at most (PER of the large form)
constexpr int kLamPerSmall = 4;        // ... of the form for K <= 4096 (the host's block sizing gives every thread <= 4)

template <int NC, int PER>
__global__ __launch_bounds__(1024) void lambda_search_kernel(const float* __restrict__ costs, int K, int Kp,
                                                             EssTarget s, float cfg_lambda,
                                                             float* __restrict__ lambda_out) {
  constexpr int NV = NC == 1 ? 2 : 32;  // sums per pass, padded to a power of two: [0, NC) sum wt, [NV/2, NV/2 + NC) sum wt^2
  static_assert(2 * NC <= NV && NC <= 16, "the candidates' sums fill one butterfly");
  __shared__ float red[2][16 * NV];
  __shared__ float red0[32];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, nt = blockDim.x, nw = nt >> 6;
  const float* c = costs + (long)b * Kp;
  // the owned costs, all loads in flight at once; the host sizes the block and picks PER so that PER * nt >= K
  float d[PER];
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int k = i * nt + tid;
    d[i] = INFINITY;
    if (k < K) {
      const float ck = c[k];
      d[i] = ess_finite(ck) ? ck : INFINITY;
    }
  }
  float m = INFINITY, cnt = 0.0f;
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    m = fminf(m, d[i]);
    cnt += d[i] < INFINITY ? 1.0f : 0.0f;  // (exact: at most 32768)
  }
  m = wave_min(m);
  cnt = wave_sum(cnt);
  if (lane == 0) {
    red0[wv] = m;
    red0[16 + wv] = cnt;
  }
  __syncthreads();
  float beta = red0[0], nf = red0[16];
  for (int i = 1; i < nw; ++i) {
    beta = fminf(beta, red0[i]);
    nf += red0[16 + i];
  }
  const int n = (int)nf;
  if (n == 0) {  // (uniform) no finite cost: the solve reports MPPI_E_NONFINITE with the configured lambda
    if (tid == 0) lambda_out[b] = cfg_lambda;
    return;
  }
#pragma unroll
  for (int i = 0; i < PER; ++i) d[i] = d[i] - beta;  // (+inf stays +inf: beta is finite)
  const float T = ess_target_count(s.ess_frac, n);
  const int per = (K + nt - 1) / nt;  // owned costs of thread 0 (uniform trip count; a slot past K holds +inf)
  int buf = 0;
  auto eval = [&](float lo, float hi, bool ends) -> unsigned {
    // lane j of every wave forms candidate j and its reciprocal (reduce_kernel's 1 / lambda) once; the loop below reads
    // them as wave-uniform values (v_readlane), so a thread pays one division per pass, not NC
    const float inv_own = 1.0f / ess_candidate<NC>(lo, hi, min(lane, NC - 1), ends);
    float v[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) v[j] = 0.0f;
#pragma unroll
    for (int j = 0; j < NC; ++j) {  // (candidate by candidate: two running sums live at a time)
      const float inv_lam = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(inv_own), j));
      float S = 0.0f, S2 = 0.0f;
#pragma unroll
      for (int i = 0; i < PER; ++i) {
        if (PER <= kLamPerSmall || i < per) {  // (the small form: no test, a slot past K holds +inf, weight 0)
          const float wt = __expf(-inv_lam * d[i]);  // reduce_kernel's weight expression on d = c_k - beta
          S = S + wt;
          S2 = fmaf(wt, wt, S2);
        }
      }
      v[j] = S;
      v[NV / 2 + j] = S2;
    }
    const float r = wave_sum_slots<NV>(v, lane);
    float* rb = red[buf];
    if (lane < NV) rb[wv * NV + wave_sum_slot<NV>(lane)] = r;
    __syncthreads();
    bool ge = false;
    if (lane < NC) {
      float S = 0.0f, S2 = 0.0f;
      for (int w = 0; w < nw; ++w) {  // fixed order
        S = S + rb[w * NV + lane];
        S2 = S2 + rb[w * NV + NV / 2 + lane];
      }
      const float sq = S * S;
      ge = sq / S2 >= T;
    }
    buf ^= 1;
    return (unsigned)__ballot(ge);
  };
  const float lam = ess_search<NC>(s, eval);
  if (tid == 0) lambda_out[b] = lam;
}

// MPPI_LAMBDA_SEARCH=bisect (read per launch; an A/B arm): plain bisection, one candidate per pass; default: 15
static bool lambda_bisect() {
  const char* e = std::getenv("MPPI_LAMBDA_SEARCH");
  return e && std::strcmp(e, "bisect") == 0;
}

hipError_t launch_lambda_search(const float* costs, int B, int K, int Kp, const EssTarget& s, float cfg_lambda,
                                float* lambda_out, hipStream_t stream) {
  if (K < 1 || K > kMaxK) return hipErrorInvalidValue;  // (mppi_create's bound: kLamPer costs per thread suffice)
  // about four costs per thread, whole waves: a pass is bound by the instructions each wave issues (the butterfly,
  // the cross-wave sum), so K = 1024 runs one wave per SIMD (16 waves of one cost each measured 38 us per search where
  // 4 waves of four took 32, before the butterfly's DPP steps); at kMaxK 1024 threads of kLamPer costs each
  int nt = ((K + 3) / 4 + 63) / 64 * 64;
  nt = nt > 1024 ? 1024 : nt;
  const bool small = (long)kLamPerSmall * nt >= K;  // K <= 4096: four register-held costs per thread
  const bool bisect = lambda_bisect();
  auto kern = bisect ? (small ? lambda_search_kernel<1, kLamPerSmall> : lambda_search_kernel<1, kLamPer>)
                     : (small ? lambda_search_kernel<15, kLamPerSmall> : lambda_search_kernel<15, kLamPer>);
  hipLaunchKernelGGL(kern, dim3(B), dim3(nt), 0, stream, costs, K, Kp, s, cfg_lambda, lambda_out);
  return hipGetLastError();
}

}  // namespace mppi
