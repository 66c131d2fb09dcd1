// Inner iterations per control step (mppi_set_iterations; the rule of the tracking is iter_best.h):
//   iter_best_kernel   the best sample of the step so far, behind the cost terms and the selections and ahead of the
//                      lambda search and the reduce (every iteration while the feature is on)
//   iter_apply_kernel  u0 <- the stored best's first control, behind the update and shift and ahead of the bounds clip
//                      (return_best, the step's last iteration)
//   iter_mean_kernel   one column of the noise zeroed, behind the kept-elite injection and ahead of the bounds
//                      projection and the rollout: the nominal itself competes (add_mean, the step's last iteration)
// All three work beside the rollout and reduce kernels, never inside them: a solve with the feature on is routed
// exactly as without it.
#include <hip/hip_runtime.h>

#include "iter_best.h"
#include "mppi_internal.h"

namespace mppi {

// ------------------------------------------------------------------------------------------------
// iter_best_kernel.  One block per solve, grid B, the selection's and the lambda search's sizing: four costs per thread
// in whole waves up to K = 4096 (NJ = 1), above that 1024 threads of up to kMaxK / 1024 = 32 costs each (NJ = 8).
// Ownership: thread tid owns, for j < NJ, the four consecutive costs k = 4 (j nt + tid) + {0..3}: one 16-B load per j,
// a wave reading 1 KiB contiguous per instruction, every cost read once and folded at once into the thread's packed
// (ordered cost bits, k) minimum -- two registers, whatever NJ.  The pads K..Kp and the non-finite costs pack to
// kIterNoCand, above every candidate.  The wave's minimum: quad permutes and row rotations (DPP operands, both halves
// of the pair) leave every lane with its row's minimum, four lane reads give the wave's, uniform.  Across waves: one
// LDS entry per wave, one barrier, every thread reads the (at most 16) entries.  All pairs are distinct (k is part of
// them), so the minimum does not depend on any order: bitwise repeatable, no atomics.  The key holds +0 for either
// zero, so the cost itself travels beside it: a thread keeps the raw cost of its own minimum, the one lane whose pair
// is the wave's writes both to LDS -- no second trip to global memory for c[k*].
// Then, uniform over the block: the stored best's cost (read by every thread ahead of the barrier, written by thread 0
// behind it), the strict comparison, and on acceptance nu H gathered 4-byte loads of column k* at pitch Kp in tiles of
// kIterTile rows per thread, every load of a tile issued before the first is consumed (the kernel is a chain of two
// cold round trips to memory, the costs and then the column; nothing else in it takes as long), with the nominal
// beside them (coalesced; the first tile's read ahead of the barrier, under the costs' latency) and coalesced stores
// of bv.  The first iteration of a step stores the reset state where nothing is accepted.  k* < K by construction: no
// index outside the row is formed.
// ------------------------------------------------------------------------------------------------
// The 1024-thread form holds 32 costs in flight per thread and gathers at most a few rows each: two per tile there.
// NJ = 1: 50 VGPRs, NJ = 8: within the 128 that 16 waves per CU leave, no scratch; 192 B of LDS.
template <int NJ>
constexpr int iter_tile() { return NJ == 1 ? 8 : 2; }  // rows of the column a thread has in flight at once
template <int CTRL>
__device__ __forceinline__ unsigned dpp_u32(unsigned x) {
  return (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, 0xF, 0xF, false);
}
template <int CTRL>
__device__ __forceinline__ uint64_t dpp_min_u64(uint64_t x) {
  const uint64_t y = ((uint64_t)dpp_u32<CTRL>((unsigned)(x >> 32)) << 32) | dpp_u32<CTRL>((unsigned)x);
  return y < x ? y : x;
}
// the wave's minimum, uniform (every lane active)
__device__ __forceinline__ uint64_t wave_min_u64(uint64_t x) {
  x = dpp_min_u64<0xB1>(x);   // quad_perm [1,0,3,2]
  x = dpp_min_u64<0x4E>(x);   // quad_perm [2,3,0,1]
  x = dpp_min_u64<0x124>(x);  // row_ror:4
  x = dpp_min_u64<0x128>(x);  // row_ror:8: every lane holds its row's minimum
  uint64_t m = kIterNoCand;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const uint64_t v = ((uint64_t)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)(x >> 32), 16 * r) << 32) |
                       (unsigned)__builtin_amdgcn_readlane((int)(unsigned)x, 16 * r);
    m = v < m ? v : m;
  }
  return m;
}

template <int NJ>
__global__ __launch_bounds__(1024) void iter_best_kernel(IterBestArgs a) {
  __shared__ uint64_t wmin[16];
  __shared__ float wraw[16];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, nt = blockDim.x;
  const float* c = a.costs + (long)b * a.Kp;
  const int nj = NJ == 1 ? 1 : (a.K + 4 * nt - 1) / (4 * nt);  // chunks in use (uniform; the host sizes 4 nt NJ >= K)

  // the owned costs, all loads in flight at once.  Kp is a multiple of 4 and the rows are 16-B aligned: a chunk that
  // starts below Kp lies inside the row
  float4 cv[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int p = 4 * (j * nt + tid);
    cv[j] = make_float4(INFINITY, INFINITY, INFINITY, INFINITY);
    if (j < nj && p < a.Kp) cv[j] = *reinterpret_cast<const float4*>(c + p);
  }
  const float bcost = a.reset ? INFINITY : a.bcost[b];  // the stored best, ahead of the barrier
  const int RB = a.nu * a.H;
  const float* Ub = a.U + (long)b * RB;
  constexpr int kIterTile = iter_tile<NJ>();
  float u[kIterTile];  // the nominal of the first tile's rows
#pragma unroll
  for (int g = 0; g < kIterTile; ++g) {
    const int r = g * nt + tid;
    u[g] = r < RB ? Ub[r] : 0.0f;
  }
  // this thread's minimum: its costs come in ascending k, so a strict comparison of the keys keeps the lowest k
  unsigned bkey = kEliteNoKey;
  int bk = 0;
  float raw = INFINITY;  // the cost the minimum stands for, as stored
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int p = 4 * (j * nt + tid);
    const float v[4] = {cv[j].x, cv[j].y, cv[j].z, cv[j].w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const unsigned key = p + e < a.K ? elite_key_or_none(v[e]) : kEliteNoKey;
      const bool lower = key < bkey;
      raw = lower ? v[e] : raw;
      bk = lower ? p + e : bk;
      bkey = lower ? key : bkey;
    }
  }
  // (iter_best_pack's pair: no finite cost has the key kEliteNoKey)
  uint64_t best = bkey == kEliteNoKey ? kIterNoCand : (((uint64_t)bkey << 32) | (unsigned)bk);
  const uint64_t wbest = wave_min_u64(best);
  if (wbest == kIterNoCand ? lane == 0 : best == wbest) {  // (one lane: the pairs are distinct)
    wmin[wv] = wbest;
    wraw[wv] = raw;
  }
  __syncthreads();
  const int nw = nt >> 6;
  best = kIterNoCand;
  float cand = INFINITY;  // the cost itself, bit for bit
  for (int w = 0; w < nw; ++w) {  // (uniform: LDS broadcast reads)
    const uint64_t q = wmin[w];
    cand = q < best ? wraw[w] : cand;
    best = q < best ? q : best;
  }

  const int ks = iter_best_k(best);  // < K, or -1
  const bool take = ks >= 0 && iter_best_accept(cand, bcost);
  if (!take && !a.reset) return;  // (uniform) the stored best stays
  float* bv = a.bv + (long)b * RB;
  if (take) {
    const float* nb = a.noise + (long)b * RB * a.Kp + ks;
    for (int r0 = 0; r0 < RB; r0 += kIterTile * nt) {  // (uniform)
      float e[kIterTile];
#pragma unroll
      for (int g = 0; g < kIterTile; ++g) {
        const int r = r0 + g * nt + tid;
        e[g] = r < RB ? nb[(long)r * a.Kp] : 0.0f;
        if (r0 > 0) u[g] = r < RB ? Ub[r] : 0.0f;
      }
#pragma unroll
      for (int g = 0; g < kIterTile; ++g) {
        const int r = r0 + g * nt + tid;
        if (r < RB) bv[r] = rate_cost_v(u[g], e[g], a.clamp);
      }
    }
  } else {
    for (int r = tid; r < RB; r += nt) bv[r] = 0.0f;
  }
  if (tid == 0) {
    a.bcost[b] = take ? cand : INFINITY;
    a.bk[b] = take ? ks : -1;
    a.biter[b] = take ? a.it : -1;
  }
}

hipError_t launch_iter_best(const IterBestArgs& a, hipStream_t stream) {
  if (a.B < 1 || a.nu < 1 || a.H < 1 || a.K < 1 || a.K > kMaxK || a.Kp < a.K || (a.Kp & 3)) return hipErrorInvalidValue;
  // the selection's sizing: four costs per thread in whole waves, then 1024 threads of up to 32
  int nt = ((a.K + 3) / 4 + 63) / 64 * 64;
  nt = nt > 1024 ? 1024 : nt;
  const bool small = 4L * nt >= a.K;  // K <= 4096
  auto kern = small ? iter_best_kernel<1> : iter_best_kernel<kMaxK / 4096>;
  hipLaunchKernelGGL(kern, dim3(a.B), dim3(nt), 0, stream, a);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// iter_apply_kernel: u0[b][u] = bv[b][u][0] where the step stored a best (bk[b] >= 0); else u0 stays as the update left
// it.  One thread per (b, u).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void iter_apply_kernel(const float* __restrict__ bv, const int32_t* __restrict__ bk,
                                                         float* __restrict__ u0, int B, int nu, int H) {
  const int i = (int)(blockIdx.x * 256 + threadIdx.x);
  if (i >= B * nu) return;
  const int b = (int)((unsigned)i / (unsigned)nu);
  if (bk[b] >= 0) u0[i] = bv[(long)i * H];
}

hipError_t launch_iter_apply(const float* bv, const int32_t* bk, float* u0, int B, int nu, int H, hipStream_t stream) {
  if (B < 1 || nu < 1 || H < 1 || (long)B * nu >= (1L << 30)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(iter_apply_kernel, dim3((unsigned)((B * nu + 255) / 256)), dim3(256), 0, stream, bv, bk, u0, B,
                     nu, H);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// iter_mean_kernel: eps[b][u][t][j0] = +0.0 for every (u, t), j0 = count[b] clamped to [0, n_keep] (the stored kept
// set's count, read on the device like the injection reads it; count == nullptr: 0).  j0 >= K writes nothing.  One
// thread per (b, row): nu H scattered 4-byte stores per solve, nothing read but the count.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void iter_mean_kernel(float* __restrict__ noise, const int32_t* __restrict__ count,
                                                        int n_keep, int B, int RB, int K, int Kp) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)B * RB) return;
  const int b = (int)(i / RB);
  int j0 = count ? count[b] : 0;
  j0 = j0 < 0 ? 0 : (j0 > n_keep ? n_keep : j0);
  if (j0 >= K) return;
  noise[i * Kp + j0] = 0.0f;
}

hipError_t launch_iter_mean(float* noise, const int32_t* count, int n_keep, int B, int nu, int H, int K, int Kp,
                            hipStream_t stream) {
  const long rows = (long)B * nu * H;
  if (B < 1 || nu < 1 || H < 1 || K < 1 || Kp < K || n_keep < 0 || rows >= (1L << 30)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(iter_mean_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, stream, noise, count, n_keep,
                     B, nu * H, K, Kp);
  return hipGetLastError();
}

}  // namespace mppi
