// Elite truncation (mppi_set_elites; the rule is elite_select.h): elite_select_kernel finds, per solve, the n_elite
// best of the costs the softmin would weigh and writes, in ONE launch, the masked costs the lambda search, the reduce
// and the statistics read instead (ecost: the cost on the elite set, +inf elsewhere), the set itself in ascending k,
// its size and its threshold.  One launch between the rollout (and the cost terms) and the lambda search; read-only on
// its input costs.
#include <hip/hip_runtime.h>

#include "elite_select.h"
#include "mppi_internal.h"

namespace mppi {

// ------------------------------------------------------------------------------------------------
// One block per solve, grid B, lambda_search_kernel's sizing: about four costs per thread in whole waves up to
// K = 4096 (NJ = 1), above that 1024 threads of up to kMaxK / 1024 = 32 costs each (NJ = 8).
// Ownership: thread tid owns, for j < NJ, the four consecutive costs k = 4 (j nt + tid) + {0..3}: one 16-B load per j,
// a wave reading 1 KiB contiguous per instruction, every cost read once.  Costs and their uint32 keys (elite_key; a
// non-finite cost and the pads K.. get kEliteNoKey) stay in registers for the whole kernel.
// Selection: a most-significant-digit-first radix select on the 32-bit keys, four passes of 8 bits.  A pass counts
// the keys that share the prefix found so far into a 256-bin LDS histogram with integer LDS adds (a count does not
// depend on the order of its adds; a thread merges a run of equal digits among its own keys into one add, which is
// what keeps the first pass -- sign and exponent, a handful of bins for any real cost distribution -- from
// serialising on one address: one add per key took 49.5 us at kMaxK where this takes 27), one barrier, and then EVERY
// wave reads the histogram (four bins per lane, one 16-B LDS read), scans it with a wave prefix sum and picks the bin
// the wanted rank falls into: all threads hold the same prefix and rank with a single barrier per pass.  Each pass has its own histogram (zeroed ahead of the first
// barrier), so no pass waits for the previous one's readers.  The first pass's total is n; after the fourth the
// prefix is the threshold key T and the remaining rank r is the number of keys equal to T that are admitted.
// The tie rule and the ascending-k compaction need, per sample, how many samples BEFORE it in index order are below T
// and how many equal T: elite <=> key < T or (key == T and equal-before < r), and its place in idx is
// below-before + min(equal-before, r).  With this ownership index order is (j, wave, lane, element), so the two
// exclusive counts come from ONE block scan, with no staging of the keys in LDS and no re-owning: per j a wave prefix
// sum of the lane's packed (below | equal << 16) count (at most 4096 per j: 16 bits hold it), the waves' totals to
// LDS, one barrier, and a second wave prefix sum over the (j, wave) totals in that order, unpacked to 32 bits.
// (Strided single-cost ownership k = tid + i nt would have needed one block scan per i; staging kMaxK keys in LDS,
// 128 KiB, would have cost a second pass over LDS and the block's residency for the same counts.)
// Nothing here is a float operation except the key's c + 0.0f; there are no global atomics; idx is written at
// positions computed from the scan, so it does not depend on scheduling and two runs are bitwise equal.
// NJ = 1: 39 VGPRs, NJ = 8: 124 VGPRs (32 costs + 32 keys; within the 128 that 16 waves per CU leave), no scratch;
// 4.1 / 4.5 KiB of LDS.  The kernel is bound by its dependent chain (load, four histogram-barrier-scan rounds, the
// block scan, the stores), not by throughput (DESIGN.md section 4 has the forms tried and their figures).
// ------------------------------------------------------------------------------------------------
constexpr int kEliteNJ = kMaxK / 4096;  // 16-B chunks per thread of the large form (1024 threads)
static_assert(kEliteNJ * 4096 == kMaxK && kEliteNJ * 16 <= 128, "the (j, wave) totals fill two entries per lane");

__device__ __forceinline__ unsigned wave_incl_scan(unsigned v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned t = __shfl_up(v, o);
    v += lane >= o ? t : 0u;
  }
  return v;
}

template <int NJ>
__global__ __launch_bounds__(1024) void elite_select_kernel(const float* __restrict__ costs, int K, int Kp,
                                                            int n_elite, float* __restrict__ ecost,
                                                            int32_t* __restrict__ idx, int32_t* __restrict__ count,
                                                            float* __restrict__ tau) {
  __shared__ __attribute__((aligned(16))) unsigned hist[4][256];
  __shared__ unsigned wtot[NJ * 16];  // entry j * 16 + wave: the wave's packed (below | equal << 16) total of chunk j
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, nt = blockDim.x;
  const float* c = costs + (long)b * Kp;
  float* eo = ecost + (long)b * Kp;
  int32_t* io = idx + (long)b * n_elite;
  const int nj = NJ == 1 ? 1 : (K + 4 * nt - 1) / (4 * nt);  // chunks in use (uniform; the host sizes 4 nt NJ >= K)

  for (int i = tid; i < 4 * 256; i += nt) (&hist[0][0])[i] = 0u;
  for (int i = tid; i < NJ * 16; i += nt) wtot[i] = 0u;

  // the owned costs, all loads in flight at once.  Kp is a multiple of 4 and the rows are 16-B aligned: a chunk that
  // starts below Kp lies inside the row
  float4 cv[NJ];
  unsigned key[NJ][4];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int p = 4 * (j * nt + tid);
    cv[j] = make_float4(INFINITY, INFINITY, INFINITY, INFINITY);
    if (j < nj && p < Kp) cv[j] = *reinterpret_cast<const float4*>(c + p);
    const float v[4] = {cv[j].x, cv[j].y, cv[j].z, cv[j].w};
#pragma unroll
    for (int e = 0; e < 4; ++e) key[j][e] = p + e < K ? elite_key_or_none(v[e]) : kEliteNoKey;
  }
  __syncthreads();  // the histograms are zero

  unsigned T = 0u, rank = 0u;
  int m = 0;
#pragma unroll
  for (int P = 0; P < 4; ++P) {
    constexpr int kBits = 8;
    const int shift = 24 - kBits * P;
    // this thread's keys under the prefix, runs of equal digits merged into one add
    unsigned cur = 0u, cnt = 0u;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      if (j < nj) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const unsigned k = key[j][e];
          bool act = k != kEliteNoKey;
          if (P > 0) act = act && (k >> (shift + kBits)) == (T >> (shift + kBits));
          const unsigned d = (k >> shift) & 255u;
          if (act) {
            if (cnt != 0u && d != cur) {
              atomicAdd(&hist[P][cur], cnt);
              cnt = 0u;
            }
            cur = d;
            cnt += 1u;
          }
        }
      }
    }
    if (cnt != 0u) atomicAdd(&hist[P][cur], cnt);
    __syncthreads();
    // every wave: the bin the rank falls into
    const uint4 h4 = *reinterpret_cast<const uint4*>(&hist[P][4 * lane]);
    const unsigned s = h4.x + h4.y + h4.z + h4.w;
    const unsigned incl = wave_incl_scan(s, lane);
    unsigned excl = incl - s;
    if (P == 0) {
      const int n = (int)__shfl(incl, 63);
      m = n_elite < n ? n_elite : n;
      rank = (unsigned)m;
      if (m == 0) break;  // (uniform) no finite cost
    }
    const bool mine = excl < rank && rank <= incl;  // exactly one lane (1 <= rank <= the pass's total)
    unsigned dg = 4u * lane, nr = rank - excl;
    if (nr > h4.x) {
      nr -= h4.x;
      dg += 1u;
      if (nr > h4.y) {
        nr -= h4.y;
        dg += 1u;
        if (nr > h4.z) {
          nr -= h4.z;
          dg += 1u;
        }
      }
    }
    const int src = __ffsll((unsigned long long)__ballot(mine)) - 1;
    T |= (unsigned)__shfl(dg, src) << shift;
    rank = (unsigned)__shfl(nr, src);
  }

  if (m == 0) {  // every ecost +inf, the set empty: the solve reports MPPI_E_NONFINITE as before
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int p = 4 * (j * nt + tid);
      if (j < nj && p < Kp) *reinterpret_cast<float4*>(eo + p) = make_float4(INFINITY, INFINITY, INFINITY, INFINITY);
    }
    for (int q = tid; q < n_elite; q += nt) io[q] = -1;
    if (tid == 0) {
      count[b] = 0;
      tau[b] = INFINITY;
    }
    return;
  }
  const unsigned r = rank;  // of the keys equal to T, the first r in index order are elite (r >= 1)

  // exclusive (below, equal) counts in index order: (j, wave, lane, element)
  unsigned lb[NJ], le[NJ];  // this lane's chunk j: the counts of the wave's lower lanes (below / equal)
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    unsigned pk = 0u;
#pragma unroll
    for (int e = 0; e < 4; ++e) pk += (key[j][e] < T ? 1u : 0u) + (key[j][e] == T ? 0x10000u : 0u);
    const unsigned incl = wave_incl_scan(pk, lane);  // (<= 256 per field)
    lb[j] = (incl - pk) & 0xFFFFu;
    le[j] = (incl - pk) >> 16;
    if (lane == 63 && j < nj) wtot[j * 16 + wv] = incl;
  }
  __syncthreads();
  // entries 2 lane and 2 lane + 1 of the (j, wave) totals; their exclusive prefix over the flattened order
  unsigned b0 = 0u, e0 = 0u, b1 = 0u, e1 = 0u;
  if (2 * lane < NJ * 16) {
    const unsigned w0 = wtot[2 * lane], w1 = wtot[2 * lane + 1];
    b0 = w0 & 0xFFFFu;
    e0 = w0 >> 16;
    b1 = w1 & 0xFFFFu;
    e1 = w1 >> 16;
  }
  const unsigned xb = wave_incl_scan(b0 + b1, lane) - (b0 + b1);
  const unsigned xe = wave_incl_scan(e0 + e1, lane) - (e0 + e1);
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int ent = j * 16 + wv, sl = ent >> 1;
    const unsigned pb = (unsigned)__shfl(xb, sl) + ((ent & 1) ? (unsigned)__shfl(b0, sl) : 0u);
    const unsigned pe = (unsigned)__shfl(xe, sl) + ((ent & 1) ? (unsigned)__shfl(e0, sl) : 0u);
    unsigned nb = pb + lb[j], ne = pe + le[j];  // below / equal strictly before this lane's chunk
    const int p = 4 * (j * nt + tid);
    const float v[4] = {cv[j].x, cv[j].y, cv[j].z, cv[j].w};
    float o[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const unsigned k = key[j][e];
      const bool below = k < T, equal = k == T;
      const bool elite = below || (equal && ne < r);
      o[e] = elite ? v[e] : INFINITY;
      if (elite) {
        const unsigned pos = nb + (ne < r ? ne : r);
        if (pos < (unsigned)n_elite) io[pos] = p + e;  // (pos < m by construction)
      }
      nb += below ? 1u : 0u;
      ne += equal ? 1u : 0u;
    }
    if (j < nj && p < Kp) *reinterpret_cast<float4*>(eo + p) = make_float4(o[0], o[1], o[2], o[3]);
  }
  for (int q = m + tid; q < n_elite; q += nt) io[q] = -1;
  if (tid == 0) {
    count[b] = m;
    tau[b] = elite_key_cost(T);
  }
}

hipError_t launch_elite_select(const float* costs, int B, int K, int Kp, int n_elite, float* ecost, int32_t* idx,
                               int32_t* count, float* tau, hipStream_t stream) {
  if (K < 1 || K > kMaxK || Kp < K || (Kp & 3) || n_elite < 1 || n_elite > K) return hipErrorInvalidValue;
  // lambda_search_kernel's sizing: four costs per thread in whole waves, then 1024 threads of up to 32
  int nt = ((K + 3) / 4 + 63) / 64 * 64;
  nt = nt > 1024 ? 1024 : nt;
  const bool small = 4L * nt >= K;  // K <= 4096
  auto kern = small ? elite_select_kernel<1> : elite_select_kernel<kEliteNJ>;
  hipLaunchKernelGGL(kern, dim3(B), dim3(nt), 0, stream, costs, K, Kp, n_elite, ecost, idx, count, tau);
  return hipGetLastError();
}

}  // namespace mppi
