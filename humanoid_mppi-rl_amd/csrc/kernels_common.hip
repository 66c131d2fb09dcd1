// Dynamics-independent MPPI kernels: device noise, softmin + weighted-noise reduce, U update/shift, trajectory
// logging (the analytic cartpole rollout: kernels_cartpole.hip).
//
// HBM layout (k fastest = "state-major", numpy's (nu,T,K) C order of src/cartpole_mppi.py:89):
//   noise [B][nu][H][Kp]   costs [B][Kp]   U/dU [B][nu][H]   x0 [B][nx]
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <algorithm>
#include "costs.h"
#include "gen_overlap.h"
#include "mppi_internal.h"
#include "philox.h"
#include "population.h"
#include "reduce_regen.h"
#include "wave_reduce.h"

namespace mppi {

// ------------------------------------------------------------------------------------------------
// a1: eps[b][u][t][k] = sigma * N(0,1) (Philox4x32-10, counter (k/4, t, u, b)); one thread = 4 consecutive k of one
// (b, u, t) row, one 16-B nontemporal store.  grid = (Kp/4/256 chunks, rows): no 64-bit div/mod per element.
// The kernel depends on nothing but the seed, so a captured stream of solves generates solve i+1's noise
// concurrently with solve i's rollout (mppi_api.hip, double-buffered).
// seed_ctr (MPPI_FLAG_SEED_COUNTER): key = seed + *seed_ctr.  The counter advances once per solve: in the reduce's
// last block for a plain solve, in bump_kernel right behind a graph's prefetched noise (mppi_api.hip).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void noise_kernel(float* __restrict__ noise, int rows, int nu, int H, int Kp,
                                                    uint64_t seed, const unsigned long long* seed_ctr, float sigma,
                                                    unsigned long long* key_out) {
  const int row = blockIdx.z * 65535 + blockIdx.y;  // (b*nu + u)*H + t
  const int kq = blockIdx.x * 256 + threadIdx.x;
  const uint64_t key = seed + (seed_ctr ? *seed_ctr : 0ull);
  // the key travels with the buffer (reduce_regen.h): one lane of one block
  if (key_out && row == 0 && kq == 0) *key_out = key;
  if (row < rows && 4 * kq < Kp) {
    const uint32_t k0 = (uint32_t)key, k1 = (uint32_t)(key >> 32);
    const int t = row % H;
    const int bu = row / H;
    const int u = bu % nu;
    const int b = bu / nu;
    float z[4];
    philox_normal4((uint32_t)kq, (uint32_t)t, (uint32_t)u, (uint32_t)b, k0, k1, z);
    typedef float f4 __attribute__((ext_vector_type(4)));
    f4 v = {sigma * z[0], sigma * z[1], sigma * z[2], sigma * z[3]};
    __builtin_nontemporal_store(v, reinterpret_cast<f4*>(noise + (long)row * Kp) + kq);
  }
}

__global__ void bump_kernel(unsigned long long* seed_ctr, long long delta) { *seed_ctr += (unsigned long long)delta; }

hipError_t launch_noise(float* noise, int B, int nu, int H, int Kp, uint64_t seed, const unsigned long long* seed_ctr,
                        float sigma, hipStream_t stream, unsigned long long* key_out) {
  const int rows = B * nu * H;
  const dim3 grid((Kp / 4 + 255) / 256, rows < 65535 ? rows : 65535, (rows + 65534) / 65535);
  hipLaunchKernelGGL(noise_kernel, grid, dim3(256), 0, stream, noise, rows, nu, H, Kp, seed, seed_ctr, sigma, key_out);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// a1 built to run BESIDE the rollout (mppi_api.hip chain_iter, gen_overlap.h): the same function of (seed + counter,
// b, u, t, k) as noise_kernel, bit for bit, with the same 16-B nontemporal stores -- shaped so that one of its waves
// fits into what two rollout waves leave of a SIMD's register file (kGenVgprs = 16 registers; fc_wave32_x3p_kernel
// holds 248 each).  One wave per block, no LDS; block i draws the whole rows [i rpb, (i + 1) rpb), a few us of work,
// and exits: not persistent, no spin, no flag, so a block placed ahead of a rollout block delays it by one block's run
// at most, and the register file itself holds the generator to one wave per SIMD while the rollout runs.
// For the register budget: the row (b, u, t), the key, the round keys and the uniform half of Philox's first two
// rounds (philox4x32_10_row) live in SGPRs, stepped -- not divided -- from row to row; the store is a buffer store
// against a resource over the block's own rows (uniform base, so the whole noise array may pass 4 GiB), the row and
// chunk as the scalar offset and the lane's 16-B offset as the one address register (the hardware drops what falls
// outside the block's rows); one quad is drawn and stored at a time: the loops are not unrolled, and q is opaque to
// the optimiser, which would otherwise carry q * 0xD2511F53 as a 64-bit induction variable per lane.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kGenWave) __attribute__((amdgpu_num_vgpr(kGenVgprs / 2)))  // (the target doubles it)
void noise_beside_kernel(float* __restrict__ noise, int rows, int nu, int H, int Kp, int rpb, uint64_t seed,
                         const unsigned long long* seed_ctr, float sigma, unsigned long long* key_out) {
  const int r0 = blockIdx.x * rpb;
  const int nr = min(rpb, rows - r0);
  if (nr <= 0) return;
  const uint64_t key = seed + (seed_ctr ? *seed_ctr : 0ull);
  // the key travels with the buffer (reduce_regen.h): one lane of one block, ahead of the loop's registers
  if (key_out && blockIdx.x == 0 && threadIdx.x == 0) *key_out = key;
  const uint32_t k0 = (uint32_t)key, k1 = (uint32_t)(key >> 32);
  const int bu = r0 / H;
  uint32_t t = (uint32_t)(r0 - bu * H), u = (uint32_t)(bu % nu), b = (uint32_t)(bu / nu);
  const uint32_t nq = (uint32_t)Kp >> 2, row_bytes = (uint32_t)Kp * 4u;
  typedef float f4 __attribute__((ext_vector_type(4)));
  typedef uint32_t u4 __attribute__((ext_vector_type(4)));
  // raw buffer (stride 0) over rows [r0, r0 + nr): 32-bit data format, offsets range-checked against its size
  const __amdgpu_buffer_rsrc_t rsrc =
      __builtin_amdgcn_make_buffer_rsrc(noise + (long)r0 * Kp, 0, (int)((uint32_t)nr * row_bytes), 0x00020000);
  const uint32_t lane_off = threadIdx.x * 16u;
  uint32_t row_off = 0;
#pragma unroll 1
  for (int i = 0; i < nr; ++i) {
#pragma unroll 1
    for (uint32_t q0 = 0; q0 < nq; q0 += kGenWave) {
      uint32_t q = q0 + threadIdx.x;
      asm volatile("" : "+v"(q));
      if (q < nq) {
        float z[4];
        philox_normal4_row(q, t, u, b, k0, k1, z);
        const f4 v = {sigma * z[0], sigma * z[1], sigma * z[2], sigma * z[3]};
        // (aux 2: the nontemporal policy, as noise_kernel's __builtin_nontemporal_store)
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u4, v), rsrc, (int)lane_off,
                                               (int)(row_off + q0 * 16u), 2);
      }
    }
    row_off += row_bytes;
    if (++t == (uint32_t)H) {
      t = 0;
      if (++u == (uint32_t)nu) {
        u = 0;
        ++b;
      }
    }
  }
}

int gen_rows_per_block() {
  // whole rows per block of noise_beside_kernel (MPPI_GEN_ROWS, read per launch: an A/B knob)
  if (const char* e = std::getenv("MPPI_GEN_ROWS")) return std::min(64, std::max(1, std::atoi(e)));
  return kGenRows;
}

hipError_t launch_noise_beside(float* noise, int B, int nu, int H, int Kp, uint64_t seed,
                               const unsigned long long* seed_ctr, float sigma, hipStream_t stream,
                               unsigned long long* key_out) {
  const long rows = (long)B * nu * H;
  const int rpb = gen_rows_per_block();
  // (a lane's offset in its block's rows is 32-bit; so is the grid)
  if (rows > 0x7fffffffL || (long)rpb * Kp * 4 > 0x7fffffffL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(noise_beside_kernel, dim3((unsigned)((rows + rpb - 1) / rpb)), dim3(kGenWave), 0, stream, noise,
                     (int)rows, nu, H, Kp, rpb, seed, seed_ctr, sigma, key_out);
  return hipGetLastError();
}

const void* noise_beside_func() { return reinterpret_cast<const void*>(noise_beside_kernel); }

hipError_t launch_seed_bump(unsigned long long* seed_ctr, long long delta, hipStream_t stream) {
  hipLaunchKernelGGL(bump_kernel, dim3(1), dim3(1), 0, stream, seed_ctr, delta);
  return hipGetLastError();
}


// a8 (update) + a9 (controller shift) for solve b, run by one block; in place (all reads before the barrier).
//   ADD: U = clamp(U + dU)   REPLACE: U = clamp(dU)   SHIFT: u0 = U[:,0]; U[:,t] = U[:,t+1]; U[:,H-1] = fill * U[:,H-1]
//   (src/cartpole_mppi.py:101-106)   U0_BEFORE: u0 = U_old[:,0] (src/quadruped_datacollection.py:170)
__device__ void update_solve(const SolveArgs& a, int b, float* su /* LDS, >= nu*H floats */) {
  const int rows = a.nu * a.H;
  float* U = a.U + (long)b * rows;
  float* dU = a.dU + (long)b * rows;
  const bool before = (a.flags & MPPI_FLAG_U0_BEFORE) != 0;
  __syncthreads();  // su may alias scratch the caller used
  for (int r = threadIdx.x; r < rows; r += blockDim.x) {
    const float old = U[r];
    const float d = __hip_atomic_load(dU + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // sc1: other blocks' rows
    float v = (a.update_mode == MPPI_UPDATE_REPLACE ? 0.0f : old) + d;
    if (a.U_clamp > 0.0f) v = fminf(a.U_clamp, fmaxf(-a.U_clamp, v));
    su[r] = v;
    const int t = r % a.H;
    if (t == 0 && a.u0) a.u0[(long)b * a.nu + r / a.H] = before ? old : v;
  }
  __syncthreads();
  const bool shift = (a.flags & MPPI_FLAG_SHIFT) != 0;
  for (int r = threadIdx.x; r < rows; r += blockDim.x) {
    const int t = r % a.H;
    float v = su[r];
    // after U[:, :-1] = U[:, 1:], the reference's U[:, -2] is the old last column: fill * su[t = H-1]
    if (shift) v = (t < a.H - 1) ? su[r + 1] : a.shift_fill * su[r];
    U[r] = v;
    if (a.Umirror) a.Umirror[(long)b * rows + r] = v;
  }
}

// ------------------------------------------------------------------------------------------------
// a7 + a8: softmin weights and dU[b][u][t] = sum_k w_k eps[b][u][t][k] / (sum_k w_k + eps_norm).
// grid = (row chunks, B), 512 threads (1024 for LOCAL and GEN). Every block recomputes beta and sum(w) for its solve from the
// K costs (<= 128 KiB, L2-resident) and stages w in LDS; then each wave streams whole noise rows
// with 16-B loads (the HBM-bound part: each noise element is read exactly once).
// References: src/cartpole_mppi.py:92-98, src/mppi.jl:87-94, src/cartpole_mppi_estimator.py:131-143.
// ------------------------------------------------------------------------------------------------
// GEN (graph streams): the same pass also generates the NEXT solve's noise rows into `gen.next` (same rows, same
// Philox counters as noise_kernel, key = gen.seed + *seed_ctr): the VALU-bound generation hides under the
// HBM-bound stream, and the next solve needs no noise launch.  The counter advances once every block of every
// solve has read it (the last solve to finish, global ticket).

// LOCAL (B*nu large enough to fill the chip with one u-row per block): block (u, b) owns the whole row U[b][u][:],
// so update + clamp + u0 + shift are block-local: no per-solve ticket, no sc1 re-read of dU (config #4: the ticketed
// tail cost ~2.3 us of a 16.6 us reduce).
// NT: nontemporal noise loads, for batches whose noise (> 128 MB) no longer sits in L2 / the Infinity Cache after the
// rollout read it (config #4 at 64 solves: 352 MB; step 0.5017 / 0.5032 -> 0.4918 / 0.4920 ms, same box; 8 solves,
// 44 MB: no change either way -- round 2 had measured nontemporal loads 2 us slower there)
// TWO (population-size decay, mppi_set_population; the extents and predicates: population.h): the next iteration samples
// another count, so its rows lie at another pitch, gen.Kp_next.  The wave's walk over a row then runs to the longer of
// the two rows: loads and fmas where q < nq -- the same quads in the same order as without TWO, so the sums are bit for
// bit those of the one-pitch form -- and generation where q < nq_next, the same counters, key, ticket and nontemporal
// stores into rows of Kp_next floats.  LDS holds w at the read pitch, as ever.  Without TWO every extent below is the
// constant it was and the instantiations compile to the code they had.
// REGEN (the read-only forms; the rule: reduce_regen.h): gen.regen eighths of the quads the pass would read are computed
// instead, gen.sigma * philox_normal4(q, t, u, b, *gen.regen_key) -- what the generator of this very noise stored, bit
// for bit -- into the registers the loads would have filled.  A row's tile loads its first slots, as ever, and computes
// its last regen_row_quads -- by the rule none or all of them: whole rows read, whole rows computed, other waves of the
// SIMD streaming meanwhile; the fmas over e and w follow in the one order there is.  Without REGEN the instantiations
// compile to the code they had.
// Its wide form holds two blocks of 16 waves per CU only at 64 registers or fewer: REGEN asks the compiler for 8 waves
// per SIMD (the others keep the 4 a block of 1,024 implies, and with it their code).
template <bool GEN, bool LOCAL, bool NT = false, bool TWO = false, bool REGEN = false>
__global__ __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(REGEN ? 8 : 4)))
void reduce_kernel(SolveArgs a, int rows_per_block, NoiseGen gen) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* w = smem;                // [max(Kp, nu*H)]
  float* red = smem + (a.Kp > a.nu * a.H ? a.Kp : a.nu * a.H);  // [40] scratch (2 per wave + the arrival flag)
  float* du_l = red + 40;         // LOCAL: dU of the block's rows [rows_per_block]
  const int b = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, nw = blockDim.x >> 6, nt = blockDim.x;
  const float* c = a.costs + (long)b * a.Kp;
  const int rows = a.nu * a.H;
  const int r0 = blockIdx.x * rows_per_block;
  const int r1 = min(rows, r0 + rows_per_block);
  typedef float f4 __attribute__((ext_vector_type(4)));
  const int nq = a.Kp >> 2;
  static_assert(!TWO || (GEN && !LOCAL), "the two-pitch form is the fused reduce + generate");
  const PopWalk walk = pop_walk(a.Kp, TWO ? gen.Kp_next : a.Kp);
  const int nq_gen = TWO ? walk.nq_next : nq, nq_walk = TWO ? walk.nq_walk : nq;
  const long gen_pitch = TWO ? (long)gen.Kp_next : (long)a.Kp;
  // each wave streams kRR rows at once, kRU quads per lane in flight per row (kRR * kRU 16-B loads outstanding)
  constexpr int kRR = 1, kRU = 4;
  static_assert(kRU == kPopTileQuads, "population.h restates the tile");
  static_assert(!(GEN && REGEN), "the fused reduce + generate has its vector ALUs taken");
  static_assert(!REGEN || (kRR == 1 && kRU == kRegenTileQuads), "reduce_regen.h restates the tile");
  f4 e[kRR][kRU];
  // (nre: the tile slots of row r that are regenerated, not loaded; wave-uniform, 0 without REGEN)
  auto issue = [&](int r, int q0, int nre) {
#pragma unroll
    for (int j = 0; j < kRU; ++j) {
      if constexpr (REGEN) {
        if (regen_slot(nre, j)) continue;
      }
      const int q = min(q0 + 64 * j, nq - 1);
#pragma unroll
      for (int i = 0; i < kRR; ++i) {
        // plain (cached) load while the rollout's read of this noise is still in L2 / the Infinity Cache (NT: the
        // large batches, where it is not)
        const f4* src = reinterpret_cast<const f4*>(a.noise + ((long)b * rows + min(r + i, r1 - 1)) * a.Kp) + q;
        if constexpr (NT)
          e[i][j] = __builtin_nontemporal_load(src);
        else
          e[i][j] = *src;
      }
    }
  };
  // the first tile of this wave's first rows does not depend on the weights: in flight during the softmin pass
  const int rfirst = r0 + wv * kRR;
  // REGEN: a wave's place in the alternation of an odd share, stepped from one of its rows to the next
  int alt = wv;
  if (rfirst < r1) issue(rfirst, lane, REGEN ? regen_row_quads(gen.regen, alt) : 0);
  uint32_t gk0 = 0, gk1 = 0;
  if constexpr (GEN) {
    const uint64_t key = gen.seed + *a.seed_ctr;
    gk0 = (uint32_t)key;
    gk1 = (uint32_t)(key >> 32);
  }
  if constexpr (REGEN) {  // the key THIS noise was drawn with, as its generator recorded it
    const uint64_t key = *gen.regen_key;
    gk0 = (uint32_t)key;
    gk1 = (uint32_t)(key >> 32);
  }
  // the tile's last nre slots of row r (quads q0 + 64 j) computed into e, beside the loads of its first ones
  auto regenerate = [&](int r, int q0, int nre) {
    const int u = r / a.H, t = r - u * a.H;
#pragma unroll
    for (int j = 0; j < kRU; ++j) {
      const int q = q0 + 64 * j;
      if (!regen_slot(nre, j) || q >= nq) continue;
      float z[4];
      philox_normal4((uint32_t)q, (uint32_t)t, (uint32_t)u, (uint32_t)b, gk0, gk1, z);
      e[0][j] = f4{gen.sigma * z[0], gen.sigma * z[1], gen.sigma * z[2], gen.sigma * z[3]};
    }
  };
  // next solve's noise for the tile (rows r, r+1; quads q0 + 64 j)
  auto generate = [&](int r, int q0) {
#pragma unroll
    for (int i = 0; i < kRR; ++i) {
      const int row = r + i;
      if (row >= r1) continue;
      const int u = row / a.H, t = row - u * a.H;
      f4* dst = reinterpret_cast<f4*>(gen.next + ((long)b * rows + row) * gen_pitch);
#pragma unroll
      for (int j = 0; j < kRU; ++j) {
        const int q = q0 + 64 * j;
        if (q >= nq_gen) continue;
        float z[4];
        philox_normal4((uint32_t)q, (uint32_t)t, (uint32_t)u, (uint32_t)b, gk0, gk1, z);
        __builtin_nontemporal_store(f4{gen.sigma * z[0], gen.sigma * z[1], gen.sigma * z[2], gen.sigma * z[3]},
                                    dst + q);
      }
    }
  };

  // beta = min over finite costs (non-finite -> +inf -> weight 0: the documented NaN guard)
  float m = INFINITY;
  for (int k = tid; k < a.K; k += nt) {
    const float ck = c[k];
    m = fminf(m, isfinite(ck) ? ck : INFINITY);
  }
  m = wave_min(m);
  if (lane == 0) red[wv] = m;
  __syncthreads();
  float beta = red[0];
  for (int i = 1; i < nw; ++i) beta = fminf(beta, red[i]);
  __syncthreads();
  const float inv_lam = 1.0f / (a.lambda_dev ? a.lambda_dev[b] : a.lambda);  // (ESS targeting: the solve's own)
  float s = 0.0f;
  for (int k = tid; k < a.Kp; k += nt) {
    float wk = 0.0f;
    if (k < a.K) {
      const float ck = c[k];
      wk = (isfinite(ck) && beta < INFINITY) ? __expf(-inv_lam * (ck - beta)) : 0.0f;
    }
    w[k] = wk;
    s += wk;
  }
  s = wave_sum(s);
  if (lane == 0) red[nw + wv] = s;
  __syncthreads();
  float S = 0.0f;
  for (int i = 0; i < nw; ++i) S += red[nw + i];  // fixed order: deterministic
  const float inv_S = 1.0f / (S + a.norm_eps);
  if (blockIdx.x == 0) {
    if (a.weights)
      for (int k = tid; k < a.Kp; k += nt) a.weights[(long)b * a.Kp + k] = w[k] * inv_S;
    if (tid == 0 && !(beta < INFINITY)) atomicOr(a.status, 1u);
  }

  const f4* w4 = reinterpret_cast<const f4*>(w);
  for (int r = rfirst; r < r1; r += nw * kRR, ++alt) {
    float acc[kRR];
#pragma unroll
    for (int i = 0; i < kRR; ++i) acc[i] = 0.0f;
    const int nre = REGEN ? regen_row_quads(gen.regen, alt) : 0;
    for (int q0 = lane; q0 < nq_walk; q0 += 64 * kRU) {
      // (the first tile is already in flight; TWO: past the read row's end there is nothing to load)
      if ((r != rfirst || q0 != lane) && (!TWO || q0 < nq)) issue(r, q0, nre);
      if constexpr (GEN) generate(r, q0);  // VALU work while the tile's loads are in flight
      if constexpr (REGEN) regenerate(r, q0, nre);  // likewise
#pragma unroll
      for (int j = 0; j < kRU; ++j) {
        if (q0 + 64 * j < nq) {
          const f4 ww = w4[q0 + 64 * j];
#pragma unroll
          for (int i = 0; i < kRR; ++i) {
            acc[i] = fmaf(e[i][j].x, ww.x, acc[i]);
            acc[i] = fmaf(e[i][j].y, ww.y, acc[i]);
            acc[i] = fmaf(e[i][j].z, ww.z, acc[i]);
            acc[i] = fmaf(e[i][j].w, ww.w, acc[i]);
          }
        }
      }
    }
#pragma unroll
    for (int i = 0; i < kRR; ++i) {
      const float sum = wave_sum(acc[i]);
      // write-through (sc1) store: visible to the last-arriving block of this solve without a release fence
      if (lane == 0 && r + i < r1) {
        if constexpr (LOCAL) du_l[r + i - r0] = sum * inv_S;
        __hip_atomic_store(a.dU + (long)b * rows + r + i, sum * inv_S, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }

  if constexpr (LOCAL) {  // a8/a9 on the block's own u-row(s) [r0, r1) (whole rows: r0 % H == 0, r1 % H == 0)
    __syncthreads();        // du_l complete, w dead
    float* su = w;
    const bool before = (a.flags & MPPI_FLAG_U0_BEFORE) != 0, shift = (a.flags & MPPI_FLAG_SHIFT) != 0;
    float* U = a.U + (long)b * rows;
    for (int r = r0 + tid; r < r1; r += nt) {
      const float old = U[r];
      float v = (a.update_mode == MPPI_UPDATE_REPLACE ? 0.0f : old) + du_l[r - r0];
      if (a.U_clamp > 0.0f) v = fminf(a.U_clamp, fmaxf(-a.U_clamp, v));
      su[r - r0] = v;
      const int u = r / a.H;
      if (r - u * a.H == 0 && a.u0) a.u0[(long)b * a.nu + u] = before ? old : v;
    }
    __syncthreads();
    for (int r = r0 + tid; r < r1; r += nt) {
      const int t = r % a.H;
      const float v = shift ? ((t < a.H - 1) ? su[r + 1 - r0] : a.shift_fill * su[r - r0]) : su[r - r0];
      U[r] = v;
      if (a.Umirror) a.Umirror[(long)b * rows + r] = v;
    }
    if (tid == 0) {
      if (blockIdx.x == 0 && b == 0 && a.seed_bump) atomicAdd(a.seed_bump, 1ull);  // noise kernel done: stream order
    }
    static_assert(!(GEN && LOCAL), "graph streams use the ticketed update");
    return;
  }

  // ---- a8/a9 fused: the last block to finish solve b applies the update + shift (guide G16, sc1 counter
  // form: sc1 payload stores drained by every storing wave, block barrier, one relaxed agent ticket; the last
  // arriver reads every dU row with sc1 loads, so no release/acquire fences). Ticket reset for the next solve.
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  // the arrival flag lives in the dynamic LDS scratch (a static __shared__ would shift the 16-B-aligned base)
  unsigned* last_flag = reinterpret_cast<unsigned*>(red + 2 * nw);
  if (tid == 0) {
    const unsigned prev = __hip_atomic_fetch_add(a.tickets + b, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    *last_flag = (prev == gridDim.x - 1) ? 1u : 0u;
  }
  __syncthreads();
  if (!*last_flag) return;
  update_solve(a, b, w);  // w (softmin weights) is dead here; the LDS region holds max(Kp, nu*H) floats
  if (tid == 0) {
    __hip_atomic_store(a.tickets + b, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // next solve's noise key (plain solves; this solve's noise kernel has completed: stream order)
    if (b == 0 && a.seed_bump) atomicAdd(a.seed_bump, 1ull);
    if constexpr (GEN) {  // every block of every solve has read the counter: advance it once
      if (__hip_atomic_fetch_add(gen.gticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.y - 1) {
        __hip_atomic_store(gen.gticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned long long ctr = atomicAdd(a.seed_ctr, 1ull);
        // the key travels with the buffer it was drawn into (reduce_regen.h): the counter every block read, from the
        // one lane that advances it
        if (gen.key_out) *gen.key_out = gen.seed + ctr;
      }
    }
  }
}

constexpr bool kReduceLocal = true;

hipError_t launch_reduce(const SolveArgs& a, const NoiseGen* gen, hipStream_t stream, bool gen_block,
                         const RegenArgs* regen) {
  const int rows = a.nu * a.H;
  // the read-only forms that regenerate a share of what they would read (reduce_regen.h; the caller applied the rule)
  const bool re = regen && regen->eighths > 0;
  if (re && (gen || !regen->key || regen->eighths > kRegenMaxEighths)) return hipErrorInvalidValue;
  // ~256 blocks of 8 waves in total (1 per CU), each wave streaming one row at a time with 4 16-B loads in flight
  // per lane (same-box sweep over rows x loads x block count on configs #4 and #5: 1 x 4 x 256 best by ~1 %)
  // Enough rows per block to amortise each block's softmin pass over the K costs.
  const bool nt = (double)a.B * rows * a.Kp * 4.0 > 128.0 * 1024 * 1024;  // noise past what the caches keep
  // The read-only pass of the overlap route (gen_block) over such a batch -- config #4 at 64 solves, 352 MB -- is
  // bandwidth-bound with nothing to hide under it: the ticketed form on 512 blocks of 16 waves, two per CU and all
  // resident in one round, 168 rows each (LOCAL's 1,344 blocks of 64 rows run in 2.6 rounds, each block with its own
  // softmin prologue and update tail: 68.5 us; ticketed 256 / 512 / 1024 blocks: step 0.5034 / 0.5017 / 0.5107 ms
  // against LOCAL's 0.5102-0.5165, the kernel 59.1 us at 512 = 6.0 TB/s; same box).  Same bits.
  const bool wide = gen_block && nt;
  int target = wide ? 512 : 256;
  if (const char* e = std::getenv("MPPI_REDUCE_BLOCKS")) target = std::max(1, std::atoi(e));  // (A/B knob)
  int rpb = (rows * a.B + target - 1) / target;
  rpb = rpb < 1 ? 1 : rpb;
  // plain solves with enough solves x controls for one u-row per block to fill the chip: block-local update
  // (LOCAL; config #4: 16.9 -> 13.9 us).  Graph streams keep the ticketed form: their next-noise generation wants
  // the wider grid (LOCAL + GEN: step 117.8 -> 120.7 us, same box).
  // MPPI_REDUCE_LOCAL=0 (read per launch; an A/B knob): the ticketed form where LOCAL would run
  const int local_knob = env_flag("MPPI_REDUCE_LOCAL");  // (1: LOCAL also where the wide ticketed form would run)
  const bool local = kReduceLocal && !gen && a.B * a.nu >= 128 && local_knob != 0 && (!wide || local_knob == 1);
  if (local) rpb = a.H;
  const dim3 grid((rows + rpb - 1) / rpb, a.B);
  const size_t lds = (size_t)((a.Kp > a.nu * a.H ? a.Kp : a.nu * a.H) + 40 + (local ? rpb : 0)) * sizeof(float);
  // population-size decay: the next iteration's rows at another pitch take the two-pitch form; equal pitches, as ever,
  // the one-pitch kernel
  const bool two = gen && gen->Kp_next != 0 && gen->Kp_next != a.Kp;
  auto kern = gen ? (two ? (nt ? reduce_kernel<true, false, true, true> : reduce_kernel<true, false, false, true>)
                         : (nt ? reduce_kernel<true, false, true> : reduce_kernel<true, false>))
                  : (local ? (nt ? reduce_kernel<false, true, true> : reduce_kernel<false, true>)
                           : (nt ? reduce_kernel<false, false, true> : reduce_kernel<false, false>));
  if (re)
    kern = local ? (nt ? reduce_kernel<false, true, true, false, true> : reduce_kernel<false, true, false, false, true>)
                 : (nt ? reduce_kernel<false, false, true, false, true>
                       : reduce_kernel<false, false, false, false, true>);
  if (lds > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)lds);
    if (e != hipSuccess) return e;
  }
  // 16 waves per block for LOCAL (fewer blocks: one per u-row) and for GEN (more waves for the VALU-bound
  // generation: config #5 step 53.0 -> 52.0 ms, config #4 -0.5 %, same box).  gen_block: the read-only pass of a chained
  // solve whose next noise is generated beside the rollout keeps GEN's block, so the softmin sum is partitioned over
  // the same threads and the solve is bit for bit the fused route's whichever route a solve takes
  NoiseGen g = gen ? *gen : NoiseGen{nullptr, 0, 0.0f, nullptr, 0};
  if (re) {
    g.sigma = regen->sigma;
    g.regen = regen->eighths;
    g.regen_key = regen->key;
  }
  hipLaunchKernelGGL(kern, grid, dim3(local || gen || gen_block ? 1024 : 512), lds, stream, a, rpb, g);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// Trajectory logging (mppi_graph_capture_traj): copy x_t [B][nx] and u_t [B][nu] into the log before the env
// step advances x.  Its own tiny launch, so the rollout kernels carry no logging code.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void record_kernel(const float* __restrict__ x, const float* __restrict__ u,
                                                     float* __restrict__ rx, float* __restrict__ ru, int nxB, int nuB) {
  for (int i = blockIdx.x * 256 + threadIdx.x; i < nxB + nuB; i += gridDim.x * 256) {
    if (i < nxB) rx[i] = x[i];
    else ru[i - nxB] = u[i - nxB];
  }
}

hipError_t launch_record(const float* x, const float* u, float* rx, float* ru, int nxB, int nuB, hipStream_t s) {
  hipLaunchKernelGGL(record_kernel, dim3((nxB + nuB + 255) / 256), dim3(256), 0, s, x, u, rx, ru, nxB, nuB);
  return hipGetLastError();
}

}  // namespace mppi
