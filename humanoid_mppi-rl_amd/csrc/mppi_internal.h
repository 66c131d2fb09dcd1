// Internal structures shared by the C-ABI host code (mppi_api.hip) and the kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdlib>
#include <cstring>

#include "../../include/mppi.h"

struct NoiseAdapt;  // noise_adapt.h: the settings of mppi_set_noise_adapt
struct EssTarget;   // ess_target.h: the settings of mppi_set_ess_target
struct NoiseCovAdapt;  // noise_cov_adapt.h: the settings of mppi_set_noise_cov_adapt
struct StepAdapt;      // step_law.h: the settings of mppi_set_noise_steps_adapt

namespace mppi {

constexpr int kWave = 64;
constexpr int kKpAlign = 64;       // device pitch of the K axis (noise rows, costs)
constexpr int kMaxK = 32768;       // softmin weights are staged in LDS (<= 128 KiB)
constexpr int kMaxNx = 64;         // fc-stack state slots (4 m-tiles of 16)
constexpr int kMaxNu = 32;         // fc-stack control slots (2 m-tiles of 16)

// Everything a solve's kernels need, passed by value (kernel arguments live in SGPRs / constant
// cache; no per-call device allocation, so a solve can be captured into a hipGraph).
struct SolveArgs {
  int B, nx, nu, H, K, Kp;
  float lambda, ctrl_clamp, U_clamp, norm_eps, shift_fill, terminal_weight;
  int update_mode, flags, cost_kind;
  float ctx_default[MPPI_CTX_MAX];
  const float* x0;      // [B][nx]
  float* U;             // [B][nu][H]   (read by rollout, updated in place by the update kernel)
  float* noise;         // [B][nu][H][Kp]
  float* costs;         // [B][Kp]
  float* dU;            // [B][nu][H]   weighted-noise sums (normalised)
  float* weights;       // [B][Kp] or nullptr
  float* u0;            // [B][nu] or nullptr
  const float* ctx;     // [B][MPPI_CTX_MAX] or nullptr (-> ctx_default)
  unsigned* status;     // [1] bit0: some solve had no finite cost
  unsigned* tickets;    // [B] reduce-block arrival counters (zero between solves)
  float* xout;          // [B][nx] or nullptr: rollouts write the final state of sample k = 0 (env step)
  float* Umirror;       // [B][nu][H] or nullptr: the update also writes the new U here (RESIDENT_U + io.U, device)
  unsigned long long* seed_ctr;   // or nullptr: noise key = seed + *seed_ctr
  unsigned long long* seed_bump;  // or nullptr: the reduce advances this counter after the solve (plain solves)
  // analytic cartpole: per-block softmin partials [B][Kp/256][2 + H] (block min, block weight sum, weighted noise
  // rows); non-null = the rollout finishes the solve itself (fused epilogue, no reduce launch)
  float* part;
  // or nullptr: device wall-clock stamps of this rollout launch (mppi_kernel_clock), [kClockSlots][2] =
  // {earliest block start, latest block end}; slot = *kclock_ctr at the block's start
  unsigned long long* kclock;
  unsigned long long* kclock_ctr;  // stamped launches since the reset (advanced by the launch's last block)
  unsigned* kclock_ticket;         // block arrivals of the current stamped launch (zero between launches)
  // ESS targeting (mppi_set_ess_target): [B] the solve's own lambda, written by lambda_search_kernel ahead of the
  // reduce; nullptr (every handle that never enables it): `lambda` above.  Last, so no other field moves.
  const float* lambda_dev;
};

// Rollout launch clock (mppi_kernel_clock): every block's leader folds its start / end stamps (s_memrealtime,
// the constant-rate device wall clock) into the launch's slot with global atomic min / max, so the launch duration
// (first block start -> last block end) is measured inside a timed region, graph replays included, with no event
// in the stream.  The slot is the clock's own launch counter, read at the block's start; the launch's LAST
// arriving block (a ticket over the whole grid) advances it, so no block of the launch can see it move whatever
// the order in which the hardware dispatches the blocks.  Three vector atomics per block: nothing measurable
// against a rollout of >= 10 us.
constexpr int kClockSlots = 65536;
struct KClock {
  unsigned long long t0;
  unsigned slot;
};
__device__ __forceinline__ KClock kclock_begin(const SolveArgs& a) {
  if (!a.kclock) return KClock{0ull, 0u};
  return KClock{(unsigned long long)wall_clock64(), (unsigned)(*a.kclock_ctr & (kClockSlots - 1))};
}
// leader: the ONE thread per block that stamps (the block's thread 0 after the block's last barrier by default).
// INVARIANT: every block of a stamped launch calls kclock_record exactly once with exactly one leader, after all of
// its work (no early exit past it, no second leader): the launch counter advances only when the ticket counts every
// block of the grid, and a launch that broke this would leave it behind, folding all later launches into one slot.
// mppi_kernel_clock_read checks the device counter against the host's count of stamped launches and fails loudly.
__device__ __forceinline__ void kclock_record(const SolveArgs& a, const KClock& c, bool leader = threadIdx.x == 0) {
  if (a.kclock && leader) {
    unsigned long long* s = a.kclock + 2 * c.slot;
    atomicMin(s, c.t0);
    atomicMax(s + 1, (unsigned long long)wall_clock64());
    const unsigned nblk = gridDim.x * gridDim.y * gridDim.z;
    if (__hip_atomic_fetch_add(a.kclock_ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == nblk - 1) {
      __hip_atomic_store(a.kclock_ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      atomicAdd(a.kclock_ctr, 1ull);
    }
  }
}

// Analytic cartpole constants (models/cartpole.xml; derivation in oracle/mppi_ref.py::_cartpole_params).
struct CartpoleParams {
  float m_cart, m_pole, l, inertia, damping, gear, ctrl_lo, ctrl_hi, g, dt;
};

// Learned-dynamics (fc stack) network description after folding + packing (mppi_nets.cpp).
enum FcArch : int { kArchNone = 0, kArchCA = 1, kArchMLP = 2, kArchGeneric = 3 };
// bf16 fc rollouts: layers (bit l = layer l) whose per-wave A fragments live in VGPRs for the whole horizon; the
// packer puts the others first, as the LDS-staged image prefix.  All layers: no weight traffic in the loop.
constexpr int kCaRegMask = 0x7;   // folded CA: 3 layers
// Folded CA, bf16 image: layer 0's bias also sits in the (zero) pad state slots 28 and 29 as a bf16 hi / lo pair, so
// a kernel whose layer-0 operand holds 1.0 in those slots gets h = W0 x + b0 from the MFMA alone (fc_pipe_kernel);
// kernels that keep the slots at 0 add the fp32 bias as before.
constexpr int kCaBiasSlotHi = 28, kCaBiasSlotLo = 29;
// ... and beta' of the folded LayerNorm as a bf16 hi / lo pair in the pad columns 30 (hi), 31 (lo) and 59 (hi again):
// an operand holding (s_hi, s_hi, s_lo) there adds beta' s (to ~2^-18) for the per-wave kernel's s = sqrt(var + eps)
constexpr int kCaBetaSlotHi0 = 30, kCaBetaSlotLo = 31, kCaBetaSlotHi1 = 59;
// ... and fc_wave32_kernel's block-diagonal layer 0 (w32_bd): the qvel-fed rows' b0 pair in pad slots 60, 61 (1.0 in
// the state) and their beta' pair in 62, 63 (against s_hi); row 30 of its Gram factor is the row mean of layer 0
constexpr int kCaBdBiasSlotHi = 60, kCaBdBiasSlotLo = 61, kCaBdBetaSlotHi = 62, kCaBdBetaSlotLo = 63;
constexpr int kCaBdMeanRow = 30;
// ... and the split per-wave image's layer 0 (L0x): a column of 1.0 in pad slots 29 (qpos rows) and 61 (qvel rows),
// against which fc_wave32_x3p_kernel's operand carries -mu (hi / lo), so the row mean leaves through the MFMA
constexpr int kCaX3MeanSlot = 29, kCaX3BdMeanSlot = 61;
// ... and, for its fp16 form (one fp16 operand, fc_common.h x3_f16_on), -mu's lo part against a second column of 1.0
constexpr int kCaX3MeanLoSlot = 31, kCaX3BdMeanLoSlot = 63;
// ... and the fp16-form M-split kernel fc_rollout_kernel_x3h: layer 0's bias in this pad column (against a state slot
// held at 1.0), so h = W0 x + b0 leaves the MFMA chain with no bias read (needs qpos <= 31)
constexpr int kCaX3hBiasSlot = 31;
#ifndef MPPI_X3_F16_L0  // the fp16 form's layer 0 and statistic: fp16 W hi + lo against one fp16 operand (1), or the
                        // bf16 three products (0); the packer (mppi_nets.cpp) and the per-wave kernels agree on it
#define MPPI_X3_F16_L0 1
#endif
constexpr int kMlpRegMask = 0xF;  // MLP(hidden 128, 2 hidden layers): 4 layers
// MLP, bf16 image: layer 0's bias as a bf16 hi / lo pair in the pad state columns 62, 63 (when nx <= 62), for the
// per-wave kernel whose state holds 1.0 there; the M-split kernel keeps those slots at 0 and adds the fp32 bias
constexpr int kMlpBiasSlotHi = 62, kMlpBiasSlotLo = 63;

// Generic fc stack (kernels_fc_generic.hip): any MLPStatePredictor (hidden width, depth, eval-mode BatchNorm folded)
// and any CrossAttentionStatePredictor (qpos / qvel / hidden; folded) that the shape-specialised kernel does not take.
// Layer 0 reads [x (nx) ; u (nu) ; 0] padded to kin[0]; layer l writes mt[l] 16-row tiles; the last layer's rows are
// the state deltas.  Fragments packed by mppi_nets.cpp::pack_frags (16x32, [mt][kb][lane]).
constexpr int kGenMaxLayers = 16;
constexpr int kGenMaxWidth = 1024;  // widest layer (padded); fp32 parity mode: 512
struct FcGenNet {
  int nl = 0;
  int kin[kGenMaxLayers] = {0};    // padded input width of layer l (multiple of 32)
  int mt[kGenMaxLayers] = {0};     // output 16-row tiles of layer l
  int w_off[kGenMaxLayers] = {0};  // packed fragments of layer l
  int b_off[kGenMaxLayers] = {0};  // fp32 bias of layer l (16 mt[l] floats)
  int relu_mask = 0;               // bit l: ReLU after layer l
  int lnb_off = -1;                // >= 0: layer 0 is followed by the folded LayerNorm (CA): beta' (16 mt[0] floats)
  int ln_n = 0;                    // true LayerNorm width
  int maxw = 0;                    // widest activation row (padded to 32)
};

// The packed image of an fc-stack net as the kernels take it (a kernel argument, by value): plain ints and one pointer.
// Byte offsets inside the image (identical layout for the LDS copy and global reads), filled by the packer
// (mppi_nets.cpp); img is set when the image is uploaded.  -1: that part is not built (other shapes or precisions).
struct FcArgs {
  const char* img = nullptr;       // device copy of the packed image
  int lds_bytes = 0;               // bf16: prefix of the image staged in LDS (the other layers live in VGPRs)
  int w_off[4] = {0, 0, 0, 0};     // per-layer packed weight fragments
  int b_off[4] = {0, 0, 0, 0};     // per-layer fp32 bias (padded rows)
  int lnb_off = 0;                 // beta' of the LayerNorm after layer 0, folded (fp32; gamma lives in layer 1)
  int ln_n = 0;                    // true LayerNorm width (pads excluded)
  // state slots: x[0, qp) -> slots [0, qp); x[qp, qp+qv) -> slots [32, 32+qv) (CA: qpos | qvel).
  int qp = 0, qv = 0;
  int groups_per_block = 1;        // set by the M-split launchers (the only non-offset field a kernel reads)
  // folded humanoid CA, bf16: the per-wave rollout (kernels_fc_wave.hip) also needs the layer-0 Gram matrix of the
  // bf16 columns as hi / lo bf16 fragments (G_hi at g_off, G_lo at g_off + 8 KiB) and beta' as bf16 hi / lo in the pad
  // state columns kCaBetaSlotHi0/Lo/Hi1 of layer 0
  int g_off = -1;
  int wave = 0;                    // the image carries what the per-wave kernel needs (CA: g_off, beta'; MLP: the b0 pair)
  int w32_off = -1;                // ... and the CA layers + Gram factor as 32x32x16 A fragments (fc_wave32_kernel)
  int w32_bd = 0;                  // ... with layer 0 block-diagonal, uncentred (the mean from the Gram factor's row 30):
                                   // 1 = 112 MFMAs per wave-step, 2 = 108 (qpos rows' bias via the accumulators); 0 = dense
  int w0bd_off = -1, gbd_off = -1;  // form 2 for fc_wave_kernel (16x16): its layer 0 and Gram factor as 16x32 fragments
  int w32x3_off = -1, w32x3_l1lo_off = -1;  // split bf16 per-wave image (fc_wave32_x3_kernel): LDS part, W1 lo part
  int wmx3_off = -1, wmx3_lo_off = -1;      // split bf16 per-wave MLP image (fc_wave_mlp_x3_kernel): LDS part, W1|W2 lo
  int wm32x3_off = -1, wm32x3_lo_off = -1;  // ... 32 samples per wave (fc_wave32_mlp_x3_kernel): LDS part, W1|W2 lo
  // the split CA's fp16 form (fc_route.h x3_f16_on): fc_wave32_x3p_kernel's image (the w32x3 LDS image in fp16),
  int w32f16_off = -1;
  int wmf16_off = -1, wmf16_x_off = -1;  // ... the M-split kernels' (fc_rollout_kernel_x3d<F16>): W1, the last layer,
  int wmf16_0_off = -1;                  //     layer 0 (fp16 hi / lo)
  int wmf16_0b_off = -1;                 //     ... with b0 in the pad column kCaX3hBiasSlot (fc_rollout_kernel_x3h)
};

struct FcNet {
  int arch = kArchNone;
  FcGenNet gen;                    // arch == kArchGeneric
  int precision = MPPI_PREC_BF16;
  FcArgs fa;                       // arch == kArchCA / kArchMLP: the packed image
  int img_bytes = 0;               // size of the packed image (what mppi_load_dynamics uploads; no kernel reads it)
  int reg_mask = 0;                // layers packed after the LDS prefix (kCaRegMask / kMlpRegMask)
  // Host-only state, read by fc_route (fc_route.h), never by a kernel.  Split bf16 (MPPI_PREC_BF16X3) CA only: products
  // on layer 1 as decided for THIS net by the engine's probe (mppi_api.hip x3_probe: the two- and three-product
  // rollouts of the first solve's own states against each other); 0 = not probed yet (three products), 2 = the probe
  // stayed within kX3ProbeTol, 3 = it did not
  int x3_l1 = 0;
  float x3_l1_err = -1.0f;         // the probe's max relative cost difference (-1: no probe ran)
  // ... and the fp16 form: the probe's decision (0 = not probed, 1 = within kX3ProbeTol, -1 = not; 2 = the opt-in
  // one-product last layer, x3_f16_l2x1) and difference
  int x3_f16 = 0;
  float x3_f16_err = -1.0f;
};

// CU count of the CURRENT device (the launchers size persistent grids by it), cached per device id: a process that
// drives several GPUs gets each one's own count.  Thread-safe (relaxed atomics; a race only repeats the query).
int current_device_cus();

// The launchers' environment knobs (read per launch; A/B and test knobs).  env_flag: NAME=0|1 -> 0 / 1, anything else
// (unset included) -> -1, the launcher's own default.  env_choice: NAME=<one>|<two> -> 1 / 2, anything else -> 0.
inline int env_flag(const char* name) {
  const char* e = std::getenv(name);
  if (!e || (e[0] != '0' && e[0] != '1') || e[1] != '\0') return -1;
  return e[0] - '0';
}
inline int env_choice(const char* name, const char* one, const char* two) {
  const char* e = std::getenv(name);
  if (!e) return 0;
  return std::strcmp(e, one) == 0 ? 1 : (std::strcmp(e, two) == 0 ? 2 : 0);
}

// The rollout kernel the last fc / FA / cartpole launch on this host thread routed to (mppi_rollout_kernel): set by
// every launcher, read by the ABI right after the launch (a handle is used from one thread).
extern thread_local const char* g_rollout_kernel;
// ... and its device function where the launcher knows it (fc_launch; nullptr otherwise): the register count of the
// routed kernel decides whether the next noise can be generated beside it (gen_overlap.h)
extern thread_local const void* g_rollout_func;
inline void note_kernel(const char* name) {
  g_rollout_kernel = name;
  g_rollout_func = nullptr;
}

// FeatureAttentionStatePredictor (learning/model.py:48-153) rollout. Blocking shared by the host packer and the
// kernel: 4 heads; attention is processed in chunks of fa_cw(D) columns (whole heads), the FFN hidden layer in
// chunks of fa_fc(D) rows; a workgroup has fa_nw(D) waves and kFaRows token rows.
// Up to 5 token n-tiles (80 rows: the full humanoid state + action, 76 tokens, learning/model.py:215), up to 8
// attention layers (learning/train.py:72 trains 7), 4 or 8 heads (num_heads, learning/train.py:72: 8).
constexpr int kFaRows = 80;
constexpr int kFaMaxLayers = 8;
constexpr int kFaHeads = 4;  // the small-net kernel: one head per wave
__host__ __device__ constexpr int fa_nt_min(int L) { return L <= 16 ? 1 : (L <= 32 ? 2 : (L <= 64 ? 4 : 5)); }
// attention chunk width (whole heads of width D / NH): 5 token tiles, and hidden 128 with 8 heads (8 probability
// tiles per chunk otherwise), take 64-wide chunks to fit the LDS
__host__ __device__ constexpr bool fa_narrow(int D, int NH, int NT) { return NT > 4 || (D == 128 && NH == 8); }
__host__ __device__ constexpr int fa_cw(int D, int NH = 4, int NT = 4) {
  return fa_narrow(D, NH, NT) ? (D / NH > 64 ? D / NH : 64) : (D / NH >= 128 ? D / NH : (D < 128 ? D : 128));
}
// waves per workgroup: 8 for wide nets; hidden 128 with 64-wide chunks takes 4 (its Q|K|V tiles split evenly)
__host__ __device__ constexpr int fa_nw(int D, int NT = 4, int NH = 4) {
  return D >= 128 && !(D == 128 && fa_narrow(D, NH, NT)) ? 8 : 4;
}
__host__ __device__ constexpr int fa_fc(int D) { return D >= 512 ? 256 : (4 * D < 512 ? 4 * D : 512); }

struct FaNet {
  int D = 0, L = 0, nlayers = 0, nh = 4, precision = MPPI_PREC_BF16;
  // fp32 vectors (byte offsets into the image)
  int we = 0, be = 0, ge = 0, bte = 0, pos = 0, wout = 0;
  int ln1g[kFaMaxLayers], ln1b[kFaMaxLayers], bqkv[kFaMaxLayers], bo[kFaMaxLayers];
  int ln2g[kFaMaxLayers], ln2b[kFaMaxLayers], b1[kFaMaxLayers], b2[kFaMaxLayers];
  // packed A-operand fragments (chunked, see mppi_nets.cpp::build_fa_net)
  int wqkv[kFaMaxLayers], wo[kFaMaxLayers], w1[kFaMaxLayers], w2[kFaMaxLayers];
  // small-net kernel (bf16, D = 64, L <= 16: kernels_fa.hip::fa_small_kernel): per-head Q|K|V and the FFN matrices
  // with the register-operand k order; small = 0: not built
  int small = 0;
  int s_wqkv[kFaMaxLayers], s_w1[kFaMaxLayers], s_w2[kFaMaxLayers];
  int s_c1 = 0, s_c2 = 0;  // encoding: (w - mean w) gamma, (b - mean b) gamma (fp32 vectors)
  int s_bqkv[kFaMaxLayers], s_b1[kFaMaxLayers];  // biases of the LayerNorm-folded Q|K|V and FFN1 (fp32 vectors)
  // closed-form LayerNorm statistics of the scalar feature encoding h = w v + b (population moments over D)
  float enc_mw = 0, enc_mb = 0, enc_vw = 0, enc_cwb = 0, enc_vb = 0, b_out = 0;
  // hidden 512, bf16: the layer-by-layer path (kernels_fa_layered.hip) reads every matrix as plain row-major bf16
  // [out][in] (Q rows pre-scaled by 1/sqrt(head dim)) and the Q|K|V bias in natural order; lay = 0: not built
  int lay = 0;
  int lwqkv[kFaMaxLayers], lwo[kFaMaxLayers], lw1[kFaMaxLayers], lw2[kFaMaxLayers], lbqkv[kFaMaxLayers];
  int img_bytes = 0;
  void* d_img = nullptr;
  // ... and its activation workspace (fa_layered_ws_bytes), allocated by mppi_load_dynamics for max_batch * K * L
  // token rows; nullptr: the fused fa_rollout_kernel runs
  void* d_ws = nullptr;
  long ws_rows = 0;
};

// Launchers (return hipSuccess or the launch error). All enqueue on `stream` only.
// device noise into noise[B][nu][H][Kp]; seed_ctr (or nullptr): device key offset
// key_out (or nullptr): the device word that receives the key the noise was drawn with, seed + *seed_ctr, written by
// one lane of one block (reduce_regen.h: the reduce that regenerates part of this noise reads the key from there)
hipError_t launch_noise(float* noise, int B, int nu, int H, int Kp, uint64_t seed, const unsigned long long* seed_ctr,
                        float sigma, hipStream_t stream, unsigned long long* key_out = nullptr);
hipError_t launch_seed_bump(unsigned long long* seed_ctr, long long delta, hipStream_t stream);  // += delta
// the same noise as launch_noise from the kernel built to run beside the rollout (noise_beside_kernel; gen_overlap.h)
hipError_t launch_noise_beside(float* noise, int B, int nu, int H, int Kp, uint64_t seed,
                               const unsigned long long* seed_ctr, float sigma, hipStream_t stream,
                               unsigned long long* key_out = nullptr);
const void* noise_beside_func();  // (for hipFuncGetAttributes: the fit rule of gen_overlap.h)
// The sampling law (mppi_set_noise_model; noise_model.h), a kernel argument by value: no device allocation, so a
// solve that generates with it stays graph-capturable.  active = 0: the default law (white noise of cfg.sigma, the
// fused generators); active = 1: eps = sigma_u[u] * AR(1)(rho) from noise_ar1_kernel (kernels_noise.hip), nu <= kMaxNu.
struct NoiseModel {
  int active = 0;
  float rho = 0.0f;
  float c = 1.0f;  // sqrtf(1 - rho*rho), fp32, computed on the host
  float sigma_u[kMaxNu] = {0};
  // the knot law (mppi_set_noise_knots; noise_knots.h): n_knots = 0: off; else the noise is drawn at n_knots knots and
  // interpolated through the table (device memory the setter owns: kidx [H][4], kw [H][4])
  int n_knots = 0, order = 0;
  const int32_t* kidx = nullptr;
  const float* kw = nullptr;
  // the cross-actuator covariance (mppi_set_noise_cov; noise_cov.h): nullptr: off; else the factor L [nu][kMaxNu] (device
  // memory the setter owns) that mixes the unit-variance AR(1) rows; sigma_u is then sqrt(diag Sigma) and not read
  const float* cov_L = nullptr;
  // the horizon basis (mppi_set_noise_basis; noise_basis.h): n_basis = 0: off; else eps = sigma_u M z over n_basis white
  // normals per (b, u, k); basis_T (device memory the setter owns) is M transposed, [basis_rows_padded(n_basis)]
  // [basis_pitch(H)]: the pad of every row zero (the coefficients of 16 consecutive steps and one r are one aligned
  // load), the rows past n_basis -0.0f (the MFMA form mixes four r at a time; a product of -0 adds nothing to a chain)
  int n_basis = 0;
  const float* basis_T = nullptr;
};
constexpr int kBasisTile = 16;  // steps noise_basis_kernel mixes per pass over the normals: the pitch's granule
constexpr int basis_pitch(int H) { return (H + kBasisTile - 1) / kBasisTile * kBasisTile; }
constexpr int basis_rows_padded(int R) { return (R + 3) / 4 * 4; }  // rows of basis_T: the MFMA form mixes four r at a time
// every explicit generation site: noise_kernel (inactive model, sigma) or, with the model active, noise_ar1_kernel /
// noise_ar1_lds_kernel (grids too small to fill the chip), noise_knot_kernel (a knot law), noise_basis_kernel (a horizon
// basis) or noise_cov_kernel (a cross-actuator covariance); kernels_noise.hip.  d_law (or nullptr): the device law of
// a handle that adapts it on the stream (mppi_set_noise_adapt) -- the same generators reading sigma_u, rho and c from
// device memory instead of the by-value model (noise_ar1_dev_kernel / noise_ar1_lds_dev_kernel).  d_steps (or nullptr):
// the table of per-step scales S [B][nu][H] of mppi_set_noise_steps (device memory the setter owns, moved on the stream
// by step_adapt_kernel) -- the same two generators reading their scale per step from it, rho and c from the model
// (noise_ar1_steps_kernel / noise_ar1_lds_steps_kernel); never beside d_law, a knot law, a basis or a covariance.
// key_out: launch_noise's, passed on with an inactive model only (no other generator's noise can be regenerated)
hipError_t launch_noise_model(float* noise, int B, int nu, int H, int Kp, uint64_t seed,
                              const unsigned long long* seed_ctr, float sigma, const NoiseModel& model,
                              hipStream_t stream, const float* d_law = nullptr, const float* d_steps = nullptr,
                              unsigned long long* key_out = nullptr);
// The device law [kLawFloats] = sigma_u[kMaxNu], rho, c: set from a by-value model on the stream, and moved one step
// by the rule of noise_adapt.h from one statistics slot (stats [B], m2 / m11 [B][nu]) after the law the solve drew
// from was recorded into hist[0..nu] (sigma_u, rho).  One wave each; capturable.
constexpr int kLawRho = kMaxNu, kLawC = kMaxNu + 1, kLawFloats = kMaxNu + 2;
hipError_t launch_noise_law_set(float* d_law, const NoiseModel& model, hipStream_t stream);
hipError_t launch_noise_adapt(float* d_law, float* hist, const mppi_solve_stats* stats, const float* m2,
                              const float* m11, int B, int nu, const NoiseAdapt& a, hipStream_t stream);
// The device covariance of a handle that adapts it (mppi_set_noise_cov_adapt): Sigma [nu][nu], the factors where the
// generator and the control-cost term read them (L [nu][kMaxNu], Sinv [nu][nu]), sqrt of the diagonal [kMaxNu] and the
// count of rejected steps.  noise_cov_adapt_kernel records Sigma into hist [nu][nu], then moves all of it one step by
// the rule of noise_cov_adapt.h from one slot of statistics (stats [B]) and cross moments (mx [B][nu][nu]).  One block;
// capturable.
struct CovLaw {
  float* S;
  float* L;
  float* Sinv;
  float* sigma_u;
  unsigned long long* rejects;
};
hipError_t launch_noise_cov_adapt(const CovLaw& law, float* hist, const mppi_solve_stats* stats, const float* mx,
                                  int B, int nu, const NoiseCovAdapt& a, hipStream_t stream);
// fc-stack rollout: fc_route (fc_route.h) decides the kernel from the shape, the image, the probe outcomes and the
// knobs; launch_fc_route launches a given route (the engine's probe passes routes of its own)
struct FcRoute;
hipError_t launch_fc_rollout(const SolveArgs& a, const FcNet& net, hipStream_t stream);
hipError_t launch_fc_route(const SolveArgs& a, const FcNet& net, const FcRoute& route, hipStream_t stream);
hipError_t launch_fc_generic(const SolveArgs& a, const FcNet& net, hipStream_t stream);  // kernels_fc_generic.hip

// LDS layout (bytes) of one block of the generic fc-stack kernel: activation rows A0 | A1 ([16][maxw] of E-byte
// elements, +16 B per row), the LayerNorm layer's fp32 raw rows, the fp32 state [16][nx], the fp32 controls of two
// steps [2][16][nu], the per-wave LayerNorm partial sums [4][16].
struct GenLay {
  int A0, A1, SCR, XS, UF, ST, total;
  __host__ __device__ GenLay(const FcGenNet& g, int E, int nx, int nu) {
    const int act_s = g.maxw * E + 16;
    A0 = 0;
    A1 = A0 + 16 * act_s;
    SCR = A1 + 16 * act_s;
    XS = SCR + (g.lnb_off >= 0 ? 16 * g.maxw * 4 : 0);
    UF = XS + 16 * nx * 4;
    ST = UF + 2 * 16 * (nu > 0 ? nu : 1) * 4;
    total = (ST + 4 * 16 * 4 + 15) / 16 * 16;
  }
};
inline int fc_generic_lds_bytes(const FcGenNet& g, int precision, int nx, int nu) {
  return GenLay(g, precision == MPPI_PREC_BF16 ? 2 : 4, nx, nu).total;
}
hipError_t launch_fa_rollout(const SolveArgs& a, const FaNet& net, hipStream_t stream);
// kernels_fa_layered.hip: the layer-by-layer hidden-512 rollout and its workspace size for `rows` token rows
hipError_t launch_fa_layered(const SolveArgs& a, const FaNet& net, hipStream_t stream);
size_t fa_layered_ws_bytes(long rows);
// reduce_kernel<GEN>: also writes the next solve's noise (graph streams)
struct NoiseGen {
  float* next;
  uint64_t seed;
  float sigma;
  unsigned* gticket;  // [1], zero between solves
  // the pitch of `next`'s rows where it differs from the pitch the reduce reads (mppi_set_population: the next
  // iteration samples another count); 0: the read pitch.  Last, so no other field moves
  int Kp_next = 0;
  // ... and behind it: the device word that receives the key `next` is drawn with (or nullptr), as launch_noise's
  unsigned long long* key_out = nullptr;
  // reduce_kernel<REGEN> (reduce_regen.h; never beside `next`): the eighths of the noise it READS that are regenerated
  // instead of loaded, from the key in *regen_key -- the word the generator of that noise wrote -- and `sigma`
  int regen = 0;
  const unsigned long long* regen_key = nullptr;
};
// The reduce that regenerates part of the noise it reads (reduce_regen.h): eighths in 1..7 and the noise's key word
struct RegenArgs {
  int eighths = 0;
  const unsigned long long* key = nullptr;
  float sigma = 0.0f;
};
hipError_t launch_reduce(const SolveArgs& a, const NoiseGen* gen, hipStream_t stream,  // softmin + reduce + update + shift
                         bool gen_block = false,  // (gen_block: no generation, reduce_kernel<GEN>'s block size)
                         const RegenArgs* regen = nullptr);  // (never beside gen)
// analytic cartpole rollout; with a.part set it also runs a7-a9 (fused epilogue) and, given gen, writes the next
// solve's noise (graph streams)
hipError_t launch_cartpole_rollout(const SolveArgs& a, const CartpoleParams& p, const NoiseGen* gen, hipStream_t stream);
// Solve diagnostics (kernels_stats.hip; MPPI_FLAG_STATS, mppi_stats_eval), by value like SolveArgs: read-only on the
// solve's costs and noise, so the launches can sit in a captured graph.
struct StatsArgs {
  int B, nu, H, K, Kp;
  float lambda, norm_eps;
  const float* costs;       // [B][Kp]
  const float* noise;       // [B][nu][H][Kp], or nullptr: only the struct is computed
  float* w;                 // [B][Kp] scratch: the normalised softmin weights (pads 0)
  float* part;              // [stats_part_floats] scratch: the moment kernel's per-cell partial sums
  mppi_solve_stats* stats;  // [B] out
  float* m2;                // [B][nu] out
  float* m11;               // [B][nu] out
  const float* lambda_dev;  // [B] the solve's own lambda (ESS targeting), or nullptr: `lambda`
};
size_t stats_part_floats(int B, int nu, int H, int Kp);
hipError_t launch_stats(const StatsArgs& a, hipStream_t stream);  // cost part, moment part, fixed-order finish
// Weighted cross moments (kernels_cross.hip; MPPI_FLAG_CROSS, mppi_cross_moments_eval; the definition: cross_moments.h),
// by value like StatsArgs and behind its launches, whose weights they read; nu <= kMaxNu.
struct CrossArgs {
  int B, nu, H, Kp;
  const float* w;      // [B][Kp] the normalised softmin weights stats_cost_kernel wrote (pads 0)
  const float* noise;  // [B][nu][H][Kp]
  float* part;         // [cross_part_floats] scratch: the per-cell partial sums, [B][pair][cell]
  float* mx;           // [B][nu][nu] out
};
size_t cross_part_floats(int B, int nu, int H, int Kp);
hipError_t launch_cross(const CrossArgs& a, hipStream_t stream);  // moment part, fixed-order finish
// Weighted per-step moments (kernels_step_moments.hip; MPPI_FLAG_STEP_MOMENTS, mppi_step_moments_eval; the definition:
// step_moments.h), by value like StatsArgs and behind its launches, whose weights they read.
struct StepMomArgs {
  int B, nu, H, Kp;
  const float* w;      // [B][Kp] the normalised softmin weights stats_cost_kernel wrote (pads 0)
  const float* noise;  // [B][nu][H][Kp]
  float* m1;           // [B][nu][H] out
  float* m2;           // [B][nu][H] out
};
hipError_t launch_step_moments(const StepMomArgs& a, hipStream_t stream);
// The refit of the per-step scales (mppi_set_noise_steps_adapt; the rule: step_law.h): S [B][nu][H] in place from one
// slot of statistics (stats [B]) and per-step moments (m1, m2 [B][nu][H]); shift: the row moves with the nominal and
// its last cell becomes fill.sigma_u[u].  One wave per row; capturable; nu <= kMaxNu.
struct StepFill {
  float sigma_u[kMaxNu];
};
hipError_t launch_step_adapt(float* S, const float* m1, const float* m2, const mppi_solve_stats* stats, int B, int nu,
                             int H, int shift, const StepAdapt& a, const StepFill& fill, hipStream_t stream);
// kernels_lambda.hip: per solve b, lambda_out[b] = the lambda in [lambda_min, lambda_max] at which costs [B][Kp] give
// the target effective sample size (the rule: ess_target.h); one block per solve, read-only on the costs, capturable
hipError_t launch_lambda_search(const float* costs, int B, int K, int Kp, const EssTarget& s, float cfg_lambda,
                                float* lambda_out, hipStream_t stream);
// kernels_elite.hip: elite truncation (mppi_set_elites; the rule: elite_select.h).  Per solve b, from costs [B][Kp]:
// ecost [B][Kp] = the cost on the n_elite best finite samples (ties by ascending k), +inf elsewhere and on the pads;
// idx [B][n_elite] the set in ascending k, -1 behind its count [B]; tau [B] its threshold.  One block per solve, one
// launch, read-only on the costs, capturable.  1 <= n_elite <= K
hipError_t launch_elite_select(const float* costs, int B, int K, int Kp, int n_elite, float* ecost, int32_t* idx,
                               int32_t* count, float* tau, hipStream_t stream);
// kernels_elite_keep.hip: keep / shift elites (mppi_set_elite_keep; the rule: elite_keep.h), by value like SolveArgs, so
// the launches can sit in a captured graph.  The stored set of solve b: v [nu][H][pitch] (pitch = n_keep rounded up to
// 4), kcost / idx [n_keep], count, steps.
struct KeepArgs {
  int B, nu, H, K, Kp;
  int n_keep, pitch;
  float clamp;               // cfg.ctrl_clamp (<= 0: none; the gather only)
  float* noise;              // [B][nu][H][Kp] the gather reads it as the rollout saw it; the injection writes it in place
  const float* U;            // [B][nu][H] the nominal: the one the rollout perturbed (gather) / will perturb (injection)
  const float* costs;        // [B][Kp] what the selection ran on (gather only)
  const int32_t* sel_idx;    // [B][n_keep] the selection's set in ascending k, -1 behind its count (gather only)
  const int32_t* sel_count;  // [B] (gather only)
  float* v;                  // [B][nu][H][pitch] the gather's output / the injection's input
  float* kcost;              // [B][n_keep] out (gather only)
  int32_t* idx;              // [B][n_keep] out (gather only)
  int32_t* count;            // [B] gather: out; injection: in, read on the device
  int32_t* steps;            // [B] likewise
};
inline int keep_pitch(int n_keep) { return (n_keep + 3) / 4 * 4; }
hipError_t launch_keep_gather(const KeepArgs& a, int shift, hipStream_t stream);  // v, kcost, idx, count, steps
hipError_t launch_keep_inject(const KeepArgs& a, hipStream_t stream);  // eps = v - U on columns < count, rows < steps
// kernels_iter.hip: inner iterations per control step (mppi_set_iterations; the tracking's rule: iter_best.h), by value
// like SolveArgs, so the launches can sit in a captured graph.  The stored best of solve b: bv [nu][H], bcost, bk, biter.
struct IterBestArgs {
  int B, nu, H, K, Kp;
  int reset;             // 1: the step's first iteration (the stored best is not read)
  int it;                // the iteration's index within its step
  float clamp;           // cfg.ctrl_clamp (<= 0: none)
  const float* costs;    // [B][Kp] the selection's input: the unmasked end of the wcost chain
  const float* noise;    // [B][nu][H][Kp] as the rollout saw it
  const float* U;        // [B][nu][H] the nominal the rollout perturbed
  float* bv;             // [B][nu][H] in/out
  float* bcost;          // [B] in/out
  int32_t* bk;           // [B] out
  int32_t* biter;        // [B] out
};
hipError_t launch_iter_best(const IterBestArgs& a, hipStream_t stream);
// u0 [B][nu] <- bv[b][u][0] where bk[b] >= 0
hipError_t launch_iter_apply(const float* bv, const int32_t* bk, float* u0, int B, int nu, int H, hipStream_t stream);
// noise[b][u][t][j0] <- +0.0, j0 = count[b] in [0, n_keep] (count == nullptr: 0); j0 >= K: nothing
hipError_t launch_iter_mean(float* noise, const int32_t* count, int n_keep, int B, int nu, int H, int K, int Kp,
                            hipStream_t stream);
// kernels_ctrl_cost.hip: the control-cost term (mppi_set_control_cost; the rule for lin: control_cost.h), by value
// like SolveArgs: read-only on the solve's U, noise and costs, so the launches can sit in a captured graph.
struct CtrlLaw {
  float gamma, sigma, rho;  // sigma: every actuator's (per_u == 0: the default law, cfg.sigma with rho 0)
  int per_u;                // sigma_u below is the law's (an active noise model: nu <= kMaxNu)
  float sigma_u[kMaxNu];
};
struct CtrlArgs {
  int B, nu, H, K, Kp;
  const float* U;       // [B][nu][H] the nominal the rollout perturbed
  const float* noise;   // [B][nu][H][Kp] the raw eps
  const float* costs;   // [B][Kp]
  float* lin;           // [B][nu][H] out
  float* term;          // [B][Kp] out (pads K..Kp: 0)
  float* wcost;         // [B][Kp] out: costs + term (pads K..Kp: costs)
  float* part;          // [term_part_floats (term_cells.h)] scratch: the split form's per-cell partial sums
  CtrlLaw law;
  const float* d_law;   // the device law [kLawFloats] of an adapting handle, or nullptr: `law`
  const float* sinv;    // Sigma^-1 [nu][nu] of a cross-actuator covariance (mppi_set_noise_cov), or nullptr: per actuator
};
hipError_t launch_ctrl_cost(const CtrlArgs& a, hipStream_t stream);  // lin, then the term and wcost (one of two forms)
// kernels_bounds.hip: per-actuator control bounds (mppi_set_control_bounds; the rule: ctrl_bounds.h), by value like
// SolveArgs (the box travels as a kernel argument: nu <= kMaxNu), so the launches can sit in a captured graph.
struct BoundsArgs {
  int B, nu, H, K, Kp;
  float* noise;         // [B][nu][H][Kp] projected in place (launch_bounds_project only)
  const float* U;       // [B][nu][H] the nominal the rollout will perturb (launch_bounds_project only)
  unsigned* part;       // [B nu H][bounds_chunks(Kp)] the projection's counts per row and 256-k chunk (scratch)
  unsigned* counts;     // [B][nu] out: the (t, k < K) elements projected (launch_bounds_clip sums part)
  float lo[kMaxNu], hi[kMaxNu];
};
int bounds_chunks(int Kp);  // 256-k chunks of a noise row
hipError_t launch_bounds_project(const BoundsArgs& a, hipStream_t stream);  // the projection; part written
// counts from part; U [B][nu][H] (or nullptr: the counts alone), Umirror (or nullptr: no copy) and u0 [B][nu] (or
// nullptr) clipped to the box
hipError_t launch_bounds_clip(const BoundsArgs& a, float* U, float* Umirror, float* u0, hipStream_t stream);
// kernels_rate_cost.hip: the control-rate cost term (mppi_set_rate_cost; the rule: rate_cost.h), by value like
// SolveArgs (the weights travel as a kernel argument: nu <= kMaxNu), read-only on the solve's U, noise and costs, so
// the launches can sit in a captured graph.
struct RateArgs {
  int B, nu, H, K, Kp;
  int anchor;           // 1: t = 0 differences against u_prev
  float clamp;          // cfg.ctrl_clamp (<= 0: none)
  const float* U;       // [B][nu][H] the nominal the rollout perturbed
  const float* noise;   // [B][nu][H][Kp] the noise as the rollout saw it
  const float* u_prev;  // [B][nu] the control applied the step before (read with anchor only)
  const float* costs;   // [B][Kp] what the term is added to: the rollout's costs, or costs + control-cost term
  float* term;          // [B][Kp] out (pads K..Kp: 0)
  float* wcost;         // [B][Kp] out: costs + term (pads K..Kp: costs)
  float* part;          // [term_part_floats (term_cells.h)] scratch: the split form's per-cell partial sums
  float r[kMaxNu];
};
hipError_t launch_rate_cost(const RateArgs& a, hipStream_t stream);  // the term and wcost (one of two forms)
hipError_t launch_rate_store_prev(const float* u0, float* u_prev, int n, hipStream_t stream);  // u_prev <- u0 [n]
// kernels_ensemble.hip: the members' costs of a dynamics-model ensemble combined per sample (mppi_set_ensemble; the rule:
// ensemble.h), by value like SolveArgs, so the launch can sit in a captured graph.
struct EnsembleArgs {
  int n;                 // members, 2..MPPI_ENS_MAX
  int mode;              // MPPI_ENS_*
  float kappa;
  float r;               // ensemble_rcp(n), computed on the host
  long n4;               // B Kp / 4: the lanes' count (the rows of one member are dense)
  long stride;           // floats between member e's and member e + 1's rows (a multiple of 4, >= B Kp)
  const float* members;  // [n][stride]
  float* costs;          // [B][Kp] out
  float* sd;             // [B][Kp] out
};
hipError_t launch_ensemble(const EnsembleArgs& a, hipStream_t stream);
hipError_t launch_record(const float* x, const float* u, float* rx, float* ru, int nxB, int nuB, hipStream_t stream);

}  // namespace mppi
