// C-ABI of the MPPI engine (include/mppi.h): handle lifecycle, device buffers, the solve pipeline
// (noise -> rollout -> reduce -> update) on one HIP stream, layout conversion at the boundary,
// per-kernel hipEvent timing, thread-local error strings. Never throws across the ABI.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "costs.h"
#include "ctrl_bounds.h"  // ctrl_bounds_valid
#include "elite_keep.h"  // (the rule of mppi_set_elite_keep)
#include "elite_select.h"  // (the rule of mppi_set_elites)
#include "ensemble.h"  // (the rule of mppi_set_ensemble)
#include "ess_target.h"  // EssTarget
#include "gen_overlap.h"  // the rule that routes the next noise beside the rollout
#include "reduce_regen.h"  // the rule by which the read-only reduce regenerates part of the noise it sums
#include "fc_route.h"  // fc_route, x3_l1_terms, kX3ProbeTol (the split CA's probe)
#include "mppi_internal.h"
#include "rate_cost.h"  // rate_cost_valid
#include "term_cells.h"  // term_part_floats
#include "noise_adapt.h"  // NoiseAdapt
#include "noise_cov.h"    // cov_factor
#include "noise_cov_adapt.h"  // NoiseCovAdapt
#include "noise_basis.h"  // basis_law_valid
#include "noise_knots.h"  // knot_table
#include "noise_model.h"  // ar1_innovation_scale
#include "population.h"  // the rule of mppi_set_population
#include "step_law.h"  // StepAdapt

namespace mppi {
std::vector<unsigned char> build_fc_net(int kind, const void* blob, size_t nbytes, int precision, int nx, int nu,
                                        FcNet& net);
std::vector<unsigned char> build_fa_net(const void* blob, size_t nbytes, int precision, int nx, int nu, FaNet& net);
int fa_lds_bytes(int D, int precision, int nh, int L);
}

using namespace mppi;

static thread_local std::string g_err;

static int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

#define HIP_TRY(expr)                                                                                        \
  do {                                                                                                       \
    hipError_t e_ = (expr);                                                                                  \
    if (e_ != hipSuccess) return fail(MPPI_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));       \
  } while (0)

namespace {

enum KernelId {
  kNoise = 0,
  kRollout = 1,
  kReduce = 2,
  kUpdate = 3,
  kStats = 4,
  kLambda = 5,
  kCtrl = 6,
  kBounds = 7,
  kRate = 8,
  kElites = 9,
  kKeep = 10,
  kCross = 11,
  kCovAdapt = 12,
  kStepMom = 13,
  kStepAdapt = 14,
  kIter = 15,
  kEnsemble = 16,
  kNumKernels = 17
};
const char* kKernelNames[kNumKernels] = {"noise", "rollout", "reduce", "update", "stats", "lambda", "ctrl_cost",
                                         "bounds", "rate_cost", "elites", "keep", "cross", "cov_adapt", "step_mom",
                                         "step_adapt", "iter", "ensemble"};

struct PendingEvt {
  int id;
  hipEvent_t a, b;
  int n;  // what the group adds to the kernel's count (0: its time joins a group already counted)
};

// Which options a solve carries (solve_opts: from the handle's settings and the solve's flags).  enqueue_solve
// launches by it, note_ran records by it, and a captured graph keeps the one it was captured under.
struct SolveOpts {
  bool stats = false;   // MPPI_FLAG_STATS
  bool cross = false;   // MPPI_FLAG_CROSS
  bool cov_adapt = false;  // mppi_set_noise_cov_adapt
  bool adapt = false;   // mppi_set_noise_adapt
  bool ess = false;     // mppi_set_ess_target
  bool ctrl = false;    // mppi_set_control_cost
  bool bounds = false;  // mppi_set_control_bounds
  bool rate = false;    // mppi_set_rate_cost
  bool elite = false;   // mppi_set_elites
  bool keep = false;    // mppi_set_elite_keep
  bool step_mom = false;    // MPPI_FLAG_STEP_MOMENTS
  bool step_adapt = false;  // mppi_set_noise_steps_adapt
  bool iter = false;        // mppi_set_iterations: the best sample of the step is tracked
  bool ens = false;         // mppi_set_ensemble: n rollouts and the combining launch
};

}  // namespace

struct mppi_handle {
  mppi_config cfg{};
  int device = 0;
  int Kp = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  int dyn_kind = 0;
  int cost_kind = 0;
  float cost_params[MPPI_CTX_MAX] = {0};
  CartpoleParams cart{};
  FcNet net;
  // MPPI_PREC_BF16X3 only: the same net packed for exact fp32, which the env step runs (launch_rollout): its output is
  // the next STATE, and the split forms are fp32-accurate in the costs (what x3_probe measures), not entry by entry
  FcNet net_env;
  FaNet fa;
  // device buffers (sized for cfg.max_batch)
  float *d_x0 = nullptr, *d_U = nullptr, *d_noise = nullptr, *d_costs = nullptr, *d_dU = nullptr;
  float *d_weights = nullptr, *d_u0 = nullptr, *d_ctx = nullptr;
  unsigned* d_status = nullptr;
  unsigned* d_tickets = nullptr;
  float* d_part = nullptr;        // analytic cartpole: per-block softmin partials of the fused epilogue
  unsigned long long* d_seed_ctr = nullptr;
  float *d_env_noise = nullptr, *d_env_costs = nullptr;  // env step (zero noise, cost scratch)
  unsigned* d_env_status = nullptr;
  // graph mode: noise double buffer (d_noise, d_noise2); solve i's reduce also generates solve i+1's noise
  // (reduce_kernel<GEN>).  One exec per start parity of the buffer pair.
  float* d_noise2 = nullptr;
  unsigned* d_gticket = nullptr;
  hipGraphExec_t graph_exec[2] = {nullptr, nullptr};
  int graph_B = 0, graph_n = 0, graph_parity = 0;
  SolveOpts graph_opts;         // the options the captured graph's solves carry
  bool prefetch_valid = false;  // d_noise / d_noise2 [graph_parity] holds the next launch's first noise
  int prefetch_B = 0;           // ... generated for this batch and seed (graph launches and chained solves)
  uint64_t prefetch_seed = 0;
  bool capturing = false;       // enqueue_solve is recording a graph (launches are counted at replay)
  uint64_t graph_seed = 0;
  std::vector<float> Uhost;  // column-major U staging between enqueue and finish
  // profiling
  bool prof = false;
  std::vector<PendingEvt> pending;
  std::vector<hipEvent_t> evt_pool;
  long prof_count[kNumKernels] = {0};
  double prof_ms[kNumKernels] = {0};
  std::vector<float> staging;
  // device launch clock of the rollouts (mppi_kernel_clock): [kClockSlots][2] {first block start, last block end}
  unsigned long long* d_kclock = nullptr;
  bool kclock = false;        // stamp rollouts enqueued (or captured) from now on
  bool graph_kclock = false;  // the captured graph stamps its rollouts
  long kclock_launches = 0;   // stamped rollout launches since the last reset
  // chained solves with the next solve's noise generated CONCURRENTLY with this solve's rollout (gen_overlap.h): a
  // low-priority generator stream running noise_beside_kernel + the counter bump, ordered by events against the solve
  // stream
  hipStream_t gstream = nullptr;
  hipEvent_t ev_gen = nullptr;  // the generator's last launch done (the noise the next rollout reads is written)
  hipEvent_t ev_red = nullptr;  // the solve stream's last reduce done (the buffer it read may be overwritten)
  hipEvent_t ev_switch = nullptr;  // mppi_set_stream: the old stream's tail, waited on by the new one
  bool gen_pending = false;     // ev_gen guards the prefetched noise: the solve stream must wait on it before use
  int gen_route = kGenRouteNone;  // where the last solve's next noise was generated (mppi_gen_route)
  // The reduce that regenerates part of the noise it reads (reduce_regen.h).  d_nkey [2]: the key each noise buffer
  // (d_noise, d_noise2) was drawn with, written on the device by the kernel that drew it.  pristine [2], the content side
  // of the rule, kept on the host: the buffer holds exactly what the plain i.i.d. generator wrote for that key, for B
  // solves at pitch Kp -- set where such a generator is enqueued, cleared wherever anything else writes the buffer
  unsigned long long* d_nkey = nullptr;
  struct Pristine {
    bool ok = false;
    int B = 0, Kp = 0;
  } pristine[2];
  int reduce_regen = 0;  // the eighths the last solve's reduce regenerated (mppi_reduce_regen)
  std::vector<std::pair<const void*, int>> func_regs;  // hipFuncGetAttributes numRegs per kernel, read once each
  const char* rollout_kernel = "";  // the kernel the last solve's rollout was routed to (mppi_rollout_kernel)
  NoiseModel noise_model;  // the sampling law (mppi_set_noise_model); inactive = white noise of cfg.sigma
  // solve diagnostics (MPPI_FLAG_STATS; kernels_stats.hip), allocated by ensure_stats before the first flagged solve or
  // capture.  Outputs are slot-major with max_batch as the batch pitch: stats_slots slots for solves (a graph's solve i
  // writes slot i) and one more, the last, for mppi_stats_eval, so an evaluation leaves a solve's statistics readable.
  mppi_solve_stats* d_stats = nullptr;              // [stats_slots + 1][max_batch]
  float *d_stats_m2 = nullptr, *d_stats_m11 = nullptr;  // [stats_slots + 1][max_batch][nu]
  float *d_stats_w = nullptr, *d_stats_part = nullptr;  // scratch: normalised weights [max_batch][Kp], cell partials
  int stats_slots = 0;
  int stats_B = 0, stats_n = 0;  // batch and slot count of the last flagged solve / graph launch (0: none ran)
  // the weighted cross moments (MPPI_FLAG_CROSS; cross_moments.h, kernels_cross.hip), allocated by ensure_cross before
  // the first flagged solve or capture, slot-major like the statistics: cross_slots slots for solves and one more, the
  // last, for mppi_cross_moments_eval
  float* d_cross_mx = nullptr;    // [cross_slots + 1][max_batch][nu][nu]
  float* d_cross_part = nullptr;  // scratch: the per-cell partial sums [cross_part_floats]
  int cross_slots = 0;
  int cross_B = 0, cross_n = 0;   // batch and slot count of the last solve / graph launch with the flag (0: none ran)
  // the law adapted on the device (mppi_set_noise_adapt; noise_adapt.h, kernels_noise.hip).  While adapt_on, d_law is
  // the law: the generators read it, noise_adapt_kernel moves it behind every solve's statistics, and noise_model
  // only keeps active = 1.  d_law_hist [hist_slots + 1][nu + 1]: the law solve i of the last solve / graph launch drew
  // its noise from (sigma_u, rho), allocated with and as large as the statistics' slots (ensure_stats).
  bool adapt_on = false;
  NoiseAdapt adapt{0.0f, 1e-3f, 10.0f, 0.95f};
  float* d_law = nullptr;
  float* d_law_hist = nullptr;
  int hist_slots = 0;
  int law_n = 0;             // history rows of the last adapting solve / graph launch (0: none ran)
  // the knot law (mppi_set_noise_knots; noise_knots.h, noise_knot_kernel).  noise_model.n_knots / .order are the law;
  // d_knots holds its table, idx [H][4] int32 then w [H][4] fp32, allocated by the first enabling call and written by
  // the setter only; knot_idx / knot_w are the host's copy (mppi_get_noise_knots)
  void* d_knots = nullptr;
  std::vector<int32_t> knot_idx;
  std::vector<float> knot_w;
  // the horizon basis (mppi_set_noise_basis; noise_basis.h, noise_basis_kernel).  noise_model.n_basis is the law; d_basis
  // holds M transposed, [min(H, kMaxBasis)][basis_pitch(H)] fp32, allocated by the first enabling call and written by
  // the setter only; basis_host is the host's copy of M [H][n_basis] as given (mppi_get_noise_basis)
  float* d_basis = nullptr;
  std::vector<float> basis_host;
  // the cross-actuator covariance (mppi_set_noise_cov; noise_cov.h, noise_cov_kernel).  noise_model.cov_L != nullptr
  // is the law; d_cov holds L [nu][kMaxNu] (rows padded) then Sinv [nu][nu], allocated by the first enabling call and written by the
  // setter and, while cov_adapt_on, by noise_cov_adapt_kernel; cov_host is the host's copy, Sigma, L, Sinv [nu][nu] each
  // (mppi_get_noise_cov; refreshed from the device while cov_adapt_on)
  float* d_cov = nullptr;
  std::vector<float> cov_host;
  // the covariance adapted on the device (mppi_set_noise_cov_adapt; noise_cov_adapt.h, noise_cov_adapt_kernel).  While
  // cov_adapt_on every solve carries MPPI_FLAG_CROSS and runs the kernel behind its cross moments: it moves d_cov (L,
  // Sinv) and d_cov_law -- the count of rejected steps (8 bytes), Sigma [nu][nu], sqrt of its diagonal [kMaxNu] --
  // allocated by the first enabling call.  d_cov_hist [cov_hist_slots + 1][nu][nu]: the Sigma solve i of the last solve /
  // graph launch drew its noise from, one row per statistics slot (ensure_cov_hist).
  bool cov_adapt_on = false;
  NoiseCovAdapt cov_adapt{0.0f, 1e-3f, 10.0f};
  float* d_cov_law = nullptr;
  float* d_cov_hist = nullptr;
  int cov_hist_slots = 0;
  int cov_law_n = 0;         // history rows of the last adapting solve / graph launch (0: none ran)
  // ESS targeting (mppi_set_ess_target; ess_target.h, kernels_lambda.hip).  While ess_on, every solve runs
  // lambda_search_kernel between its rollout and its reduce; the reduce and the statistics read the solve's lambda from
  // d_lambda [lambda_slots + 1][max_batch], slot-major like the statistics (a graph's solve i writes slot i; the last
  // slot is mppi_lambda_eval's), allocated by ensure_lambda before the first such solve or capture.
  bool ess_on = false;
  EssTarget ess{0.0f, 1e-3f, 1e3f};
  float* d_lambda = nullptr;
  int lambda_slots = 0;
  int lam_B = 0, lam_n = 0;  // batch and slot count of the last targeting solve / graph launch (0: none ran)
  // the control-cost term (mppi_set_control_cost; control_cost.h, kernels_ctrl_cost.hip).  While ctrl_gamma > 0 every
  // solve runs ctrl_lin_kernel + the term kernel between its rollout and everything that weighs its costs; the lambda
  // search, the reduce and the statistics then read d_wcost = d_costs + term where they read d_costs otherwise.  All
  // buffers are allocated by mppi_set_control_cost, two slots each where an evaluation must not disturb a solve's:
  // slot 0 the last solve's (no per-step slots), slot 1 mppi_control_term_eval's.
  float ctrl_gamma = 0.0f;        // 0: off
  float* d_wcost = nullptr;       // [2][max_batch][Kp]
  float* d_term = nullptr;        // [2][max_batch][Kp]
  float* d_lin = nullptr;         // [2][max_batch][nu][H]
  float* d_ctrl_part = nullptr;   // [term_part_floats] the split form's partials (scratch)
  float* d_ctrl_U = nullptr;      // [max_batch][nu][H] mppi_control_term_eval's U (the resident d_U stays as it is)
  int ctrl_B = 0;                 // batch of the last solve / graph launch with the term (0: none ran)
  // per-actuator control bounds (mppi_set_control_bounds; ctrl_bounds.h, kernels_bounds.hip).  While bounds_on every
  // solve projects its noise in place ahead of its rollout (the buffer then holds clip(U + eps, lo, hi) - U) and clips
  // U, the Umirror copy and u0 behind its update; the box travels by value in the launches.  The buffers are allocated
  // by mppi_set_control_bounds: the counts in two slots (0: the last solve's, 1: mppi_bounds_eval's), summed by the
  // clip's launch from the per-row counts the projection leaves in d_bpart.
  bool bounds_on = false;
  float bounds_lo[kMaxNu] = {0}, bounds_hi[kMaxNu] = {0};
  unsigned* d_bcounts = nullptr;  // [2][max_batch][nu]
  unsigned* d_bpart = nullptr;    // [max_batch nu H][bounds_chunks(Kp)] the projection's per-row counts (scratch)
  float* d_bounds_U = nullptr;    // [max_batch][nu][H] mppi_bounds_eval's U (the resident d_U stays as it is)
  int bounds_B = 0;               // batch of the last bounded solve / graph launch (0: none ran)
  // the control-rate cost term (mppi_set_rate_cost; rate_cost.h, kernels_rate_cost.hip).  While rate_on every solve runs
  // the term kernel between its rollout (and the control-cost term) and everything that weighs its costs; the lambda
  // search, the reduce and the statistics then read d_rate_wcost = (costs [+ control term]) + rate term.  The weights
  // travel by value in the launch.  d_uprev is the control applied the step before: zeros until mppi_set_prev_control
  // writes it or a MPPI_FLAG_SHIFT solve with the anchor on stores its u0 there.  All buffers are allocated by the two
  // setters, two slots each where an evaluation must not disturb a solve's: slot 0 the last solve's / the handle's,
  // slot 1 mppi_rate_term_eval's.
  bool rate_on = false;
  int rate_anchor = 0;
  float rate_r[kMaxNu] = {0};
  float* d_rate_wcost = nullptr;  // [2][max_batch][Kp]
  float* d_rate_term = nullptr;   // [2][max_batch][Kp]
  float* d_rate_part = nullptr;   // [term_part_floats] the split form's partials (scratch)
  float* d_rate_U = nullptr;      // [max_batch][nu][H] mppi_rate_term_eval's U (the resident d_U stays as it is)
  float* d_uprev = nullptr;       // [2][max_batch][nu]
  int rate_B = 0;                 // batch of the last solve / graph launch with the term (0: none ran)
  // elite truncation (mppi_set_elites; elite_select.h, kernels_elite.hip).  While elite_n > 0 every solve runs
  // elite_select_kernel behind its rollout and the cost terms and ahead of everything that weighs its costs; the lambda
  // search, the reduce and the statistics then read d_elite_wcost = the end of the wcost chain on the elite set, +inf
  // elsewhere.  All buffers are allocated by mppi_set_elites, two slots each: slot 0 the last solve's, slot 1
  // mppi_elites_eval's.
  int elite_n = 0;                   // n_elite (0: off)
  float* d_elite_wcost = nullptr;    // [2][max_batch][Kp]
  int32_t* d_elite_idx = nullptr;    // [2][max_batch][elite_n]
  int32_t* d_elite_count = nullptr;  // [2][max_batch]
  float* d_elite_tau = nullptr;      // [2][max_batch]
  int elite_B = 0;                   // batch of the last solve / graph launch with elites (0: none ran)
  // keep / shift elites (mppi_set_elite_keep; elite_keep.h, kernels_elite_keep.hip).  While keep_n > 0 every solve
  // injects the stored set into the first columns of its noise ahead of the bounds projection and the rollout
  // (keep_inject_kernel; count and steps are read on the device, so an empty set changes nothing), and stores its own
  // n_keep best behind the cost terms and the selection, ahead of the lambda search (a second elite_select launch on
  // the unmasked chain, or the elites' own set when n_elite == n_keep, then keep_gather_kernel).  The set persists per
  // batch slot b over max_batch, like u_prev.  All buffers are allocated by mppi_set_elite_keep, two slots each where
  // an evaluation must not disturb the handle's: slot 0 the handle's set, slot 1 the eval entries'.
  int keep_n = 0;                    // n_keep (0: off)
  float* d_keep_v = nullptr;         // [2][max_batch][nu][H][keep_pitch(n_keep)]
  float* d_keep_cost = nullptr;      // [2][max_batch][n_keep]
  int32_t* d_keep_idx = nullptr;     // [2][max_batch][n_keep]
  int32_t* d_keep_count = nullptr;   // [2][max_batch]
  int32_t* d_keep_steps = nullptr;   // [2][max_batch]
  int32_t* d_keep_sel = nullptr;     // [max_batch][n_keep] the selection's own idx (scratch: the gather copies it)
  int32_t* d_keep_selcount = nullptr;  // [max_batch] (scratch)
  float* d_keep_tau = nullptr;       // [max_batch] (scratch: the selection's threshold, never read)
  float* d_keep_ecost = nullptr;     // [max_batch][Kp] (scratch: the selection's masked costs, never read)
  float* d_keep_U = nullptr;         // [max_batch][nu][H] the eval entries' U (the resident d_U stays as it is)
  int keep_B = 0;                    // slots 0..keep_B hold a set: stored by a solve or written by mppi_set_kept (0: none)
  // the per-step sampling scale (mppi_set_noise_steps; kernels_noise.hip StepLaw).  While steps_on, d_steps is the scale
  // of the law: S [max_batch][nu][H], one table per batch slot, allocated by the first enabling call, written by the
  // setter on the stream and, while steps_adapt_on, by step_adapt_kernel; the AR(1) generators read it per step, and
  // noise_model.sigma_u is the fill a step entering the horizon starts with.  steps_host: the table as last set, all
  // max_batch slots (what "the table in effect" is compared with while the refit is off).
  bool steps_on = false;
  float* d_steps = nullptr;
  std::vector<float> steps_host;
  // the per-step moments (MPPI_FLAG_STEP_MOMENTS; step_moments.h, kernels_step_moments.hip), allocated by
  // ensure_step_mom before the first flagged solve or capture, slot-major like the statistics: step_slots slots for
  // solves and one more, the last, for mppi_step_moments_eval; m1 of every slot first, then m2
  float* d_step_mom = nullptr;       // [2][step_slots + 1][max_batch][nu][H]
  int step_slots = 0;
  int stepm_B = 0, stepm_n = 0;      // batch and slot count of the last solve / graph launch with the flag (0: none ran)
  // the refit (mppi_set_noise_steps_adapt; step_law.h, step_adapt_kernel).  While steps_adapt_on every solve carries
  // MPPI_FLAG_STEP_MOMENTS and runs the kernel behind its per-step moments: it moves d_steps
  bool steps_adapt_on = false;
  StepAdapt steps_adapt{0.0f, 1e-3f, 10.0f, 1};
  // inner iterations per control step (mppi_set_iterations; iter_best.h, kernels_iter.hip).  A control step is iter_n
  // calls of enqueue_solve on the same x0 and ctx: all but the last without MPPI_FLAG_SHIFT and MPPI_FLAG_ENV_STEP, each
  // with its own noise key and per-step slot.  While iter_on() every iteration runs iter_best_kernel behind the cost
  // terms and the selections; the step's last iteration also runs iter_mean_kernel ahead of its rollout (iter_mean) and
  // iter_apply_kernel behind its update (iter_best).  The stored best persists per batch slot b; the buffers are
  // allocated by mppi_set_iterations or mppi_iter_best_eval, two slots each: slot 0 the handle's, slot 1 the eval's.
  int iter_n = 1;
  int iter_best = 0, iter_mean = 0;  // return_best, add_mean
  float* d_best_v = nullptr;         // [2][max_batch][nu][H]
  float* d_best_cost = nullptr;      // [2][max_batch]
  int32_t* d_best_k = nullptr;       // [2][max_batch]
  int32_t* d_best_iter = nullptr;    // [2][max_batch]
  float* d_best_U = nullptr;         // [max_batch][nu][H] mppi_iter_best_eval's U (the resident d_U stays as it is)
  int best_B = 0;                    // batch of the last tracking solve / graph launch (0: none ran)
  bool iter_on() const { return iter_n > 1 || iter_best || iter_mean; }
  // population-size decay (mppi_set_population; population.h).  While pop_n > 0 (== iter_n), iteration i of every
  // control step draws, rolls out and weighs pop_K[i] samples: enqueue_solve sets `shape` to the iteration's own (K_i,
  // Kp_i) for as long as it enqueues that iteration, and every helper it calls reads the sample count and the K axis'
  // pitch from there -- the buffers, sized for cfg.K, are re-read densely at that shape.  Outside enqueue_solve, and
  // on every handle without a table, shape is (cfg.K, Kp): the *_eval entries stay at cfg.K.  Slot offsets inside a
  // buffer ([2][max_batch][Kp] and the like) stay those of Kp.
  int pop_n = 0;  // 0: off (a table whose entries all equal cfg.K is stored as off)
  int32_t pop_K[kPopMaxIter] = {0};
  struct Shape {
    int K, Kp;
  } shape{0, 0};
  Shape iter_shape(int it) const {
    return pop_n > 0 ? Shape{(int)pop_K[it], pop_pitch((int)pop_K[it])} : Shape{cfg.K, Kp};
  }
  // the shape of a control step's last iteration: what io.costs / io.weights and the [B][K] read-outs of slot 0 hold
  Shape last_shape() const { return iter_shape(pop_n > 0 ? pop_n - 1 : 0); }
  // the kernel iteration `it` of the last control step was routed to (mppi_iter_rollout_kernel)
  const char* iter_kernel[kPopMaxIter] = {nullptr};
  // dynamics-model ensembles (mppi_set_ensemble; ensemble.h, kernels_ensemble.hip).  Member 0 is what
  // mppi_load_dynamics loaded (net / net_env / fa / cart above); members 1..ens_extra, loaded densely by
  // mppi_load_member through the same build and upload path, live in ens_mem[1..] (entry 0 is never read).  While
  // ens_n > 1 every solve launches one rollout per member e < ens_n on the same x0, U, ctx and noise, member e writing
  // row e of d_ens_costs, then ensemble_kernel, which writes d_costs and d_ens_sd; everything behind reads d_costs as
  // before.  The env step runs member ens_env.  The buffers are allocated by the first enabling call, zero-filled; the
  // member rows are max_batch * Kp apart whatever the iteration's shape (each row is re-read densely at it).
  // d_ens_eval: mppi_ensemble_eval's own members [MPPI_ENS_MAX][max_batch][Kp], costs and sd [max_batch][Kp] each,
  // allocated by its first call: an evaluation touches nothing a solve reads or writes.
  struct Member {
    CartpoleParams cart{};
    FcNet net, net_env;
    FaNet fa;
  } ens_mem[MPPI_ENS_MAX];
  int ens_extra = 0;               // members loaded behind member 0
  int ens_n = 1;                   // n_members (1: off)
  int ens_mode = MPPI_ENS_MEAN;
  float ens_kappa = 0.0f;
  int ens_env = 0;                 // env_member
  float* d_ens_costs = nullptr;    // [MPPI_ENS_MAX][max_batch][Kp]
  float* d_ens_sd = nullptr;       // [max_batch][Kp]
  float* d_ens_eval = nullptr;     // [MPPI_ENS_MAX + 2][max_batch][Kp]
  int ens_B = 0;                   // batch of the last solve / graph launch with an ensemble (0: none ran)
  int graph_ens = 1;               // the members the captured graph's solves roll (stamped launches per solve)
  int ens_loaded() const { return dyn_kind ? 1 + ens_extra : 0; }
};

// The shape a [B][K] read-out of output slot `slot` was written at: slot 0 is the last solve's -- with a population
// table the step's last iteration's, K_last samples at pitch Kp_last -- and every other slot an evaluation's, at cfg.K.
static mppi_handle::Shape readout_shape(const mppi_handle* h, int slot) {
  return slot == 0 ? h->last_shape() : mppi_handle::Shape{h->cfg.K, h->Kp};
}

static int pop_check(const mppi_handle* h, const char* who, int n_iter, int n_elite, int n_keep, int add_mean);

// enqueue_solve's iteration shape on the handle, restored on every way out
struct ShapeScope {
  mppi_handle* h;
  mppi_handle::Shape saved;
  ShapeScope(mppi_handle* h_, mppi_handle::Shape s) : h(h_), saved(h_->shape) { h->shape = s; }
  ~ShapeScope() { h->shape = saved; }
  ShapeScope(const ShapeScope&) = delete;
  ShapeScope& operator=(const ShapeScope&) = delete;
};

static hipEvent_t take_event(mppi_handle* h) {
  if (!h->evt_pool.empty()) {
    hipEvent_t e = h->evt_pool.back();
    h->evt_pool.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  (void)hipEventCreate(&e);
  return e;
}

static void harvest_events(mppi_handle* h) {
  for (auto& p : h->pending) {
    float ms = 0.0f;
    if (hipEventSynchronize(p.b) == hipSuccess && hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
      h->prof_count[p.id] += p.n;
      h->prof_ms[p.id] += ms;
    }
    h->evt_pool.push_back(p.a);
    h->evt_pool.push_back(p.b);
  }
  h->pending.clear();
}

// Enqueue `launch` on the handle's stream, bracketed by events when profiling.  count = 0: the group's time is added
// to a kernel name whose launches of this solve were counted already (the bounds' second launch group).
template <class F>
static hipError_t timed(mppi_handle* h, int id, F&& launch, int count = 1) {
  if (!h->prof) return launch();
  if (h->pending.size() > 4096) harvest_events(h);
  PendingEvt p{id, take_event(h), take_event(h), count};
  (void)hipEventRecord(p.a, h->stream);
  hipError_t e = launch();
  (void)hipEventRecord(p.b, h->stream);
  h->pending.push_back(p);
  return e;
}

#define MPPI_TRY(expr)                 \
  do {                                 \
    const int rc_ = (expr);            \
    if (rc_ != MPPI_OK) return rc_;    \
  } while (0)

// The captured graphs hold the handle's settings in their kernel arguments: a setter that changes one destroys them.
// wait: a launch still in flight finishes first (a caller that has waited already, or that knows the stream's state,
// passes false).  The prefetched noise is not touched: whether it stays valid is the caller's decision.
static int drop_graphs(mppi_handle* h, bool wait) {
  if (wait && (h->graph_exec[0] || h->graph_exec[1])) HIP_TRY(hipStreamSynchronize(h->stream));
  for (hipGraphExec_t& g : h->graph_exec)
    if (g) {
      HIP_TRY(hipGraphExecDestroy(g));
      g = nullptr;
    }
  return MPPI_OK;
}

// The overlapped generator's last launch (and its counter bump) precede anything enqueued on the stream from here on.
static hipError_t wait_gen(mppi_handle* h) {
  if (!h->gen_pending) return hipSuccess;
  const hipError_t e = hipStreamWaitEvent(h->stream, h->ev_gen, 0);
  if (e == hipSuccess) h->gen_pending = false;
  return e;
}

// `rows` noise rows [K] (host, or device with `kind`) into the device rows [Kp] of d_noise, the pads K..Kp zeroed
static int stage_noise(mppi_handle* h, const float* src, size_t rows, hipMemcpyKind kind = hipMemcpyHostToDevice) {
  const size_t K = (size_t)h->cfg.K, Kp = (size_t)h->Kp;
  if (K != Kp) HIP_TRY(hipMemsetAsync(h->d_noise, 0, rows * Kp * 4, h->stream));
  HIP_TRY(hipMemcpy2DAsync(h->d_noise, Kp * 4, src, K * 4, K * 4, rows, kind, h->stream));
  return MPPI_OK;
}

// host costs [B][K] into the staging costs [B][Kp] of an evaluation (the pads keep whatever they hold: no kernel of an
// evaluation counts them)
static int stage_costs(mppi_handle* h, const float* src, int B) {
  const size_t K = (size_t)h->cfg.K, Kp = (size_t)h->Kp;
  HIP_TRY(hipMemcpy2DAsync(h->d_costs, Kp * 4, src, K * 4, K * 4, B, hipMemcpyHostToDevice, h->stream));
  return MPPI_OK;
}

// An option's buffers, all or none: every (pointer, bytes) of the list is allocated, then all are committed; a failure
// frees what it got and leaves the pointers as they were.  No buffer is cleared: every entry is written before it is read.
struct BufReq {
  void** p;
  size_t bytes;
};
static int alloc_group(const char* who, const std::vector<BufReq>& reqs) {
  std::vector<void*> got;
  for (const BufReq& r : reqs) {
    void* p = nullptr;
    const hipError_t e = hipMalloc(&p, r.bytes);
    if (e != hipSuccess) {
      for (void* g : got) (void)hipFree(g);
      return fail(MPPI_E_HIP, std::string(who) + ": " + hipGetErrorString(e));
    }
    got.push_back(p);
  }
  for (size_t i = 0; i < reqs.size(); ++i) *reqs[i].p = got[i];
  return MPPI_OK;
}
static size_t at_least16(size_t bytes) { return bytes < 16 ? 16 : bytes; }

// dst [B][cols][rows] <- src [B][rows][cols].  Julia's U (nu, H) column-major is [H][nu] in memory: (H, nu) brings it to
// the engine's [nu][H], (nu, H) takes it back
static void transpose_batched(float* dst, const float* src, int B, int rows, int cols) {
  for (int b = 0; b < B; ++b)
    for (int r = 0; r < rows; ++r)
      for (int c = 0; c < cols; ++c) dst[((size_t)b * cols + c) * rows + r] = src[((size_t)b * rows + r) * cols + c];
}

static CartpoleParams default_cartpole() {
  // models/cartpole.xml compiled as MuJoCo does (oracle/mppi_ref.py::_cartpole_params states the derivation).
  const double rho = 1000.0, r = 0.045, L = 0.6, pi = 3.14159265358979323846;
  const double m_cyl = rho * pi * r * r * L, m_sph = rho * 4.0 / 3.0 * pi * r * r * r;
  const double I = m_cyl * (L * L / 12.0 + r * r / 4.0) + m_sph * (2.0 * r * r / 5.0 + L * L / 4.0 + 3.0 * L * r / 8.0);
  CartpoleParams p;
  p.m_cart = (float)(rho * 0.4 * 0.2 * 0.1);
  p.m_pole = (float)(m_cyl + m_sph);
  p.l = (float)(L / 2.0);
  p.inertia = (float)I;
  p.damping = 0.05f;
  p.gear = 50.0f;
  p.ctrl_lo = -1.0f;
  p.ctrl_hi = 1.0f;
  p.g = 9.81f;
  p.dt = 0.01f;
  return p;
}

// The ensemble's members behind member 0 (mppi_load_member): their device images freed, the slots as new.  The stream
// is idle and no captured graph holds them (the callers see to both).
static void free_member(mppi_handle::Member& m) {
  if (m.net.fa.img) (void)hipFree(const_cast<char*>(m.net.fa.img));
  if (m.net_env.fa.img) (void)hipFree(const_cast<char*>(m.net_env.fa.img));
  if (m.fa.d_img) (void)hipFree(m.fa.d_img);
  if (m.fa.d_ws) (void)hipFree(m.fa.d_ws);
  m = mppi_handle::Member();
}
static void free_members(mppi_handle* h) {
  for (int e = 1; e < MPPI_ENS_MAX; ++e) free_member(h->ens_mem[e]);
  h->ens_extra = 0;
}

// --------------------------------------------------------------------------------------- presets

struct PresetRow {
  const char* name;
  int nx, nu, K, H;
  float lambda, sigma, ctrl_clamp, U_clamp, norm_eps, shift_fill, terminal_weight;
  int update_mode;
};

// SURVEY 8a variant table; constants cited from the reference scripts.
static const PresetRow kPresets[] = {
    {"cartpole_py", 4, 1, 30, 100, 1.0f, 1.0f, 0, 0, 0, 0.1f, 10.0f, MPPI_UPDATE_ADD},          // cartpole_mppi.py:12-15
    {"cartpole_jl", 4, 1, 30, 100, 1.0f, 1.0f, 0, 0, 0, 0.1f, 10.0f, MPPI_UPDATE_ADD},          // cartpole_mppi.jl:11-14
    {"cartpole_collect", 4, 1, 75, 100, 1.0f, 0.75f, 0, 0, 0, 0.1f, 10.0f, MPPI_UPDATE_ADD},    // cartpole_datacollection.py:13-16
    {"quad_mppi_jl", 37, 12, 50, 30, 0.2f, 0.3f, 10.0f, 10.0f, 1e-10f, 0.0f, 0.0f, MPPI_UPDATE_ADD},  // mppi.jl:10-13
    {"humanoid_v3", 55, 21, 30, 75, 1.0f, 0.75f, 0, 0, 0, 0.1f, 10.0f, MPPI_UPDATE_ADD},        // Humanoid_mppi_v3.jl:13-16
    {"humanoid_v1", 55, 21, 50, 100, 1.0f, 1.0f, 0, 0, 0, 0.1f, 10.0f, MPPI_UPDATE_ADD},        // Humanoid_mppi.jl:22-25
    {"humanoid_collect_v2", 55, 21, 50, 100, 1.0f, 0.5f, 0, 0, 0, 0.1f, 10.0f, MPPI_UPDATE_ADD},  // Humanoid_datacollection_v2.jl:46-49
    {"cartpole_est", 4, 1, 2048, 100, 10.0f, 0.5f, 0, 0, 0, 0.1f, 10.0f, MPPI_UPDATE_REPLACE},  // cartpole_mppi_estimator.py:37-40
    {"quad_est", 37, 12, 2048, 50, 10.0f, 0.4f, 0, 0, 0, 0.1f, 10.0f, MPPI_UPDATE_REPLACE},     // quadruped_mppi_estimator.py:38-41
};

extern "C" {

const char* mppi_last_error(void) { return g_err.c_str(); }
int mppi_abi_version(void) { return MPPI_ABI_VERSION; }
#ifndef MPPI_BUILD_ID
#define MPPI_BUILD_ID "unknown"
#endif
const char* mppi_build_id(void) { return MPPI_BUILD_ID; }  // build.py passes the source hash

int mppi_preset(const char* name, mppi_config* cfg) {
  if (!name || !cfg) return fail(MPPI_E_ARG, "mppi_preset: null argument");
  for (const PresetRow& p : kPresets) {
    if (std::strcmp(p.name, name) == 0) {
      std::memset(cfg, 0, sizeof(*cfg));
      cfg->nx = p.nx;
      cfg->nu = p.nu;
      cfg->K = p.K;
      cfg->H = p.H;
      cfg->max_batch = 1;
      cfg->lambda = p.lambda;
      cfg->sigma = p.sigma;
      cfg->ctrl_clamp = p.ctrl_clamp;
      cfg->U_clamp = p.U_clamp;
      cfg->norm_eps = p.norm_eps;
      cfg->shift_fill = p.shift_fill;
      cfg->terminal_weight = p.terminal_weight;
      cfg->update_mode = p.update_mode;
      cfg->precision = MPPI_PREC_BF16;
      return MPPI_OK;
    }
  }
  return fail(MPPI_E_ARG, std::string("mppi_preset: unknown preset ") + name);
}

void mppi_destroy(mppi_handle* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  harvest_events(h);
  for (hipEvent_t e : h->evt_pool) (void)hipEventDestroy(e);
  void* bufs[] = {h->d_x0, h->d_U, h->d_noise, h->d_costs, h->d_dU, h->d_weights, h->d_u0, h->d_ctx, h->d_status,
                  h->d_tickets, const_cast<char*>(h->net.fa.img), const_cast<char*>(h->net_env.fa.img), h->fa.d_img,
                  h->fa.d_ws, h->d_seed_ctr, h->d_env_noise, h->d_env_costs, h->d_env_status, h->d_noise2, h->d_gticket, h->d_part, h->d_kclock,
                  h->d_stats, h->d_stats_m2, h->d_stats_m11, h->d_stats_w, h->d_stats_part, h->d_cross_mx, h->d_cross_part, h->d_cov_law, h->d_cov_hist, h->d_law, h->d_law_hist, h->d_knots, h->d_cov, h->d_basis,
                  h->d_lambda, h->d_wcost, h->d_term, h->d_lin, h->d_ctrl_part, h->d_ctrl_U, h->d_bcounts,
                  h->d_bpart, h->d_bounds_U, h->d_rate_wcost, h->d_rate_term, h->d_rate_part, h->d_rate_U, h->d_uprev,
                  h->d_elite_wcost, h->d_elite_idx, h->d_elite_count, h->d_elite_tau, h->d_keep_v, h->d_keep_cost,
                  h->d_keep_idx, h->d_keep_count, h->d_keep_steps, h->d_keep_sel, h->d_keep_selcount, h->d_keep_tau,
                  h->d_keep_ecost, h->d_keep_U, h->d_steps, h->d_step_mom, h->d_best_v, h->d_best_cost, h->d_best_k,
                  h->d_best_iter, h->d_best_U, h->d_nkey, h->d_ens_costs, h->d_ens_sd, h->d_ens_eval};
  for (hipGraphExec_t& g : h->graph_exec)
    if (g) (void)hipGraphExecDestroy(g);
  if (h->gstream) (void)hipStreamSynchronize(h->gstream);
  free_members(h);
  for (void* p : bufs)
    if (p) (void)hipFree(p);
  if (h->ev_gen) (void)hipEventDestroy(h->ev_gen);
  if (h->ev_red) (void)hipEventDestroy(h->ev_red);
  if (h->ev_switch) (void)hipEventDestroy(h->ev_switch);
  if (h->gstream) (void)hipStreamDestroy(h->gstream);
  if (h->own_stream) (void)hipStreamDestroy(h->own_stream);
  delete h;
}

int mppi_create(const mppi_config* cfg, int device, mppi_handle** out) {
  if (!cfg || !out) return fail(MPPI_E_ARG, "mppi_create: null argument");
  *out = nullptr;
  const mppi_config& c = *cfg;
  if (c.nx < 1 || c.nx > 4096 || c.nu < 1 || c.nu > 4096 || c.H < 1 || c.K < 1 || c.K > kMaxK || c.max_batch < 1)
    return fail(MPPI_E_ARG, "mppi_create: bad dimensions (need nx,nu,H,K,max_batch >= 1, K <= 32768)");
  if (!(c.lambda > 0.0f)) return fail(MPPI_E_ARG, "mppi_create: lambda must be > 0");
  if (c.update_mode != MPPI_UPDATE_ADD && c.update_mode != MPPI_UPDATE_REPLACE)
    return fail(MPPI_E_ARG, "mppi_create: bad update_mode");
  if (c.precision != MPPI_PREC_FP32 && c.precision != MPPI_PREC_BF16 && c.precision != MPPI_PREC_BF16X3)
    return fail(MPPI_E_ARG, "mppi_create: bad precision");
  if ((size_t)c.nu * c.H * sizeof(float) > 64 * 1024) return fail(MPPI_E_ARG, "mppi_create: nu*H too large (> 16384)");
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) return fail(MPPI_E_ARG, "mppi_create: no such device");
  HIP_TRY(hipSetDevice(device));
  mppi_handle* h = new (std::nothrow) mppi_handle();
  if (!h) return fail(MPPI_E_ARG, "mppi_create: out of host memory");
  h->cfg = c;
  h->device = device;
  h->Kp = (c.K + kKpAlign - 1) / kKpAlign * kKpAlign;
  h->shape = {c.K, h->Kp};
  h->cart = default_cartpole();
  const size_t B = (size_t)c.max_batch;
  auto alloc = [&](void** p, size_t bytes) -> hipError_t {
    hipError_t e = hipMalloc(p, bytes < 16 ? 16 : bytes);
    if (e == hipSuccess) e = hipMemset(*p, 0, bytes < 16 ? 16 : bytes);
    return e;
  };
  hipError_t e = hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = alloc((void**)&h->d_x0, B * c.nx * 4);
  if (e == hipSuccess) e = alloc((void**)&h->d_U, B * c.nu * c.H * 4);
  if (e == hipSuccess) e = alloc((void**)&h->d_noise, B * c.nu * c.H * (size_t)h->Kp * 4);
  if (e == hipSuccess) e = alloc((void**)&h->d_costs, B * h->Kp * 4);
  if (e == hipSuccess) e = alloc((void**)&h->d_dU, B * c.nu * c.H * 4);
  if (e == hipSuccess) e = alloc((void**)&h->d_weights, B * h->Kp * 4);
  if (e == hipSuccess) e = alloc((void**)&h->d_u0, B * c.nu * 4);
  if (e == hipSuccess) e = alloc((void**)&h->d_ctx, B * MPPI_CTX_MAX * 4);
  if (e == hipSuccess) e = alloc((void**)&h->d_status, 16);
  if (e == hipSuccess) e = alloc((void**)&h->d_tickets, B * 4);
  if (e == hipSuccess) e = alloc((void**)&h->d_seed_ctr, 8);
  if (e == hipSuccess) e = alloc((void**)&h->d_nkey, 16);
  if (e == hipSuccess) e = alloc((void**)&h->d_env_noise, B * c.nu * kKpAlign * 4);
  if (e == hipSuccess) e = alloc((void**)&h->d_env_costs, B * kKpAlign * 4);
  if (e == hipSuccess) e = alloc((void**)&h->d_env_status, 16);
  if (e != hipSuccess) {
    mppi_destroy(h);
    return fail(MPPI_E_HIP, std::string("mppi_create: ") + hipGetErrorString(e));
  }
  h->stream = h->own_stream;
  *out = h;
  return MPPI_OK;
}

// One dynamics model built, uploaded and put into (cart, net_dst, env_dst, fa_dst): the handle's own for
// mppi_load_dynamics (member 0), a slot of ens_mem for mppi_load_member.  A failure leaves the destination as it was.
static int load_dyn(mppi_handle* h, const char* who_, int kind, const void* blob, size_t nbytes, CartpoleParams& cart,
                    FcNet& net_dst, FcNet& env_dst, FaNet& fa_dst) {
  const std::string who = std::string(who_) + ": ";
  if (kind == MPPI_DYN_CARTPOLE) {
    if (h->cfg.nx != 4 || h->cfg.nu != 1) return fail(MPPI_E_ARG, "cartpole dynamics need nx=4, nu=1");
    cart = default_cartpole();
    if (!h->d_part) {  // [max_batch][Kp/256][2 + H] partial records (fixed by the config: allocated once)
      const size_t n = (size_t)h->cfg.max_batch * ((h->Kp + 255) / 256) * (2 + h->cfg.H) * sizeof(float);
      HIP_TRY(hipMalloc(&h->d_part, n));
      HIP_TRY(hipMemset(h->d_part, 0, n));
    }
    if (blob) {
      if (nbytes != 10 * sizeof(float)) return fail(MPPI_E_ARG, "cartpole params: expected 10 floats");
      std::memcpy(&cart, blob, sizeof(CartpoleParams));
    }
    return MPPI_OK;
  }
  if (kind == MPPI_DYN_MLP || kind == MPPI_DYN_CROSS_ATTN) {
    if (!blob || nbytes == 0) return fail(MPPI_E_ARG, who + "weight blob required");
    std::vector<unsigned char> img, img_env;
    FcNet net, net_env;
    try {
      img = build_fc_net(kind, blob, nbytes, h->cfg.precision, h->cfg.nx, h->cfg.nu, net);
      if (h->cfg.precision == MPPI_PREC_BF16X3)
        img_env = build_fc_net(kind, blob, nbytes, MPPI_PREC_FP32, h->cfg.nx, h->cfg.nu, net_env);
    } catch (const std::exception& ex) {
      return fail(MPPI_E_UNSUPPORTED, who + ex.what());
    }
    if (h->cfg.precision == MPPI_PREC_BF16 && net.fa.lds_bytes > 128 * 1024)
      return fail(MPPI_E_UNSUPPORTED, who + "LDS part of the packed bf16 image exceeds 128 KiB");
    HIP_TRY(hipStreamSynchronize(h->stream));
    void* d = nullptr;
    HIP_TRY(hipMalloc(&d, img.size()));
    if (const hipError_t e = hipMemcpy(d, img.data(), img.size(), hipMemcpyHostToDevice); e != hipSuccess) {
      (void)hipFree(d);
      return fail(MPPI_E_HIP, who + "image upload: " + hipGetErrorString(e));
    }
    void* d_env = nullptr;
    if (!img_env.empty()) {
      hipError_t e = hipMalloc(&d_env, img_env.size());
      if (e == hipSuccess) e = hipMemcpy(d_env, img_env.data(), img_env.size(), hipMemcpyHostToDevice);
      if (e != hipSuccess) {
        (void)hipFree(d);
        (void)hipFree(d_env);
        return fail(MPPI_E_HIP, who + "env-step image upload: " + hipGetErrorString(e));
      }
    }
    if (net_dst.fa.img) (void)hipFree(const_cast<char*>(net_dst.fa.img));
    if (env_dst.fa.img) (void)hipFree(const_cast<char*>(env_dst.fa.img));
    net.fa.img = static_cast<const char*>(d);
    net_env.fa.img = static_cast<const char*>(d_env);
    env_dst = net_env;
    net.x3_l1 = 0;  // a new net: the split layer-1 probe runs again at the next solve (x3_probe)
    net_dst = net;
    return MPPI_OK;
  }
  if (kind == MPPI_DYN_FEATURE_ATTN) {
    if (!blob || nbytes == 0) return fail(MPPI_E_ARG, who + "weight blob required");
    if (h->cfg.precision == MPPI_PREC_BF16X3)
      return fail(MPPI_E_UNSUPPORTED, who + "MPPI_PREC_BF16X3 is built for the fc nets (MLP, CA) only");
    std::vector<unsigned char> img;
    FaNet net;
    try {
      img = build_fa_net(blob, nbytes, h->cfg.precision, h->cfg.nx, h->cfg.nu, net);
    } catch (const std::exception& ex) {
      return fail(MPPI_E_UNSUPPORTED, who + ex.what());
    }
    const int lds = fa_lds_bytes(net.D, net.precision, net.nh, net.L);
    if (lds <= 0 || lds > 160 * 1024)
      return fail(MPPI_E_UNSUPPORTED, who + "feature-attention shape does not fit the kernel's LDS");
    HIP_TRY(hipStreamSynchronize(h->stream));
    // the new image first: the loaded net stays in place (and usable) if anything below fails
    void* d = nullptr;
    HIP_TRY(hipMalloc(&d, img.size()));
    if (const hipError_t e = hipMemcpy(d, img.data(), img.size(), hipMemcpyHostToDevice); e != hipSuccess) {
      (void)hipFree(d);
      return fail(MPPI_E_HIP, who + "image upload: " + hipGetErrorString(e));
    }
    net.d_img = d;
    const char* lay_env = getenv("MPPI_FA_LAYERED");
    if (net.lay && lay_env && atoi(lay_env) == 1) {  // the layer-by-layer hidden-512 path's activations (~10 KB per
                                                      // token row; skipped above 32 GiB), only when it is selected
      const long rows = (long)h->cfg.max_batch * h->cfg.K * net.L;
      const size_t ws = fa_layered_ws_bytes(rows);
      // an optional workspace: if it cannot be had, the fused kernel runs (net.d_ws stays null), no error
      if (ws <= ((size_t)32 << 30) && hipMalloc(&net.d_ws, ws) == hipSuccess) {
        if (hipMemset(net.d_ws, 0, ws) == hipSuccess) {
          net.ws_rows = rows;
        } else {
          (void)hipFree(net.d_ws);
          net.d_ws = nullptr;
        }
      }
      (void)hipGetLastError();  // a failed optional allocation leaves no sticky error behind
    }
    if (fa_dst.d_img) (void)hipFree(fa_dst.d_img);
    if (fa_dst.d_ws) (void)hipFree(fa_dst.d_ws);
    fa_dst = net;
    return MPPI_OK;
  }
  return fail(MPPI_E_UNSUPPORTED, who + "unknown dynamics kind");
}

int mppi_load_dynamics(mppi_handle* h, int kind, const void* blob, size_t nbytes) {
  if (!h) return fail(MPPI_E_ARG, "mppi_load_dynamics: null handle");
  if (h->ens_n > 1)
    return fail(MPPI_E_STATE, "mppi_load_dynamics: an ensemble is on (call mppi_set_ensemble(h, 1, ...) first, or "
                              "replace a member with mppi_load_member)");
  HIP_TRY(hipSetDevice(h->device));
  MPPI_TRY(load_dyn(h, "mppi_load_dynamics", kind, blob, nbytes, h->cart, h->net, h->net_env, h->fa));
  h->dyn_kind = kind;
  free_members(h);  // member 0 is new, maybe of another kind: the members behind it go (the stream is idle, no graph holds them)
  return MPPI_OK;
}

int mppi_load_member(mppi_handle* h, int e, int kind, const void* blob, size_t nbytes) {
  if (!h) return fail(MPPI_E_ARG, "mppi_load_member: null handle");
  if (e < 1 || e >= MPPI_ENS_MAX) return fail(MPPI_E_ARG, "mppi_load_member: e must be in [1, MPPI_ENS_MAX)");
  if (h->dyn_kind == 0) return fail(MPPI_E_STATE, "mppi_load_member: call mppi_load_dynamics first (member 0)");
  if (kind != h->dyn_kind) return fail(MPPI_E_ARG, "mppi_load_member: the members are of member 0's kind");
  if (e > h->ens_loaded())
    return fail(MPPI_E_ARG, "mppi_load_member: members are loaded densely (e beyond the number loaded)");
  if (kind == MPPI_DYN_CROSS_ATTN && h->cfg.precision == MPPI_PREC_BF16X3)
    return fail(MPPI_E_UNSUPPORTED, "mppi_load_member / mppi_set_ensemble: the CrossAttention net at MPPI_PREC_BF16X3 "
                                    "takes its split form from a probe of member 0 alone; no ensemble of it is built");
  if (kind == MPPI_DYN_CARTPOLE && blob && nbytes != 10 * sizeof(float))
    return fail(MPPI_E_ARG, "mppi_load_member: cartpole params: expected 10 floats");
  HIP_TRY(hipSetDevice(h->device));
  // built and uploaded beside the member it replaces, so that a blob the loader refuses changes nothing
  mppi_handle::Member m;
  MPPI_TRY(load_dyn(h, "mppi_load_member", kind, blob, nbytes, m.cart, m.net, m.net_env, m.fa));
  // a member in use sits by value in the captured graphs' launches: they go before its image does (load_dyn has waited
  // for the stream)
  if (e < h->ens_n) {
    if (const int rc = drop_graphs(h, true); rc != MPPI_OK) {
      free_member(m);
      return rc;
    }
  }
  free_member(h->ens_mem[e]);
  h->ens_mem[e] = m;
  if (e == h->ens_loaded()) h->ens_extra += 1;
  return MPPI_OK;
}

int mppi_set_cost(mppi_handle* h, int kind, const float* params, int nparams) {
  if (!h) return fail(MPPI_E_ARG, "mppi_set_cost: null handle");
  if (kind < MPPI_COST_CARTPOLE || kind > MPPI_COST_HUMANOID_V1) return fail(MPPI_E_UNSUPPORTED, "unknown cost kind");
  const CostIdx ci = cost_idx(kind);
  for (int i = 0; i < ci.n; ++i)
    if (ci.idx[i] >= h->cfg.nx) return fail(MPPI_E_ARG, "mppi_set_cost: cost reads state entries beyond nx");
  if (nparams < 0 || nparams > MPPI_CTX_MAX || (nparams > 0 && !params))
    return fail(MPPI_E_ARG, "mppi_set_cost: params must be <= 8 floats");
  float def[MPPI_CTX_MAX] = {0};
  if (kind == MPPI_COST_HUMANOID_V3 || kind == MPPI_COST_HUMANOID_V1) {
    // src/Humanoid_mppi_v3.jl:12 target (v1: the constants of src/Humanoid_mppi.jl:36,56); no real-env terms by default
    def[0] = 2.0f;
    def[1] = 0.0f;
    def[2] = 1.28f;
  } else if (kind == MPPI_COST_QUAD_EST) {  // src/quadruped_mppi_estimator.py:45
    def[0] = 2.0f;
    def[1] = 0.0f;
    def[2] = 0.35f;
  }
  for (int i = 0; i < nparams; ++i) def[i] = params[i];
  if (h->net.x3_l1 != 0) {
    // the split CA's probe (x3_probe) measured a relative COST error under the cost it found: a new cost returns the
    // handle to "not probed" and the next solve (or capture) probes again.  Graphs captured under the old decision
    // are stale the way mppi_set_noise_model's are (a launch still in flight finishes first)
    HIP_TRY(hipSetDevice(h->device));
    MPPI_TRY(drop_graphs(h, true));
    h->net.x3_l1 = 0;
    h->net.x3_l1_err = -1.0f;
    h->net.x3_f16 = 0;
    h->net.x3_f16_err = -1.0f;
  }
  std::memcpy(h->cost_params, def, sizeof(def));
  h->cost_kind = kind;
  return MPPI_OK;
}

int mppi_set_stream(mppi_handle* h, void* s) {
  if (!h) return fail(MPPI_E_ARG, "mppi_set_stream: null handle");
  const hipStream_t ns = s ? (hipStream_t)s : h->own_stream;
  if (ns != h->stream && (h->gen_pending || h->prefetch_valid)) {
    // chained-solve state spans the switch: the next chained solve reads the noise the previous one prefetched, and
    // (with the generator beside the rollout) the generator stream orders itself behind ev_red recorded on the CURRENT
    // stream as "the previous reduce".  Order the new stream behind everything already on the old one, so that both
    // hold across it.
    HIP_TRY(hipSetDevice(h->device));
    if (!h->ev_switch) HIP_TRY(hipEventCreateWithFlags(&h->ev_switch, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(h->ev_switch, h->stream));
    HIP_TRY(hipStreamWaitEvent(ns, h->ev_switch, 0));
  }
  h->stream = ns;
  return MPPI_OK;
}

int mppi_sync(mppi_handle* h) {
  if (!h) return fail(MPPI_E_ARG, "mppi_sync: null handle");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return MPPI_OK;
}

int mppi_profile(mppi_handle* h, int enable) {
  if (!h) return fail(MPPI_E_ARG, "mppi_profile: null handle");
  if (enable && !h->prof) {
    harvest_events(h);
    for (int i = 0; i < kNumKernels; ++i) {
      h->prof_count[i] = 0;
      h->prof_ms[i] = 0.0;
    }
  }
  h->prof = enable != 0;
  return MPPI_OK;
}

int mppi_kernel_time(mppi_handle* h, const char* kernel, int* count, double* total_ms) {
  if (!h || !kernel) return fail(MPPI_E_ARG, "mppi_kernel_time: null argument");
  harvest_events(h);
  for (int i = 0; i < kNumKernels; ++i) {
    if (std::strcmp(kernel, kKernelNames[i]) == 0) {
      if (count) *count = (int)h->prof_count[i];
      if (total_ms) *total_ms = h->prof_ms[i];
      return MPPI_OK;
    }
  }
  return fail(MPPI_E_ARG, std::string("mppi_kernel_time: unknown kernel ") + kernel);
}

int mppi_kernel_clock(mppi_handle* h, int enable) {
  if (!h) return fail(MPPI_E_ARG, "mppi_kernel_clock: null handle");
  HIP_TRY(hipSetDevice(h->device));
  if (enable) {
    // [kClockSlots][2] stamps, then the launch counter and the block-arrival ticket (mppi_internal.h::KClock)
    const size_t n = 2 * (size_t)kClockSlots + 2;
    if (!h->d_kclock) HIP_TRY(hipMalloc(&h->d_kclock, n * sizeof(unsigned long long)));
    std::vector<unsigned long long> init(n, 0ull);
    for (size_t i = 0; i < 2 * (size_t)kClockSlots; i += 2) init[i] = ~0ull;  // start = min, end = max over blocks
    HIP_TRY(hipMemcpyAsync(h->d_kclock, init.data(), n * sizeof(unsigned long long), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->kclock_launches = 0;
  }
  h->kclock = enable != 0;
  return MPPI_OK;
}

int mppi_kernel_clock_read(mppi_handle* h, int* launches, double* total_us, double* max_us) {
  if (!h || !launches || !total_us) return fail(MPPI_E_ARG, "mppi_kernel_clock_read: null argument");
  *launches = 0;
  *total_us = 0.0;
  if (max_us) *max_us = 0.0;
  if (!h->d_kclock) return fail(MPPI_E_STATE, "mppi_kernel_clock_read: call mppi_kernel_clock(h, 1) first");
  if (h->kclock_launches > kClockSlots)
    return fail(MPPI_E_UNSUPPORTED, "mppi_kernel_clock_read: more stamped launches than clock slots since the reset");
  HIP_TRY(hipSetDevice(h->device));
  int rate_khz = 0;  // s_memrealtime frequency
  HIP_TRY(hipDeviceGetAttribute(&rate_khz, hipDeviceAttributeWallClockRate, h->device));
  if (rate_khz <= 0) return fail(MPPI_E_HIP, "mppi_kernel_clock_read: no device wall-clock rate");
  std::vector<unsigned long long> v(2 * (size_t)kClockSlots + 1);  // the slots, then the device launch counter
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipMemcpy(v.data(), h->d_kclock, v.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  const unsigned long long dev_launches = v.back();
  v.pop_back();
  // kclock_record's invariant (one stamping leader per block of every stamped launch): the device counter has
  // advanced once per launch the host issued; a kernel that broke it would fold later launches into one slot
  if (dev_launches != (unsigned long long)h->kclock_launches)
    return fail(MPPI_E_STATE, "mppi_kernel_clock_read: device launch counter (" + std::to_string(dev_launches) +
                                  ") != stamped launches (" + std::to_string(h->kclock_launches) +
                                  "): a stamped kernel broke kclock_record's one-leader-per-block invariant");
  for (size_t i = 0; i < v.size(); i += 2) {
    if (v[i + 1] == 0ull || v[i] == ~0ull || v[i + 1] < v[i]) continue;
    const double us = (double)(v[i + 1] - v[i]) * 1e3 / rate_khz;
    *launches += 1;
    *total_us += us;
    if (max_us && us > *max_us) *max_us = us;
  }
  if (*launches != h->kclock_launches)
    return fail(MPPI_E_STATE, "mppi_kernel_clock_read: stamped slots (" + std::to_string(*launches) +
                                  ") != stamped launches (" + std::to_string(h->kclock_launches) + ")");
  return MPPI_OK;
}

int mppi_device_buffers(mppi_handle* h, void** dU, void** du0, void** dcosts) {
  if (!h) return fail(MPPI_E_ARG, "mppi_device_buffers: null handle");
  if (dU) *dU = h->d_U;
  if (du0) *du0 = h->d_u0;
  if (dcosts) *dcosts = h->d_costs;
  return MPPI_OK;
}

int mppi_get_U(mppi_handle* h, int B, float* U) {
  if (!h || !U || B < 1 || B > h->cfg.max_batch) return fail(MPPI_E_ARG, "mppi_get_U: bad argument");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipMemcpyAsync(U, h->d_U, (size_t)B * h->cfg.nu * h->cfg.H * 4, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return MPPI_OK;
}

int mppi_set_U(mppi_handle* h, int B, const float* U) {
  if (!h || !U || B < 1 || B > h->cfg.max_batch) return fail(MPPI_E_ARG, "mppi_set_U: bad argument");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipMemcpyAsync(h->d_U, U, (size_t)B * h->cfg.nu * h->cfg.H * 4, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return MPPI_OK;
}

}  // extern "C"

// The diagnostics' buffers for `slots` solve slots (+ 1 for mppi_stats_eval).  Growing them (a graph with more solves
// than any before) waits for the stream and forgets the statistics held so far.  Never called inside a capture.
static int ensure_stats(mppi_handle* h, int slots) {
  const mppi_config& c = h->cfg;
  const size_t B = (size_t)c.max_batch;
  if (!h->d_stats_w) {
    const size_t nw = B * h->Kp * 4, np = stats_part_floats(c.max_batch, c.nu, c.H, h->Kp) * 4;
    HIP_TRY(hipMalloc(&h->d_stats_w, nw));
    HIP_TRY(hipMemset(h->d_stats_w, 0, nw));
    HIP_TRY(hipMalloc(&h->d_stats_part, np));
    HIP_TRY(hipMemset(h->d_stats_part, 0, np));
  }
  if (slots > h->stats_slots) {
    HIP_TRY(hipStreamSynchronize(h->stream));
    void* old[] = {h->d_stats, h->d_stats_m2, h->d_stats_m11};
    for (void* p : old)
      if (p) (void)hipFree(p);
    h->d_stats = nullptr;
    h->d_stats_m2 = h->d_stats_m11 = nullptr;
    h->stats_slots = 0;
    h->stats_B = h->stats_n = 0;
    const size_t n = (size_t)(slots + 1) * B;
    // (cleared in stream order: a memset on the null stream is not ordered against the handle's non-blocking stream)
    HIP_TRY(hipMalloc(&h->d_stats, n * sizeof(mppi_solve_stats)));
    HIP_TRY(hipMemsetAsync(h->d_stats, 0, n * sizeof(mppi_solve_stats), h->stream));
    HIP_TRY(hipMalloc(&h->d_stats_m2, n * c.nu * 4));
    HIP_TRY(hipMemsetAsync(h->d_stats_m2, 0, n * c.nu * 4, h->stream));
    HIP_TRY(hipMalloc(&h->d_stats_m11, n * c.nu * 4));
    HIP_TRY(hipMemsetAsync(h->d_stats_m11, 0, n * c.nu * 4, h->stream));
    h->stats_slots = slots;
  }
  if (h->adapt_on && h->hist_slots < h->stats_slots) {  // the law history: one row per statistics slot, grown alike
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (h->d_law_hist) (void)hipFree(h->d_law_hist);
    h->d_law_hist = nullptr;
    h->hist_slots = 0;
    h->law_n = 0;
    const size_t n = (size_t)(h->stats_slots + 1) * (c.nu + 1) * 4;
    HIP_TRY(hipMalloc(&h->d_law_hist, n));
    HIP_TRY(hipMemsetAsync(h->d_law_hist, 0, n, h->stream));  // in stream order, ahead of the kernels that write rows
    h->hist_slots = h->stats_slots;
  }
  return MPPI_OK;
}

// The cross moments' buffers for `slots` solve slots (+ 1 for mppi_cross_moments_eval), beside the statistics' (whose
// weights the cross pass reads: the caller runs ensure_stats first).  Growing them waits for the stream and forgets the
// moments held so far.  Never called inside a capture.
static int ensure_cross(mppi_handle* h, int slots) {
  const mppi_config& c = h->cfg;
  if (c.nu > kMaxNu) return fail(MPPI_E_UNSUPPORTED, "cross moments (MPPI_FLAG_CROSS) need nu <= 32");
  if (!h->d_cross_part) {
    const size_t np = cross_part_floats(c.max_batch, c.nu, c.H, h->Kp) * 4;
    HIP_TRY(hipMalloc(&h->d_cross_part, np));
    HIP_TRY(hipMemset(h->d_cross_part, 0, np));
  }
  if (slots <= h->cross_slots) return MPPI_OK;
  HIP_TRY(hipStreamSynchronize(h->stream));
  if (h->d_cross_mx) (void)hipFree(h->d_cross_mx);
  h->d_cross_mx = nullptr;
  h->cross_slots = 0;
  h->cross_B = h->cross_n = 0;
  const size_t n = (size_t)(slots + 1) * c.max_batch * c.nu * c.nu * 4;
  HIP_TRY(hipMalloc(&h->d_cross_mx, n));
  HIP_TRY(hipMemsetAsync(h->d_cross_mx, 0, n, h->stream));  // in stream order, ahead of the kernels that write slots
  h->cross_slots = slots;
  return MPPI_OK;
}

// The adapted covariance's history for `slots` solve slots, grown like the cross moments' slots.  Never called inside
// a capture.
static int ensure_cov_hist(mppi_handle* h, int slots) {
  if (slots <= h->cov_hist_slots) return MPPI_OK;
  HIP_TRY(hipStreamSynchronize(h->stream));
  if (h->d_cov_hist) (void)hipFree(h->d_cov_hist);
  h->d_cov_hist = nullptr;
  h->cov_hist_slots = 0;
  h->cov_law_n = 0;
  const size_t n = (size_t)(slots + 1) * h->cfg.nu * h->cfg.nu * 4;
  HIP_TRY(hipMalloc(&h->d_cov_hist, n));
  HIP_TRY(hipMemsetAsync(h->d_cov_hist, 0, n, h->stream));  // in stream order, ahead of the kernels that write rows
  h->cov_hist_slots = slots;
  return MPPI_OK;
}

// The per-step moments' buffers for `slots` solve slots (+ 1 for mppi_step_moments_eval), beside the statistics' (whose
// weights the pass reads: the caller runs ensure_stats first).  Growing them waits for the stream and forgets the
// moments held so far.  Never called inside a capture.
static size_t step_mom_slot_floats(const mppi_handle* h) { return (size_t)h->cfg.max_batch * h->cfg.nu * h->cfg.H; }
static int ensure_step_mom(mppi_handle* h, int slots) {
  if (slots <= h->step_slots) return MPPI_OK;
  HIP_TRY(hipStreamSynchronize(h->stream));
  if (h->d_step_mom) (void)hipFree(h->d_step_mom);
  h->d_step_mom = nullptr;
  h->step_slots = 0;
  h->stepm_B = h->stepm_n = 0;
  const size_t n = 2 * (size_t)(slots + 1) * step_mom_slot_floats(h) * 4;
  HIP_TRY(hipMalloc(&h->d_step_mom, n));
  HIP_TRY(hipMemsetAsync(h->d_step_mom, 0, n, h->stream));  // in stream order, ahead of the kernels that write slots
  h->step_slots = slots;
  return MPPI_OK;
}
static float* step_m1(const mppi_handle* h, int slot) { return h->d_step_mom + (size_t)slot * step_mom_slot_floats(h); }
static float* step_m2(const mppi_handle* h, int slot) { return step_m1(h, h->step_slots + 1 + slot); }

// The per-step moments of B solves from noise [B][nu][H][Kp] into output slot `slot`, behind enqueue_stats of the same
// solves (d_stats_w holds their weights).
static hipError_t enqueue_step_mom(mppi_handle* h, int B, const float* noise, int slot) {
  const mppi_config& c = h->cfg;
  const StepMomArgs sa{B, c.nu, c.H, h->shape.Kp, h->d_stats_w, noise, step_m1(h, slot), step_m2(h, slot)};
  return launch_step_moments(sa, h->stream);
}

// Behind the per-step moments of slot `slot`: every solve's rows of the table refit from its own moments and, with
// shift, moved along the horizon with the nominal (the fill: the model's sigma_u).
static hipError_t enqueue_step_adapt(mppi_handle* h, int B, int slot, bool shift) {
  const mppi_config& c = h->cfg;
  StepFill fill;
  std::memcpy(fill.sigma_u, h->noise_model.sigma_u, sizeof(fill.sigma_u));
  return launch_step_adapt(h->d_steps, step_m1(h, slot), step_m2(h, slot), h->d_stats + (size_t)slot * c.max_batch, B,
                           c.nu, c.H, shift ? 1 : 0, h->steps_adapt, fill, h->stream);
}

// the device covariance of an adapting handle (d_cov_law: the rejects counter, Sigma, sigma_u; d_cov: L, Sinv)
static CovLaw cov_law(const mppi_handle* h) {
  const size_t nu = (size_t)h->cfg.nu;
  float* S = h->d_cov_law + 2;
  return CovLaw{S, h->d_cov, h->d_cov + nu * kMaxNu, S + nu * nu, reinterpret_cast<unsigned long long*>(h->d_cov_law)};
}

// Behind the cross moments of slot `slot`: record the Sigma the solve drew from, move the device covariance one step.
static hipError_t enqueue_cov_adapt(mppi_handle* h, int B, int slot) {
  const mppi_config& c = h->cfg;
  const size_t nn = (size_t)c.nu * c.nu, off = (size_t)slot * c.max_batch;
  return launch_noise_cov_adapt(cov_law(h), h->d_cov_hist + (size_t)slot * nn, h->d_stats + off,
                                h->d_cross_mx + off * nn, B, c.nu, h->cov_adapt, h->stream);
}

// The per-solve lambdas of ESS targeting for `slots` solve slots (+ 1 for mppi_lambda_eval).  Growing them waits for the
// stream and forgets the values held so far.  Never called inside a capture.
static int ensure_lambda(mppi_handle* h, int slots) {
  if (slots <= h->lambda_slots) return MPPI_OK;
  HIP_TRY(hipStreamSynchronize(h->stream));
  if (h->d_lambda) (void)hipFree(h->d_lambda);
  h->d_lambda = nullptr;
  h->lambda_slots = 0;
  h->lam_B = h->lam_n = 0;
  const size_t n = (size_t)(slots + 1) * h->cfg.max_batch * 4;
  HIP_TRY(hipMalloc(&h->d_lambda, n));
  HIP_TRY(hipMemsetAsync(h->d_lambda, 0, n, h->stream));  // in stream order, ahead of the kernels that write slots
  h->lambda_slots = slots;
  return MPPI_OK;
}

// slot `slot` of the targeting handle's lambdas (nullptr while targeting is off: the by-value lambda)
static float* lambda_slot(const mppi_handle* h, int slot) {
  return h->ess_on ? h->d_lambda + (size_t)slot * h->cfg.max_batch : nullptr;
}

// the generators' law argument: the device law of an adapting handle, else nullptr (the by-value model)
static const float* gen_law(const mppi_handle* h) { return h->adapt_on ? h->d_law : nullptr; }
// ... and their table argument: the per-step scales of mppi_set_noise_steps, else nullptr
static const float* gen_steps(const mppi_handle* h) { return h->steps_on ? h->d_steps : nullptr; }

// Behind the statistics of slot `slot`: record the law the solve drew from, move the device law one step.
static hipError_t enqueue_adapt(mppi_handle* h, int B, int slot) {
  const mppi_config& c = h->cfg;
  const size_t off = (size_t)slot * c.max_batch;
  return launch_noise_adapt(h->d_law, h->d_law_hist + (size_t)slot * (c.nu + 1), h->d_stats + off,
                            h->d_stats_m2 + off * c.nu, h->d_stats_m11 + off * c.nu, B, c.nu, h->adapt, h->stream);
}

// The diagnostics of B solves from costs [B][Kp] and noise [B][nu][H][Kp] (or nullptr) into output slot `slot`.
// lambda_dev: the solves' own lambdas (ESS targeting), or nullptr: cfg.lambda.
static hipError_t enqueue_stats(mppi_handle* h, int B, const float* costs, const float* noise, int slot,
                                const float* lambda_dev = nullptr) {
  const mppi_config& c = h->cfg;
  const size_t off = (size_t)slot * c.max_batch;
  const StatsArgs sa{B, c.nu, c.H, h->shape.K, h->shape.Kp, c.lambda, c.norm_eps, costs, noise, h->d_stats_w, h->d_stats_part,
                     h->d_stats + off, h->d_stats_m2 + off * c.nu, h->d_stats_m11 + off * c.nu, lambda_dev};
  return launch_stats(sa, h->stream);
}

// The cross moments of B solves from noise [B][nu][H][Kp] into output slot `slot`, behind enqueue_stats of the same
// solves (d_stats_w holds their weights).
static hipError_t enqueue_cross(mppi_handle* h, int B, const float* noise, int slot) {
  const mppi_config& c = h->cfg;
  const CrossArgs ca{B, c.nu, c.H, h->shape.Kp, h->d_stats_w, noise, h->d_cross_part,
                     h->d_cross_mx + (size_t)slot * c.max_batch * c.nu * c.nu};
  return launch_cross(ca, h->stream);
}

// The control-cost launches of B solves into output slot `slot` (0: a solve, 1: mppi_control_term_eval): lin from U
// and the law, the term from lin and the noise, wcost = costs + term.
static hipError_t enqueue_ctrl(mppi_handle* h, int B, const float* U, const float* noise, const float* costs,
                               int slot) {
  const mppi_config& c = h->cfg;
  const size_t ok = (size_t)slot * c.max_batch * h->Kp, ol = (size_t)slot * c.max_batch * c.nu * c.H;
  CtrlArgs ca;
  std::memset(&ca, 0, sizeof(ca));
  ca.B = B;
  ca.nu = c.nu;
  ca.H = c.H;
  ca.K = h->shape.K;
  ca.Kp = h->shape.Kp;
  ca.U = U;
  ca.noise = noise;
  ca.costs = costs;
  ca.lin = h->d_lin + ol;
  ca.term = h->d_term + ok;
  ca.wcost = h->d_wcost + ok;
  ca.part = h->d_ctrl_part;
  ca.law.gamma = h->ctrl_gamma;
  ca.law.sigma = c.sigma;
  const NoiseModel& m = h->noise_model;
  ca.law.rho = m.active ? m.rho : 0.0f;
  ca.law.per_u = m.active;
  if (m.active) std::memcpy(ca.law.sigma_u, m.sigma_u, sizeof(ca.law.sigma_u));
  ca.d_law = gen_law(h);
  ca.sinv = m.cov_L ? h->d_cov + (size_t)c.nu * kMaxNu : nullptr;
  return launch_ctrl_cost(ca, h->stream);
}

// The bounds' launches of B solves.  Projection: noise [B][nu][H][Kp] in place against the nominal U.  Clip: the
// projection's counts summed into slot `slot` (0: a solve, 1: mppi_bounds_eval), and U, its mirror and u0 clipped
// behind the update (an evaluation passes none).
static BoundsArgs bounds_args(const mppi_handle* h, int B, int slot = 0) {
  const mppi_config& c = h->cfg;
  BoundsArgs ba;
  std::memset(&ba, 0, sizeof(ba));
  ba.B = B;
  ba.nu = c.nu;
  ba.H = c.H;
  ba.K = h->shape.K;
  ba.Kp = h->shape.Kp;
  ba.part = h->d_bpart;
  ba.counts = h->d_bcounts + (size_t)slot * c.max_batch * c.nu;
  std::memcpy(ba.lo, h->bounds_lo, sizeof(ba.lo));
  std::memcpy(ba.hi, h->bounds_hi, sizeof(ba.hi));
  return ba;
}

static hipError_t enqueue_bounds_project(mppi_handle* h, int B, const float* U, float* noise) {
  BoundsArgs ba = bounds_args(h, B);
  ba.noise = noise;
  ba.U = U;
  return launch_bounds_project(ba, h->stream);
}

// The rate term's launch of B solves into output slot `slot` (0: a solve, 1: mppi_rate_term_eval): the term from U, the
// noise and u_prev, wcost = costs + term.
static hipError_t enqueue_rate(mppi_handle* h, int B, const float* U, const float* noise, const float* u_prev,
                               const float* costs, int slot) {
  const mppi_config& c = h->cfg;
  const size_t ok = (size_t)slot * c.max_batch * h->Kp;
  RateArgs ra;
  std::memset(&ra, 0, sizeof(ra));
  ra.B = B;
  ra.nu = c.nu;
  ra.H = c.H;
  ra.K = h->shape.K;
  ra.Kp = h->shape.Kp;
  ra.anchor = h->rate_anchor;
  ra.clamp = c.ctrl_clamp;
  ra.U = U;
  ra.noise = noise;
  ra.u_prev = u_prev;
  ra.costs = costs;
  ra.term = h->d_rate_term + ok;
  ra.wcost = h->d_rate_wcost + ok;
  ra.part = h->d_rate_part;
  std::memcpy(ra.r, h->rate_r, sizeof(ra.r));
  return launch_rate_cost(ra, h->stream);
}

// The elite selection of B solves on `costs` [B][Kp] into output slot `slot` (0: a solve, 1: mppi_elites_eval).
static hipError_t enqueue_elite(mppi_handle* h, int B, const float* costs, int slot) {
  const mppi_config& c = h->cfg;
  const size_t ob = (size_t)slot * c.max_batch;
  return launch_elite_select(costs, B, h->shape.K, h->shape.Kp, h->elite_n, h->d_elite_wcost + ob * h->Kp,
                             h->d_elite_idx + ob * h->elite_n, h->d_elite_count + ob, h->d_elite_tau + ob, h->stream);
}

// Keep / shift elites: the launches' arguments for B solves on output / input slot `slot` (0: the handle's set, 1: the
// eval entries').
static KeepArgs keep_args(const mppi_handle* h, int B, const float* U, float* noise, int slot) {
  const mppi_config& c = h->cfg;
  const size_t ob = (size_t)slot * c.max_batch, n = (size_t)h->keep_n;
  KeepArgs ka;
  std::memset(&ka, 0, sizeof(ka));
  ka.B = B;
  ka.nu = c.nu;
  ka.H = c.H;
  ka.K = h->shape.K;
  ka.Kp = h->shape.Kp;
  ka.n_keep = h->keep_n;
  ka.pitch = keep_pitch(h->keep_n);
  ka.clamp = c.ctrl_clamp;
  ka.noise = noise;
  ka.U = U;
  ka.v = h->d_keep_v + ob * c.nu * c.H * ka.pitch;
  ka.kcost = h->d_keep_cost + ob * n;
  ka.idx = h->d_keep_idx + ob * n;
  ka.count = h->d_keep_count + ob;
  ka.steps = h->d_keep_steps + ob;
  return ka;
}

// The store of B solves into slot `slot`: the n_keep best of `costs` [B][Kp] (the unmasked end of the wcost chain)
// selected by elite_select.h's rule -- `shared`: the elites' selection of this solve ran on the same costs with
// n_elite == n_keep and its set (slot 0 of the elites' buffers) is the kept set; else a second launch of the same
// kernel into the feature's scratch -- then the gather.
static hipError_t enqueue_keep_store(mppi_handle* h, int B, const float* U, float* noise, const float* costs, int shift,
                                     bool shared, int slot) {
  KeepArgs ka = keep_args(h, B, U, noise, slot);
  ka.costs = costs;
  if (shared) {
    ka.sel_idx = h->d_elite_idx;
    ka.sel_count = h->d_elite_count;
  } else {
    const hipError_t e = launch_elite_select(costs, B, h->shape.K, h->shape.Kp, h->keep_n, h->d_keep_ecost, h->d_keep_sel,
                                             h->d_keep_selcount, h->d_keep_tau, h->stream);
    if (e != hipSuccess) return e;
    ka.sel_idx = h->d_keep_sel;
    ka.sel_count = h->d_keep_selcount;
  }
  return launch_keep_gather(ka, shift, h->stream);
}

// Validate one solve request against the handle.
static int check_solve(mppi_handle* h, int B, const mppi_io* io, int flags) {
  if (!h || !io) return fail(MPPI_E_ARG, "mppi_solve: null argument");
  const mppi_config& c = h->cfg;
  if (B < 1 || B > c.max_batch) return fail(MPPI_E_ARG, "mppi_solve: B out of range [1, max_batch]");
  if (h->dyn_kind == 0) return fail(MPPI_E_STATE, "mppi_solve: call mppi_load_dynamics first");
  if (h->cost_kind == 0) return fail(MPPI_E_STATE, "mppi_solve: call mppi_set_cost first");
  const bool dev = (flags & MPPI_FLAG_DEVICE) != 0;
  if (!io->x0) return fail(MPPI_E_ARG, "mppi_solve: x0 is required");
  if (!io->U && !(flags & MPPI_FLAG_RESIDENT_U)) return fail(MPPI_E_ARG, "mppi_solve: U is required unless MPPI_FLAG_RESIDENT_U");
  if (dev && (flags & MPPI_FLAG_COLMAJOR)) return fail(MPPI_E_ARG, "mppi_solve: MPPI_FLAG_COLMAJOR applies to host arrays only");
  if ((flags & MPPI_FLAG_ENV_STEP) && !dev) return fail(MPPI_E_ARG, "mppi_solve: MPPI_FLAG_ENV_STEP needs MPPI_FLAG_DEVICE");
  if (h->dyn_kind == MPPI_DYN_CARTPOLE && h->cost_kind != MPPI_COST_CARTPOLE && h->cost_kind != MPPI_COST_CARTPOLE_EST)
    return fail(MPPI_E_UNSUPPORTED, "cartpole dynamics take a cartpole cost (cartpole or cartpole_est)");
  if (h->dyn_kind == MPPI_DYN_CARTPOLE && (c.nx != 4 || c.nu != 1))
    return fail(MPPI_E_UNSUPPORTED, "cartpole dynamics need nx=4, nu=1");
  if ((h->dyn_kind == MPPI_DYN_MLP || h->dyn_kind == MPPI_DYN_CROSS_ATTN) && h->net.arch != kArchGeneric &&
      (c.nx > kMaxNx || c.nu > kMaxNu))
    return fail(MPPI_E_UNSUPPORTED, "learned dynamics: nx <= 64, nu <= 32");
  if (io->noise && h->pop_n > 0)
    return fail(MPPI_E_UNSUPPORTED, "mppi_solve: injected noise with a mppi_set_population table (the iterations' "
                                    "sample counts differ)");
  if (io->noise && h->iter_n > 1)
    return fail(MPPI_E_ARG, "mppi_solve: injected noise with mppi_set_iterations n_iter > 1 (one array cannot serve "
                            "every iteration)");
  if ((flags & MPPI_FLAG_U0_BEFORE) && h->iter_n > 1)
    return fail(MPPI_E_UNSUPPORTED, "mppi_solve: MPPI_FLAG_U0_BEFORE with mppi_set_iterations n_iter > 1");
  if ((flags & MPPI_FLAG_U0_BEFORE) && h->iter_best)
    return fail(MPPI_E_UNSUPPORTED, "mppi_solve: MPPI_FLAG_U0_BEFORE with mppi_set_iterations return_best");
  return MPPI_OK;
}

// member: which model of an ensemble rolls (mppi_set_ensemble); 0, every handle without one: what mppi_load_dynamics loaded
static hipError_t launch_rollout(mppi_handle* h, const SolveArgs& a, hipStream_t s, int member = 0) {
  const mppi_handle::Member* m = member > 0 ? &h->ens_mem[member] : nullptr;
  if (h->dyn_kind == MPPI_DYN_CARTPOLE) return launch_cartpole_rollout(a, m ? m->cart : h->cart, nullptr, s);
  if (h->dyn_kind == MPPI_DYN_FEATURE_ATTN) return launch_fa_rollout(a, m ? m->fa : h->fa, s);
  const FcNet& env = m ? m->net_env : h->net_env;
  if (a.xout && env.fa.img) return launch_fc_rollout(a, env, s);  // the split mode's env step: exact fp32
  return launch_fc_rollout(a, m ? m->net : h->net, s);
}

// A graph launch leaves the next launch's first noise prefetched, generated with one counter value ahead.  When
// that noise will not be used (a plain solve comes next, or a re-capture for another batch/seed), the counter is
// stepped back so the next consumer draws exactly the key the prefetch took: the key sequence of any interleaving
// of plain solves and graph launches equals a loop of plain solves.
static hipError_t drop_prefetch(mppi_handle* h) {
  // (every caller goes on to write d_noise, or to draw the buffers again: nothing is pristine until a generator says so)
  h->pristine[0].ok = h->pristine[1].ok = false;
  if (const hipError_t e = wait_gen(h); e != hipSuccess) return e;
  if (!h->prefetch_valid) return hipSuccess;
  h->prefetch_valid = false;
  return launch_seed_bump(h->d_seed_ctr, -1, h->stream);
}

// Graph mode (captured streams of solves): this solve's noise is already in `cur` (generated by the previous
// solve's reduce, or primed by mppi_graph_launch); this solve's reduce writes the next solve's into `next`.
// overlap (chained solves; chain_iter): the next noise may be drawn BESIDE this solve's rollout on the generator stream,
// which chain_iter has already ordered behind the previous reduce -- kGenForced: it is; kGenByFit: it is if the routed
// rollout kernel leaves room for the generator's wave (gen_overlap.h gen_fits), else the reduce draws it as without.
enum { kGenFused = 0, kGenForced = 1, kGenByFit = 2 };
struct NoiseStep {
  float* cur;
  float* next;
  int overlap = kGenFused;
};

// reduce_regen.h's content side.  noise_slot: which of the pair a noise pointer is; noise_drawn: a generator was enqueued
// that writes all of it for B solves at pitch Kp with the key word beside it (plain: noise_kernel, noise_beside_kernel
// or reduce_kernel<GEN>, the three that evaluate one function); noise_written: anything else wrote into it.  A capture
// records launches that run later, any number of times: it leaves the host's view alone, and mppi_graph_launch clears it
static int noise_slot(const mppi_handle* h, const float* noise) { return h->d_noise2 && noise == h->d_noise2 ? 1 : 0; }
static void noise_drawn(mppi_handle* h, const float* noise, bool plain, int B, int Kp) {
  if (h->capturing) return;
  mppi_handle::Pristine& p = h->pristine[noise_slot(h, noise)];
  p.ok = plain;
  p.B = B;
  p.Kp = Kp;
}
static void noise_written(mppi_handle* h, const float* noise) {
  if (!h->capturing) h->pristine[noise_slot(h, noise)].ok = false;
}
static bool noise_pristine(const mppi_handle* h, const float* noise, int B, int Kp) {
  const mppi_handle::Pristine& p = h->pristine[noise_slot(h, noise)];
  return !h->capturing && p.ok && p.Kp == Kp && p.B >= B;
}

// registers per wave of a kernel of this library (hipFuncGetAttributes, once per kernel and handle; 0: unknown)
static int func_regs(mppi_handle* h, const void* f) {
  if (!f) return 0;
  for (const auto& e : h->func_regs)
    if (e.first == f) return e.second;
  hipFuncAttributes at;
  const int n = hipFuncGetAttributes(&at, f) == hipSuccess ? at.numRegs : 0;
  if (n <= 0) (void)hipGetLastError();
  h->func_regs.emplace_back(f, n);
  return n;
}

// the options of a solve enqueued (or captured) now with these flags
static SolveOpts solve_opts(const mppi_handle* h, int flags) {
  SolveOpts o;
  o.stats = (flags & MPPI_FLAG_STATS) != 0;
  o.cross = (flags & MPPI_FLAG_CROSS) != 0;
  o.cov_adapt = h->cov_adapt_on;
  o.adapt = h->adapt_on;
  o.ess = h->ess_on;
  o.ctrl = h->ctrl_gamma > 0.0f;
  o.bounds = h->bounds_on;
  o.rate = h->rate_on;
  o.elite = h->elite_n > 0;
  o.keep = h->keep_n > 0;
  o.step_mom = (flags & MPPI_FLAG_STEP_MOMENTS) != 0;
  o.step_adapt = h->steps_adapt_on;
  o.iter = h->iter_on();
  o.ens = h->ens_n > 1;
  return o;
}

// n solves of batch B with these options were enqueued (a plain or chained solve: its n_iter iterations, slots 0..; a
// graph launch: its solves' iterations, iteration it of solve i in slot i n_iter + it): what the getters may read from
// now on.  The options without per-step slots keep the chain's last solve.
static void note_ran(mppi_handle* h, const SolveOpts& o, int B, int n) {
  if (o.stats) {
    h->stats_B = B;
    h->stats_n = n;
  }
  if (o.cross) {
    h->cross_B = B;
    h->cross_n = n;
  }
  if (o.adapt) h->law_n = n;
  if (o.cov_adapt) h->cov_law_n = n;
  if (o.ess) {
    h->lam_B = B;
    h->lam_n = n;
  }
  if (o.ctrl) h->ctrl_B = B;
  if (o.bounds) h->bounds_B = B;
  if (o.rate) h->rate_B = B;
  if (o.elite) h->elite_B = B;
  if (o.keep && B > h->keep_B) h->keep_B = B;  // (slots beyond B keep the set they hold)
  if (o.step_mom) {
    h->stepm_B = B;
    h->stepm_n = n;
  }
  if (o.iter) h->best_B = B;
  if (o.ens) h->ens_B = B;
}

// One iteration of a control step (mppi_set_iterations): its index and the step's count.  The first iteration stages the
// step's inputs and the last copies its outputs; with host pointers the iterations between run on the staged copies
// (d_x0, d_ctx, d_U), which hold bit for bit what a host round trip would bring back.
struct IterStep {
  int it, n;
};
// the flags iteration `it` of n carries: all but the last neither shift nor step the environment
static int iter_flags(int flags, int it, int n) {
  return it + 1 < n ? flags & ~(MPPI_FLAG_SHIFT | MPPI_FLAG_ENV_STEP) : flags;
}

// Enqueue one solve on the handle's stream: inputs, noise, rollout, reduce (+ update, shift), env step, outputs.
// Synchronises only for host-side column-major staging. Capturable into a hipGraph in device mode.
static int enqueue_solve(mppi_handle* h, int B, const mppi_io* io, uint64_t seed, int flags, float* rec_x = nullptr,
                         float* rec_u = nullptr, const NoiseStep* ns = nullptr, int stats_slot = 0,
                         const IterStep* is = nullptr) {
  const mppi_config& c = h->cfg;
  const bool dev = (flags & MPPI_FLAG_DEVICE) != 0;
  const bool resident = (flags & MPPI_FLAG_RESIDENT_U) != 0;
  const bool colmajor = (flags & MPPI_FLAG_COLMAJOR) != 0;
  hipStream_t s = h->stream;
  const int it = is ? is->it : 0;
  // population-size decay: this iteration's own sample count and pitch -- every launch below, and every helper through
  // h->shape, is the solve of a handle created with cfg.K = K; the next iteration's pitch is what the generators of
  // ns->next write (the step's last iteration is followed by the next step's first: the full pitch).  No table: cfg.K
  // and h->Kp, all three
  const mppi_handle::Shape sh = h->iter_shape(it);
  const ShapeScope shape_scope(h, sh);
  const int nx = c.nx, nu = c.nu, H = c.H, K = sh.K, Kp = sh.Kp;
  const int Kp_next = h->iter_shape(is && is->it + 1 < is->n ? is->it + 1 : 0).Kp;
  const size_t rowsU = (size_t)B * nu * H;
  const bool first = it == 0, last = !is || is->it + 1 == is->n;  // of the control step's iterations

  SolveArgs a;
  std::memset(&a, 0, sizeof(a));
  a.B = B;
  a.nx = nx;
  a.nu = nu;
  a.H = H;
  a.K = K;
  a.Kp = Kp;
  a.lambda = c.lambda;
  a.ctrl_clamp = c.ctrl_clamp;
  a.U_clamp = c.U_clamp;
  a.norm_eps = c.norm_eps;
  a.shift_fill = c.shift_fill;
  a.terminal_weight = c.terminal_weight;
  a.update_mode = c.update_mode;
  a.flags = flags & ~(MPPI_FLAG_STATS | MPPI_FLAG_CROSS | MPPI_FLAG_STEP_MOMENTS);  // (host-side only: the kernels see the arguments of a solve without it)
  a.cost_kind = h->cost_kind;
  std::memcpy(a.ctx_default, h->cost_params, sizeof(a.ctx_default));
  a.noise = ns ? ns->cur : h->d_noise;
  // the device word beside a noise buffer: the key its generator records there (reduce_regen.h)
  auto key_word = [&](const float* noise) { return h->d_nkey + noise_slot(h, noise); };
  a.costs = h->d_costs;
  a.dU = h->d_dU;
  a.weights = io->weights ? h->d_weights : nullptr;
  a.u0 = (dev && io->u0) ? io->u0 : h->d_u0;  // device mode: kernels write u0 straight to the caller
  a.status = h->d_status;
  a.tickets = h->d_tickets;
  a.seed_ctr = (flags & MPPI_FLAG_SEED_COUNTER) ? h->d_seed_ctr : nullptr;
  a.seed_bump = ns ? nullptr : a.seed_ctr;  // graph mode: reduce_kernel<GEN> advances the counter instead
  a.xout = nullptr;
  // ESS targeting: the solve's slot of lambdas, written by the search between the rollout and the reduce (below)
  float* const lam = lambda_slot(h, stats_slot);
  a.lambda_dev = lam;
  // o.ctrl: the softmin weighs d_wcost = costs + term; o.rate: d_rate_wcost = (costs [+ control term]) + rate term;
  // o.elite: d_elite_wcost, the chain's end on the elite set (below)
  const SolveOpts o = solve_opts(h, flags);
  const bool cart_unfused =
      (lam || o.ctrl || o.rate || o.elite || o.keep || o.iter || o.ens) && h->dyn_kind == MPPI_DYN_CARTPOLE;
  int iter_count = 1;  // "iter" is counted once per iteration, by the first of its launches
  // launch clock: only solves that use the seed counter are stamped (bench.py's timed paths); the cartpole's unfused
  // rollout carries no stamp
  a.kclock = (h->kclock && a.seed_ctr && !cart_unfused) ? h->d_kclock : nullptr;
  a.kclock_ctr = h->d_kclock ? h->d_kclock + 2 * (size_t)kClockSlots : nullptr;
  a.kclock_ticket = h->d_kclock ? reinterpret_cast<unsigned*>(h->d_kclock + 2 * (size_t)kClockSlots + 1) : nullptr;
  // graph replays count graph_n each (mppi_graph_launch); an ensemble stamps every member's launch
  if (a.kclock && !h->capturing) h->kclock_launches += o.ens ? h->ens_n : 1;

  // ---- inputs
  if (dev) {
    a.x0 = io->x0;
    a.ctx = io->ctx;
    a.U = resident ? h->d_U : io->U;
    a.Umirror = (resident && io->U) ? io->U : nullptr;  // written by the update kernels themselves
  } else {
    if (first) HIP_TRY(hipMemcpyAsync(h->d_x0, io->x0, (size_t)B * nx * 4, hipMemcpyHostToDevice, s));
    a.x0 = h->d_x0;
    if (io->ctx && first)
      HIP_TRY(hipMemcpyAsync(h->d_ctx, io->ctx, (size_t)B * MPPI_CTX_MAX * 4, hipMemcpyHostToDevice, s));
    a.ctx = io->ctx ? h->d_ctx : nullptr;
    a.U = h->d_U;
    if (!resident && first) {
      const float* src = io->U;
      if (colmajor) {  // Julia U (nu,H) column-major -> [nu][H]
        h->staging.resize(rowsU);
        transpose_batched(h->staging.data(), io->U, B, H, nu);
        src = h->staging.data();
      }
      HIP_TRY(hipMemcpyAsync(h->d_U, src, rowsU * 4, hipMemcpyHostToDevice, s));
      if (colmajor) HIP_TRY(hipStreamSynchronize(s));  // staging reused below
    }
  }

  // ---- a1: noise
  if (io->noise) {
    const float* src = io->noise;
    std::vector<float> tmp;
    if (colmajor) {  // Julia noise (nu,H,K) column-major -> [nu][H][K]
      tmp.resize(rowsU * K);
      for (int b = 0; b < B; ++b)
        for (int k = 0; k < K; ++k)
          for (int t = 0; t < H; ++t)
            for (int u = 0; u < nu; ++u)
              tmp[(((size_t)b * nu + u) * H + t) * K + k] = io->noise[(((size_t)b * K + k) * H + t) * nu + u];
      src = tmp.data();
    }
    MPPI_TRY(stage_noise(h, src, rowsU, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
    if (!tmp.empty()) HIP_TRY(hipStreamSynchronize(s));
    noise_written(h, a.noise);
  } else if (!ns) {
    HIP_TRY(timed(h, kNoise, [&] {
      return launch_noise_model(a.noise, B, nu, H, Kp, seed, a.seed_ctr, c.sigma, h->noise_model, s, gen_law(h),
                                gen_steps(h), key_word(a.noise));
    }));
    noise_drawn(h, a.noise, !h->noise_model.active, B, Kp);
  }

  // keep / shift elites: the stored set into the first columns of this solve's noise, behind whatever filled it -- the
  // launch above, the copy of an injected io.noise (never the caller's array), or, for ns, the previous solve's fused
  // generator (reduce_kernel<GEN>, earlier on this stream), its gen_after launch (likewise), the overlap arm's
  // generator stream (chain_solve waits on ev_gen ahead of this call) or prime_prefetch (on this stream) -- and ahead of
  // the bounds projection and the rollout.  The x3 probe runs before any of this with buffers of its own and the env
  // step reads d_env_noise: neither sees the injection.  count and steps are read on the device: the launch is there
  // for every solve of a handle with the feature on and changes nothing while the set is empty
  if (o.keep) {
    HIP_TRY(timed(h, kKeep, [&] { return launch_keep_inject(keep_args(h, B, a.U, a.noise, 0), s); }));
    noise_written(h, a.noise);
  }

  // add_mean (mppi_set_iterations), the step's last iteration: the column behind the carried set zeroed, so the nominal
  // itself is one of the candidates -- behind the injection (which never writes that column) and ahead of the bounds
  // projection and the rollout.  The kept set's count is read on the device, as the injection reads it
  if (o.iter && h->iter_mean && last) {
    HIP_TRY(timed(h, kIter, [&] {
      return launch_iter_mean(a.noise, o.keep ? h->d_keep_count : nullptr, h->keep_n, B, nu, H, K, Kp, s);
    }, iter_count));
    iter_count = 0;
    noise_written(h, a.noise);
  }

  // per-actuator bounds: the solve's noise -- drawn above, prefetched by the previous solve's generator, or the copy of
  // an injected io.noise (never the caller's array) -- projected in place against the nominal U, ahead of the rollout
  // and of every other reader of this solve's noise
  if (o.bounds) {
    HIP_TRY(timed(h, kBounds, [&] { return enqueue_bounds_project(h, B, a.U, a.noise); }));
    noise_written(h, a.noise);
  }
  // the reduce may regenerate part of this solve's noise instead of reading it (reduce_regen.h): the content side, now
  // that everything that writes a.noise ahead of the rollout is enqueued, and the knob (read per launch)
  const bool regen_ok = noise_pristine(h, a.noise, B, Kp);
  const int regen_force = regen_knob(std::getenv("MPPI_REDUCE_REGEN"));
  h->reduce_regen = 0;

  // ---- a2-a6: rollout + cost; a7-a9: softmin + weighted-noise reduce + update + shift
  const NoiseGen gen{ns ? ns->next : nullptr, seed, c.sigma, h->d_gticket, Kp_next != Kp ? Kp_next : 0,
                     ns && ns->next ? key_word(ns->next) : nullptr};
  // an active noise model's rows depend on the row before them, which the fused generators (one row at a time, in
  // reduce order) cannot give: the next noise then comes from its own launch behind the reduce (below)
  // (ov: the overlap the chain asked for; the analytic cartpole's fused launch generates inside the rollout, whose
  // registers nobody reads ahead of it: by fit it stays fused)
  int ov = ns && ns->next ? ns->overlap : kGenFused;
  if (ov == kGenByFit && (h->dyn_kind == MPPI_DYN_CARTPOLE || h->noise_model.active)) ov = kGenFused;
  bool gen_after = ns && ns->next && ov != kGenForced && h->noise_model.active;
  const NoiseGen* pg = ns && ns->next && ov != kGenForced && !gen_after ? &gen : nullptr;
  // population-size decay, an A/B knob read per launch: MPPI_GEN_TWO_PITCH=0 takes the next noise at another pitch out
  // of the reduce into a launch of its own behind it (noise_kernel; the reduce keeps GEN's block, so the bits stay);
  // =shrink / =grow keep the two-pitch form only where the next pitch is the smaller / the larger.  Unset: the
  // two-pitch form at every such boundary (DESIGN.md section 4 has the measurements)
  bool two_sep = false;
  if (pg && Kp_next != Kp) {
    const int side = env_choice("MPPI_GEN_TWO_PITCH", "shrink", "grow");
    two_sep = env_flag("MPPI_GEN_TWO_PITCH") == 0 || (side == 1 && Kp_next > Kp) || (side == 2 && Kp_next < Kp);
  }
  // the generator stream's launches, directly behind the rollout's on the host: the next noise into ns->next (the
  // stream is ordered behind the previous reduce, which read that buffer), then the counter bump -- the generator stream
  // alone reads and bumps the key counter while the overlap runs, in launch order -- and ev_gen for the next consumer
  auto gen_beside = [&]() -> int {
    if (h->noise_model.active)
      HIP_TRY(launch_noise_model(ns->next, B, nu, H, Kp_next, seed, h->d_seed_ctr, c.sigma, h->noise_model, h->gstream,
                                 nullptr, gen_steps(h)));
    else
      HIP_TRY(launch_noise_beside(ns->next, B, nu, H, Kp_next, seed, h->d_seed_ctr, c.sigma, h->gstream,
                                  key_word(ns->next)));
    noise_drawn(h, ns->next, !h->noise_model.active, B, Kp_next);
    HIP_TRY(launch_seed_bump(h->d_seed_ctr, 1, h->gstream));
    HIP_TRY(hipEventRecord(h->ev_gen, h->gstream));
    h->gen_pending = true;
    // the solve stream waits for it right here, ahead of this solve's reduce (the generator ends well inside the
    // rollout it runs beside): whatever follows on the stream -- the next solve, a stream switch, a counter read --
    // finds the noise written and the counter bumped.  Each cross-stream packet costs the stream ~6 us (kernel
    // trace: 6.5 us between rollout and reduce for this wait, 7.5 us between reduce and rollout for ev_red's record)
    HIP_TRY(wait_gen(h));
    return MPPI_OK;
  };
  float* wcost = a.costs;  // what the search, the reduce and the statistics weigh: the end of the chain below
  if (h->dyn_kind == MPPI_DYN_CARTPOLE && !cart_unfused) {  // one launch: the rollout blocks finish the solve (fused)
    a.part = h->d_part;
    HIP_TRY(timed(h, kRollout, [&] { return launch_cartpole_rollout(a, h->cart, pg, s); }));
    h->rollout_kernel = h->iter_kernel[it] = g_rollout_kernel;
    if (pg) noise_written(h, ns->next);  // (its generator records no key)
    if (ov == kGenForced) MPPI_TRY(gen_beside());
  } else {
    // (a targeting cartpole too: its fused epilogue forms the softmin partials with lambda before all costs exist, so
    // it runs the unfused rollout of the env step, a.part == nullptr, then the search and reduce_kernel: 3 launches;
    // and a cartpole with the control-cost or the rate term, whose epilogue would weigh costs the term has not reached
    // yet, or with elites or kept elites, whose selection needs every cost of the solve)
    // an ensemble (mppi_set_ensemble): member e rolls the same x0, U, ctx and noise into row e of the members' costs --
    // rows max_batch * Kp apart whatever this iteration's shape, each written densely at it.  Member 0 first: the
    // kernel reports, the fit decision of the noise overlap and the generator beside the rollout are its launch's
    auto member_args = [&](int e) {
      SolveArgs m = a;
      m.costs = h->d_ens_costs + (size_t)e * c.max_batch * h->Kp;
      return m;
    };
    HIP_TRY(timed(h, kRollout, [&] { return launch_rollout(h, o.ens ? member_args(0) : a, s); }));
    h->rollout_kernel = h->iter_kernel[it] = g_rollout_kernel;
    if (ov == kGenByFit) {  // the rule's last condition, on the kernel this very launch (this iteration's) was routed to
      if (gen_fits(func_regs(h, g_rollout_func), func_regs(h, noise_beside_func()))) {
        ov = kGenForced;
        pg = nullptr;  // the read-only reduce
      } else {
        ov = kGenFused;
      }
    }
    if (two_sep && pg) {  // (the overlap did not take it: the separate launch behind the reduce, below)
      gen_after = true;
      pg = nullptr;
    } else {
      two_sep = false;
    }
    // a forced share (MPPI_REDUCE_REGEN=1..7) reaches the fused route too, by the same separation: the next noise in a
    // launch of its own behind the reduce, which keeps GEN's block and becomes a read-only form (the rule by itself
    // leaves the fused routes alone: their vector ALUs are taken, or their reduce is latency-bound)
    bool regen_sep = false;
    if (pg && regen_force > 0 && regen_ok) {
      regen_sep = gen_after = true;
      pg = nullptr;
    }
    if (ov == kGenForced) MPPI_TRY(gen_beside());
    if (o.ens) {
      // the members behind member 0, in order on the stream, then the one combining launch: d_costs and the spread
      // from the n rows.  From here on the solve is the single-model solve on those costs
      for (int e = 1; e < h->ens_n; ++e)
        HIP_TRY(timed(h, kRollout, [&] { return launch_rollout(h, member_args(e), s, e); }));
      const EnsembleArgs ea{h->ens_n, h->ens_mode, h->ens_kappa, ensemble_rcp(h->ens_n), (long)B * Kp / 4,
                            (long)c.max_batch * h->Kp, h->d_ens_costs, a.costs, h->d_ens_sd};
      HIP_TRY(timed(h, kEnsemble, [&] { return launch_ensemble(ea, s); }));
    }
    if (o.ctrl) {
      // the control-cost term, behind the rollout (its costs exist) and ahead of the reduce (a.U is still the nominal the
      // rollout perturbed).  An adapting handle's ctrl_lin_kernel reads d_law on the stream: at this point it still
      // holds the law that drew THIS solve's noise -- the adapt kernel runs behind the reduce and the statistics
      // (below), and the generators of the next solve's noise behind that
      HIP_TRY(timed(h, kCtrl, [&] { return enqueue_ctrl(h, B, a.U, a.noise, a.costs, 0); }));
      wcost = h->d_wcost;
    }
    if (o.rate) {
      // the rate term, behind the control-cost term (wcost = (costs + control term) + rate term, in this order) and ahead
      // of the reduce: a.U is still the nominal the rollout perturbed, a.noise what the rollout saw (projected, with
      // bounds on), d_uprev the control the previous step applied (its store sits behind that step's update, below)
      HIP_TRY(timed(h, kRate, [&] { return enqueue_rate(h, B, a.U, a.noise, h->d_uprev, wcost, 0); }));
      wcost = h->d_rate_wcost;
    }
    const float* const sel_cost = wcost;  // the unmasked end of the chain: what the selections and the tracking read
    if (o.elite) {
      // elite truncation, behind the terms (it selects on what the softmin would otherwise weigh) and ahead of the lambda
      // search: the search, the reduce and the statistics see the cost on the elite set and +inf elsewhere
      HIP_TRY(timed(h, kElites, [&] { return enqueue_elite(h, B, wcost, 0); }));
      if (!o.keep) wcost = h->d_elite_wcost;
    }
    if (o.keep) {
      // keep / shift elites: this solve's n_keep best by the unmasked chain (wcost is still the selection's input),
      // gathered behind the terms and the elites' selection (whose set serves both when n_elite == n_keep) and ahead of
      // the lambda search and the reduce: a.U is still the nominal the rollout perturbed, a.noise what the rollout saw
      // (injected, then projected with bounds on).  The gather overwrites the set the injection above read, on the
      // same stream behind it (its time joins "keep", counted once per solve above)
      const bool shared = o.elite && h->elite_n == h->keep_n;
      HIP_TRY(timed(h, kKeep, [&] {
        return enqueue_keep_store(h, B, a.U, a.noise, wcost, (flags & MPPI_FLAG_SHIFT) != 0, shared, 0);
      }, 0));
      if (o.elite) wcost = h->d_elite_wcost;
    }
    if (o.iter) {
      // the best sample of the step so far (mppi_set_iterations), on the unmasked chain like the keep store and at the
      // same place: a.U is still the nominal the rollout perturbed, a.noise what the rollout saw
      IterBestArgs ia{B, nu, H, K, Kp, first ? 1 : 0, it, c.ctrl_clamp, sel_cost, a.noise, a.U,
                      h->d_best_v, h->d_best_cost, h->d_best_k, h->d_best_iter};
      HIP_TRY(timed(h, kIter, [&] { return launch_iter_best(ia, s); }, iter_count));
      iter_count = 0;
    }
    if (lam)
      HIP_TRY(timed(h, kLambda, [&] { return launch_lambda_search(wcost, B, K, Kp, h->ess, c.lambda, lam, s); }));
    SolveArgs r = a;  // the reduce's arguments: a's, weighing wcost
    r.costs = wcost;
    // the share of its noise the reduce regenerates: none for the fused reduce + generate
    const RegenArgs rg{pg ? 0 : regen_share(regen_ok, regen_noise_bytes(B, nu, H, Kp), regen_force), key_word(a.noise),
                       c.sigma};
    HIP_TRY(timed(h, kReduce, [&] {
      return launch_reduce(r, pg, s, ov == kGenForced || two_sep || regen_sep, rg.eighths ? &rg : nullptr);
    }));
    h->reduce_regen = rg.eighths;
    if (pg) noise_drawn(h, ns->next, true, B, Kp_next);  // reduce_kernel<GEN> drew it, key word included
  }
  // return_best (mppi_set_iterations), the step's last iteration: u0 becomes the first control of the step's best sample
  // -- behind the update and shift (U, the nominal that warm-starts the next step, is untouched), ahead of the clip (so
  // lo <= u0 <= hi still holds exactly), of the u_prev store, the trajectory record and the env step.  A step without
  // a finite sample keeps the update's u0
  if (o.iter && h->iter_best && last)
    HIP_TRY(timed(h, kIter, [&] { return launch_iter_apply(h->d_best_v, h->d_best_k, a.u0, B, nu, H, s); }, iter_count));
  // per-actuator bounds: behind the update and shift (the cartpole's fused epilogue included), ahead of the env step,
  // the trajectory record and the output copies, U, its mirror and u0 are clipped: this removes the last rounding of
  // U + sum w (v - U), brings a shift-filled last column into a box that excludes zero, and makes lo <= U, u0 <= hi
  // hold exactly whatever the update mode and flags; the same launch sums the projection's counts (its time joins
  // "bounds", counted once per solve above)
  if (o.bounds)
    HIP_TRY(timed(h, kBounds, [&] { return launch_bounds_clip(bounds_args(h, B), a.U, a.Umirror, a.u0, s); }, 0));
  // the rate term's anchor: the u0 this solve returns (clipped above; the pre-update column with MPPI_FLAG_U0_BEFORE) is
  // what the next step differences its t = 0 against -- one small launch behind the update and the clip, ahead of the
  // env step, so chained and captured streams anchor step i + 1 to step i with no host round trip (its time joins
  // "rate_cost", counted once per solve above)
  if (o.rate && h->rate_anchor && (flags & MPPI_FLAG_SHIFT))
    HIP_TRY(timed(h, kRate, [&] { return launch_rate_store_prev(a.u0, h->d_uprev, B * nu, s); }, 0));
  // diagnostics (MPPI_FLAG_STATS): read-only on this solve's costs and noise, behind the reduce (or the cartpole's fused
  // epilogue) and ahead of everything that may write a.noise -- the next solve's generators, on this stream or ordered
  // behind it (ev_red), only ever write the OTHER buffer of the pair before this point
  if (o.stats)
    HIP_TRY(timed(h, kStats, [&] { return enqueue_stats(h, B, wcost, a.noise, stats_slot, lam); }));
  // the cross moments (MPPI_FLAG_CROSS; every such solve carries MPPI_FLAG_STATS): behind the statistics, whose weights
  // they read, and like them ahead of everything that may write a.noise
  if (o.cross) HIP_TRY(timed(h, kCross, [&] { return enqueue_cross(h, B, a.noise, stats_slot); }));
  // the adapted law (mppi_set_noise_adapt; every such solve carries the flag): one wave directly behind the statistics
  // and ahead of the launch below that draws the next solve's noise, so chained and captured streams draw solve i + 1
  // from the law adapted on solve i, as a loop of plain solves does
  if (o.adapt) HIP_TRY(timed(h, kStats, [&] { return enqueue_adapt(h, B, stats_slot); }));
  // the adapted covariance (mppi_set_noise_cov_adapt; every such solve carries MPPI_FLAG_CROSS): one block directly
  // behind the cross moments and, like the law's kernel above, ahead of the launch that draws the next solve's noise
  // from L; this solve's control-cost term (far above) has read the Sinv its own noise was drawn under
  if (o.cov_adapt) HIP_TRY(timed(h, kCovAdapt, [&] { return enqueue_cov_adapt(h, B, stats_slot); }));
  // the per-step moments (MPPI_FLAG_STEP_MOMENTS; every such solve carries MPPI_FLAG_STATS): one more pass over a.noise
  // behind the statistics, whose weights it reads, and like them ahead of everything that may write a.noise
  if (o.step_mom) HIP_TRY(timed(h, kStepMom, [&] { return enqueue_step_mom(h, B, a.noise, stats_slot); }));
  // the refit of the per-step scales (mppi_set_noise_steps_adapt; every such solve carries the flag): directly behind
  // the moments and, like the laws' kernels above, ahead of the launch that draws the next solve's noise from the table
  if (o.step_adapt)
    HIP_TRY(timed(h, kStepAdapt, [&] {
      return enqueue_step_adapt(h, B, stats_slot, (flags & MPPI_FLAG_SHIFT) != 0);
    }));
  if (ns && ns->next) h->gen_route = ov == kGenForced ? kGenRouteOverlap : kGenRouteFused;
  if (gen_after) {  // the overlap arm's key and counter protocol, on the solve stream: noise with seed + counter, bump
    HIP_TRY(timed(h, kNoise, [&] {
      return launch_noise_model(ns->next, B, nu, H, Kp_next, seed, h->d_seed_ctr, c.sigma, h->noise_model, s,
                                gen_law(h), gen_steps(h), key_word(ns->next));
    }));
    HIP_TRY(launch_seed_bump(h->d_seed_ctr, 1, s));
    noise_drawn(h, ns->next, !h->noise_model.active, B, Kp_next);
  }

  // ---- env step: x0 <- f(x0, u0), the rollout kernel over one sample, one step, zero noise, U = u0, final
  // state written straight back to x0.  Kp = 16 makes it ONE 16-sample group (fc: one block; FA: one block;
  // cartpole: only wave 0 works), so every read of x0 precedes the single writer's store in program order or
  // behind the kernel's own barriers.
  if (flags & MPPI_FLAG_ENV_STEP) {
    SolveArgs e = a;
    e.K = 1;
    e.Kp = 16;
    e.H = 1;
    e.U = a.u0;  // [B][nu] == [B][nu][1]
    e.noise = h->d_env_noise;
    e.costs = h->d_env_costs;
    e.weights = nullptr;
    e.status = h->d_env_status;
    e.seed_ctr = nullptr;
    e.seed_bump = nullptr;
    e.part = nullptr;  // plain rollout (no fused epilogue)
    e.kclock = nullptr;
    e.terminal_weight = 0.0f;
    e.xout = const_cast<float*>(io->x0);
    if (rec_x) HIP_TRY(launch_record(io->x0, a.u0, rec_x, rec_u, B * nx, B * nu, s));
    HIP_TRY(launch_rollout(h, e, s, o.ens ? h->ens_env : 0));  // (an ensemble steps under its env_member)
  }

  // ---- outputs (the step's last iteration's: rows of cfg.K, of which that iteration's K samples are written -- with a
  // population table the rest of each row is left as the caller holds it)
  if (!last) return MPPI_OK;
  const hipMemcpyKind d2x = dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  if (io->costs)
    HIP_TRY(hipMemcpy2DAsync(io->costs, (size_t)c.K * 4, h->d_costs, (size_t)Kp * 4, (size_t)K * 4, B, d2x, s));
  if (io->weights)
    HIP_TRY(hipMemcpy2DAsync(io->weights, (size_t)c.K * 4, h->d_weights, (size_t)Kp * 4, (size_t)K * 4, B, d2x, s));
  if (io->u0 && !dev) HIP_TRY(hipMemcpyAsync(io->u0, h->d_u0, (size_t)B * nu * 4, d2x, s));
  h->Uhost.clear();
  if (!dev && (!resident || io->U)) {  // (RESIDENT_U with a host io.U: a copy of the resident U)
    if (colmajor) {
      h->Uhost.resize(rowsU);
      HIP_TRY(hipMemcpyAsync(h->Uhost.data(), h->d_U, rowsU * 4, hipMemcpyDeviceToHost, s));
    } else {
      HIP_TRY(hipMemcpyAsync(io->U, h->d_U, rowsU * 4, hipMemcpyDeviceToHost, s));
    }
  }
  return MPPI_OK;
}

// The device status word (bit 0: some solve had no finite cost).  The fc/FA rollouts reset it per launch; the fused
// cartpole epilogue only sets it, so it is cleared here once read (sticky between reads).  Read with the stream idle
// and reported under the entry's name.
static int report_status(mppi_handle* h, const char* entry) {
  unsigned st = 0;
  HIP_TRY(hipMemcpy(&st, h->d_status, 4, hipMemcpyDeviceToHost));
  if (st) HIP_TRY(hipMemset(h->d_status, 0, 4));
  if (st & 1u) return fail(MPPI_E_NONFINITE, std::string(entry) + ": every sample of some solve had a non-finite cost");
  return MPPI_OK;
}

// Wait for the stream, finish host-side layout conversion, report non-finite solves.
static int finish_solve(mppi_handle* h, int B, const mppi_io* io) {
  HIP_TRY(hipStreamSynchronize(h->stream));
  if (!h->Uhost.empty()) transpose_batched(io->U, h->Uhost.data(), B, h->cfg.nu, h->cfg.H);
  h->Uhost.clear();
  return report_status(h, "mppi_solve");
}

// The graph-stream noise double buffer (d_noise, d_noise2) and the generators' ticket, allocated on first use.
static int ensure_stream_buffers(mppi_handle* h) {
  const mppi_config& c = h->cfg;
  if (!h->d_noise2) {
    HIP_TRY(hipMalloc(&h->d_noise2, (size_t)c.max_batch * c.nu * c.H * (size_t)h->Kp * 4));
    HIP_TRY(hipMemset(h->d_noise2, 0, (size_t)c.max_batch * c.nu * c.H * (size_t)h->Kp * 4));  // K..Kp pads stay 0
  }
  if (!h->d_gticket) {
    HIP_TRY(hipMalloc(&h->d_gticket, 16));
    HIP_TRY(hipMemset(h->d_gticket, 0, 16));
  }
  return MPPI_OK;
}

// Make d_noise / d_noise2 [graph_parity] hold the noise of the next solve of batch B with key seed + counter: keep a
// matching prefetch, otherwise generate it now (one noise launch, counter bumped behind it).
static int prime_prefetch(mppi_handle* h, int B, uint64_t seed) {
  if (h->prefetch_valid && (h->prefetch_B != B || h->prefetch_seed != seed)) HIP_TRY(drop_prefetch(h));
  if (h->prefetch_valid) return MPPI_OK;
  const mppi_config& c = h->cfg;
  float* const buf = h->graph_parity ? h->d_noise2 : h->d_noise;
  HIP_TRY(launch_noise_model(buf, B, c.nu, c.H, h->Kp, seed, h->d_seed_ctr, c.sigma, h->noise_model, h->stream,
                             gen_law(h), gen_steps(h), h->d_nkey + noise_slot(h, buf)));
  HIP_TRY(launch_seed_bump(h->d_seed_ctr, 1, h->stream));
  noise_drawn(h, buf, !h->noise_model.active, B, h->Kp);
  h->prefetch_valid = true;
  h->prefetch_B = B;
  h->prefetch_seed = seed;
  return MPPI_OK;
}

// Where a chained solve's NEXT noise is generated (gen_overlap.h states the rule and why): beside this solve's rollout,
// on a second, low-priority stream (noise_beside_kernel + the counter bump, the plain solves' exact keys; the reduce is
// then the read-only pass), or inside this solve's reduce (reduce_kernel<GEN>) behind the rollout.  The outputs are
// bitwise the same either way and the routes mix freely from solve to solve.
// MPPI_GEN_OVERLAP (read per call): 1 forces the overlap (any sampling law: an active noise model's own generator
// then runs on the second stream), 0 forces the fused route, unset lets the rule decide -- the plain i.i.d. law, a
// batch whose noise is past gen_size_ok, and a routed rollout kernel that leaves the generator's wave its registers
// (checked behind the rollout's launch, enqueue_solve).  DESIGN.md section 4 has the measurements that set the rule.
// Kp_gen: the pitch of the noise to generate (the next iteration's: mppi_set_population)
static int gen_overlap_mode(const mppi_handle* h, int B, int Kp_gen) {
  const int force = env_flag("MPPI_GEN_OVERLAP");
  if (force == 0) return kGenFused;
  if (force == 1) return kGenForced;
  const mppi_config& c = h->cfg;
  return !h->noise_model.active && gen_size_ok(gen_noise_bytes(B, c.nu, c.H, Kp_gen)) ? kGenByFit : kGenFused;
}

static int ensure_gen_stream(mppi_handle* h) {
  if (h->gstream) return MPPI_OK;
  int lo = 0, hi = 0;
  HIP_TRY(hipDeviceGetStreamPriorityRange(&lo, &hi));  // lo: the numerically greatest = lowest priority
  HIP_TRY(hipStreamCreateWithPriority(&h->gstream, hipStreamNonBlocking, lo));
  HIP_TRY(hipEventCreateWithFlags(&h->ev_gen, hipEventDisableTiming));
  HIP_TRY(hipEventCreateWithFlags(&h->ev_red, hipEventDisableTiming));
  return MPPI_OK;
}

// MPPI_FLAG_CHAIN: one solve of a graph stream, launched on the stream (rollout -> reduce_kernel<GEN>, or with
// gen_overlap the generator stream's noise launch beside the rollout, then the read-only reduce).  A graph launch pays
// a fixed gap at its boundary (~8.5 us on the box, rocprof trace) that back-to-back stream launches do not, so
// one-solve-per-step loops chain on the stream and multi-solve streams replay graphs.
// chain_iter: one iteration of the step (flags: the iteration's own), its statistics in slot is.it.
static int chain_iter(mppi_handle* h, int B, const mppi_io* io, uint64_t seed, int flags, const IterStep& is) {
  // (a capture keeps the fused route: no parallel branches in any graph; an adapting handle too: the overlap would
  // draw the next noise ahead of this solve's update of the law)
  const int Kp_gen = h->iter_shape(is.it + 1 < is.n ? is.it + 1 : 0).Kp;
  const int overlap = h->capturing || h->adapt_on || h->cov_adapt_on || h->steps_adapt_on
                          ? kGenFused
                          : gen_overlap_mode(h, B, Kp_gen);
  // the solve stream behind the last generator launch: this solve's noise (buf[p]) and the counter's bump
  HIP_TRY(wait_gen(h));
  MPPI_TRY(prime_prefetch(h, B, seed));
  float* buf[2] = {h->d_noise, h->d_noise2};
  if (overlap != kGenFused) {
    // the generator stream behind the previous solve's reduce, which read buf[p ^ 1] (everything enqueued so far); its
    // launches follow the rollout's (enqueue_solve)
    MPPI_TRY(ensure_gen_stream(h));
    HIP_TRY(hipEventRecord(h->ev_red, h->stream));
    HIP_TRY(hipStreamWaitEvent(h->gstream, h->ev_red, 0));
  }
  // this solve's reduce, or the generator beside its rollout, prefetches the next one's noise into buf[p ^ 1]
  const NoiseStep ns{buf[h->graph_parity], buf[h->graph_parity ^ 1], overlap};
  const int rc = enqueue_solve(h, B, io, seed, flags, nullptr, nullptr, &ns, is.it, &is);
  if (rc != MPPI_OK) return rc;
  h->graph_parity ^= 1;  // (still key-valid for B, seed)
  return MPPI_OK;
}

static int chain_solve(mppi_handle* h, int B, const mppi_io* io, uint64_t seed, int flags) {
  if (!(flags & MPPI_FLAG_DEVICE)) return fail(MPPI_E_ARG, "mppi_solve: MPPI_FLAG_CHAIN needs MPPI_FLAG_DEVICE");
  if (io->noise) return fail(MPPI_E_ARG, "mppi_solve: MPPI_FLAG_CHAIN draws device noise (no injected noise)");
  flags |= MPPI_FLAG_SEED_COUNTER;
  MPPI_TRY(ensure_stream_buffers(h));
  // the control step's iterations, each a chained solve of its own: every one draws the counter's next key and
  // prefetches the next one's noise, exactly as consecutive chained solves do
  const int n = h->iter_n;
  for (int it = 0; it < n; ++it) MPPI_TRY(chain_iter(h, B, io, seed, iter_flags(flags, it, n), IterStep{it, n}));
  note_ran(h, solve_opts(h, flags), B, n);
  if (flags & MPPI_FLAG_ASYNC) return MPPI_OK;
  return finish_solve(h, B, io);
}

// The split CA's two-product layer 1 (fc_route.h x3_l1_terms; fc_common.h) as a CHECKED property of the loaded weights.  Before
// the first split-mode solve of a CrossAttention net the engine rolls the first solve's own states and U (up to
// kProbeB solves, kProbeK samples each, seeded device noise of the configured sigma, the configured horizon, cost and
// context) through the same routed kernel twice, with two and with three products on layer 1, and keeps the two-product
// form only if the costs agree within kX3ProbeTol (relative, every finite cost; a non-finite mismatch fails it).  Three
// products are within ~1.5e-6 of the fp32 oracle (profiles/r05_x3_error_budget.txt), so the difference measures the
// two-product form's own error on this net, these states, this cost and this horizon.  Runs once per loaded net and
// cost (mppi_load_dynamics and mppi_set_cost reset it), on the handle's stream, with its own buffers (no effect on the
// noise counter, the prefetched noise or U), before any graph capture.  The decision then holds for every later solve
// and every replay of a captured graph, on states the probe never saw: tests/test_gpu_split_offprobe.py holds those to
// the same 1e-4 bar (DESIGN.md §4 has the figures).
// Horizons beyond kX3TwoTermMaxH keep three products without a probe (the error grows ~H^2); MPPI_X3_L1_TERMS forces.
// The same run decides the fp16 form (fc_route.h x3_f16_on): one more rollout of the same inputs through each kernel
// the probe covers -- fc_wave32_x3p_kernel (the large batches) and fc_rollout_kernel_x3h (the few-tiles shards), by
// routes of its own (launch_fc_route) whatever the probe's batch -- kept only if both are within kX3ProbeTol of the
// three-product costs
// (FcNet::x3_f16 = 1, x3_f16_err = the larger error), else not (-1).  A kernel that cannot hold the shape
// (fc_route_can_run: fc_wave32_x3p_kernel outside 20 <= nu <= 22) is left out of the probe, as no route reaches it; if
// neither can, the form stays off.  The probe covers up to kProbeB of the first batch's solves at kProbeK samples
// each: the CA surrogate's dynamics do not depend on the controls (its action encoder never reaches the output), so
// the form's error is one number per state -- more states, not more samples, find the worst.  For the same reason the
// probe keeps its own white noise of cfg.sigma whatever mppi_set_noise_model selected: it is a per-state measure.
// With a population table (mppi_set_population) the iterations of a step run at several shapes, each routed by fc_route
// on its own (B, Kp_i).  The probe is not per shape and needs no second run: it decides per loaded net and cost, on
// min(Kp, 64) samples of the full population, by routes of its own (above) -- the two kernels of the fp16 form whatever
// the batch -- so one decision covers whichever of x3p, x3h and the M-split kernel an iteration is routed to.
static int x3_probe(mppi_handle* h, int B, const mppi_io* io, int flags) {
  if (h->dyn_kind != MPPI_DYN_CROSS_ATTN || h->cfg.precision != MPPI_PREC_BF16X3 || h->net.arch != kArchCA ||
      h->net.x3_l1 != 0)
    return MPPI_OK;
  const mppi_config& c = h->cfg;
  const FcKnobs knobs = fc_knobs_from_env();
  if (knobs.x3_l1_terms || c.H > kX3TwoTermMaxH) {
    h->net.x3_l1 = c.H > kX3TwoTermMaxH ? 3 : knobs.x3_l1_terms;
    h->net.x3_l1_err = -1.0f;
    h->net.x3_f16 = -1;  // (MPPI_X3_F16=1 still forces it: x3_f16_on)
    h->net.x3_f16_err = -1.0f;
    return MPPI_OK;
  }
  const bool f16 = h->net.fa.w32f16_off >= 0;
  constexpr int kProbeB = 64, kProbeK = 64;
  const int Bp = B < kProbeB ? B : kProbeB, Kpr = h->Kp < kProbeK ? h->Kp : kProbeK;
  const bool dev = (flags & MPPI_FLAG_DEVICE) != 0, colmajor = (flags & MPPI_FLAG_COLMAJOR) != 0;
  const size_t nU = (size_t)Bp * c.nu * c.H, nN = nU * Kpr, nC = (size_t)Bp * Kpr;
  char* buf = nullptr;
  const size_t bytes = (nN + nU + 4 * nC + (size_t)Bp * c.nx + (size_t)Bp * MPPI_CTX_MAX + 16) * 4;
  HIP_TRY(hipMalloc(&buf, bytes));
  float* p_noise = reinterpret_cast<float*>(buf);
  float* p_U = p_noise + nN;
  float* p_c2 = p_U + nU;
  float* p_c3 = p_c2 + nC;
  float* p_c1 = p_c3 + nC;
  float* p_ch = p_c1 + nC;  // the fp16 form on fc_rollout_kernel_x3h
  float* p_x0 = p_ch + nC;
  float* p_ctx = p_x0 + (size_t)Bp * c.nx;
  unsigned* p_st = reinterpret_cast<unsigned*>(p_ctx + (size_t)Bp * MPPI_CTX_MAX);
  hipStream_t s = h->stream;
  std::vector<float> hc1(nC), hc2(nC), hc3(nC), hch(nC), stage;
  bool x3h = false, x3p = false;
  auto run = [&]() -> hipError_t {
    const hipMemcpyKind k = dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    hipError_t e = hipMemcpyAsync(p_x0, io->x0, (size_t)Bp * c.nx * 4, k, s);
    const float* U = io->U;
    hipMemcpyKind ku = k;
    if (flags & MPPI_FLAG_RESIDENT_U) {  // the handle's resident U is the input
      U = h->d_U;
      ku = hipMemcpyDeviceToDevice;
    } else if (colmajor) {  // Julia U (nu,H) column-major -> [nu][H]
      stage.resize(nU);
      transpose_batched(stage.data(), io->U, Bp, c.H, c.nu);
      U = stage.data();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(p_U, U, nU * 4, ku, s);
    if (e == hipSuccess && io->ctx) e = hipMemcpyAsync(p_ctx, io->ctx, (size_t)Bp * MPPI_CTX_MAX * 4, k, s);
    if (e == hipSuccess) e = launch_noise(p_noise, Bp, c.nu, c.H, Kpr, 0x5EEDC0DEull, nullptr, c.sigma, s);
    SolveArgs a;
    std::memset(&a, 0, sizeof(a));
    a.B = Bp;
    a.nx = c.nx;
    a.nu = c.nu;
    a.H = c.H;
    a.K = Kpr < c.K ? Kpr : c.K;
    a.Kp = Kpr;
    a.lambda = c.lambda;
    a.ctrl_clamp = c.ctrl_clamp;
    a.terminal_weight = c.terminal_weight;
    a.cost_kind = h->cost_kind;
    std::memcpy(a.ctx_default, h->cost_params, sizeof(a.ctx_default));
    a.x0 = p_x0;
    a.U = p_U;
    a.noise = p_noise;
    a.ctx = io->ctx ? p_ctx : nullptr;
    a.status = p_st;
    const FcNet& n = h->net;
    const int cus = current_device_cus();
    for (int terms : {2, 3}) {  // as routed for the probe's batch, the fp16 form decided off
      a.costs = terms == 2 ? p_c2 : p_c3;
      const FcRoute r = fc_route(n.arch, n.precision, a, n.fa, terms, -1, cus, knobs);
      if (e == hipSuccess) e = launch_fc_route(a, n, r, s);
    }
    if (f16) {  // the fp16 form (form 1; a knob that forces the form forces the probe's too) on fc_wave32_x3p_kernel,
                // where that kernel holds the shape (its operands take 20 <= nu <= 22: no route reaches it elsewhere)
      x3p = fc_route_can_run(FcKernel::x3p, a, n.fa);
      if (x3p) {
        a.costs = p_c1;
        const FcRoute rp = {FcKernel::x3p, x3_form(c.H, 3, 1, n.fa.w32f16_off, knobs), 1};
        if (e == hipSuccess) e = launch_fc_route(a, n, rp, s);
        if (e == hipSuccess) e = hipMemcpyAsync(hc1.data(), p_c1, nC * 4, hipMemcpyDeviceToHost, s);
      }
      a.costs = p_ch;
      x3h = fc_route_can_run(FcKernel::x3h, a, n.fa) && x3_f16_on(c.H, 1, n.fa.wmf16_off, knobs) && knobs.x3h;
      if (x3h) {  // ... and on fc_rollout_kernel_x3h
        const FcRoute rh = {FcKernel::x3h, x3_form(c.H, 3, 1, n.fa.wmf16_off, knobs), x3h_tiles(a.Kp, knobs)};
        if (e == hipSuccess) e = launch_fc_route(a, n, rh, s);
        if (e == hipSuccess) e = hipMemcpyAsync(hch.data(), p_ch, nC * 4, hipMemcpyDeviceToHost, s);
      }
    }
    if (e == hipSuccess) e = hipMemcpyAsync(hc2.data(), p_c2, nC * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(hc3.data(), p_c3, nC * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    return e;
  };
  const hipError_t e = run();
  (void)hipFree(buf);
  if (e != hipSuccess) return fail(MPPI_E_HIP, std::string("x3 layer-1 probe: ") + hipGetErrorString(e));
  const int Kv = Kpr < c.K ? Kpr : c.K;
  auto diff = [&](const std::vector<float>& hc) {  // max relative difference to three products (inf: a finiteness mismatch)
    double worst = 0.0;
    for (int b = 0; b < Bp; ++b)
      for (int k = 0; k < Kv; ++k) {
        const float v = hc[(size_t)b * Kpr + k], v3 = hc3[(size_t)b * Kpr + k];
        if (!std::isfinite(v3) && !std::isfinite(v)) continue;
        if (!std::isfinite(v) || !std::isfinite(v3)) return (double)INFINITY;
        const double d = std::fabs((double)v - v3) / std::fmax(std::fabs((double)v3), 1e-30);
        worst = d > worst ? d : worst;
      }
    return worst;
  };
  const double w2 = diff(hc2);
  h->net.x3_l1 = w2 <= kX3ProbeTol ? 2 : 3;
  h->net.x3_l1_err = (float)w2;
  const bool f16_ran = f16 && (x3p || x3h);  // (neither kernel holds the shape: the form stays off, unmeasured)
  const double w1 = f16_ran ? std::fmax(x3p ? diff(hc1) : 0.0, x3h ? diff(hch) : 0.0) : (double)INFINITY;
  h->net.x3_f16 = w1 <= kX3ProbeTol ? 1 : -1;
  h->net.x3_f16_err = f16_ran ? (float)w1 : -1.0f;
  return MPPI_OK;
}

extern "C" {

int mppi_x3_layer1(mppi_handle* h, int* products, float* probe_rel_err) {
  if (!h) return fail(MPPI_E_ARG, "mppi_x3_layer1: null handle");
  const bool split_ca = h->dyn_kind == MPPI_DYN_CROSS_ATTN && h->cfg.precision == MPPI_PREC_BF16X3 &&
                        h->net.arch == kArchCA;
  if (products) *products = split_ca && h->net.x3_l1 ? x3_l1_terms(h->cfg.H, h->net.x3_l1, fc_knobs_from_env()) : 0;
  if (probe_rel_err) *probe_rel_err = split_ca ? h->net.x3_l1_err : -1.0f;
  return MPPI_OK;
}

int mppi_x3_f16(mppi_handle* h, int* on, float* probe_rel_err) {
  if (!h) return fail(MPPI_E_ARG, "mppi_x3_f16: null handle");
  const bool split_ca = h->dyn_kind == MPPI_DYN_CROSS_ATTN && h->cfg.precision == MPPI_PREC_BF16X3 &&
                        h->net.arch == kArchCA;
  if (on) {
    const FcKnobs k = fc_knobs_from_env();
    *on = split_ca && x3_f16_on(h->cfg.H, h->net.x3_f16, h->net.fa.w32f16_off, k) ? (x3_f16_l2x1(h->net.x3_f16, k) ? 2 : 1)
                                                                                  : 0;
  }
  if (probe_rel_err) *probe_rel_err = split_ca ? h->net.x3_f16_err : -1.0f;
  return MPPI_OK;
}

const char* mppi_rollout_kernel(mppi_handle* h) { return h ? h->rollout_kernel : ""; }

int mppi_reduce_regen(mppi_handle* h) { return h ? h->reduce_regen : 0; }

const char* mppi_gen_route(mppi_handle* h) {
  static const char* const n[3] = {"", "fused", "overlap"};
  return h ? n[h->gen_route] : "";
}

int mppi_noise_beside_eval(mppi_handle* h, int B, uint64_t seed, float* noise_out) {
  if (!h || !noise_out) return fail(MPPI_E_ARG, "mppi_noise_beside_eval: null argument");
  const mppi_config& c = h->cfg;
  if (B < 1 || B > c.max_batch) return fail(MPPI_E_ARG, "mppi_noise_beside_eval: B out of range [1, max_batch]");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(drop_prefetch(h));  // d_noise may hold the next chained solve's noise: its key is drawn again
  hipStream_t s = h->stream;
  const size_t K = (size_t)c.K, Kp = (size_t)h->Kp, rows = (size_t)B * c.nu * c.H;
  HIP_TRY(launch_noise_beside(h->d_noise, B, c.nu, c.H, h->Kp, seed, nullptr, c.sigma, s));
  HIP_TRY(hipMemcpy2DAsync(noise_out, K * 4, h->d_noise, Kp * 4, K * 4, rows, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return MPPI_OK;
}

int mppi_solve_ex(mppi_handle* h, int B, const mppi_io* io, uint64_t seed, int flags) {
  int rc = check_solve(h, B, io, flags);
  if (rc != MPPI_OK) return rc;
  HIP_TRY(hipSetDevice(h->device));
  if ((rc = x3_probe(h, B, io, flags)) != MPPI_OK) return rc;
  if (h->adapt_on) flags |= MPPI_FLAG_STATS;  // the adaptation reads the solve's moments
  if (h->cov_adapt_on) flags |= MPPI_FLAG_CROSS;  // the covariance's adaptation reads the solve's cross moments
  if (h->steps_adapt_on) flags |= MPPI_FLAG_STEP_MOMENTS;  // the table's refit reads the solve's per-step moments
  if (flags & (MPPI_FLAG_CROSS | MPPI_FLAG_STEP_MOMENTS)) flags |= MPPI_FLAG_STATS;  // both read the statistics' weights
  const int n = h->iter_n;  // the step's iterations: one per-step slot each
  if ((flags & MPPI_FLAG_STATS) && (rc = ensure_stats(h, n)) != MPPI_OK) return rc;
  if ((flags & MPPI_FLAG_CROSS) && (rc = ensure_cross(h, n)) != MPPI_OK) return rc;
  if ((flags & MPPI_FLAG_STEP_MOMENTS) && (rc = ensure_step_mom(h, n)) != MPPI_OK) return rc;
  if (h->cov_adapt_on && (rc = ensure_cov_hist(h, n)) != MPPI_OK) return rc;
  if (h->ess_on && (rc = ensure_lambda(h, n)) != MPPI_OK) return rc;
  if (flags & MPPI_FLAG_CHAIN) return chain_solve(h, B, io, seed, flags);
  HIP_TRY(drop_prefetch(h));  // a plain solve generates its own noise into d_noise
  for (int it = 0; it < n; ++it) {  // (the counter advances per iteration by itself; a by-value seed: key seed + it)
    const IterStep is{it, n};
    rc = enqueue_solve(h, B, io, (flags & MPPI_FLAG_SEED_COUNTER) ? seed : seed + (uint64_t)it, iter_flags(flags, it, n),
                       nullptr, nullptr, nullptr, it, &is);
    if (rc != MPPI_OK) return rc;
  }
  note_ran(h, solve_opts(h, flags), B, n);
  if ((flags & MPPI_FLAG_DEVICE) && (flags & MPPI_FLAG_ASYNC)) return MPPI_OK;
  return finish_solve(h, B, io);
}

int mppi_graph_capture(mppi_handle* h, int B, const mppi_io* io, uint64_t seed, int flags, int n_solves) {
  return mppi_graph_capture_traj(h, B, io, seed, flags, n_solves, nullptr, nullptr);
}

int mppi_graph_capture_traj(mppi_handle* h, int B, const mppi_io* io, uint64_t seed, int flags, int n_solves,
                            float* traj_x, float* traj_u) {
  if (n_solves < 1) return fail(MPPI_E_ARG, "mppi_graph_capture: n_solves must be >= 1");
  if ((traj_x != nullptr) != (traj_u != nullptr)) return fail(MPPI_E_ARG, "mppi_graph_capture: traj_x and traj_u go together");
  if (traj_x && !(flags & MPPI_FLAG_ENV_STEP))
    return fail(MPPI_E_ARG, "mppi_graph_capture: trajectory logging needs MPPI_FLAG_ENV_STEP");
  if (!(flags & MPPI_FLAG_DEVICE)) return fail(MPPI_E_ARG, "mppi_graph_capture: device pointers (MPPI_FLAG_DEVICE) required");
  if (io && io->noise) return fail(MPPI_E_ARG, "mppi_graph_capture: injected noise is not replayable; use device noise");
  flags = (flags | MPPI_FLAG_SEED_COUNTER | MPPI_FLAG_ASYNC) & ~MPPI_FLAG_COLMAJOR;
  int rc = check_solve(h, B, io, flags);
  if (rc != MPPI_OK) return rc;
  if (h->adapt_on) flags |= MPPI_FLAG_STATS;  // the adaptation reads solve i's moments out of slot i
  if (h->cov_adapt_on) flags |= MPPI_FLAG_CROSS;  // ... and the covariance's its cross moments
  if (h->steps_adapt_on) flags |= MPPI_FLAG_STEP_MOMENTS;  // ... and the table's refit its per-step moments
  if (flags & (MPPI_FLAG_CROSS | MPPI_FLAG_STEP_MOMENTS)) flags |= MPPI_FLAG_STATS;  // both read the statistics' weights
  HIP_TRY(hipSetDevice(h->device));
  if ((rc = x3_probe(h, B, io, flags)) != MPPI_OK) return rc;  // before the capture: it synchronises the stream
  MPPI_TRY(drop_graphs(h, false));
  // a prefetched noise stays valid for a graph of the same batch and seed (checked again at launch)
  if (h->prefetch_valid && (B != h->prefetch_B || seed != h->prefetch_seed)) HIP_TRY(drop_prefetch(h));
  const mppi_config& c = h->cfg;
  if (const int e = ensure_stream_buffers(h); e != MPPI_OK) return e;
  // the statistics' slots exist before the capture begins: solve i's launches carry slot i's pointers
  const int n_iter = h->iter_n;
  if ((long)n_solves * n_iter > (1L << 24)) return fail(MPPI_E_ARG, "mppi_graph_capture: n_solves * n_iter too large");
  const int n_total = n_solves * n_iter;  // one per-step slot per iteration
  if ((flags & MPPI_FLAG_STATS) && (rc = ensure_stats(h, n_total)) != MPPI_OK) return rc;
  if ((flags & MPPI_FLAG_CROSS) && (rc = ensure_cross(h, n_total)) != MPPI_OK) return rc;
  if ((flags & MPPI_FLAG_STEP_MOMENTS) && (rc = ensure_step_mom(h, n_total)) != MPPI_OK) return rc;
  if (h->cov_adapt_on && (rc = ensure_cov_hist(h, n_total)) != MPPI_OK) return rc;
  if (h->ess_on && (rc = ensure_lambda(h, n_total)) != MPPI_OK) return rc;  // ... and the lambdas' slots
  float* buf[2] = {h->d_noise, h->d_noise2};
  const bool prof = h->prof;
  h->prof = false;  // no event nodes inside the graph
  h->capturing = true;
  // exec p starts from noise buffer p (an odd stream flips the parity every launch; a re-capture keeps the parity
  // of a valid prefetch)
  for (int p = 0; p < 2 && rc == MPPI_OK; ++p) {
    HIP_TRY(hipStreamBeginCapture(h->stream, hipStreamCaptureModeRelaxed));
    for (int j = 0; j < n_total && rc == MPPI_OK; ++j) {  // iteration it of control step i: slot and noise pair j
      const int i = j / n_iter;
      const IterStep is{j - i * n_iter, n_iter};
      const NoiseStep ns{buf[(p + j) % 2], buf[(p + j + 1) % 2]};
      rc = enqueue_solve(h, B, io, seed, iter_flags(flags, is.it, n_iter),
                         traj_x ? traj_x + (size_t)i * B * c.nx : nullptr,
                         traj_u ? traj_u + (size_t)i * B * c.nu : nullptr, &ns, j, &is);
    }
    hipGraph_t g = nullptr;
    const hipError_t ec = hipStreamEndCapture(h->stream, &g);
    if (rc != MPPI_OK || ec != hipSuccess) {
      if (g) (void)hipGraphDestroy(g);
      h->prof = prof;
      h->capturing = false;
      if (rc != MPPI_OK) return rc;
      return fail(MPPI_E_HIP, std::string("mppi_graph_capture: ") + hipGetErrorString(ec));
    }
    const hipError_t ei = hipGraphInstantiate(&h->graph_exec[p], g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (ei != hipSuccess) {
      h->graph_exec[p] = nullptr;
      h->prof = prof;
      h->capturing = false;
      return fail(MPPI_E_HIP, std::string("mppi_graph_capture: instantiate: ") + hipGetErrorString(ei));
    }
  }
  h->prof = prof;
  h->capturing = false;
  h->graph_kclock = h->kclock;
  h->graph_opts = solve_opts(h, flags);
  h->graph_ens = h->ens_n;
  h->graph_B = B;
  h->graph_n = n_total;  // (what a launch counts: slots, stamped rollouts, the noise pair's parity)
  h->graph_seed = seed;
  return MPPI_OK;
}

int mppi_graph_launch(mppi_handle* h, int sync) {
  if (!h) return fail(MPPI_E_ARG, "mppi_graph_launch: null handle");
  if (!h->graph_exec[0] || !h->graph_exec[1])
    return fail(MPPI_E_STATE, "mppi_graph_launch: call mppi_graph_capture first");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(wait_gen(h));  // chained solves with the overlapped generator came before: its noise and bump first
  // first launch (or after plain solves / a counter reset / chained solves of another batch): generate the noise
  MPPI_TRY(prime_prefetch(h, h->graph_B, h->graph_seed));
  HIP_TRY(hipGraphLaunch(h->graph_exec[h->graph_parity], h->stream));
  h->pristine[0].ok = h->pristine[1].ok = false;  // (the replay wrote both buffers; the host followed none of it)
  if (h->graph_kclock) h->kclock_launches += (long)h->graph_n * h->graph_ens;
  note_ran(h, h->graph_opts, h->graph_B, h->graph_n);
  h->graph_parity = (h->graph_parity + h->graph_n) % 2;  // the launch prefetched the next one's first noise
  if (!sync) return MPPI_OK;
  HIP_TRY(hipStreamSynchronize(h->stream));
  return report_status(h, "mppi_graph_launch");
}

int mppi_set_seed_counter(mppi_handle* h, uint64_t value) {
  if (!h) return fail(MPPI_E_ARG, "mppi_set_seed_counter: null handle");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(wait_gen(h));  // the generator's last bump lands before the new value
  HIP_TRY(hipMemcpyAsync(h->d_seed_ctr, &value, 8, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  h->prefetch_valid = false;  // a prefetched noise used the old counter
  return MPPI_OK;
}

int mppi_get_seed_counter(mppi_handle* h, uint64_t* value) {
  if (!h || !value) return fail(MPPI_E_ARG, "mppi_get_seed_counter: null argument");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(wait_gen(h));  // the overlapped generator's bump is part of the counter's value
  uint64_t v = 0;
  HIP_TRY(hipMemcpyAsync(&v, h->d_seed_ctr, 8, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  // the LOGICAL counter: the key the next solve draws.  After chained solves or a graph launch the next solve's noise
  // is already prefetched and the device counter already advanced past its key (drop_prefetch steps it back for the
  // same reason), so mppi_set_seed_counter(value) -- which drops any prefetch -- resumes the stream exactly
  *value = h->prefetch_valid ? v - 1 : v;
  return MPPI_OK;
}

int mppi_set_noise_model(mppi_handle* h, const float* sigma_u, float rho) {
  if (!h) return fail(MPPI_E_ARG, "mppi_set_noise_model: null handle");
  if (!(rho >= 0.0f && rho < 1.0f)) return fail(MPPI_E_ARG, "mppi_set_noise_model: rho must be in [0, 1)");
  const int nu = h->cfg.nu;
  if (sigma_u)
    for (int u = 0; u < nu; ++u)
      if (!(std::isfinite(sigma_u[u]) && sigma_u[u] >= 0.0f))
        return fail(MPPI_E_ARG, "mppi_set_noise_model: sigma_u[" + std::to_string(u) + "] must be finite and >= 0");
  // (NULL, 0) = the default law, exactly the code path of a handle without a model
  const bool active = sigma_u != nullptr || rho != 0.0f;
  if (active && nu > kMaxNu)
    return fail(MPPI_E_UNSUPPORTED, "mppi_set_noise_model: the model travels as a kernel argument (nu <= 32)");
  if (!active && h->noise_model.n_knots > 0)
    return fail(MPPI_E_STATE, "mppi_set_noise_model: (NULL, 0) is the default path, which has no knot law: "
                              "call mppi_set_noise_knots(h, 0, 0) first");
  if (!active && h->noise_model.n_basis > 0)
    return fail(MPPI_E_STATE, "mppi_set_noise_model: (NULL, 0) is the default path, which has no horizon basis: "
                              "call mppi_set_noise_basis(h, 0, NULL) first");
  if (rho != 0.0f && h->noise_model.n_basis > 0)
    return fail(MPPI_E_UNSUPPORTED, "mppi_set_noise_model: rho != 0 not together with mppi_set_noise_basis (the basis "
                                    "is the horizon correlation)");
  if (!active && h->steps_on)
    return fail(MPPI_E_STATE, "mppi_set_noise_model: (NULL, 0) is the default path, which has no per-step scales: "
                              "call mppi_set_noise_steps(h, 0, NULL) first");
  if (h->noise_model.cov_L && !active)
    return fail(MPPI_E_STATE, "mppi_set_noise_model: (NULL, 0) is the default path, which has no covariance: "
                              "call mppi_set_noise_cov(h, NULL) first");
  if (h->noise_model.cov_L && sigma_u)
    return fail(MPPI_E_STATE, "mppi_set_noise_model: the scales are the covariance's while mppi_set_noise_cov is on: "
                              "pass sigma_u = NULL (rho alone), or call mppi_set_noise_cov(h, NULL) first");
  HIP_TRY(hipSetDevice(h->device));
  // stale state: a prefetched noise was drawn with the old law (the counter steps back: the key sequence is unchanged),
  // and the captured graphs hold the old model in their kernel arguments (a launch still in flight finishes first)
  HIP_TRY(drop_prefetch(h));
  MPPI_TRY(drop_graphs(h, true));
  NoiseModel m;
  m.n_knots = h->noise_model.n_knots, m.order = h->noise_model.order;  // the knot law stays (mppi_set_noise_knots)
  m.kidx = h->noise_model.kidx, m.kw = h->noise_model.kw;
  m.cov_L = h->noise_model.cov_L;  // ... and so does the covariance (mppi_set_noise_cov): only rho changes under it
  m.n_basis = h->noise_model.n_basis, m.basis_T = h->noise_model.basis_T;  // ... and the basis (mppi_set_noise_basis)
  m.active = active || h->adapt_on ? 1 : 0;  // (an adapting handle's model stays active: (NULL, 0) is its values)
  m.rho = rho;
  m.c = ar1_innovation_scale(rho);
  if (m.active)
    for (int u = 0; u < nu; ++u)
      m.sigma_u[u] = sigma_u ? sigma_u[u] : (m.cov_L ? h->noise_model.sigma_u[u] : h->cfg.sigma);
  if (h->adapt_on) HIP_TRY(launch_noise_law_set(h->d_law, m, h->stream));  // the device law starts again from here
  h->noise_model = m;
  return MPPI_OK;
}

static int fetch_cov_law(mppi_handle* h);  // (below, beside mppi_set_noise_cov_adapt)

// the device law -> h->noise_model (waits for the stream); c is the host's, as for every by-value model
static int fetch_law(mppi_handle* h) {
  float law[kLawFloats];
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipMemcpy(law, h->d_law, sizeof(law), hipMemcpyDeviceToHost));
  NoiseModel& m = h->noise_model;
  m.active = 1;
  for (int u = 0; u < h->cfg.nu; ++u) m.sigma_u[u] = law[u];
  m.rho = law[kLawRho];
  m.c = ar1_innovation_scale(m.rho);
  return MPPI_OK;
}

int mppi_set_noise_adapt(mppi_handle* h, float rate, float sigma_min, float sigma_max, float rho_max) {
  if (!h) return fail(MPPI_E_ARG, "mppi_set_noise_adapt: null handle");
  if (!(rate >= 0.0f && rate <= 1.0f)) return fail(MPPI_E_ARG, "mppi_set_noise_adapt: rate must be in [0, 1]");
  if (!(sigma_min >= 0.0f && sigma_min <= sigma_max && std::isfinite(sigma_max)))
    return fail(MPPI_E_ARG, "mppi_set_noise_adapt: need 0 <= sigma_min <= sigma_max < inf");
  if (!(rho_max >= 0.0f && rho_max < 1.0f)) return fail(MPPI_E_ARG, "mppi_set_noise_adapt: rho_max must be in [0, 1)");
  const bool on = rate > 0.0f;
  if (on && h->cfg.nu > kMaxNu)
    return fail(MPPI_E_UNSUPPORTED, "mppi_set_noise_adapt: the adapted law is an active noise model (nu <= 32)");
  if (on && h->noise_model.n_knots > 0)
    return fail(MPPI_E_UNSUPPORTED, "mppi_set_noise_adapt: not together with mppi_set_noise_knots (the moments of "
                                    "interpolated noise do not estimate sigma_u and rho)");
  if (on && h->noise_model.cov_L)
    return fail(MPPI_E_UNSUPPORTED, "mppi_set_noise_adapt: not together with mppi_set_noise_cov (the rule adapts "
                                    "sigma_u, which is not the law under a full covariance)");
  if (on && h->noise_model.n_basis > 0)
    return fail(MPPI_E_UNSUPPORTED, "mppi_set_noise_adapt: not together with mppi_set_noise_basis (the moment "
                                    "estimates of sigma_u and rho assume AR(1))");
  if (on && h->steps_on)
    return fail(MPPI_E_UNSUPPORTED, "mppi_set_noise_adapt: not together with mppi_set_noise_steps (the rule adapts one "
                                    "sigma_u per actuator, which is not the scale under a per-step table)");
  if (!on && !h->adapt_on) {  // nothing to disable: only the limits are kept
    h->adapt = NoiseAdapt{0.0f, sigma_min, sigma_max, rho_max};
    return MPPI_OK;
  }
  HIP_TRY(hipSetDevice(h->device));
  // stale state, as in mppi_set_noise_model: the prefetched noise (the counter steps back: the key sequence is
  // unchanged) and the captured graphs, whose generators are those of the other path
  HIP_TRY(drop_prefetch(h));
  MPPI_TRY(drop_graphs(h, true));
  if (on && !h->adapt_on) {
    // (no memset: noise_law_set_kernel below writes every entry, in stream order; a memset on the null stream is not
    // ordered against the handle's stream and could land behind it)
    if (!h->d_law) HIP_TRY(hipMalloc(&h->d_law, kLawFloats * sizeof(float)));
    NoiseModel m = h->noise_model;
    if (!m.active) {  // the default law as an active model: value for value the same noise
      m = NoiseModel{};
      m.active = 1;
      for (int u = 0; u < h->cfg.nu; ++u) m.sigma_u[u] = h->cfg.sigma;
    }
    HIP_TRY(launch_noise_law_set(h->d_law, m, h->stream));
    h->noise_model = m;
    h->adapt_on = true;
    h->law_n = 0;
  } else if (!on) {  // back to the by-value path with the law as it stands
    MPPI_TRY(fetch_law(h));
    h->adapt_on = false;
  }
  h->adapt = NoiseAdapt{rate, sigma_min, sigma_max, rho_max};
  return MPPI_OK;
}

int mppi_get_noise_adapt(mppi_handle* h, float* rate, float* sigma_min, float* sigma_max, float* rho_max) {
  if (!h) return fail(MPPI_E_ARG, "mppi_get_noise_adapt: null handle");
  if (rate) *rate = h->adapt_on ? h->adapt.rate : 0.0f;
  if (sigma_min) *sigma_min = h->adapt.sigma_min;
  if (sigma_max) *sigma_max = h->adapt.sigma_max;
  if (rho_max) *rho_max = h->adapt.rho_max;
  return MPPI_OK;
}

int mppi_get_noise_law(mppi_handle* h, int step, float* sigma_u, float* rho) {
  if (!h) return fail(MPPI_E_ARG, "mppi_get_noise_law: null handle");
  if (h->law_n == 0) return fail(MPPI_E_STATE, "mppi_get_noise_law: no adapting solve has run on the handle");
  if (step < 0 || step >= h->law_n)
    return fail(MPPI_E_ARG, "mppi_get_noise_law: step beyond the solves of the last adapting solve or graph");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipStreamSynchronize(h->stream));
  const int nu = h->cfg.nu;
  float row[kMaxNu + 1];
  HIP_TRY(hipMemcpy(row, h->d_law_hist + (size_t)step * (nu + 1), (size_t)(nu + 1) * 4, hipMemcpyDeviceToHost));
  if (sigma_u)
    for (int u = 0; u < nu; ++u) sigma_u[u] = row[u];
  if (rho) *rho = row[nu];
  return MPPI_OK;
}

int mppi_get_noise_model(mppi_handle* h, float* sigma_u, float* rho, int* active) {
  if (!h) return fail(MPPI_E_ARG, "mppi_get_noise_model: null handle");
  if (h->adapt_on) {  // the live law: every enqueued solve's update included
    HIP_TRY(hipSetDevice(h->device));
    MPPI_TRY(fetch_law(h));
  }
  if (h->cov_adapt_on) {  // ... an adapted covariance's scales: sqrt of its live diagonal
    HIP_TRY(hipSetDevice(h->device));
    MPPI_TRY(fetch_cov_law(h));
  }
  const NoiseModel& m = h->noise_model;
  if (sigma_u)
    for (int u = 0; u < h->cfg.nu; ++u) sigma_u[u] = m.active ? m.sigma_u[u] : h->cfg.sigma;
  if (rho) *rho = m.rho;
  if (active) *active = m.active;
  return MPPI_OK;
}

int mppi_set_noise_knots(mppi_handle* h, int n_knots, int order) {
  if (!h) return fail(MPPI_E_ARG, "mppi_set_noise_knots: null handle");
  const mppi_config& c = h->cfg;
  const bool on = n_knots != 0;
  if (on && !knot_law_valid(c.H, n_knots, order))
    return fail(MPPI_E_ARG, "mppi_set_noise_knots: need n_knots in 1..H with order 0, 1 or 3, or n_knots == 0");
  NoiseModel m = h->noise_model;
  if (!on && m.n_knots == 0) return MPPI_OK;                                // nothing to disable
  if (on && m.n_knots == n_knots && m.order == order) return MPPI_OK;  // no change: prefetch and graphs stay
  if (on && c.nu > kMaxNu)
    return fail(MPPI_E_UNSUPPORTED, "mppi_set_noise_knots: a knot law is an active noise model (nu <= 32)");
  if (on && h->ctrl_gamma > 0.0f)
    return fail(MPPI_E_UNSUPPORTED, "mppi_set_noise_knots: not together with mppi_set_control_cost (the term needs the "
                                    "inverse of the sampling covariance, which a knot law leaves singular)");
  if (on && h->adapt_on)
    return fail(MPPI_E_UNSUPPORTED, "mppi_set_noise_knots: not together with mppi_set_noise_adapt (the moments of "
                                    "interpolated noise do not estimate sigma_u and rho)");
  if (on && m.cov_L)
    return fail(MPPI_E_UNSUPPORTED, "mppi_set_noise_knots: not together with mppi_set_noise_cov (the knot generator "
                                    "does not mix the actuators)");
  if (on && m.n_basis > 0)
    return fail(MPPI_E_UNSUPPORTED, "mppi_set_noise_knots: not together with mppi_set_noise_basis (both are horizon "
                                    "laws)");
  if (on && h->steps_on)
    return fail(MPPI_E_UNSUPPORTED, "mppi_set_noise_knots: not together with mppi_set_noise_steps (the knot generator "
                                    "reads no per-step scale)");
  HIP_TRY(hipSetDevice(h->device));
  const size_t n = (size_t)c.H * 4;
  if (on && !h->d_knots) HIP_TRY(hipMalloc(&h->d_knots, n * (sizeof(int32_t) + sizeof(float))));
  // stale state, as in mppi_set_noise_model: the prefetched noise (the counter steps back: the key sequence is
  // unchanged) and the captured graphs, whose generators are those of the other law
  HIP_TRY(drop_prefetch(h));
  MPPI_TRY(drop_graphs(h, true));
  if (on) {
    std::vector<int32_t> idx(n);
    std::vector<float> w(n);
    knot_table(c.H, n_knots, order, idx.data(), w.data());
    // every launch that reads the table has finished before it changes (the generator stream included: drop_prefetch
    // made the stream wait for it)
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(h->d_knots, idx.data(), n * sizeof(int32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy((char*)h->d_knots + n * sizeof(int32_t), w.data(), n * sizeof(float), hipMemcpyHostToDevice));
    h->knot_idx.swap(idx);
    h->knot_w.swap(w);
    if (!m.active) {  // the default law as an active model: value for value the same normals
      m = NoiseModel{};
      m.active = 1;
      for (int u = 0; u < c.nu; ++u) m.sigma_u[u] = c.sigma;
    }
    m.n_knots = n_knots, m.order = order;
    m.kidx = (const int32_t*)h->d_knots;
    m.kw = (const float*)((const char*)h->d_knots + n * sizeof(int32_t));
  } else {  // sigma_u and rho stay as they stand: the AR(1) generators again
    m.n_knots = 0, m.order = 0;
    m.kidx = nullptr, m.kw = nullptr;
  }
  h->noise_model = m;
  return MPPI_OK;
}

int mppi_get_noise_knots(mppi_handle* h, int* n_knots, int* order, int32_t* idx, float* w) {
  if (!h) return fail(MPPI_E_ARG, "mppi_get_noise_knots: null handle");
  const NoiseModel& m = h->noise_model;
  if (n_knots) *n_knots = m.n_knots;
  if (order) *order = m.order;
  if (m.n_knots > 0) {  // (off: the arrays are left untouched)
    if (idx) std::memcpy(idx, h->knot_idx.data(), h->knot_idx.size() * sizeof(int32_t));
    if (w) std::memcpy(w, h->knot_w.data(), h->knot_w.size() * sizeof(float));
  }
  return MPPI_OK;
}

int mppi_set_noise_basis(mppi_handle* h, int n_basis, const float* M) {
  if (!h) return fail(MPPI_E_ARG, "mppi_set_noise_basis: null handle");
  const mppi_config& c = h->cfg;
  const bool on = n_basis != 0;
  if (on && (!basis_law_valid(c.H, n_basis) || !M))
    return fail(MPPI_E_ARG, "mppi_set_noise_basis: need n_basis in 1..H with M [H][n_basis], or n_basis == 0");
  if (on && !basis_table_finite(M, c.H, n_basis))
    return fail(MPPI_E_ARG, "mppi_set_noise_basis: every entry of M must be finite");
  if (on && n_basis > kMaxBasis)
    return fail(MPPI_E_UNSUPPORTED, "mppi_set_noise_basis: n_basis <= 128 (it bounds the generators' registers and "
                                    "LDS)");
  NoiseModel m = h->noise_model;
  if (!on && m.n_basis == 0) return MPPI_OK;  // nothing to disable
  const size_t n = on ? (size_t)c.H * n_basis : 0;
  // the table in effect, bitwise: prefetch and graphs stay
  if (on && m.n_basis == n_basis && std::memcmp(M, h->basis_host.data(), n * sizeof(float)) == 0) return MPPI_OK;
  if (on && c.nu > kMaxNu)
    return fail(MPPI_E_UNSUPPORTED, "mppi_set_noise_basis: a horizon basis is an active noise model (nu <= 32)");
  if (on && m.n_knots > 0)
    return fail(MPPI_E_UNSUPPORTED, "mppi_set_noise_basis: not together with mppi_set_noise_knots (both are horizon "
                                    "laws)");
  if (on && m.cov_L)
    return fail(MPPI_E_UNSUPPORTED, "mppi_set_noise_basis: not together with mppi_set_noise_cov / "
                                    "mppi_set_noise_cov_adapt (the basis generator does not mix the actuators)");
  if (on && h->adapt_on)
    return fail(MPPI_E_UNSUPPORTED, "mppi_set_noise_basis: not together with mppi_set_noise_adapt (the moment "
                                    "estimates of sigma_u and rho assume AR(1))");
  if (on && h->ctrl_gamma > 0.0f)
    return fail(MPPI_E_UNSUPPORTED, "mppi_set_noise_basis: not together with mppi_set_control_cost (the term needs the "
                                    "inverse of M M^T, singular for n_basis < H)");
  if (on && h->steps_on)
    return fail(MPPI_E_UNSUPPORTED, "mppi_set_noise_basis: not together with mppi_set_noise_steps (the basis generators "
                                    "read no per-step scale)");
  if (on && m.active && m.rho != 0.0f)
    return fail(MPPI_E_UNSUPPORTED, "mppi_set_noise_basis: not together with rho != 0 of mppi_set_noise_model (the "
                                    "basis is the horizon correlation)");
  HIP_TRY(hipSetDevice(h->device));
  const int pitch = basis_pitch(c.H);
  if (on && !h->d_basis)
    HIP_TRY(hipMalloc(&h->d_basis, (size_t)basis_rows_padded(c.H < kMaxBasis ? c.H : kMaxBasis) * pitch * sizeof(float)));
  // stale state, as in mppi_set_noise_model: the prefetched noise (the counter steps back: the key sequence is
  // unchanged) and the captured graphs, whose generators are those of the other law
  HIP_TRY(drop_prefetch(h));
  MPPI_TRY(drop_graphs(h, true));
  if (on) {
    // M^T, the pad of every row zero; the rows up to a multiple of four -0.0f (they add -0 to a chain: nothing)
    std::vector<float> host(M, M + n), mt((size_t)basis_rows_padded(n_basis) * pitch, 0.0f);
    std::fill(mt.begin() + (size_t)n_basis * pitch, mt.end(), -0.0f);
    for (int t = 0; t < c.H; ++t)
      for (int r = 0; r < n_basis; ++r) mt[(size_t)r * pitch + t] = M[(size_t)t * n_basis + r];
    // every launch that reads the table has finished before it changes (the generator stream included: drop_prefetch
    // made the stream wait for it)
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(h->d_basis, mt.data(), mt.size() * sizeof(float), hipMemcpyHostToDevice));
    h->basis_host.swap(host);
    if (!m.active) {  // the default law as an active model: value for value the same normals
      m = NoiseModel{};
      m.active = 1;
      for (int u = 0; u < c.nu; ++u) m.sigma_u[u] = c.sigma;
    }
    m.n_basis = n_basis;
    m.basis_T = h->d_basis;
  } else {  // sigma_u stays as it stands: the rho = 0 generators again
    m.n_basis = 0;
    m.basis_T = nullptr;
  }
  h->noise_model = m;
  return MPPI_OK;
}

int mppi_get_noise_basis(mppi_handle* h, int* n_basis, float* M) {
  if (!h) return fail(MPPI_E_ARG, "mppi_get_noise_basis: null handle");
  const NoiseModel& m = h->noise_model;
  if (n_basis) *n_basis = m.n_basis;
  if (m.n_basis > 0 && M) std::memcpy(M, h->basis_host.data(), h->basis_host.size() * sizeof(float));  // (off: untouched)
  return MPPI_OK;
}

// the host's covariance (cov_host's Sigma, noise_model.sigma_u) -> d_cov_law; the stream is idle.  reset: the count of
// rejected steps starts again
static int upload_cov_law(mppi_handle* h, bool reset) {
  const size_t nn = (size_t)h->cfg.nu * h->cfg.nu;
  const CovLaw law = cov_law(h);
  if (reset) HIP_TRY(hipMemset(law.rejects, 0, sizeof(unsigned long long)));
  HIP_TRY(hipMemcpy(law.S, h->cov_host.data(), nn * sizeof(float), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(law.sigma_u, h->noise_model.sigma_u, kMaxNu * sizeof(float), hipMemcpyHostToDevice));
  HIP_TRY(hipDeviceSynchronize());  // (the null stream's copies are not ordered against the handle's stream)
  return MPPI_OK;
}

// the device covariance -> cov_host (Sigma, L, Sinv) and noise_model.sigma_u (waits for the stream)
static int fetch_cov_law(mppi_handle* h) {
  const int nu = h->cfg.nu;
  const size_t nn = (size_t)nu * nu;
  const CovLaw law = cov_law(h);
  HIP_TRY(hipStreamSynchronize(h->stream));
  float* host = h->cov_host.data();
  HIP_TRY(hipMemcpy(host, law.S, nn * sizeof(float), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy2D(host + nn, nu * sizeof(float), law.L, kMaxNu * sizeof(float), nu * sizeof(float), nu,
                      hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(host + 2 * nn, law.Sinv, nn * sizeof(float), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(h->noise_model.sigma_u, law.sigma_u, (size_t)nu * sizeof(float), hipMemcpyDeviceToHost));
  return MPPI_OK;
}

int mppi_set_noise_cov_adapt(mppi_handle* h, float rate, float sigma_min, float sigma_max) {
  if (!h) return fail(MPPI_E_ARG, "mppi_set_noise_cov_adapt: null handle");
  if (!(rate >= 0.0f && rate <= 1.0f)) return fail(MPPI_E_ARG, "mppi_set_noise_cov_adapt: rate must be in [0, 1]");
  if (!(sigma_min > 0.0f && sigma_min <= sigma_max && std::isfinite(sigma_max)))
    return fail(MPPI_E_ARG, "mppi_set_noise_cov_adapt: need 0 < sigma_min <= sigma_max < inf");
  const bool on = rate > 0.0f;
  if (on && h->cfg.nu > kMaxNu)
    return fail(MPPI_E_UNSUPPORTED, "mppi_set_noise_cov_adapt: the adapted covariance needs nu <= 32");
  if (on && h->noise_model.n_basis > 0)
    return fail(MPPI_E_UNSUPPORTED, "mppi_set_noise_cov_adapt: not together with mppi_set_noise_basis (the basis "
                                    "generator does not mix the actuators)");
  if (on && !h->noise_model.cov_L)
    return fail(MPPI_E_STATE, "mppi_set_noise_cov_adapt: no covariance to adapt: call mppi_set_noise_cov first");
  if (!on && !h->cov_adapt_on) {  // nothing to disable: only the limits are kept
    h->cov_adapt = NoiseCovAdapt{0.0f, sigma_min, sigma_max};
    return MPPI_OK;
  }
  HIP_TRY(hipSetDevice(h->device));
  // stale state, as in mppi_set_noise_adapt: the prefetched noise (the counter steps back: the key sequence is
  // unchanged) and the captured graphs, which hold the settings in their kernel arguments
  HIP_TRY(drop_prefetch(h));
  MPPI_TRY(drop_graphs(h, true));
  if (on && !h->cov_adapt_on) {
    const size_t bytes = 8 + ((size_t)h->cfg.nu * h->cfg.nu + kMaxNu) * sizeof(float);
    if (!h->d_cov_law) HIP_TRY(hipMalloc(&h->d_cov_law, bytes));
    HIP_TRY(hipStreamSynchronize(h->stream));
    MPPI_TRY(upload_cov_law(h, true));
    h->cov_adapt_on = true;
    h->cov_law_n = 0;
  } else if (!on) {  // back to the setter's law with the covariance as it stands
    MPPI_TRY(fetch_cov_law(h));
    h->cov_adapt_on = false;
  }
  h->cov_adapt = NoiseCovAdapt{rate, sigma_min, sigma_max};
  return MPPI_OK;
}

int mppi_get_noise_cov_adapt(mppi_handle* h, float* rate, float* sigma_min, float* sigma_max, uint64_t* rejects) {
  if (!h) return fail(MPPI_E_ARG, "mppi_get_noise_cov_adapt: null handle");
  if (rate) *rate = h->cov_adapt_on ? h->cov_adapt.rate : 0.0f;
  if (sigma_min) *sigma_min = h->cov_adapt.sigma_min;
  if (sigma_max) *sigma_max = h->cov_adapt.sigma_max;
  if (rejects) {
    unsigned long long r = 0;
    if (h->d_cov_law) {  // (it stays readable after the adaptation was disabled)
      HIP_TRY(hipSetDevice(h->device));
      HIP_TRY(hipStreamSynchronize(h->stream));
      HIP_TRY(hipMemcpy(&r, h->d_cov_law, sizeof(r), hipMemcpyDeviceToHost));
    }
    *rejects = r;
  }
  return MPPI_OK;
}

int mppi_get_noise_cov_law(mppi_handle* h, int step, float* Sigma) {
  if (!h || !Sigma) return fail(MPPI_E_ARG, "mppi_get_noise_cov_law: null argument");
  if (h->cov_law_n == 0)
    return fail(MPPI_E_STATE, "mppi_get_noise_cov_law: no solve that adapts the covariance has run on the handle");
  if (step < 0 || step >= h->cov_law_n)
    return fail(MPPI_E_ARG, "mppi_get_noise_cov_law: step beyond the solves of the last adapting solve or graph");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipStreamSynchronize(h->stream));
  const size_t nn = (size_t)h->cfg.nu * h->cfg.nu;
  HIP_TRY(hipMemcpy(Sigma, h->d_cov_hist + (size_t)step * nn, nn * sizeof(float), hipMemcpyDeviceToHost));
  return MPPI_OK;
}

int mppi_set_noise_cov(mppi_handle* h, const float* Sigma) {
  if (!h) return fail(MPPI_E_ARG, "mppi_set_noise_cov: null handle");
  const mppi_config& c = h->cfg;
  const size_t nn = (size_t)c.nu * c.nu;
  NoiseModel m = h->noise_model;
  if (!Sigma && !m.cov_L) return MPPI_OK;  // nothing to disable
  if (!Sigma && h->cov_adapt_on)
    return fail(MPPI_E_STATE, "mppi_set_noise_cov: the covariance is being adapted: disable it first "
                              "(mppi_set_noise_cov_adapt with rate 0)");
  std::vector<float> host;
  if (Sigma) {
    if (c.nu > kMaxNu)
      return fail(MPPI_E_UNSUPPORTED, "mppi_set_noise_cov: a covariance is an active noise model (nu <= 32)");
    host.resize(3 * nn);
    std::vector<double> scratch(3 * nn);
    float sig[kMaxNu];
    std::memcpy(host.data(), Sigma, nn * sizeof(float));
    if (!cov_factor(Sigma, c.nu, host.data() + nn, host.data() + 2 * nn, sig, scratch.data(), scratch.data() + nn))
      return fail(MPPI_E_ARG, "mppi_set_noise_cov: Sigma must be finite, symmetric bit for bit and positive definite "
                              "(every Cholesky pivot > 0)");
    // the value in effect, bitwise: prefetch and graphs stay (an adapting handle's law has moved: it is reset below)
    if (m.cov_L && !h->cov_adapt_on && std::memcmp(host.data(), h->cov_host.data(), nn * sizeof(float)) == 0) return MPPI_OK;
    if (m.n_knots > 0)
      return fail(MPPI_E_UNSUPPORTED, "mppi_set_noise_cov: not together with mppi_set_noise_knots (the knot generator "
                                      "does not mix the actuators)");
    if (h->adapt_on)
      return fail(MPPI_E_UNSUPPORTED, "mppi_set_noise_cov: not together with mppi_set_noise_adapt (the rule adapts "
                                      "sigma_u, which is not the law under a full covariance)");
    if (m.n_basis > 0)
      return fail(MPPI_E_UNSUPPORTED, "mppi_set_noise_cov: not together with mppi_set_noise_basis (the basis generator "
                                      "does not mix the actuators)");
    if (h->steps_on)
      return fail(MPPI_E_UNSUPPORTED, "mppi_set_noise_cov: not together with mppi_set_noise_steps (the covariance "
                                      "generator reads no per-step scale)");
    HIP_TRY(hipSetDevice(h->device));
    if (!h->d_cov) HIP_TRY(hipMalloc(&h->d_cov, ((size_t)c.nu * kMaxNu + nn) * sizeof(float)));
    if (!m.active) {  // the default law as an active model: rho = 0, the same normals
      const NoiseModel none{};
      m.active = 1, m.rho = none.rho, m.c = none.c;
    }
    for (int u = 0; u < c.nu; ++u) m.sigma_u[u] = sig[u];
  } else {
    HIP_TRY(hipSetDevice(h->device));
  }
  // stale state, as in mppi_set_noise_model: the prefetched noise (the counter steps back: the key sequence is
  // unchanged) and the captured graphs, whose generators are those of the other law
  HIP_TRY(drop_prefetch(h));
  MPPI_TRY(drop_graphs(h, true));
  if (Sigma) {
    // every launch that reads L or Sinv has finished before they change (the generator stream included: drop_prefetch
    // made the stream wait for it)
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy2D(h->d_cov, kMaxNu * sizeof(float), host.data() + nn, c.nu * sizeof(float), c.nu * sizeof(float),
                        c.nu, hipMemcpyHostToDevice));  // (the pad of a row is never read)
    HIP_TRY(hipMemcpy(h->d_cov + (size_t)c.nu * kMaxNu, host.data() + 2 * nn, nn * sizeof(float), hipMemcpyHostToDevice));
    h->cov_host.swap(host);
    m.cov_L = h->d_cov;
    if (h->cov_adapt_on) {  // the device law starts again from here (the count of rejected steps goes on)
      h->noise_model = m;
      MPPI_TRY(upload_cov_law(h, false));
    }
  } else {  // sigma_u (= sqrt of the diagonal) and rho stay as they stand: the AR(1) generators again
    m.cov_L = nullptr;
  }
  h->noise_model = m;
  return MPPI_OK;
}

int mppi_get_noise_cov(mppi_handle* h, float* Sigma, float* L, float* Sinv, int* active) {
  if (!h) return fail(MPPI_E_ARG, "mppi_get_noise_cov: null handle");
  const bool on = h->noise_model.cov_L != nullptr;
  if (active) *active = on ? 1 : 0;
  if (h->cov_adapt_on) {  // the live law: every enqueued solve's update included
    HIP_TRY(hipSetDevice(h->device));
    MPPI_TRY(fetch_cov_law(h));
  }
  if (on) {  // (off: the arrays are left untouched)
    const size_t nn = (size_t)h->cfg.nu * h->cfg.nu;
    if (Sigma) std::memcpy(Sigma, h->cov_host.data(), nn * sizeof(float));
    if (L) std::memcpy(L, h->cov_host.data() + nn, nn * sizeof(float));
    if (Sinv) std::memcpy(Sinv, h->cov_host.data() + 2 * nn, nn * sizeof(float));
  }
  return MPPI_OK;
}

int mppi_set_noise_steps(mppi_handle* h, int B, const float* sigma) {
  if (!h) return fail(MPPI_E_ARG, "mppi_set_noise_steps: null handle");
  const mppi_config& c = h->cfg;
  if (!sigma) {  // off: sigma_u and rho stay as they stand, the AR(1) generators again
    if (!h->steps_on) return MPPI_OK;  // nothing to disable
    if (h->steps_adapt_on)
      return fail(MPPI_E_STATE, "mppi_set_noise_steps: the table is being refit: disable it first "
                                "(mppi_set_noise_steps_adapt with rate 0)");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(drop_prefetch(h));
    MPPI_TRY(drop_graphs(h, true));
    h->steps_on = false;
    return MPPI_OK;
  }
  if (B < 1 || B > c.max_batch) return fail(MPPI_E_ARG, "mppi_set_noise_steps: B out of range [1, max_batch]");
  const size_t row = (size_t)c.nu * c.H;
  for (size_t i = 0; i < (size_t)B * row; ++i)
    if (!(std::isfinite(sigma[i]) && sigma[i] >= 0.0f))
      return fail(MPPI_E_ARG, "mppi_set_noise_steps: sigma[" + std::to_string(i) + "] must be finite and >= 0");
  if (c.nu > kMaxNu)
    return fail(MPPI_E_UNSUPPORTED, "mppi_set_noise_steps: a table of per-step scales is an active noise model (nu <= 32)");
  NoiseModel m = h->noise_model;
  if (m.n_knots > 0)
    return fail(MPPI_E_UNSUPPORTED, "mppi_set_noise_steps: not together with mppi_set_noise_knots (the knot generator "
                                    "reads no per-step scale)");
  if (m.n_basis > 0)
    return fail(MPPI_E_UNSUPPORTED, "mppi_set_noise_steps: not together with mppi_set_noise_basis (the basis generators "
                                    "read no per-step scale)");
  if (m.cov_L)
    return fail(MPPI_E_UNSUPPORTED, "mppi_set_noise_steps: not together with mppi_set_noise_cov / "
                                    "mppi_set_noise_cov_adapt (the covariance generator reads no per-step scale)");
  if (h->adapt_on)
    return fail(MPPI_E_UNSUPPORTED, "mppi_set_noise_steps: not together with mppi_set_noise_adapt (the rule adapts one "
                                    "sigma_u per actuator, which is not the scale under a per-step table)");
  if (h->ctrl_gamma > 0.0f)
    return fail(MPPI_E_UNSUPPORTED, "mppi_set_noise_steps: not together with mppi_set_control_cost (under AR(1) the term "
                                    "needs D^-1 P D^-1 per cell of the table, which is not built)");
  // every slot of the handle: slot b takes row b mod B (B = 1 broadcasts one table)
  std::vector<float> host((size_t)c.max_batch * row);
  for (int b = 0; b < c.max_batch; ++b) std::memcpy(host.data() + (size_t)b * row, sigma + (size_t)(b % B) * row, row * 4);
  // the table in effect, bitwise: prefetch and graphs stay (a refitting handle's table has moved: it is set again below)
  if (h->steps_on && !h->steps_adapt_on && std::memcmp(host.data(), h->steps_host.data(), host.size() * 4) == 0)
    return MPPI_OK;
  HIP_TRY(hipSetDevice(h->device));
  if (!h->d_steps) HIP_TRY(hipMalloc(&h->d_steps, at_least16(host.size() * 4)));
  // stale state, as in mppi_set_noise_model: the prefetched noise (the counter steps back: the key sequence is
  // unchanged) and the captured graphs, whose generators are those of the other law
  HIP_TRY(drop_prefetch(h));
  MPPI_TRY(drop_graphs(h, true));
  // on the handle's stream, behind every launch that reads the table (the generator stream included: drop_prefetch made
  // the stream wait for it); the source stays alive in the handle
  h->steps_host.swap(host);
  HIP_TRY(hipMemcpyAsync(h->d_steps, h->steps_host.data(), h->steps_host.size() * 4, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));  // (the next call may replace steps_host)
  if (!m.active) {  // the default law as an active model: value for value the same normals
    m = NoiseModel{};
    m.active = 1;
    for (int u = 0; u < c.nu; ++u) m.sigma_u[u] = c.sigma;
  }
  h->noise_model = m;
  h->steps_on = true;
  return MPPI_OK;
}

int mppi_get_noise_steps(mppi_handle* h, int B, float* sigma, int* active) {
  if (!h) return fail(MPPI_E_ARG, "mppi_get_noise_steps: null handle");
  if (B < 1 || B > h->cfg.max_batch) return fail(MPPI_E_ARG, "mppi_get_noise_steps: B out of range [1, max_batch]");
  if (active) *active = h->steps_on ? 1 : 0;
  if (h->steps_on && sigma) {  // the live table: every enqueued solve's refit included (off: the array is left untouched)
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipMemcpyAsync(sigma, h->d_steps, (size_t)B * h->cfg.nu * h->cfg.H * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
  }
  return MPPI_OK;
}

int mppi_set_noise_steps_adapt(mppi_handle* h, float rate, float sigma_min, float sigma_max, int centred) {
  if (!h) return fail(MPPI_E_ARG, "mppi_set_noise_steps_adapt: null handle");
  if (!(rate >= 0.0f && rate <= 1.0f)) return fail(MPPI_E_ARG, "mppi_set_noise_steps_adapt: rate must be in [0, 1]");
  if (!(sigma_min > 0.0f && sigma_min <= sigma_max && std::isfinite(sigma_max)))
    return fail(MPPI_E_ARG, "mppi_set_noise_steps_adapt: need 0 < sigma_min <= sigma_max < inf");
  if (centred != 0 && centred != 1) return fail(MPPI_E_ARG, "mppi_set_noise_steps_adapt: centred must be 0 or 1");
  const bool on = rate > 0.0f;
  if (on && !h->steps_on)
    return fail(MPPI_E_STATE, "mppi_set_noise_steps_adapt: no table to refit: call mppi_set_noise_steps first");
  if (!on && !h->steps_adapt_on) {  // nothing to disable: only the settings are kept
    h->steps_adapt = StepAdapt{0.0f, sigma_min, sigma_max, centred};
    return MPPI_OK;
  }
  HIP_TRY(hipSetDevice(h->device));
  // stale state, as in mppi_set_noise_adapt: the prefetched noise (the counter steps back: the key sequence is
  // unchanged) and the captured graphs, which hold the settings in their kernel arguments
  HIP_TRY(drop_prefetch(h));
  MPPI_TRY(drop_graphs(h, true));
  if (!on) {  // the table stays as it stands on the device; the host's copy of "the table in effect" follows it
    HIP_TRY(hipMemcpyAsync(h->steps_host.data(), h->d_steps, h->steps_host.size() * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
  }
  h->steps_adapt_on = on;
  h->steps_adapt = StepAdapt{rate, sigma_min, sigma_max, centred};
  return MPPI_OK;
}

int mppi_get_noise_steps_adapt(mppi_handle* h, float* rate, float* sigma_min, float* sigma_max, int* centred) {
  if (!h) return fail(MPPI_E_ARG, "mppi_get_noise_steps_adapt: null handle");
  if (rate) *rate = h->steps_adapt_on ? h->steps_adapt.rate : 0.0f;
  if (sigma_min) *sigma_min = h->steps_adapt.sigma_min;
  if (sigma_max) *sigma_max = h->steps_adapt.sigma_max;
  if (centred) *centred = h->steps_adapt.centred;
  return MPPI_OK;
}

int mppi_noise_eval(mppi_handle* h, int B, uint64_t seed, float* noise_out) {
  if (!h || !noise_out) return fail(MPPI_E_ARG, "mppi_noise_eval: null argument");
  const mppi_config& c = h->cfg;
  if (B < 1 || B > c.max_batch) return fail(MPPI_E_ARG, "mppi_noise_eval: B out of range [1, max_batch]");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(drop_prefetch(h));  // d_noise may hold the next chained solve's noise: its key is drawn again
  hipStream_t s = h->stream;
  const size_t K = (size_t)c.K, Kp = (size_t)h->Kp, rows = (size_t)B * c.nu * c.H;
  // the generator of a solve's a1 under the law in effect, key = seed (no counter); no projection, no injection
  HIP_TRY(timed(h, kNoise, [&] {
    return launch_noise_model(h->d_noise, B, c.nu, c.H, h->Kp, seed, nullptr, c.sigma, h->noise_model, s, gen_law(h),
                              gen_steps(h));
  }));
  HIP_TRY(hipMemcpy2DAsync(noise_out, K * 4, h->d_noise, Kp * 4, K * 4, rows, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return MPPI_OK;
}

int mppi_set_ess_target(mppi_handle* h, float ess_frac, float lambda_min, float lambda_max) {
  if (!h) return fail(MPPI_E_ARG, "mppi_set_ess_target: null handle");
  if (!(ess_frac >= 0.0f && ess_frac <= 1.0f)) return fail(MPPI_E_ARG, "mppi_set_ess_target: ess_frac must be in [0, 1]");
  if (!(lambda_min > 0.0f && lambda_min <= lambda_max && std::isfinite(lambda_max)))
    return fail(MPPI_E_ARG, "mppi_set_ess_target: need 0 < lambda_min <= lambda_max < inf");
  const bool on = ess_frac > 0.0f;
  const EssTarget t{ess_frac, lambda_min, lambda_max};
  if (!on && !h->ess_on) {  // nothing to disable: only the limits are kept
    h->ess = t;
    return MPPI_OK;
  }
  if (on && h->ess_on && std::memcmp(&t, &h->ess, sizeof(t)) == 0) return MPPI_OK;  // no change
  HIP_TRY(hipSetDevice(h->device));
  // stale state: the captured graphs hold the settings (or their absence) in their launches; a launch still in flight
  // finishes first.  A prefetched noise is kept: lambda does not enter the noise, the key sequence is unchanged
  MPPI_TRY(drop_graphs(h, true));
  h->ess = t;
  h->ess_on = on;
  return MPPI_OK;
}

int mppi_get_ess_target(mppi_handle* h, float* ess_frac, float* lambda_min, float* lambda_max) {
  if (!h) return fail(MPPI_E_ARG, "mppi_get_ess_target: null handle");
  if (ess_frac) *ess_frac = h->ess_on ? h->ess.ess_frac : 0.0f;
  if (lambda_min) *lambda_min = h->ess.lambda_min;
  if (lambda_max) *lambda_max = h->ess.lambda_max;
  return MPPI_OK;
}

int mppi_get_lambda(mppi_handle* h, int B, int step, float* lambda) {
  if (!h || !lambda) return fail(MPPI_E_ARG, "mppi_get_lambda: null argument");
  if (h->lam_n == 0) return fail(MPPI_E_STATE, "mppi_get_lambda: no solve with ESS targeting has run on the handle");
  if (B < 1 || B > h->lam_B) return fail(MPPI_E_ARG, "mppi_get_lambda: B beyond the batch of the last targeting solve");
  if (step < 0 || step >= h->lam_n)
    return fail(MPPI_E_ARG, "mppi_get_lambda: step beyond the solves of the last targeting solve or graph");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipMemcpy(lambda, h->d_lambda + (size_t)step * h->cfg.max_batch, (size_t)B * 4, hipMemcpyDeviceToHost));
  return MPPI_OK;
}

int mppi_lambda_eval(mppi_handle* h, int B, const float* costs, float* lambda) {
  if (!h || !costs || !lambda) return fail(MPPI_E_ARG, "mppi_lambda_eval: null argument");
  const mppi_config& c = h->cfg;
  if (B < 1 || B > c.max_batch) return fail(MPPI_E_ARG, "mppi_lambda_eval: B out of range [1, max_batch]");
  if (!h->ess_on) return fail(MPPI_E_STATE, "mppi_lambda_eval: call mppi_set_ess_target first");
  HIP_TRY(hipSetDevice(h->device));
  MPPI_TRY(ensure_lambda(h, 1));
  hipStream_t s = h->stream;
  MPPI_TRY(stage_costs(h, costs, B));
  float* out = h->d_lambda + (size_t)h->lambda_slots * c.max_batch;  // the evaluation's own slot
  HIP_TRY(timed(h, kLambda, [&] { return launch_lambda_search(h->d_costs, B, c.K, h->Kp, h->ess, c.lambda, out, s); }));
  HIP_TRY(hipMemcpyAsync(lambda, out, (size_t)B * 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return MPPI_OK;
}

int mppi_set_control_cost(mppi_handle* h, float gamma) {
  if (!h) return fail(MPPI_E_ARG, "mppi_set_control_cost: null handle");
  if (!(gamma >= 0.0f && std::isfinite(gamma)))
    return fail(MPPI_E_ARG, "mppi_set_control_cost: gamma must be finite and >= 0");
  if (gamma == h->ctrl_gamma) return MPPI_OK;  // no change: captured graphs stay
  if (gamma > 0.0f && h->noise_model.n_knots > 0)
    return fail(MPPI_E_UNSUPPORTED, "mppi_set_control_cost: not together with mppi_set_noise_knots (the term needs the "
                                    "inverse of the sampling covariance, which a knot law leaves singular)");
  if (gamma > 0.0f && h->noise_model.n_basis > 0)
    return fail(MPPI_E_UNSUPPORTED, "mppi_set_control_cost: not together with mppi_set_noise_basis (the term needs the "
                                    "inverse of M M^T, singular for n_basis < H)");
  if (gamma > 0.0f && h->steps_on)
    return fail(MPPI_E_UNSUPPORTED, "mppi_set_control_cost: not together with mppi_set_noise_steps (under AR(1) the "
                                    "term needs D^-1 P D^-1 per cell of the table, which is not built)");
  HIP_TRY(hipSetDevice(h->device));
  const mppi_config& c = h->cfg;
  if (gamma > 0.0f && !h->d_wcost) {  // all of the term's buffers, once, or none (every entry is written before it is read)
    const size_t nk = (size_t)2 * c.max_batch * h->Kp * 4, nl = (size_t)c.max_batch * c.nu * c.H * 4;
    const size_t np = term_part_floats(c.max_batch, c.nu, c.H, h->Kp) * 4;
    MPPI_TRY(alloc_group("mppi_set_control_cost", {{(void**)&h->d_wcost, nk},
                                                   {(void**)&h->d_term, nk},
                                                   {(void**)&h->d_lin, 2 * nl},
                                                   {(void**)&h->d_ctrl_part, at_least16(np)},
                                                   {(void**)&h->d_ctrl_U, nl}}));
  }
  // stale state: the captured graphs hold gamma (or the term's absence) in their launches; a launch still in flight
  // finishes first.  A prefetched noise is kept: gamma does not enter the noise, the key sequence is unchanged
  MPPI_TRY(drop_graphs(h, true));
  h->ctrl_gamma = gamma;
  return MPPI_OK;
}

int mppi_get_control_cost(mppi_handle* h, float* gamma) {
  if (!h) return fail(MPPI_E_ARG, "mppi_get_control_cost: null handle");
  if (gamma) *gamma = h->ctrl_gamma;
  return MPPI_OK;
}

// slot `slot` of the term's outputs -> host (the stream is idle)
static int copy_ctrl(mppi_handle* h, int B, int slot, float* term, float* lin) {
  const mppi_config& c = h->cfg;
  const size_t K = (size_t)c.K, Kp = (size_t)h->Kp, rows = (size_t)c.nu * c.H;
  const mppi_handle::Shape sh = readout_shape(h, slot);  // (rows of cfg.K, of which the solve's K samples are written)
  if (term)
    HIP_TRY(hipMemcpy2D(term, K * 4, h->d_term + (size_t)slot * c.max_batch * Kp, (size_t)sh.Kp * 4, (size_t)sh.K * 4, B,
                        hipMemcpyDeviceToHost));
  if (lin)
    HIP_TRY(hipMemcpy(lin, h->d_lin + (size_t)slot * c.max_batch * rows, (size_t)B * rows * 4, hipMemcpyDeviceToHost));
  return MPPI_OK;
}

int mppi_get_control_term(mppi_handle* h, int B, float* term, float* lin) {
  if (!h) return fail(MPPI_E_ARG, "mppi_get_control_term: null handle");
  if (h->ctrl_B == 0)
    return fail(MPPI_E_STATE, "mppi_get_control_term: no solve with the control-cost term has run on the handle");
  if (B < 1 || B > h->ctrl_B)
    return fail(MPPI_E_ARG, "mppi_get_control_term: B beyond the batch of the last solve with the term");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return copy_ctrl(h, B, 0, term, lin);
}

int mppi_control_term_eval(mppi_handle* h, int B, const float* U, const float* noise, float* term, float* lin) {
  if (!h || !U || !noise) return fail(MPPI_E_ARG, "mppi_control_term_eval: null argument");
  const mppi_config& c = h->cfg;
  if (B < 1 || B > c.max_batch) return fail(MPPI_E_ARG, "mppi_control_term_eval: B out of range [1, max_batch]");
  if (!(h->ctrl_gamma > 0.0f)) return fail(MPPI_E_STATE, "mppi_control_term_eval: call mppi_set_control_cost first");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(drop_prefetch(h));  // d_noise may hold the next chained solve's noise: its key is drawn again
  hipStream_t s = h->stream;
  const size_t rows = (size_t)B * c.nu * c.H;
  HIP_TRY(hipMemcpyAsync(h->d_ctrl_U, U, rows * 4, hipMemcpyHostToDevice, s));
  MPPI_TRY(stage_noise(h, noise, rows));
  // (the evaluation's own slot; its wcost adds the term to whatever the staging costs hold and is never read)
  HIP_TRY(timed(h, kCtrl, [&] { return enqueue_ctrl(h, B, h->d_ctrl_U, h->d_noise, h->d_costs, 1); }));
  HIP_TRY(hipStreamSynchronize(s));
  return copy_ctrl(h, B, 1, term, lin);
}

int mppi_set_control_bounds(mppi_handle* h, const float* lo, const float* hi) {
  if (!h) return fail(MPPI_E_ARG, "mppi_set_control_bounds: null handle");
  const mppi_config& c = h->cfg;
  const bool on = lo != nullptr || hi != nullptr;
  if (!on && !h->bounds_on) return MPPI_OK;  // nothing to disable
  if (on && c.nu > kMaxNu)
    return fail(MPPI_E_UNSUPPORTED, "mppi_set_control_bounds: the box travels as a kernel argument (nu <= 32)");
  float nlo[kMaxNu] = {0}, nhi[kMaxNu] = {0};
  if (on) {
    for (int u = 0; u < c.nu; ++u) {
      nlo[u] = lo ? lo[u] : -INFINITY;
      nhi[u] = hi ? hi[u] : INFINITY;
    }
    if (!ctrl_bounds_valid(nlo, nhi, c.nu))
      return fail(MPPI_E_ARG, "mppi_set_control_bounds: need lo[u] <= hi[u], neither a NaN, for every actuator");
    if (h->bounds_on && std::memcmp(nlo, h->bounds_lo, sizeof(nlo)) == 0 &&
        std::memcmp(nhi, h->bounds_hi, sizeof(nhi)) == 0)
      return MPPI_OK;  // no change: captured graphs stay
  }
  HIP_TRY(hipSetDevice(h->device));
  if (on && !h->d_bcounts) {  // all three buffers, once, or none (every entry is written before it is read)
    const size_t nc = (size_t)2 * c.max_batch * c.nu * sizeof(unsigned), nU = (size_t)c.max_batch * c.nu * c.H * 4;
    const size_t np = (size_t)c.max_batch * c.nu * c.H * bounds_chunks(h->Kp) * sizeof(unsigned);
    MPPI_TRY(alloc_group("mppi_set_control_bounds", {{(void**)&h->d_bcounts, at_least16(nc)},
                                                     {(void**)&h->d_bpart, at_least16(np)},
                                                     {(void**)&h->d_bounds_U, at_least16(nU)}}));
  }
  // stale state: the captured graphs hold the box (or its absence) in their launches; a launch still in flight finishes
  // first.  A prefetched noise is kept: it is projected at the start of the solve that consumes it, with the box in
  // effect then, so the key sequence is unchanged
  MPPI_TRY(drop_graphs(h, true));
  std::memcpy(h->bounds_lo, nlo, sizeof(nlo));
  std::memcpy(h->bounds_hi, nhi, sizeof(nhi));
  h->bounds_on = on;
  return MPPI_OK;
}

int mppi_get_control_bounds(mppi_handle* h, float* lo, float* hi, int* active) {
  if (!h) return fail(MPPI_E_ARG, "mppi_get_control_bounds: null handle");
  for (int u = 0; u < h->cfg.nu; ++u) {
    if (lo) lo[u] = h->bounds_on ? h->bounds_lo[u] : -INFINITY;
    if (hi) hi[u] = h->bounds_on ? h->bounds_hi[u] : INFINITY;
  }
  if (active) *active = h->bounds_on ? 1 : 0;
  return MPPI_OK;
}

int mppi_get_bound_counts(mppi_handle* h, int B, uint32_t* counts) {
  if (!h || !counts) return fail(MPPI_E_ARG, "mppi_get_bound_counts: null argument");
  if (h->bounds_B == 0) return fail(MPPI_E_STATE, "mppi_get_bound_counts: no solve with control bounds has run on the handle");
  if (B < 1 || B > h->bounds_B)
    return fail(MPPI_E_ARG, "mppi_get_bound_counts: B beyond the batch of the last bounded solve");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipMemcpy(counts, h->d_bcounts, (size_t)B * h->cfg.nu * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return MPPI_OK;
}

int mppi_bounds_eval(mppi_handle* h, int B, const float* U, const float* noise_in, float* noise_out, uint32_t* counts) {
  if (!h || !U || !noise_in) return fail(MPPI_E_ARG, "mppi_bounds_eval: null argument");
  const mppi_config& c = h->cfg;
  if (B < 1 || B > c.max_batch) return fail(MPPI_E_ARG, "mppi_bounds_eval: B out of range [1, max_batch]");
  if (!h->bounds_on) return fail(MPPI_E_STATE, "mppi_bounds_eval: call mppi_set_control_bounds first");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(drop_prefetch(h));  // d_noise may hold the next chained solve's noise: its key is drawn again
  hipStream_t s = h->stream;
  const size_t K = (size_t)c.K, Kp = (size_t)h->Kp, rows = (size_t)B * c.nu * c.H;
  HIP_TRY(hipMemcpyAsync(h->d_bounds_U, U, rows * 4, hipMemcpyHostToDevice, s));
  MPPI_TRY(stage_noise(h, noise_in, rows));
  HIP_TRY(timed(h, kBounds, [&] {  // the projection, then its counts into the evaluation's own slot (no U to clip)
    const hipError_t e = enqueue_bounds_project(h, B, h->d_bounds_U, h->d_noise);
    return e != hipSuccess ? e : launch_bounds_clip(bounds_args(h, B, 1), nullptr, nullptr, nullptr, s);
  }));
  if (noise_out)
    HIP_TRY(hipMemcpy2DAsync(noise_out, K * 4, h->d_noise, Kp * 4, K * 4, rows, hipMemcpyDeviceToHost, s));
  if (counts)
    HIP_TRY(hipMemcpyAsync(counts, h->d_bcounts + (size_t)c.max_batch * c.nu, (size_t)B * c.nu * sizeof(uint32_t),
                           hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return MPPI_OK;
}

// u_prev [2][max_batch][nu], zeroed: by whichever of mppi_set_rate_cost / mppi_set_prev_control comes first
static int ensure_uprev(mppi_handle* h) {
  if (h->d_uprev) return MPPI_OK;
  const size_t n = (size_t)2 * h->cfg.max_batch * h->cfg.nu * 4;
  float* p = nullptr;
  HIP_TRY(hipMalloc(&p, n < 16 ? 16 : n));
  // zeroed ON THE HANDLE'S STREAM and waited for: a memset on the null stream is not ordered against the copies and
  // launches the (non-blocking) stream receives next, and could land behind mppi_set_prev_control's values
  hipError_t e = hipMemsetAsync(p, 0, n, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess) {
    (void)hipFree(p);
    return fail(MPPI_E_HIP, std::string("u_prev: ") + hipGetErrorString(e));
  }
  h->d_uprev = p;
  return MPPI_OK;
}

int mppi_set_rate_cost(mppi_handle* h, const float* r, int anchor) {
  if (!h) return fail(MPPI_E_ARG, "mppi_set_rate_cost: null handle");
  const mppi_config& c = h->cfg;
  const bool on = r != nullptr;
  if (!on && !h->rate_on) return MPPI_OK;  // nothing to disable
  if (on && c.nu > kMaxNu)
    return fail(MPPI_E_UNSUPPORTED, "mppi_set_rate_cost: the weights travel as a kernel argument (nu <= 32)");
  float nr[kMaxNu] = {0};
  const int na = on && anchor ? 1 : 0;
  if (on) {
    std::memcpy(nr, r, (size_t)c.nu * 4);
    if (!rate_cost_valid(nr, c.nu))
      return fail(MPPI_E_ARG, "mppi_set_rate_cost: r must be finite, every entry >= 0 and at least one > 0");
    if (h->rate_on && na == h->rate_anchor && std::memcmp(nr, h->rate_r, sizeof(nr)) == 0)
      return MPPI_OK;  // no change: captured graphs stay
  }
  HIP_TRY(hipSetDevice(h->device));
  if (on) MPPI_TRY(ensure_uprev(h));
  if (on && !h->d_rate_wcost) {  // the term's buffers, once, all or none (every entry is written before it is read)
    const size_t nk = (size_t)2 * c.max_batch * h->Kp * 4, nl = (size_t)c.max_batch * c.nu * c.H * 4;
    const size_t np = term_part_floats(c.max_batch, c.nu, c.H, h->Kp) * 4;
    MPPI_TRY(alloc_group("mppi_set_rate_cost", {{(void**)&h->d_rate_wcost, nk},
                                                {(void**)&h->d_rate_term, nk},
                                                {(void**)&h->d_rate_part, at_least16(np)},
                                                {(void**)&h->d_rate_U, nl}}));
  }
  // stale state: the captured graphs hold r and the anchor (or the term's absence) in their launches; a launch still in
  // flight finishes first.  A prefetched noise is kept: the term does not enter the noise, the key sequence is unchanged
  MPPI_TRY(drop_graphs(h, true));
  std::memcpy(h->rate_r, nr, sizeof(nr));
  h->rate_anchor = na;
  h->rate_on = on;
  return MPPI_OK;
}

int mppi_get_rate_cost(mppi_handle* h, float* r, int* anchor, int* active) {
  if (!h) return fail(MPPI_E_ARG, "mppi_get_rate_cost: null handle");
  if (r)
    for (int u = 0; u < h->cfg.nu; ++u) r[u] = h->rate_on ? h->rate_r[u] : 0.0f;
  if (anchor) *anchor = h->rate_on ? h->rate_anchor : 0;
  if (active) *active = h->rate_on ? 1 : 0;
  return MPPI_OK;
}

int mppi_set_prev_control(mppi_handle* h, int B, const float* u_prev) {
  if (!h || !u_prev) return fail(MPPI_E_ARG, "mppi_set_prev_control: null argument");
  if (B < 1 || B > h->cfg.max_batch) return fail(MPPI_E_ARG, "mppi_set_prev_control: B out of range [1, max_batch]");
  HIP_TRY(hipSetDevice(h->device));
  MPPI_TRY(ensure_uprev(h));
  // data, not a launch argument: ordered on the stream behind every solve enqueued so far, captured graphs stay
  HIP_TRY(hipMemcpyAsync(h->d_uprev, u_prev, (size_t)B * h->cfg.nu * 4, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));  // (the caller's array may go)
  return MPPI_OK;
}

int mppi_get_prev_control(mppi_handle* h, int B, float* u_prev) {
  if (!h || !u_prev) return fail(MPPI_E_ARG, "mppi_get_prev_control: null argument");
  if (B < 1 || B > h->cfg.max_batch) return fail(MPPI_E_ARG, "mppi_get_prev_control: B out of range [1, max_batch]");
  const size_t n = (size_t)B * h->cfg.nu;
  if (!h->d_uprev) {  // never set, never stored: zeros
    std::memset(u_prev, 0, n * 4);
    return MPPI_OK;
  }
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipMemcpy(u_prev, h->d_uprev, n * 4, hipMemcpyDeviceToHost));
  return MPPI_OK;
}

// slot `slot` of the rate term -> host (the stream is idle)
static int copy_rate(mppi_handle* h, int B, int slot, float* term) {
  const size_t K = (size_t)h->cfg.K, Kp = (size_t)h->Kp;
  const mppi_handle::Shape sh = readout_shape(h, slot);  // (rows of cfg.K, of which the solve's K samples are written)
  HIP_TRY(hipMemcpy2D(term, K * 4, h->d_rate_term + (size_t)slot * h->cfg.max_batch * Kp, (size_t)sh.Kp * 4,
                      (size_t)sh.K * 4, B, hipMemcpyDeviceToHost));
  return MPPI_OK;
}

int mppi_get_rate_term(mppi_handle* h, int B, float* term) {
  if (!h || !term) return fail(MPPI_E_ARG, "mppi_get_rate_term: null argument");
  if (h->rate_B == 0) return fail(MPPI_E_STATE, "mppi_get_rate_term: no solve with the rate term has run on the handle");
  if (B < 1 || B > h->rate_B) return fail(MPPI_E_ARG, "mppi_get_rate_term: B beyond the batch of the last solve with the term");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return copy_rate(h, B, 0, term);
}

int mppi_rate_term_eval(mppi_handle* h, int B, const float* U, const float* noise, const float* u_prev, float* term) {
  if (!h || !U || !noise || !term) return fail(MPPI_E_ARG, "mppi_rate_term_eval: null argument");
  const mppi_config& c = h->cfg;
  if (B < 1 || B > c.max_batch) return fail(MPPI_E_ARG, "mppi_rate_term_eval: B out of range [1, max_batch]");
  if (!h->rate_on) return fail(MPPI_E_STATE, "mppi_rate_term_eval: call mppi_set_rate_cost first");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(drop_prefetch(h));  // d_noise may hold the next chained solve's noise: its key is drawn again
  hipStream_t s = h->stream;
  const size_t rows = (size_t)B * c.nu * c.H;
  float* const up = h->d_uprev + (size_t)c.max_batch * c.nu;  // the evaluation's own u_prev (the handle's stays)
  HIP_TRY(hipMemcpyAsync(h->d_rate_U, U, rows * 4, hipMemcpyHostToDevice, s));
  if (u_prev) HIP_TRY(hipMemcpyAsync(up, u_prev, (size_t)B * c.nu * 4, hipMemcpyHostToDevice, s));
  MPPI_TRY(stage_noise(h, noise, rows));
  // (the evaluation's own slot; its wcost adds the term to whatever the staging costs hold and is never read)
  HIP_TRY(timed(h, kRate, [&] {
    return enqueue_rate(h, B, h->d_rate_U, h->d_noise, u_prev ? up : h->d_uprev, h->d_costs, 1);
  }));
  HIP_TRY(hipStreamSynchronize(s));
  return copy_rate(h, B, 1, term);
}

int mppi_set_elites(mppi_handle* h, int n_elite) {
  if (!h) return fail(MPPI_E_ARG, "mppi_set_elites: null handle");
  const mppi_config& c = h->cfg;
  if (n_elite < 0 || n_elite > c.K) return fail(MPPI_E_ARG, "mppi_set_elites: n_elite must be in [0, K] (0 disables)");
  if (n_elite == h->elite_n) return MPPI_OK;  // no change: captured graphs stay
  MPPI_TRY(pop_check(h, "mppi_set_elites", h->iter_n, n_elite, h->keep_n, h->iter_mean));
  HIP_TRY(hipSetDevice(h->device));
  // stale state: the captured graphs hold n_elite (or the selection's absence) in their launches, and the set's rows
  // have n_elite entries; everything in flight finishes first.  A prefetched noise is kept: the selection does not
  // enter the noise, the key sequence is unchanged
  HIP_TRY(hipStreamSynchronize(h->stream));
  if (n_elite > 0) {  // the feature's buffers (every entry is written before it is read); the set's by its row length
    const size_t nb = (size_t)2 * c.max_batch;
    int32_t* ni = nullptr;  // (the old set stays until the new one exists)
    std::vector<BufReq> reqs{{(void**)&ni, nb * n_elite * 4}};
    if (!h->d_elite_wcost) {
      reqs.push_back({(void**)&h->d_elite_wcost, nb * h->Kp * 4});
      reqs.push_back({(void**)&h->d_elite_count, nb * 4});
      reqs.push_back({(void**)&h->d_elite_tau, nb * 4});
    }
    MPPI_TRY(alloc_group("mppi_set_elites", reqs));
    if (h->d_elite_idx) (void)hipFree(h->d_elite_idx);
    h->d_elite_idx = ni;
  }
  MPPI_TRY(drop_graphs(h, false));
  h->elite_n = n_elite;
  h->elite_B = 0;  // the last set had another row length: none to read until the next solve
  return MPPI_OK;
}

int mppi_get_elites(mppi_handle* h, int* n_elite) {
  if (!h) return fail(MPPI_E_ARG, "mppi_get_elites: null handle");
  if (n_elite) *n_elite = h->elite_n;
  return MPPI_OK;
}

// slot `slot` of the elite set -> host (the stream is idle); each pointer may be nullptr
static int copy_elites(mppi_handle* h, int B, int slot, int32_t* idx, int32_t* count, float* tau, float* ecost) {
  const size_t ob = (size_t)slot * h->cfg.max_batch, K = (size_t)h->cfg.K, Kp = (size_t)h->Kp;
  if (idx)
    HIP_TRY(hipMemcpy(idx, h->d_elite_idx + ob * h->elite_n, (size_t)B * h->elite_n * 4, hipMemcpyDeviceToHost));
  if (count) HIP_TRY(hipMemcpy(count, h->d_elite_count + ob, (size_t)B * 4, hipMemcpyDeviceToHost));
  if (tau) HIP_TRY(hipMemcpy(tau, h->d_elite_tau + ob, (size_t)B * 4, hipMemcpyDeviceToHost));
  const mppi_handle::Shape sh = readout_shape(h, slot);  // (rows of cfg.K, of which the solve's K samples are written)
  if (ecost)
    HIP_TRY(hipMemcpy2D(ecost, K * 4, h->d_elite_wcost + ob * Kp, (size_t)sh.Kp * 4, (size_t)sh.K * 4, B,
                        hipMemcpyDeviceToHost));
  return MPPI_OK;
}

int mppi_get_elite_set(mppi_handle* h, int B, int32_t* idx, int32_t* count, float* tau) {
  if (!h) return fail(MPPI_E_ARG, "mppi_get_elite_set: null handle");
  if (h->elite_B == 0 || h->elite_n == 0)
    return fail(MPPI_E_STATE, "mppi_get_elite_set: no solve with the current elites setting has run on the handle");
  if (B < 1 || B > h->elite_B) return fail(MPPI_E_ARG, "mppi_get_elite_set: B beyond the batch of the last solve with elites");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return copy_elites(h, B, 0, idx, count, tau, nullptr);
}

int mppi_elites_eval(mppi_handle* h, int B, const float* costs, int32_t* idx, int32_t* count, float* tau,
                     float* ecost) {
  if (!h || !costs) return fail(MPPI_E_ARG, "mppi_elites_eval: null argument");
  const mppi_config& c = h->cfg;
  if (B < 1 || B > c.max_batch) return fail(MPPI_E_ARG, "mppi_elites_eval: B out of range [1, max_batch]");
  if (h->elite_n == 0) return fail(MPPI_E_STATE, "mppi_elites_eval: call mppi_set_elites first");
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  MPPI_TRY(stage_costs(h, costs, B));  // through the staging costs, as mppi_lambda_eval
  HIP_TRY(timed(h, kElites, [&] { return enqueue_elite(h, B, h->d_costs, 1); }));  // the evaluation's own slot
  HIP_TRY(hipStreamSynchronize(s));
  return copy_elites(h, B, 1, idx, count, tau, ecost);
}

int mppi_set_elite_keep(mppi_handle* h, int n_keep) {
  if (!h) return fail(MPPI_E_ARG, "mppi_set_elite_keep: null handle");
  const mppi_config& c = h->cfg;
  if (n_keep < 0 || n_keep > c.K) return fail(MPPI_E_ARG, "mppi_set_elite_keep: n_keep must be in [0, K] (0 disables)");
  if (n_keep == h->keep_n) return MPPI_OK;  // no change: captured graphs and the stored set stay
  MPPI_TRY(pop_check(h, "mppi_set_elite_keep", h->iter_n, h->elite_n, n_keep, h->iter_mean));
  HIP_TRY(hipSetDevice(h->device));
  // stale state: the captured graphs hold n_keep (or the feature's absence) in their launches, and the set's rows have
  // n_keep entries; everything in flight finishes first.  A prefetched noise is kept: the injection happens in the
  // solve that consumes it, the key sequence is unchanged
  HIP_TRY(hipStreamSynchronize(h->stream));
  if (n_keep > 0) {  // the set's buffers by its row length, the rest once; all here, none inside a solve
    const size_t mb = (size_t)c.max_batch, nb = 2 * mb, n = (size_t)n_keep;
    const size_t nv = nb * c.nu * c.H * keep_pitch(n_keep) * 4;
    float *nvp = nullptr, *ncost = nullptr;  // (the old set stays until the new one exists)
    int32_t *nidx = nullptr, *nsel = nullptr;
    std::vector<BufReq> reqs{{(void**)&nvp, nv}, {(void**)&ncost, nb * n * 4}, {(void**)&nidx, nb * n * 4},
                             {(void**)&nsel, mb * n * 4}};
    if (!h->d_keep_count) {
      reqs.push_back({(void**)&h->d_keep_count, at_least16(nb * 4)});
      reqs.push_back({(void**)&h->d_keep_steps, at_least16(nb * 4)});
      reqs.push_back({(void**)&h->d_keep_selcount, at_least16(mb * 4)});
      reqs.push_back({(void**)&h->d_keep_tau, at_least16(mb * 4)});
      reqs.push_back({(void**)&h->d_keep_ecost, mb * h->Kp * 4});
      reqs.push_back({(void**)&h->d_keep_U, mb * c.nu * c.H * 4});
    }
    MPPI_TRY(alloc_group("mppi_set_elite_keep", reqs));
    void* old[] = {h->d_keep_v, h->d_keep_cost, h->d_keep_idx, h->d_keep_sel};
    for (void* p : old)
      if (p) (void)hipFree(p);
    h->d_keep_v = nvp;
    h->d_keep_cost = ncost;
    h->d_keep_idx = nidx;
    h->d_keep_sel = nsel;
    // the stored set reads as empty: count = steps = 0 in both slots, v zeroed (cleared ON THE HANDLE'S STREAM and waited
    // for: a memset on the null stream is not ordered against what the non-blocking stream receives next)
    HIP_TRY(hipMemsetAsync(h->d_keep_count, 0, nb * 4, h->stream));
    HIP_TRY(hipMemsetAsync(h->d_keep_steps, 0, nb * 4, h->stream));
    HIP_TRY(hipMemsetAsync(h->d_keep_v, 0, nv, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
  }
  MPPI_TRY(drop_graphs(h, false));
  h->keep_n = n_keep;
  h->keep_B = 0;  // the last set had another row length: none to read until a solve stores or mppi_set_kept writes one
  return MPPI_OK;
}

int mppi_get_elite_keep(mppi_handle* h, int* n_keep) {
  if (!h) return fail(MPPI_E_ARG, "mppi_get_elite_keep: null handle");
  if (n_keep) *n_keep = h->keep_n;
  return MPPI_OK;
}

// slot `slot` of the kept set -> host (the stream is idle); each pointer may be nullptr
static int copy_kept(mppi_handle* h, int B, int slot, float* v, float* kcost, int32_t* idx, int32_t* count,
                     int32_t* steps) {
  const mppi_config& c = h->cfg;
  const size_t ob = (size_t)slot * c.max_batch, n = (size_t)h->keep_n, pitch = (size_t)keep_pitch(h->keep_n);
  const size_t rows = (size_t)B * c.nu * c.H;
  if (v)
    HIP_TRY(hipMemcpy2D(v, n * 4, h->d_keep_v + ob * c.nu * c.H * pitch, pitch * 4, n * 4, rows, hipMemcpyDeviceToHost));
  if (kcost) HIP_TRY(hipMemcpy(kcost, h->d_keep_cost + ob * n, (size_t)B * n * 4, hipMemcpyDeviceToHost));
  if (idx) HIP_TRY(hipMemcpy(idx, h->d_keep_idx + ob * n, (size_t)B * n * 4, hipMemcpyDeviceToHost));
  if (count) HIP_TRY(hipMemcpy(count, h->d_keep_count + ob, (size_t)B * 4, hipMemcpyDeviceToHost));
  if (steps) HIP_TRY(hipMemcpy(steps, h->d_keep_steps + ob, (size_t)B * 4, hipMemcpyDeviceToHost));
  return MPPI_OK;
}

int mppi_get_kept(mppi_handle* h, int B, float* v, float* kcost, int32_t* idx, int32_t* count, int32_t* steps) {
  if (!h) return fail(MPPI_E_ARG, "mppi_get_kept: null handle");
  if (h->keep_B == 0 || h->keep_n == 0)
    return fail(MPPI_E_STATE, "mppi_get_kept: no solve has stored and no mppi_set_kept has written a set under the "
                              "current mppi_set_elite_keep setting");
  if (B < 1 || B > h->keep_B) return fail(MPPI_E_ARG, "mppi_get_kept: B beyond the slots that hold a set");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return copy_kept(h, B, 0, v, kcost, idx, count, steps);
}

// count [B] in 0..n_keep and steps [B] in 0..H (what mppi_set_kept and mppi_keep_inject_eval accept)
static bool kept_sizes_valid(const mppi_handle* h, int B, const int32_t* count, const int32_t* steps) {
  for (int b = 0; b < B; ++b)
    if (count[b] < 0 || count[b] > h->keep_n || steps[b] < 0 || steps[b] > h->cfg.H) return false;
  return true;
}

// host v [B][nu][H][n_keep], count [B], steps [B] -> slot `slot` of the set, on the stream (the caller waits)
static int upload_kept(mppi_handle* h, int B, int slot, const float* v, const int32_t* count, const int32_t* steps) {
  const mppi_config& c = h->cfg;
  const size_t ob = (size_t)slot * c.max_batch, n = (size_t)h->keep_n, pitch = (size_t)keep_pitch(h->keep_n);
  const size_t rows = (size_t)B * c.nu * c.H;
  hipStream_t s = h->stream;
  if (pitch != n) HIP_TRY(hipMemsetAsync(h->d_keep_v + ob * c.nu * c.H * pitch, 0, rows * pitch * 4, s));
  HIP_TRY(hipMemcpy2DAsync(h->d_keep_v + ob * c.nu * c.H * pitch, pitch * 4, v, n * 4, n * 4, rows,
                           hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(h->d_keep_count + ob, count, (size_t)B * 4, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(h->d_keep_steps + ob, steps, (size_t)B * 4, hipMemcpyHostToDevice, s));
  return MPPI_OK;
}

int mppi_set_kept(mppi_handle* h, int B, const float* v, const int32_t* count, const int32_t* steps) {
  if (!h) return fail(MPPI_E_ARG, "mppi_set_kept: null handle");
  const mppi_config& c = h->cfg;
  if (B < 1 || B > c.max_batch) return fail(MPPI_E_ARG, "mppi_set_kept: B out of range [1, max_batch]");
  if (h->keep_n == 0) return fail(MPPI_E_STATE, "mppi_set_kept: call mppi_set_elite_keep first");
  if (v && (!count || !steps)) return fail(MPPI_E_ARG, "mppi_set_kept: count and steps go with v");
  if (v && !kept_sizes_valid(h, B, count, steps))
    return fail(MPPI_E_ARG, "mppi_set_kept: count must be in [0, n_keep] and steps in [0, H]");
  HIP_TRY(hipSetDevice(h->device));
  // data, not a launch argument: ordered on the stream behind every solve enqueued so far (the set they stored is
  // replaced), captured graphs stay -- their first solve injects this set when they replay
  hipStream_t s = h->stream;
  const size_t n = (size_t)h->keep_n, pitch = (size_t)keep_pitch(h->keep_n), rows = (size_t)B * c.nu * c.H;
  if (v) {
    MPPI_TRY(upload_kept(h, B, 0, v, count, steps));
  } else {  // empty slots 0..B
    HIP_TRY(hipMemsetAsync(h->d_keep_count, 0, (size_t)B * 4, s));
    HIP_TRY(hipMemsetAsync(h->d_keep_steps, 0, (size_t)B * 4, s));
    HIP_TRY(hipMemsetAsync(h->d_keep_v, 0, rows * pitch * 4, s));
  }
  // a written set has no costs and no sample indices of a solve: kcost = +inf, idx = -1
  const std::vector<float> inf((size_t)B * n, INFINITY);
  const std::vector<int32_t> none((size_t)B * n, -1);
  HIP_TRY(hipMemcpyAsync(h->d_keep_cost, inf.data(), inf.size() * 4, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(h->d_keep_idx, none.data(), none.size() * 4, hipMemcpyHostToDevice, s));
  HIP_TRY(hipStreamSynchronize(s));  // (the caller's and the local arrays may go)
  if (B > h->keep_B) h->keep_B = B;
  return MPPI_OK;
}

int mppi_keep_store_eval(mppi_handle* h, int B, const float* U, const float* noise, const float* costs, int shift,
                         float* v, float* kcost, int32_t* idx, int32_t* count, int32_t* steps) {
  if (!h || !U || !noise || !costs) return fail(MPPI_E_ARG, "mppi_keep_store_eval: null argument");
  const mppi_config& c = h->cfg;
  if (B < 1 || B > c.max_batch) return fail(MPPI_E_ARG, "mppi_keep_store_eval: B out of range [1, max_batch]");
  if (h->keep_n == 0) return fail(MPPI_E_STATE, "mppi_keep_store_eval: call mppi_set_elite_keep first");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(drop_prefetch(h));  // d_noise may hold the next chained solve's noise: its key is drawn again
  hipStream_t s = h->stream;
  const size_t rows = (size_t)B * c.nu * c.H;
  HIP_TRY(hipMemcpyAsync(h->d_keep_U, U, rows * 4, hipMemcpyHostToDevice, s));
  MPPI_TRY(stage_noise(h, noise, rows));
  MPPI_TRY(stage_costs(h, costs, B));
  // the solve's own kernels (the selection never shared: its scratch is rewritten by every storing solve before it is
  // read) into the evaluation's slot: the handle's stored set is untouched
  HIP_TRY(timed(h, kKeep, [&] {
    return enqueue_keep_store(h, B, h->d_keep_U, h->d_noise, h->d_costs, shift != 0, false, 1);
  }));
  HIP_TRY(hipStreamSynchronize(s));
  return copy_kept(h, B, 1, v, kcost, idx, count, steps);
}

int mppi_keep_inject_eval(mppi_handle* h, int B, const float* U, const float* noise_in, const float* v,
                          const int32_t* count, const int32_t* steps, float* noise_out) {
  if (!h || !U || !noise_in || !v || !count || !steps || !noise_out)
    return fail(MPPI_E_ARG, "mppi_keep_inject_eval: null argument");
  const mppi_config& c = h->cfg;
  if (B < 1 || B > c.max_batch) return fail(MPPI_E_ARG, "mppi_keep_inject_eval: B out of range [1, max_batch]");
  if (h->keep_n == 0) return fail(MPPI_E_STATE, "mppi_keep_inject_eval: call mppi_set_elite_keep first");
  if (!kept_sizes_valid(h, B, count, steps))
    return fail(MPPI_E_ARG, "mppi_keep_inject_eval: count must be in [0, n_keep] and steps in [0, H]");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(drop_prefetch(h));  // d_noise may hold the next chained solve's noise: its key is drawn again
  hipStream_t s = h->stream;
  const size_t K = (size_t)c.K, Kp = (size_t)h->Kp, rows = (size_t)B * c.nu * c.H;
  HIP_TRY(hipMemcpyAsync(h->d_keep_U, U, rows * 4, hipMemcpyHostToDevice, s));
  MPPI_TRY(stage_noise(h, noise_in, rows));
  MPPI_TRY(upload_kept(h, B, 1, v, count, steps));  // the evaluation's slot: the handle's stored set is untouched
  HIP_TRY(timed(h, kKeep, [&] { return launch_keep_inject(keep_args(h, B, h->d_keep_U, h->d_noise, 1), s); }));
  HIP_TRY(hipMemcpy2DAsync(noise_out, K * 4, h->d_noise, Kp * 4, K * 4, rows, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return MPPI_OK;
}

// A population table in effect (mppi_set_population) against the settings a setter is about to make: the one check
// (population.h pop_validate) that mppi_set_population itself runs, so the refusal holds in either order of the calls.
static int pop_check(const mppi_handle* h, const char* who, int n_iter, int n_elite, int n_keep, int add_mean) {
  if (h->pop_n == 0) return MPPI_OK;
  const int e = pop_validate(h->pop_K, h->pop_n, h->cfg.K, n_iter, n_elite, n_keep, add_mean);
  if (e == kPopOk) return MPPI_OK;
  return fail(MPPI_E_ARG, std::string(who) + ": against the mppi_set_population table in effect, " + pop_error_text(e) +
                              " (call mppi_set_population(h, NULL, 0) first)");
}

// The tracking's buffers (mppi_set_iterations, mppi_iter_best_eval): allocated once, never inside a solve.
static int ensure_iter(mppi_handle* h) {
  if (h->d_best_v) return MPPI_OK;
  const mppi_config& c = h->cfg;
  const size_t mb = (size_t)c.max_batch, nb = 2 * mb;
  return alloc_group("mppi_set_iterations", {{(void**)&h->d_best_v, nb * c.nu * c.H * 4},
                                             {(void**)&h->d_best_cost, at_least16(nb * 4)},
                                             {(void**)&h->d_best_k, at_least16(nb * 4)},
                                             {(void**)&h->d_best_iter, at_least16(nb * 4)},
                                             {(void**)&h->d_best_U, mb * c.nu * c.H * 4}});
}

int mppi_set_iterations(mppi_handle* h, int n_iter, int return_best, int add_mean) {
  if (!h) return fail(MPPI_E_ARG, "mppi_set_iterations: null handle");
  if (n_iter < 1 || n_iter > 16) return fail(MPPI_E_ARG, "mppi_set_iterations: n_iter must be in [1, 16]");
  if ((return_best != 0 && return_best != 1) || (add_mean != 0 && add_mean != 1))
    return fail(MPPI_E_ARG, "mppi_set_iterations: return_best and add_mean must be 0 or 1");
  if (n_iter == h->iter_n && return_best == h->iter_best && add_mean == h->iter_mean) return MPPI_OK;  // graphs stay
  MPPI_TRY(pop_check(h, "mppi_set_iterations", n_iter, h->elite_n, h->keep_n, add_mean));
  HIP_TRY(hipSetDevice(h->device));
  // stale state: the captured graphs hold the iteration structure in their launches; everything in flight finishes
  // first.  A prefetched noise is kept: the key sequence does not depend on the setting
  HIP_TRY(hipStreamSynchronize(h->stream));
  if (n_iter > 1 || return_best || add_mean) MPPI_TRY(ensure_iter(h));
  MPPI_TRY(drop_graphs(h, false));
  h->iter_n = n_iter;
  h->iter_best = return_best;
  h->iter_mean = add_mean;
  return MPPI_OK;
}

int mppi_get_iterations(mppi_handle* h, int* n_iter, int* return_best, int* add_mean) {
  if (!h) return fail(MPPI_E_ARG, "mppi_get_iterations: null handle");
  if (n_iter) *n_iter = h->iter_n;
  if (return_best) *return_best = h->iter_best;
  if (add_mean) *add_mean = h->iter_mean;
  return MPPI_OK;
}

int mppi_set_population(mppi_handle* h, const int32_t* K_it, int n) {
  if (!h) return fail(MPPI_E_ARG, "mppi_set_population: null handle");
  if (!K_it && n != 0) return fail(MPPI_E_ARG, "mppi_set_population: NULL (off) goes with n == 0");
  int32_t tab[kPopMaxIter] = {0};
  int tn = 0;
  if (K_it) {
    const int e = pop_validate(K_it, n, h->cfg.K, h->iter_n, h->elite_n, h->keep_n, h->iter_mean);
    if (e != kPopOk) return fail(MPPI_E_ARG, std::string("mppi_set_population: ") + pop_error_text(e));
    if (!pop_is_off(K_it, n, h->cfg.K)) {  // (every entry cfg.K: the feature off, stored as such)
      tn = n;
      std::memcpy(tab, K_it, (size_t)n * sizeof(int32_t));
    }
  }
  if (tn == h->pop_n && std::memcmp(tab, h->pop_K, sizeof(tab)) == 0) return MPPI_OK;  // in effect: graphs, prefetch stay
  HIP_TRY(hipSetDevice(h->device));
  // stale state, as in mppi_set_noise_model: the captured graphs hold every iteration's shape in their launches (a
  // launch still in flight finishes first), and a prefetched noise is dropped (the counter steps back: the key sequence
  // is unchanged).  Nothing is allocated: every buffer was sized for cfg.K and is re-read at the iterations' shapes
  HIP_TRY(drop_prefetch(h));
  MPPI_TRY(drop_graphs(h, true));
  h->pop_n = tn;
  std::memcpy(h->pop_K, tab, sizeof(tab));
  // the [B][K] read-outs of the last solve lie at the old table's last shape: none to read until the next solve
  h->ctrl_B = h->rate_B = h->elite_B = h->ens_B = 0;
  return MPPI_OK;
}

int mppi_get_population(mppi_handle* h, int32_t* K_it, int* n) {
  if (!h) return fail(MPPI_E_ARG, "mppi_get_population: null handle");
  if (K_it)
    for (int i = 0; i < kPopMaxIter; ++i) K_it[i] = i < h->pop_n ? h->pop_K[i] : 0;
  if (n) *n = h->pop_n;
  return MPPI_OK;
}

int mppi_population_icem(int K, int n_iter, double gamma, int k_min, int32_t* K_it) {
  if (!K_it) return fail(MPPI_E_ARG, "mppi_population_icem: null argument");
  if (pop_icem(K, n_iter, gamma, k_min, K_it) != 0)
    return fail(MPPI_E_ARG, "mppi_population_icem: need gamma >= 1, 1 <= k_min <= K and n_iter in [1, 16]");
  return MPPI_OK;
}

const char* mppi_iter_rollout_kernel(mppi_handle* h, int it) {
  if (!h || it < 0 || it >= h->iter_n || !h->iter_kernel[it]) return "";
  return h->iter_kernel[it];
}

// slot `slot` of the stored best -> host (the stream is idle); each pointer may be nullptr
static int copy_best(mppi_handle* h, int B, int slot, float* v, float* cost, int32_t* k, int32_t* iter) {
  const mppi_config& c = h->cfg;
  const size_t ob = (size_t)slot * c.max_batch;
  if (v) HIP_TRY(hipMemcpy(v, h->d_best_v + ob * c.nu * c.H, (size_t)B * c.nu * c.H * 4, hipMemcpyDeviceToHost));
  if (cost) HIP_TRY(hipMemcpy(cost, h->d_best_cost + ob, (size_t)B * 4, hipMemcpyDeviceToHost));
  if (k) HIP_TRY(hipMemcpy(k, h->d_best_k + ob, (size_t)B * 4, hipMemcpyDeviceToHost));
  if (iter) HIP_TRY(hipMemcpy(iter, h->d_best_iter + ob, (size_t)B * 4, hipMemcpyDeviceToHost));
  return MPPI_OK;
}

int mppi_get_best(mppi_handle* h, int B, float* v, float* cost, int32_t* k, int32_t* iter) {
  if (!h) return fail(MPPI_E_ARG, "mppi_get_best: null handle");
  if (h->best_B == 0)
    return fail(MPPI_E_STATE, "mppi_get_best: no solve has tracked a best sample on the handle (mppi_set_iterations)");
  if (B < 1 || B > h->best_B) return fail(MPPI_E_ARG, "mppi_get_best: B beyond the batch of the last tracking solve");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return copy_best(h, B, 0, v, cost, k, iter);
}

int mppi_iter_best_eval(mppi_handle* h, int B, const float* U, const float* noise, const float* costs, int reset, int it,
                        float* v, float* cost, int32_t* k, int32_t* iter) {
  if (!h || !U || !noise || !costs) return fail(MPPI_E_ARG, "mppi_iter_best_eval: null argument");
  const mppi_config& c = h->cfg;
  if (B < 1 || B > c.max_batch) return fail(MPPI_E_ARG, "mppi_iter_best_eval: B out of range [1, max_batch]");
  if (!reset && (!v || !cost || !k || !iter))
    return fail(MPPI_E_ARG, "mppi_iter_best_eval: reset == 0 carries the stored best in (v, cost, k, iter)");
  HIP_TRY(hipSetDevice(h->device));
  MPPI_TRY(ensure_iter(h));
  HIP_TRY(drop_prefetch(h));  // d_noise may hold the next chained solve's noise: its key is drawn again
  hipStream_t s = h->stream;
  const size_t mb = (size_t)c.max_batch, rows = (size_t)B * c.nu * c.H;
  float* bv = h->d_best_v + mb * c.nu * c.H;  // the evaluation's own slot: the handle's stored best is untouched
  HIP_TRY(hipMemcpyAsync(h->d_best_U, U, rows * 4, hipMemcpyHostToDevice, s));
  MPPI_TRY(stage_noise(h, noise, rows));
  MPPI_TRY(stage_costs(h, costs, B));
  if (!reset) {
    HIP_TRY(hipMemcpyAsync(bv, v, rows * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(h->d_best_cost + mb, cost, (size_t)B * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(h->d_best_k + mb, k, (size_t)B * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(h->d_best_iter + mb, iter, (size_t)B * 4, hipMemcpyHostToDevice, s));
  }
  const IterBestArgs ia{B, c.nu, c.H, c.K, h->Kp, reset ? 1 : 0, it, c.ctrl_clamp, h->d_costs, h->d_noise,
                        h->d_best_U, bv, h->d_best_cost + mb, h->d_best_k + mb, h->d_best_iter + mb};
  HIP_TRY(timed(h, kIter, [&] { return launch_iter_best(ia, s); }));
  HIP_TRY(hipStreamSynchronize(s));
  return copy_best(h, B, 1, v, cost, k, iter);
}

int mppi_set_ensemble(mppi_handle* h, int n_members, int mode, float kappa, int env_member) {
  if (!h) return fail(MPPI_E_ARG, "mppi_set_ensemble: null handle");
  if (n_members < 1 || n_members > MPPI_ENS_MAX)
    return fail(MPPI_E_ARG, "mppi_set_ensemble: n_members must be in [1, MPPI_ENS_MAX]");
  if (!ensemble_mode_valid(mode)) return fail(MPPI_E_ARG, "mppi_set_ensemble: mode must be one of MPPI_ENS_*");
  if (!ensemble_kappa_valid(kappa)) return fail(MPPI_E_ARG, "mppi_set_ensemble: kappa must be finite");
  if (env_member < 0 || env_member >= n_members)
    return fail(MPPI_E_ARG, "mppi_set_ensemble: env_member must be in [0, n_members)");
  if (n_members > 1 && n_members > h->ens_loaded())
    return fail(MPPI_E_ARG, "mppi_set_ensemble: n_members beyond the members loaded (mppi_load_dynamics is member 0, "
                            "mppi_load_member the others)");
  if (n_members == h->ens_n && (n_members == 1 || (mode == h->ens_mode && kappa == h->ens_kappa &&
                                                   env_member == h->ens_env))) {
    if (n_members == 1) h->ens_mode = mode, h->ens_kappa = kappa;  // (read by nothing while off)
    return MPPI_OK;  // in effect: graphs and prefetch stay
  }
  HIP_TRY(hipSetDevice(h->device));
  if (n_members > 1 && !h->d_ens_costs) {  // the first enabling call: the members' rows and the spread, zero-filled
    const size_t row = (size_t)h->cfg.max_batch * h->Kp * 4;
    float *mc = nullptr, *sd = nullptr;
    MPPI_TRY(alloc_group("mppi_set_ensemble", {{(void**)&mc, MPPI_ENS_MAX * row}, {(void**)&sd, row}}));
    hipError_t e = hipMemset(mc, 0, MPPI_ENS_MAX * row);
    if (e == hipSuccess) e = hipMemset(sd, 0, row);
    if (e != hipSuccess) {
      (void)hipFree(mc);
      (void)hipFree(sd);
      return fail(MPPI_E_HIP, std::string("mppi_set_ensemble: ") + hipGetErrorString(e));
    }
    h->d_ens_costs = mc;
    h->d_ens_sd = sd;
  }
  // stale state, as in mppi_set_noise_model: the captured graphs hold the members and the rule's settings in their
  // launches (a launch still in flight finishes first), and a prefetched noise is dropped (the counter steps back: the
  // key sequence is unchanged)
  HIP_TRY(drop_prefetch(h));
  MPPI_TRY(drop_graphs(h, true));
  h->ens_n = n_members;
  h->ens_mode = mode;
  h->ens_kappa = kappa;
  h->ens_env = env_member;
  h->ens_B = 0;  // the read-outs describe a solve under the setting in effect: none yet
  return MPPI_OK;
}

int mppi_get_ensemble(mppi_handle* h, int* n_members, int* mode, float* kappa, int* env_member, int* n_loaded) {
  if (!h) return fail(MPPI_E_ARG, "mppi_get_ensemble: null handle");
  if (n_members) *n_members = h->ens_n;
  if (mode) *mode = h->ens_mode;
  if (kappa) *kappa = h->ens_kappa;
  if (env_member) *env_member = h->ens_env;
  if (n_loaded) *n_loaded = h->ens_loaded();
  return MPPI_OK;
}

// [B][K] of a [max_batch][Kp] device row written by the last solve -> host (the stream is idle)
static int copy_ens_row(mppi_handle* h, int B, const float* src, float* dst) {
  const mppi_handle::Shape sh = readout_shape(h, 0);  // (rows of cfg.K, of which the solve's K samples are written)
  HIP_TRY(hipMemcpy2D(dst, (size_t)h->cfg.K * 4, src, (size_t)sh.Kp * 4, (size_t)sh.K * 4, B, hipMemcpyDeviceToHost));
  return MPPI_OK;
}

static int ens_readout_check(mppi_handle* h, const char* who, int B) {
  if (h->ens_B == 0)
    return fail(MPPI_E_STATE, std::string(who) + ": no solve with the ensemble in effect has run on the handle");
  if (B < 1 || B > h->ens_B) return fail(MPPI_E_ARG, std::string(who) + ": B beyond the batch of the last ensemble solve");
  return MPPI_OK;
}

int mppi_get_member_costs(mppi_handle* h, int B, int e, float* costs) {
  if (!h || !costs) return fail(MPPI_E_ARG, "mppi_get_member_costs: null argument");
  MPPI_TRY(ens_readout_check(h, "mppi_get_member_costs", B));
  if (e < 0 || e >= h->ens_n) return fail(MPPI_E_ARG, "mppi_get_member_costs: e must be in [0, n_members)");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return copy_ens_row(h, B, h->d_ens_costs + (size_t)e * h->cfg.max_batch * h->Kp, costs);
}

int mppi_get_ensemble_spread(mppi_handle* h, int B, float* sd) {
  if (!h || !sd) return fail(MPPI_E_ARG, "mppi_get_ensemble_spread: null argument");
  MPPI_TRY(ens_readout_check(h, "mppi_get_ensemble_spread", B));
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return copy_ens_row(h, B, h->d_ens_sd, sd);
}

int mppi_ensemble_eval(mppi_handle* h, int B, int n, int mode, float kappa, const float* member_costs, float* costs,
                       float* sd) {
  if (!h || !member_costs) return fail(MPPI_E_ARG, "mppi_ensemble_eval: null argument");
  const mppi_config& c = h->cfg;
  if (B < 1 || B > c.max_batch) return fail(MPPI_E_ARG, "mppi_ensemble_eval: B out of range [1, max_batch]");
  if (n < 2 || n > MPPI_ENS_MAX) return fail(MPPI_E_ARG, "mppi_ensemble_eval: n must be in [2, MPPI_ENS_MAX]");
  if (!ensemble_mode_valid(mode)) return fail(MPPI_E_ARG, "mppi_ensemble_eval: mode must be one of MPPI_ENS_*");
  if (!ensemble_kappa_valid(kappa)) return fail(MPPI_E_ARG, "mppi_ensemble_eval: kappa must be finite");
  HIP_TRY(hipSetDevice(h->device));
  const size_t K = (size_t)c.K, Kp = (size_t)h->Kp, row = (size_t)c.max_batch * Kp;
  if (!h->d_ens_eval) {  // the evaluation's own members, costs and spread: no buffer of a solve is touched
    float* p = nullptr;
    MPPI_TRY(alloc_group("mppi_ensemble_eval", {{(void**)&p, (MPPI_ENS_MAX + 2) * row * 4}}));
    if (const hipError_t e = hipMemset(p, 0, (MPPI_ENS_MAX + 2) * row * 4); e != hipSuccess) {  // (the pads K..Kp)
      (void)hipFree(p);
      return fail(MPPI_E_HIP, std::string("mppi_ensemble_eval: ") + hipGetErrorString(e));
    }
    h->d_ens_eval = p;
  }
  hipStream_t s = h->stream;
  float* const d_costs = h->d_ens_eval + MPPI_ENS_MAX * row;
  float* const d_sd = d_costs + row;
  for (int e = 0; e < n; ++e)  // member e's [B][K] host rows into its device rows [B][Kp]
    HIP_TRY(hipMemcpy2DAsync(h->d_ens_eval + (size_t)e * row, Kp * 4, member_costs + (size_t)e * B * K, K * 4, K * 4, B,
                             hipMemcpyHostToDevice, s));
  const EnsembleArgs ea{n, mode, kappa, ensemble_rcp(n), (long)((size_t)B * Kp / 4), (long)row, h->d_ens_eval, d_costs, d_sd};
  HIP_TRY(timed(h, kEnsemble, [&] { return launch_ensemble(ea, s); }));
  if (costs) HIP_TRY(hipMemcpy2DAsync(costs, K * 4, d_costs, Kp * 4, K * 4, B, hipMemcpyDeviceToHost, s));
  if (sd) HIP_TRY(hipMemcpy2DAsync(sd, K * 4, d_sd, Kp * 4, K * 4, B, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return MPPI_OK;
}

// slot `slot` of the diagnostics' buffers -> host (the stream is idle)
static int copy_stats(mppi_handle* h, int B, int slot, mppi_solve_stats* stats, float* eps_m2, float* eps_m11) {
  const size_t off = (size_t)slot * h->cfg.max_batch, nu = (size_t)h->cfg.nu;
  if (stats) HIP_TRY(hipMemcpy(stats, h->d_stats + off, (size_t)B * sizeof(mppi_solve_stats), hipMemcpyDeviceToHost));
  if (eps_m2) HIP_TRY(hipMemcpy(eps_m2, h->d_stats_m2 + off * nu, (size_t)B * nu * 4, hipMemcpyDeviceToHost));
  if (eps_m11) HIP_TRY(hipMemcpy(eps_m11, h->d_stats_m11 + off * nu, (size_t)B * nu * 4, hipMemcpyDeviceToHost));
  return MPPI_OK;
}

int mppi_get_stats(mppi_handle* h, int B, int step, mppi_solve_stats* stats, float* eps_m2, float* eps_m11) {
  if (!h) return fail(MPPI_E_ARG, "mppi_get_stats: null handle");
  if (h->stats_n == 0) return fail(MPPI_E_STATE, "mppi_get_stats: no solve with MPPI_FLAG_STATS has run on the handle");
  if (B < 1 || B > h->stats_B) return fail(MPPI_E_ARG, "mppi_get_stats: B beyond the batch of the last flagged solve");
  if (step < 0 || step >= h->stats_n)
    return fail(MPPI_E_ARG, "mppi_get_stats: step beyond the solves of the last flagged solve or graph");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return copy_stats(h, B, step, stats, eps_m2, eps_m11);
}

int mppi_device_stats(mppi_handle* h, void** d_stats, void** d_m2, void** d_m11) {
  if (!h) return fail(MPPI_E_ARG, "mppi_device_stats: null handle");
  HIP_TRY(hipSetDevice(h->device));
  MPPI_TRY(ensure_stats(h, 1));
  if (d_stats) *d_stats = h->d_stats;
  if (d_m2) *d_m2 = h->d_stats_m2;
  if (d_m11) *d_m11 = h->d_stats_m11;
  return MPPI_OK;
}

int mppi_stats_eval(mppi_handle* h, int B, const float* costs, const float* noise, mppi_solve_stats* stats,
                    float* eps_m2, float* eps_m11) {
  if (!h || !costs) return fail(MPPI_E_ARG, "mppi_stats_eval: null argument");
  const mppi_config& c = h->cfg;
  if (B < 1 || B > c.max_batch) return fail(MPPI_E_ARG, "mppi_stats_eval: B out of range [1, max_batch]");
  HIP_TRY(hipSetDevice(h->device));
  MPPI_TRY(ensure_stats(h, 1));
  HIP_TRY(drop_prefetch(h));  // d_noise may hold the next chained solve's noise: its key is drawn again
  hipStream_t s = h->stream;
  MPPI_TRY(stage_costs(h, costs, B));
  if (noise) MPPI_TRY(stage_noise(h, noise, (size_t)B * c.nu * c.H));
  const int slot = h->stats_slots;  // the evaluation's own slot
  HIP_TRY(timed(h, kStats, [&] { return enqueue_stats(h, B, h->d_costs, noise ? h->d_noise : nullptr, slot); }));
  HIP_TRY(hipStreamSynchronize(s));
  return copy_stats(h, B, slot, stats, noise ? eps_m2 : nullptr, noise ? eps_m11 : nullptr);
}

int mppi_get_cross_moments(mppi_handle* h, int B, int step, float* mx) {
  if (!h || !mx) return fail(MPPI_E_ARG, "mppi_get_cross_moments: null argument");
  if (h->cross_n == 0)
    return fail(MPPI_E_STATE, "mppi_get_cross_moments: no solve with MPPI_FLAG_CROSS has run on the handle");
  if (B < 1 || B > h->cross_B)
    return fail(MPPI_E_ARG, "mppi_get_cross_moments: B beyond the batch of the last flagged solve");
  if (step < 0 || step >= h->cross_n)
    return fail(MPPI_E_ARG, "mppi_get_cross_moments: step beyond the solves of the last flagged solve or graph");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipStreamSynchronize(h->stream));
  const size_t nn = (size_t)h->cfg.nu * h->cfg.nu;
  HIP_TRY(hipMemcpy(mx, h->d_cross_mx + (size_t)step * h->cfg.max_batch * nn, (size_t)B * nn * 4,
                    hipMemcpyDeviceToHost));
  return MPPI_OK;
}

int mppi_cross_moments_eval(mppi_handle* h, int B, const float* costs, const float* noise, float* mx) {
  if (!h || !costs || !noise || !mx) return fail(MPPI_E_ARG, "mppi_cross_moments_eval: null argument");
  const mppi_config& c = h->cfg;
  if (B < 1 || B > c.max_batch) return fail(MPPI_E_ARG, "mppi_cross_moments_eval: B out of range [1, max_batch]");
  if (c.nu > kMaxNu) return fail(MPPI_E_UNSUPPORTED, "mppi_cross_moments_eval: needs nu <= 32");
  HIP_TRY(hipSetDevice(h->device));
  MPPI_TRY(ensure_stats(h, 1));
  MPPI_TRY(ensure_cross(h, 1));
  HIP_TRY(drop_prefetch(h));  // d_noise may hold the next chained solve's noise: its key is drawn again
  hipStream_t s = h->stream;
  MPPI_TRY(stage_costs(h, costs, B));
  MPPI_TRY(stage_noise(h, noise, (size_t)B * c.nu * c.H));
  // the evaluations' own slots: the statistics and cross moments of the last solve stay readable
  HIP_TRY(timed(h, kStats, [&] { return enqueue_stats(h, B, h->d_costs, h->d_noise, h->stats_slots); }));
  HIP_TRY(timed(h, kCross, [&] { return enqueue_cross(h, B, h->d_noise, h->cross_slots); }));
  HIP_TRY(hipStreamSynchronize(s));
  const size_t nn = (size_t)c.nu * c.nu;
  HIP_TRY(hipMemcpy(mx, h->d_cross_mx + (size_t)h->cross_slots * c.max_batch * nn, (size_t)B * nn * 4,
                    hipMemcpyDeviceToHost));
  return MPPI_OK;
}

// slot `slot` of the per-step moments -> host (the stream is idle)
static int copy_step_mom(mppi_handle* h, int B, int slot, float* m1, float* m2) {
  const size_t n = (size_t)B * h->cfg.nu * h->cfg.H * 4;
  if (m1) HIP_TRY(hipMemcpy(m1, step_m1(h, slot), n, hipMemcpyDeviceToHost));
  if (m2) HIP_TRY(hipMemcpy(m2, step_m2(h, slot), n, hipMemcpyDeviceToHost));
  return MPPI_OK;
}

int mppi_get_step_moments(mppi_handle* h, int B, int step, float* m1, float* m2) {
  if (!h) return fail(MPPI_E_ARG, "mppi_get_step_moments: null handle");
  if (h->stepm_n == 0)
    return fail(MPPI_E_STATE, "mppi_get_step_moments: no solve with MPPI_FLAG_STEP_MOMENTS has run on the handle");
  if (B < 1 || B > h->stepm_B)
    return fail(MPPI_E_ARG, "mppi_get_step_moments: B beyond the batch of the last flagged solve");
  if (step < 0 || step >= h->stepm_n)
    return fail(MPPI_E_ARG, "mppi_get_step_moments: step beyond the solves of the last flagged solve or graph");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return copy_step_mom(h, B, step, m1, m2);
}

int mppi_step_moments_eval(mppi_handle* h, int B, const float* costs, const float* noise, float* m1, float* m2) {
  if (!h || !costs || !noise) return fail(MPPI_E_ARG, "mppi_step_moments_eval: null argument");
  const mppi_config& c = h->cfg;
  if (B < 1 || B > c.max_batch) return fail(MPPI_E_ARG, "mppi_step_moments_eval: B out of range [1, max_batch]");
  HIP_TRY(hipSetDevice(h->device));
  MPPI_TRY(ensure_stats(h, 1));
  MPPI_TRY(ensure_step_mom(h, 1));
  HIP_TRY(drop_prefetch(h));  // d_noise may hold the next chained solve's noise: its key is drawn again
  hipStream_t s = h->stream;
  MPPI_TRY(stage_costs(h, costs, B));
  MPPI_TRY(stage_noise(h, noise, (size_t)B * c.nu * c.H));
  // the evaluations' own slots: the statistics and per-step moments of the last solve stay readable; never refits
  HIP_TRY(timed(h, kStats, [&] { return enqueue_stats(h, B, h->d_costs, h->d_noise, h->stats_slots); }));
  HIP_TRY(timed(h, kStepMom, [&] { return enqueue_step_mom(h, B, h->d_noise, h->step_slots); }));
  HIP_TRY(hipStreamSynchronize(s));
  return copy_step_mom(h, B, h->step_slots, m1, m2);
}

int mppi_solve(mppi_handle* h, int B, const float* x0, float* U, const float* noise, uint64_t seed, float* costs_out,
               float* u0_out, int flags) {
  mppi_io io;
  std::memset(&io, 0, sizeof(io));
  io.x0 = x0;
  io.U = U;
  io.noise = noise;
  io.costs = costs_out;
  io.u0 = u0_out;
  return mppi_solve_ex(h, B, &io, seed, flags);
}

}  // extern "C"
