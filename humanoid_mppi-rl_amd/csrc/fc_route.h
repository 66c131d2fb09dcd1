// Which kernel runs an fc-stack rollout (CrossAttention / MLP surrogates): ONE pure function of the solve's shape, the
// packed image's offsets, the engine's probe outcomes, the device's CU count and the routing knobs.  No HIP call, no
// getenv, no static in fc_route: it is evaluated on the CPU by tests/test_fc_route.py against recorded routes
// (tests/golden/fc_routes.json).  The launchers (launch_fc_route, kernels_fc.hip) only launch what it names.
#pragma once
#include <cstdlib>

#include "mppi_internal.h"

namespace mppi {

// One value per launchable kernel family.
enum class FcKernel : int {
  generic,     // fc_generic_kernel (kernels_fc_generic.hip): any other fc-stack shape
  msplit,      // fc_rollout_kernel (fc_rollout.h): bf16, or the streamed fp32 path (FcRoute::form = its MPPI_PREC_*)
  msplit_f32,  // fc_rollout_kernel_f32: exact fp32, fragments in registers
  msplit_x3,   // fc_rollout_kernel_x3: split bf16, one tile per wave
  msplit_x3w,  // fc_rollout_kernel_x3w: split bf16, two tiles per wave
  wave,        // fc_wave_kernel (kernels_fc_wave.hip): bf16 CA per wave, NS = 1 / 2
  wave32,      // fc_wave32_kernel: its 32x32x16 variant
  wave_mlp,    // fc_wave_mlp_kernel: bf16 MLP per wave, NS = 1 / 2
  x3_wave32,   // fc_wave32_x3_kernel (kernels_fc_x3.hip): split CA per wave, one wave per SIMD
  x3p,         // fc_wave32_x3p_kernel (kernels_fc_x3p.hip): two waves per SIMD
  x3d,         // fc_rollout_kernel_x3d (kernels_fc_x3d.hip): split M-split CA, two groups per block
  x3h,         // fc_rollout_kernel_x3h / _x3hw (kernels_fc_x3h.hip): its fp16 form, NS = 1 / 2 / 4
  x3m,         // fc_wave_mlp_x3_kernel (kernels_fc_x3m.hip): split MLP per wave
  x3mp,        // fc_wave32_mlp_x3_kernel (kernels_fc_x3mp.hip): 32 samples per wave
#ifdef MPPI_AB_ARMS  // the A/B-only library (csrc/ab/)
  pipe,        // fc_pipe_kernel
  wide,        // fc_rollout_kernel_wide
#endif
};

// form: the split CA's numeric form where it applies (x3_form below: 0 = fp16 with the one-product last layer, 1 = fp16,
// 2 = bf16 with the two-product layer 1, 3 = bf16 three products); msplit: the instantiation's precision.  ns: sample
// tiles per wave where the family has several.
struct FcRoute {
  FcKernel kernel;
  int form;
  int ns;
};

// Waves per block of the per-wave kernels whose batch thresholds count wave-tiles per CU (their *Lay::WAVES).
constexpr int kWaveX3Waves = 4;       // fc_wave32_x3_kernel: one wave per SIMD
constexpr int kWaveMlpX3Waves = 8;    // fc_wave_mlp_x3_kernel
constexpr int kWaveMlp32X3Waves = 8;  // fc_wave32_mlp_x3_kernel
// bf16 per-wave kernels (fc_wave_kernel, fc_wave_mlp_kernel): 16-sample tiles per CU from which NS = 1 / NS = 2 run,
// from a same-box sweep over config #4 batches
constexpr int kWaveTilesNs1 = 6, kWaveTilesNs2 = 12;
// CUs the A/B-only wide kernel's halved grid must still cover
constexpr int kWideMinGroups = 2 * 256;

// The split CA's two-product layer 1 and fp16 form are CHECKED properties of the loaded net (mppi_api.hip x3_probe),
// kept only within kX3ProbeTol and never beyond kX3TwoTermMaxH steps (the error grows with the horizon; fc_common.h)
constexpr int kX3TwoTermMaxH = 64;
constexpr float kX3ProbeTol = 7.5e-5f;  // 3/4 of the fp32-accurate bar (costs rtol 1e-4 against the fp32 oracle);
                                        // model_cross.pth on config #4's logged states: 4.95e-5 (CPU emulation)

#ifndef X3H_B0MMA  // fc_rollout_kernel_x3h: layer 0's bias through the MFMA chain (needs FcArgs::wmf16_0b_off)
#define X3H_B0MMA 1
#endif

// Every routing knob (environment variables; A/B arms and tests).  Defaults = unset.
struct FcKnobs {
  int fc_wave = -1;         // MPPI_FC_WAVE: bf16 per-wave kernels: 0 never, 1 / 2 always with NS = 1 / 2, 3 the 32x32x16 one
  int x3_wave = 1;          // MPPI_X3_WAVE: split CA: 0 always the M-split kernels, 2 always the per-wave kernels
  int x3_pair = -1;         // MPPI_X3_PAIR: two waves per SIMD (x3p): 0 never, 1 always
  bool x3d = true;          // MPPI_X3D=0: never fc_rollout_kernel_x3d (keeps fc_rollout_kernel_x3w)
  bool x3h = true;          // MPPI_X3H=0: never fc_rollout_kernel_x3h (x3d keeps the fp16 form)
  int x3h_ns = 1;           // MPPI_X3H_NS=2/4: x3h with that many tiles per wave, one block per CU (A/B arms)
  int x3m = -1;             // MPPI_X3M: split per-wave MLP: 0 never, 1 always (when the image carries it)
  int x3m32 = -1;           // MPPI_X3M32: the same at 32 samples per wave
  int x3_tiles = 2;         // MPPI_X3_TILES=1/2: split M-split sample tiles per wave
  bool f32_stream = false;  // MPPI_F32_STREAM=1: the streamed fp32 kernel (A/B; read once per process)
  int fc_wide = 0;          // MPPI_FC_WIDE=1: bf16 with two tiles per wave (MPPI_AB_ARMS only; read once per process)
  bool fc_pipe = false;     // MPPI_FC_PIPE=1: the layer-pipelined CA kernel (MPPI_AB_ARMS only)
  int x3_l1_terms = 0;      // MPPI_X3_L1_TERMS=2/3: forces the products on the split CA's layer 1, no probe
  int x3_f16 = 0;           // MPPI_X3_F16=0/1: forces the fp16 form off (-1) / on (1), no probe
  bool x3_f16_l2 = false;   // MPPI_X3_F16_L2=1: opts into the fp16 form's one-product last layer
};

// The only place that reads these variables.  Per launch (tests flip the knobs between solves in one process), but for
// MPPI_F32_STREAM and MPPI_FC_WIDE, which are read once per process.
inline FcKnobs fc_knobs_from_env() {
  auto env = [](const char* name) { return std::getenv(name); };
  auto is = [](const char* e, char c) { return e && e[0] == c; };
  FcKnobs k;
  if (const char* e = env("MPPI_FC_WAVE")) k.fc_wave = std::atoi(e);
  const char* e = env("MPPI_X3_WAVE");
  k.x3_wave = is(e, '0') ? 0 : (is(e, '2') ? 2 : 1);
  e = env("MPPI_X3_PAIR");
  k.x3_pair = is(e, '0') ? 0 : (is(e, '1') ? 1 : -1);
  k.x3d = !is(env("MPPI_X3D"), '0');
  k.x3h = !is(env("MPPI_X3H"), '0');
  if ((e = env("MPPI_X3H_NS"))) k.x3h_ns = std::atoi(e);
  if (k.x3h_ns != 1 && k.x3h_ns != 2 && k.x3h_ns != 4) k.x3h_ns = 1;
  e = env("MPPI_X3M");
  k.x3m = is(e, '0') ? 0 : (is(e, '1') ? 1 : -1);
  e = env("MPPI_X3M32");
  k.x3m32 = is(e, '0') ? 0 : (is(e, '1') ? 1 : -1);
  if ((e = env("MPPI_X3_TILES"))) k.x3_tiles = std::atoi(e);
  static const bool f32_stream = is(env("MPPI_F32_STREAM"), '1');
  k.f32_stream = f32_stream;
#ifdef MPPI_AB_ARMS
  static const int wide = is(env("MPPI_FC_WIDE"), '1') ? 1 : 0;
  k.fc_wide = wide;
  if ((e = env("MPPI_FC_PIPE"))) k.fc_pipe = std::atoi(e) == 1;
#endif
  e = env("MPPI_X3_L1_TERMS");
  k.x3_l1_terms = is(e, '2') ? 2 : (is(e, '3') ? 3 : 0);
  e = env("MPPI_X3_F16");
  k.x3_f16 = is(e, '1') ? 1 : (is(e, '0') ? -1 : 0);
  k.x3_f16_l2 = is(env("MPPI_X3_F16_L2"), '1');
  return k;
}

// ------------------------------------------------------------------------------------------------ the split CA's form
// (what each form computes, and the measurements behind it: fc_common.h)

// products on layer 1; decided = FcNet::x3_l1 (the probe: 0 not probed, 2 within kX3ProbeTol, 3 not)
inline int x3_l1_terms(int H, int decided, const FcKnobs& k) {
  if (k.x3_l1_terms) return k.x3_l1_terms;
  return H <= kX3TwoTermMaxH && decided == 2 ? 2 : 3;
}
// the fp16 form; decided = FcNet::x3_f16 (0 not probed, 1 within kX3ProbeTol, -1 not), img_off = the kernel's fp16 image
inline bool x3_f16_on(int H, int decided, int img_off, const FcKnobs& k) {
  if (img_off < 0) return false;
  if (k.x3_f16) return k.x3_f16 > 0;
  return H <= kX3TwoTermMaxH && decided >= 1;
}
// ... with the last layer as one fp16 product: opt-in only, the probe does not pick it
inline bool x3_f16_l2x1(int decided, const FcKnobs& k) { return k.x3_f16_l2 || decided == 2; }
// 0 = fp16 with the one-product last layer, 1 = fp16, 2 = bf16 with the two-product layer 1, 3 = bf16 three products
// (the kernels' L1T template argument)
inline int x3_form(int H, int l1_decided, int f16_decided, int f16_img, const FcKnobs& k) {
  if (x3_f16_on(H, f16_decided, f16_img, k)) return x3_f16_l2x1(f16_decided, k) ? 0 : 1;
  return x3_l1_terms(H, l1_decided, k);
}

// fc_rollout_kernel_x3h's tiles per wave: MPPI_X3H_NS, halved until a block's tiles belong to one solve
inline int x3h_tiles(int Kp, const FcKnobs& k) {
  int ns = k.x3h_ns;
  while (ns > 1 && (Kp >> 4) % ns != 0) ns >>= 1;
  return ns;
}

// ------------------------------------------------------------------------------------------------ the route

// Whether kernel `kn` can run this shape on this image at all (whole wave-tiles, the image parts it reads, the slots
// its operands use): what gates it in fc_route, whatever the batch and the knobs.
inline bool fc_route_can_run(FcKernel kn, const SolveArgs& a, const FcArgs& fa) {
  const bool tiles32 = a.Kp >= 32 && a.Kp % 32 == 0;  // a wave owns 32 samples of one solve
  const bool humanoid_nu = a.nu >= 20 && a.nu <= 22;
  const bool mlp_slots = a.nx <= kMlpBiasSlotHi && a.nu <= 32;
  switch (kn) {
    // (the env-step launch, Kp = 16, always takes the M-split kernel, also when MPPI_FC_WAVE forces these)
    case FcKernel::wave: return fa.lds_bytes == 0 && a.nu <= 24 && fa.g_off >= 0 && fa.ln_n == 256 && tiles32;
    case FcKernel::wave32: return fc_route_can_run(FcKernel::wave, a, fa) && fa.w32_off >= 0 && humanoid_nu;
    case FcKernel::wave_mlp: return fa.wave && fa.lds_bytes == 0 && mlp_slots && tiles32;
    case FcKernel::x3_wave32:
    case FcKernel::x3p: return fa.w32x3_off >= 0 && fa.ln_n == 256 && tiles32 && humanoid_nu;
    case FcKernel::x3d: return fa.w_off[1] >= 0 && fa.ln_n == 256 && a.Kp % 64 == 0;
    case FcKernel::x3h:
      return MPPI_X3_F16_L0 && fa.w_off[1] >= 0 && fa.ln_n == 256 && a.Kp % 16 == 0 && fa.wmf16_0_off >= 0 &&
             !(X3H_B0MMA && fa.wmf16_0b_off < 0) && fa.wmf16_off >= 0;
    case FcKernel::x3m: return fa.wmx3_off >= 0 && a.Kp >= 16 && a.Kp % 16 == 0 && mlp_slots;
    case FcKernel::x3mp: return fa.wm32x3_off >= 0 && tiles32 && mlp_slots;
    default: return true;
  }
}

// The M-split kernels (fc_rollout.h), which take every fc-stack shape of their arch.
inline FcRoute fc_route_msplit(int arch, int precision, const SolveArgs& a, int x3_l1, const FcKnobs& k) {
  const int tiles = a.Kp >> 4;
  if (precision == MPPI_PREC_BF16X3) {  // (the MLP keeps three products: fc_common.h)
    const int form = arch == kArchCA && x3_l1_terms(a.H, x3_l1, k) == 2 ? 2 : 3;
    return {k.x3_tiles == 2 && tiles % 2 == 0 ? FcKernel::msplit_x3w : FcKernel::msplit_x3, form, 1};
  }
  if (precision == MPPI_PREC_FP32) return {k.f32_stream ? FcKernel::msplit : FcKernel::msplit_f32, MPPI_PREC_FP32, 1};
#ifdef MPPI_AB_ARMS
  if (k.fc_wide && tiles % 2 == 0 && a.B * tiles >= kWideMinGroups) return {FcKernel::wide, MPPI_PREC_BF16, 2};
#endif
  return {FcKernel::msplit, MPPI_PREC_BF16, 1};
}

// arch / precision: FcNet's; a: the solve's shape (B, Kp, H, nx, nu); fa: the image; x3_l1 / x3_f16: FcNet's probe
// outcomes; cus: the device's CU count.  The fp16 form (form 0 / 1) runs on x3p and x3h, which the engine's probe both
// checks on the loaded net, and on x3_wave32, which it does not (tests/test_gpu_split_offprobe.py does).
inline FcRoute fc_route(int arch, int precision, const SolveArgs& a, const FcArgs& fa, int x3_l1, int x3_f16, int cus,
                        const FcKnobs& k) {
  if (arch == kArchGeneric) return {FcKernel::generic, precision, 1};
  const int tiles = a.B * (a.Kp >> 4);  // 16-sample tiles
  const int wts32 = a.B * (a.Kp / 32);  // 32-sample wave-tiles
  // the bf16 per-wave kernels' tiles per wave by batch size (0: the M-split kernel, which spreads a tile over 4 SIMDs)
  const int wave_ns = k.fc_wave == 1 || k.fc_wave == 2 ? k.fc_wave
                      : k.fc_wave == 0                 ? 0
                      : tiles >= kWaveTilesNs2 * cus   ? 2
                      : tiles >= kWaveTilesNs1 * cus   ? 1
                                                       : 0;
  if (arch == kArchCA) {
#ifdef MPPI_AB_ARMS
    if (precision == MPPI_PREC_BF16 && fa.lds_bytes == 0 && k.fc_pipe) return {FcKernel::pipe, MPPI_PREC_BF16, 1};
#endif
    if (precision == MPPI_PREC_BF16X3) {
      // the per-wave kernels from 4 wave-tiles per CU (one per SIMD).  BOUNDARY: x3_wave32 takes wts32 >= 4 cus, but
      // x3p only wts32 > 4 cus, so at EXACTLY 4 wave-tiles per CU (the 32-solve shard of config #4 on 256 CUs) the
      // form -- the fp16 one included -- runs on x3_wave32, a kernel the probe does not run (ADVICE.md, round 6,
      // second item).  Its fp16 form is held to the fp32 oracle at the full horizon, on logged states and on states
      // no probe saw, and to x3p within 8e-5, by tests/test_gpu_split_offprobe.py
      // (test_wave32_fp16_form_at_full_horizon, test_fp16_form_holds_off_probe[x3_wave32-*]).  Kept as it is
      // (tests/test_fc_route.py pins it); moving it is a behaviour change.
      if (fc_route_can_run(FcKernel::x3_wave32, a, fa) &&
          (k.x3_wave == 2 || (k.x3_wave == 1 && wts32 >= kWaveX3Waves * cus))) {
        const bool pair = k.x3_pair >= 0 ? k.x3_pair == 1 : wts32 > kWaveX3Waves * cus;
        return {pair ? FcKernel::x3p : FcKernel::x3_wave32, x3_form(a.H, x3_l1, x3_f16, fa.w32f16_off, k), 1};
      }
      // below that the M-split kernels: the fp16 form on x3h, the two-product bf16 layer 1 (or the fp16 form with
      // MPPI_X3H=0) on x3d, three products on the plain M-split kernels
      const bool f16 = x3_f16_on(a.H, x3_f16, fa.wmf16_off, k);
      if (fc_route_can_run(FcKernel::x3d, a, fa) && (x3_l1_terms(a.H, x3_l1, k) == 2 || f16) && k.x3d) {
        const int form = x3_form(a.H, x3_l1, x3_f16, fa.wmf16_off, k);
        if (fc_route_can_run(FcKernel::x3h, a, fa) && f16 && k.x3h) return {FcKernel::x3h, form, x3h_tiles(a.Kp, k)};
        return {FcKernel::x3d, form, 1};
      }
    }
    if (precision == MPPI_PREC_BF16 && fc_route_can_run(FcKernel::wave, a, fa)) {
      const bool w32 = fc_route_can_run(FcKernel::wave32, a, fa);
      const int ns = k.fc_wave == 3 ? 2 : wave_ns;
      if (ns == 2 && w32 && k.fc_wave != 2) return {FcKernel::wave32, 3, 2};  // the 32x32x16 variant where it applies
      if (ns) return {FcKernel::wave, 3, ns};
    }
    return fc_route_msplit(arch, precision, a, x3_l1, k);
  }
  // kArchMLP
  if (precision == MPPI_PREC_BF16 && fc_route_can_run(FcKernel::wave_mlp, a, fa) && wave_ns)
    return {FcKernel::wave_mlp, 3, wave_ns};
  if (precision == MPPI_PREC_BF16X3 && fc_route_can_run(FcKernel::x3mp, a, fa) &&
      (k.x3m32 >= 0 ? k.x3m32 == 1 : wts32 >= kWaveMlp32X3Waves * cus))
    return {FcKernel::x3mp, 3, 1};
  if (precision == MPPI_PREC_BF16X3 && fc_route_can_run(FcKernel::x3m, a, fa) &&
      (k.x3m >= 0 ? k.x3m == 1 : tiles >= kWaveMlpX3Waves * cus))
    return {FcKernel::x3m, 3, 1};
  return fc_route_msplit(arch, precision, a, x3_l1, k);
}

// The name mppi_rollout_kernel reports: the single table.
inline const char* fc_route_name(const FcRoute& r) {
  const int f = r.form & 3;
  switch (r.kernel) {
    case FcKernel::generic: return "fc_generic_kernel";
    case FcKernel::msplit: return r.form == MPPI_PREC_FP32 ? "fc_rollout_kernel<fp32>" : "fc_rollout_kernel";
    case FcKernel::msplit_f32: return "fc_rollout_kernel_f32";
    case FcKernel::msplit_x3: return r.form == 2 ? "fc_rollout_kernel_x3<l1=2>" : "fc_rollout_kernel_x3<l1=3>";
    case FcKernel::msplit_x3w: return r.form == 2 ? "fc_rollout_kernel_x3w<l1=2>" : "fc_rollout_kernel_x3w<l1=3>";
    case FcKernel::wave: return r.ns == 1 ? "fc_wave_kernel<ns=1>" : "fc_wave_kernel<ns=2>";
    case FcKernel::wave32: return "fc_wave32_kernel";
    case FcKernel::wave_mlp: return r.ns == 1 ? "fc_wave_mlp_kernel<ns=1>" : "fc_wave_mlp_kernel<ns=2>";
    case FcKernel::x3_wave32: {
      static const char* const n[4] = {
          MPPI_X3_F16_L0 ? "fc_wave32_x3_kernel<f16,l2=1>" : "fc_wave32_x3_kernel<l1=f16,l2=1>",
          MPPI_X3_F16_L0 ? "fc_wave32_x3_kernel<f16>" : "fc_wave32_x3_kernel<l1=f16>", "fc_wave32_x3_kernel<l1=2>",
          "fc_wave32_x3_kernel<l1=3>"};
      return n[f];
    }
    case FcKernel::x3p: {
      static const char* const n[4] = {
          MPPI_X3_F16_L0 ? "fc_wave32_x3p_kernel<f16,l2=1>" : "fc_wave32_x3p_kernel<l1=f16,l2=1>",
          MPPI_X3_F16_L0 ? "fc_wave32_x3p_kernel<f16>" : "fc_wave32_x3p_kernel<l1=f16>", "fc_wave32_x3p_kernel<l1=2>",
          "fc_wave32_x3p_kernel<l1=3>"};
      return n[f];
    }
    case FcKernel::x3d: {  // (no three-product form: launch_fc_x3d refuses it)
      static const char* const n[4] = {
          MPPI_X3_F16_L0 ? "fc_rollout_kernel_x3d<f16,l2=1>" : "fc_rollout_kernel_x3d<l1=f16,l2=1>",
          MPPI_X3_F16_L0 ? "fc_rollout_kernel_x3d<f16>" : "fc_rollout_kernel_x3d<l1=f16>", "fc_rollout_kernel_x3d<l1=2>",
          "fc_rollout_kernel_x3d<l1=3>"};
      return n[f];
    }
    case FcKernel::x3h: {  // (the fp16 forms only)
      static const char* const n[2][3] = {
          {"fc_rollout_kernel_x3h<f16>", "fc_rollout_kernel_x3hw<f16,ns=2>", "fc_rollout_kernel_x3hw<f16,ns=4>"},
          {"fc_rollout_kernel_x3h<f16,l2=1>", "fc_rollout_kernel_x3hw<f16,l2=1,ns=2>",
           "fc_rollout_kernel_x3hw<f16,l2=1,ns=4>"}};
      return n[r.form == 0][r.ns == 1 ? 0 : (r.ns == 2 ? 1 : 2)];
    }
    case FcKernel::x3m: return "fc_wave_mlp_x3_kernel";
    case FcKernel::x3mp: return "fc_wave32_mlp_x3_kernel";
#ifdef MPPI_AB_ARMS
    case FcKernel::pipe: return "fc_pipe_kernel";
    case FcKernel::wide: return "fc_rollout_kernel_wide";
#endif
  }
  return "";
}

}  // namespace mppi
