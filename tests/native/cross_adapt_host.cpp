// The weighted cross moments (csrc/cross_moments.h) and the adapted covariance (csrc/noise_cov_adapt.h) on the host,
// through g++: the statements the device kernels run, for tests/test_cross_moments.py and tests/test_noise_cov_adapt.py
// (bitwise against the numpy restatements) and, built with -fsanitize=address,undefined, as a memory check of both
// headers at the smallest and the largest nu.
//   cross  B nu H Kp w.f32 noise.f32                 ->  mx [B][nu][nu], one matrix row per line (hex floats)
//   adapt  B nu rate smin smax S.f32 mx.f32 nf.i32   ->  "moved" | "unchanged" | "rejected", then S, L, Sinv [nu][nu]
//                                                        (one row per line) and sigma_u (one line) as they stand
//   factor nu S.f32                                  ->  "ok" + L, Sinv, sigma_u by BOTH cov_factor (noise_cov.h) and
//                                                        the adaptation's element functions, or "refused"; exit 3 if
//                                                        the two disagree in a bit or in the verdict
//   self   nu                                        ->  every mode on generated data (the sanitizer run)
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>  // (built as host-only HIP: the headers' host + device qualifiers)
#endif
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string_view>
#include <vector>

#include "cross_moments.h"
#include "noise_cov.h"
#include "noise_cov_adapt.h"

static bool read_f32(const char* path, std::vector<float>& v) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  const bool ok = fread(v.data(), sizeof(float), v.size(), f) == v.size();
  fclose(f);
  return ok;
}

static void print_rows(const float* m, int rows, int cols) {
  for (int r = 0; r < rows; ++r)
    for (int c = 0; c < cols; ++c) printf("%a%c", m[(size_t)r * cols + c], c + 1 < cols ? ' ' : '\n');
}

// the adaptation's factor alone: its step with rate-free inputs (S2 = S): the element functions on S itself
static bool factor_by_elements(const float* S, int nu, float* L, float* Sinv, float* sig) {
  std::vector<double> Ld((size_t)nu * nu, 0.0), Wd((size_t)nu * nu, 0.0);
  for (int v = 0; v < nu; ++v)
    for (int u = v; u < nu; ++u) {
      const double x = nca_chol_chain(Ld.data() + (size_t)u * nu, Ld.data() + (size_t)v * nu, v, S[u * nu + v]);
      if (u == v) {
        if (!nca_pivot_ok(x)) return false;
        Ld[(size_t)v * nu + v] = sqrt(x);
      } else {
        Ld[(size_t)u * nu + v] = x / Ld[(size_t)v * nu + v];
      }
    }
  for (int c = 0; c < nu; ++c)
    for (int r = c; r < nu; ++r) Wd[(size_t)r * nu + c] = nca_winv_elem(Ld.data(), Wd.data(), nu, r, c);
  for (int u = 0; u < nu; ++u)
    for (int v = 0; v <= u; ++v) {
      const double x = nca_sinv_elem(Wd.data(), nu, nu, u, v);
      if (!nca_sinv_ok(x)) return false;
      Sinv[u * nu + v] = Sinv[v * nu + u] = (float)x;
    }
  for (int u = 0; u < nu; ++u) {
    for (int v = 0; v < nu; ++v) L[u * nu + v] = v <= u ? (float)Ld[(size_t)u * nu + v] : 0.0f;
    sig[u] = nca_sigma(S[u * nu + u]);
  }
  return true;
}

static int run_cross(int B, int nu, int H, int Kp, const float* w, const float* noise) {
  int nwc, L, nseg;
  moment_cells(H, Kp, &nwc, &L, &nseg);
  std::vector<float> mx((size_t)B * nu * nu), part((size_t)nwc * nseg);
  cross_moments_host(w, noise, B, nu, H, Kp, mx.data(), part.data());
  print_rows(mx.data(), B * nu, nu);
  return 0;
}

static int run_adapt(int B, int nu, const NoiseCovAdapt& a, std::vector<float>& S, const float* mx, const int* nf) {
  const size_t nn = (size_t)nu * nu;
  std::vector<float> L(nn), Sinv(nn), sig(nu);
  std::vector<double> scratch(3 * nn);
  if (!cov_factor(S.data(), nu, L.data(), Sinv.data(), sig.data(), scratch.data(), scratch.data() + nn)) return 2;
  const int rc = noise_cov_adapt_step(a, S.data(), L.data(), Sinv.data(), sig.data(), mx, nf, 1, B, nu, scratch.data());
  printf("%s\n", rc == 1 ? "moved" : (rc == 0 ? "unchanged" : "rejected"));
  print_rows(S.data(), nu, nu);
  print_rows(L.data(), nu, nu);
  print_rows(Sinv.data(), nu, nu);
  print_rows(sig.data(), 1, nu);
  return 0;
}

static int run_factor(int nu, const float* S) {
  const size_t nn = (size_t)nu * nu;
  std::vector<float> L(nn), Sinv(nn), sig(nu), L2(nn), Sinv2(nn), sig2(nu);
  std::vector<double> scratch(3 * nn);
  const bool a = cov_factor(S, nu, L.data(), Sinv.data(), sig.data(), scratch.data(), scratch.data() + nn);
  bool sym = true;  // (cov_factor also refuses what the adaptation never forms: a non-finite or asymmetric matrix)
  for (int u = 0; u < nu; ++u)
    for (int v = 0; v < nu; ++v) sym = sym && isfinite(S[u * nu + v]) && S[u * nu + v] == S[v * nu + u];
  const bool b = sym && factor_by_elements(S, nu, L2.data(), Sinv2.data(), sig2.data());
  if (a != b) return 3;
  if (!a) {
    printf("refused\n");
    return 0;
  }
  if (memcmp(L.data(), L2.data(), nn * 4) || memcmp(Sinv.data(), Sinv2.data(), nn * 4) ||
      memcmp(sig.data(), sig2.data(), (size_t)nu * 4))
    return 3;
  printf("ok\n");
  print_rows(L.data(), nu, nu);
  print_rows(Sinv.data(), nu, nu);
  print_rows(sig.data(), 1, nu);
  return 0;
}

static int run_self(int nu) {
  const int B = 2, H = 33, K = 1030, Kp = (K + 63) / 64 * 64;
  uint32_t r = 12345u + (uint32_t)nu;
  auto rnd = [&]() {
    r = r * 1664525u + 1013904223u;
    return (float)(r >> 8) * (1.0f / 16777216.0f) - 0.5f;
  };
  std::vector<float> w((size_t)B * Kp, 0.0f), noise((size_t)B * nu * H * Kp, 0.0f);
  for (int b = 0; b < B; ++b)
    for (int k = 0; k < K; ++k) w[(size_t)b * Kp + k] = 1.0f / K;
  for (size_t i = 0; i < noise.size(); ++i)
    if ((int)(i % Kp) < K) noise[i] = rnd();
  if (run_cross(B, nu, H, Kp, w.data(), noise.data())) return 1;
  int nwc, L, nseg;
  moment_cells(H, Kp, &nwc, &L, &nseg);
  std::vector<float> mx((size_t)B * nu * nu), part((size_t)nwc * nseg);
  cross_moments_host(w.data(), noise.data(), B, nu, H, Kp, mx.data(), part.data());
  std::vector<float> S((size_t)nu * nu, 0.0f);
  for (int u = 0; u < nu; ++u) S[(size_t)u * nu + u] = 0.25f + 0.01f * u;
  if (run_factor(nu, S.data())) return 1;
  const int nf[2] = {K, K};
  for (float rate : {0.3f, 1.0f}) {
    std::vector<float> S0 = S;
    if (run_adapt(B, nu, NoiseCovAdapt{rate, 0.28f, 0.3f}, S0, mx.data(), nf)) return 1;
  }
  const int dead[2] = {K, 0};
  std::vector<float> S0 = S;
  if (run_adapt(B, nu, NoiseCovAdapt{1.0f, 1e-3f, 10.0f}, S0, mx.data(), dead)) return 1;
  std::vector<float> zero((size_t)B * nu * nu, 0.0f);  // all-zero moments at rate 1: rejected
  S0 = S;
  return run_adapt(B, nu, NoiseCovAdapt{1.0f, 1e-3f, 10.0f}, S0, zero.data(), nf);
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const std::string_view mode = argv[1];
  if (mode == "self" && argc == 3) {
    const int nu = atoi(argv[2]);
    return nu >= 1 && nu <= 32 ? run_self(nu) : 2;
  }
  if (mode == "cross" && argc == 8) {
    const int B = atoi(argv[2]), nu = atoi(argv[3]), H = atoi(argv[4]), Kp = atoi(argv[5]);
    if (B < 1 || nu < 1 || nu > 32 || H < 1 || Kp < 4 || Kp % 4) return 2;
    std::vector<float> w((size_t)B * Kp), noise((size_t)B * nu * H * Kp);
    if (!read_f32(argv[6], w) || !read_f32(argv[7], noise)) return 2;
    return run_cross(B, nu, H, Kp, w.data(), noise.data());
  }
  if (mode == "adapt" && argc == 10) {
    const int B = atoi(argv[2]), nu = atoi(argv[3]);
    if (B < 1 || nu < 1 || nu > 32) return 2;
    const NoiseCovAdapt a{strtof(argv[4], 0), strtof(argv[5], 0), strtof(argv[6], 0)};
    std::vector<float> S((size_t)nu * nu), mx((size_t)B * nu * nu), nff(B);
    if (!read_f32(argv[7], S) || !read_f32(argv[8], mx) || !read_f32(argv[9], nff)) return 2;
    std::vector<int> nf(B);
    memcpy(nf.data(), nff.data(), (size_t)B * 4);  // (int32 bit patterns travel in the float reader)
    return run_adapt(B, nu, a, S, mx.data(), nf.data());
  }
  if (mode == "factor" && argc == 4) {
    const int nu = atoi(argv[2]);
    if (nu < 1 || nu > 32) return 2;
    std::vector<float> S((size_t)nu * nu);
    if (!read_f32(argv[3], S)) return 2;
    return run_factor(nu, S.data());
  }
  return 2;
}
