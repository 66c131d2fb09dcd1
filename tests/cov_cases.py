"""Cases shared by tests/test_noise_cov.py (host) and tests/test_gpu_noise_cov.py (device): the smallest shapes at which
the cross-actuator covariance (csrc/noise_cov.h, noise_cov_kernel) can go wrong."""
import numpy as np

K, B = 130, 2            # K: no multiple of 4 (pad lanes K..Kp = 192 exist); B: more than one block per launch
HS = (1, 7)              # one step (no recursion, no tridiagonal P); odd
RHOS = (0.0, 0.9)
NUS = (1, 3, 21, 32)     # the degenerate triangle; off-diagonals on every row; config #4's width; the limit (kMaxNu)


def scales(nu):
    """per-actuator standard deviations (float64)"""
    if nu <= 3:
        return np.array([0.7, 0.2, 1.3][:nu])
    return 0.2 + 0.05 * np.arange(nu)


def sigma_of(nu):
    """Sigma[u][v] = s_u s_v 0.6^|u-v| rounded to float32: symmetric bit for bit by construction (the product is
    formed once per unordered pair), positive definite (condition numbers 97 / 204 / 474 at nu = 3 / 21 / 32)."""
    s = scales(nu)
    u = np.arange(nu)
    d = np.abs(u[:, None] - u[None, :])
    lo = np.tril(s[:, None] * s[None, :] * 0.6 ** d)
    S = (lo + np.tril(lo, -1).T).astype(np.float32)
    assert np.array_equal(S, S.T)
    return S


def bits(a):
    """float32 array -> its bit patterns"""
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# the control-cost coefficients under the law on the host: csrc/control_cost.h through g++ (the device test compares
# ctrl_lin_kernel with it bit for bit)
LIN_HARNESS = r"""
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "control_cost.h"
// argv: nu H gamma rho Sinv.f32 U.f32  ->  lin [nu][H], one row per line (hex floats)
int main(int argc, char** argv) {
  if (argc != 7) return 2;
  const int nu = atoi(argv[1]), H = atoi(argv[2]);
  const float gamma = strtof(argv[3], 0), rho = strtof(argv[4], 0);
  std::vector<float> Sinv((size_t)nu * nu), U((size_t)nu * H);
  FILE* f = fopen(argv[5], "rb");
  if (!f || fread(Sinv.data(), 4, Sinv.size(), f) != Sinv.size()) return 2;
  fclose(f);
  f = fopen(argv[6], "rb");
  if (!f || fread(U.data(), 4, U.size(), f) != U.size()) return 2;
  fclose(f);
  for (int u = 0; u < nu; ++u)
    for (int t = 0; t < H; ++t)
      printf("%a%c", ctrl_lin_cov_entry(gamma, rho, Sinv.data() + (size_t)u * nu, nu, U.data(), t, H),
             t + 1 < H ? ' ' : '\n');
  return 0;
}
"""


def build_lin_host(d, csrc):
    """LIN_HARNESS built with g++ in directory d (a pathlib.Path) -> lin_host(Sinv [nu, nu], U [B, nu, H], gamma, rho)
    -> lin [B, nu, H] float32"""
    import subprocess
    src, exe = d / "lin.cpp", d / "lin"
    src.write_text(LIN_HARNESS)
    r = subprocess.run(["g++", "-O2", "-I", str(csrc), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def lin_host(Sinv, U, gamma, rho):
        U = np.ascontiguousarray(U, np.float32)
        nb, nu, H = U.shape
        np.ascontiguousarray(Sinv, np.float32).tofile(d / "Sinv.f32")
        out = np.empty_like(U)
        for b in range(nb):
            U[b].tofile(d / "U.f32")
            r = subprocess.run([str(exe), str(nu), str(H), float(np.float32(gamma)).hex(), float(np.float32(rho)).hex(),
                                str(d / "Sinv.f32"), str(d / "U.f32")], capture_output=True, text=True, check=True)
            out[b] = np.array([[float.fromhex(x) for x in ln.split()] for ln in r.stdout.strip().splitlines()])
        return out
    return lin_host
