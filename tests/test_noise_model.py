"""The sampling law (per-actuator sigma, AR(1) along the horizon) on the host: mppi_hip.noise.ar1_filter, the
recursion header csrc/noise_model.h through g++, and the NULL-handle paths of the C ABI (no GPU needed)."""
import ctypes
import os
import subprocess
import tempfile
from fractions import Fraction

import numpy as np
import pytest

from conftest import PKG
from philox_ref import device_noise


def _loop(z, rho, sigma_u):
    """The law as an explicit triple loop over (u, t, k) of one [nu, H, K] array (float64)."""
    nu, H, K = z.shape
    c = np.sqrt(1.0 - rho * rho)
    out = np.empty_like(z)
    for u in range(nu):
        for k in range(K):
            e = 0.0
            for t in range(H):
                e = z[u, t, k] if t == 0 else rho * e + c * z[u, t, k]
                out[u, t, k] = sigma_u[u] * e
    return out


def test_ar1_filter_matches_explicit_loops():
    from mppi_hip.noise import ar1_filter
    rs = np.random.RandomState(3)
    z = rs.randn(2, 3, 7, 5)  # [B, nu, H, K]
    sig = np.array([0.5, 2.0, 0.0])
    out = ar1_filter(z, 0.8, sig)
    assert out.dtype == np.float64 and out.shape == z.shape
    for b in range(2):
        np.testing.assert_allclose(out[b], _loop(z[b], 0.8, sig), rtol=1e-14, atol=1e-15)
    assert np.all(out[:, 2] == 0.0)  # sigma 0 freezes an actuator


def test_ar1_filter_rho_zero_is_plain_scaling():
    from mppi_hip.noise import ar1_filter
    z = np.random.RandomState(4).randn(3, 6, 8)
    sig = np.array([0.3, 1.0, 1.7])
    assert np.array_equal(ar1_filter(z, 0.0, sig), sig[:, None, None] * z)
    assert np.array_equal(ar1_filter(z, 0.0), z)
    assert np.array_equal(ar1_filter(z, 0.0, 0.75), 0.75 * z)  # a scalar is one sigma for every actuator


def test_ar1_filter_sigma_broadcasts_along_u_only():
    from mppi_hip.noise import ar1_filter
    z = np.random.RandomState(5).randn(3, 3, 3)  # nu == H == K: a wrong axis would still broadcast
    sig = np.array([1.0, 10.0, 100.0])
    out = ar1_filter(z, 0.5, sig)
    unit = ar1_filter(z, 0.5)
    for u in range(3):
        assert np.array_equal(out[u], sig[u] * unit[u])
    with pytest.raises(ValueError):
        ar1_filter(z, 0.5, [1.0, 2.0])
    with pytest.raises(ValueError):
        ar1_filter(z, 1.0, sig)
    with pytest.raises(ValueError):
        ar1_filter(z, 0.5, [1.0, -1.0, 1.0])


def test_ar1_statistics_of_the_device_normals():
    """std and lag-1 autocorrelation over N = 64 * 4096 = 262,144 values per actuator: a standard error near
    1 / sqrt(N) = 0.002, so the 0.02 bars are ten of them."""
    from mppi_hip.noise import ar1_filter
    rho, sig = 0.8, np.array([0.5, 2.0])
    z = device_noise(0x1234, 1, 2, 64, 4096, 1.0)
    eps = ar1_filter(z, rho, sig)[0]
    for u in range(2):
        std = eps[u].std()
        e = eps[u] / sig[u]
        lag1 = np.mean(e[1:] * e[:-1]) / np.sqrt(np.mean(e[1:] ** 2) * np.mean(e[:-1] ** 2))
        print(f"u={u}: std {std:.5f} (sigma {sig[u]}), lag-1 autocorrelation {lag1:.5f} (rho {rho})")
        assert abs(std - sig[u]) < 0.02 * sig[u]
        assert abs(lag1 - rho) < 0.02


# ---- the recursion header, through g++

def _round_f32(v: Fraction) -> np.float32:
    """The exact rational v rounded once to fp32 (nearest, ties to even)."""
    f = np.float32(float(v))
    cands = [f, np.nextafter(f, np.float32(np.inf)), np.nextafter(f, np.float32(-np.inf))]
    best = None
    for c in cands:
        d = abs(Fraction(float(c)) - v)
        even = (int(np.float32(c).view(np.uint32)) & 1) == 0
        if best is None or d < best[0] or (d == best[0] and even and not best[2]):
            best = (d, np.float32(c), even)
    return best[1]


def _fma32(a, b, c) -> np.float32:
    return _round_f32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def _ar1_row_f32(z, rho):
    """numpy fp32 restatement of csrc/noise_model.h: c = sqrtf(1 - rho*rho); e[t] = fmaf(rho, e[t-1], c * z[t])."""
    rho = np.float32(rho)
    c = np.sqrt(np.float32(1.0) - rho * rho, dtype=np.float32)
    z = np.asarray(z, np.float32)
    e = np.empty_like(z)
    e[0] = z[0]
    for t in range(1, len(z)):
        e[t] = _fma32(rho, e[t - 1], np.float32(c * z[t]))
    return c, e


HARNESS = r"""
#include <stdio.h>
#include <stdlib.h>
#include "noise_model.h"
int main(int argc, char** argv) {
  const float rho = strtof(argv[1], 0);
  const int H = argc - 2;
  float z[64], e[64], s[64];
  for (int t = 0; t < H; ++t) z[t] = strtof(argv[2 + t], 0);
  const float c = ar1_innovation_scale(rho);
  ar1_row(rho, c, z, e, H);
  float prev = 0.0f;  // ... and step by step, as the kernel walks it
  for (int t = 0; t < H; ++t) s[t] = prev = t == 0 ? z[0] : ar1_step(rho, c, prev, z[t]);
  printf("%a\n", c);
  for (int t = 0; t < H; ++t) printf("%a %a\n", e[t], s[t]);
  return 0;
}
"""


@pytest.mark.parametrize("rho", [0.0, 0.5, 0.9, 0.999])
def test_recursion_header_matches_fp32_restatement_bitwise(rho):
    z = device_noise(0xABCDEF, 1, 1, 48, 4, 1.0)[0, 0, :, 1].astype(np.float32)
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "h.cpp")
        open(src, "w").write(HARNESS)
        exe = os.path.join(d, "h")
        r = subprocess.run(["g++", "-O2", "-I", os.path.join(PKG, "csrc"), src, "-o", exe], capture_output=True,
                           text=True)
        if r.returncode != 0:
            pytest.fail(r.stderr)
        args = [float(np.float32(rho)).hex()] + [float(v).hex() for v in z]
        out = subprocess.run([exe, *args], capture_output=True, text=True, check=True).stdout.split("\n")
    c_ref, e_ref = _ar1_row_f32(z, rho)
    print("c", out[0], float(c_ref).hex())
    assert float.fromhex(out[0]) == float(c_ref)
    for t in range(len(z)):
        row, step = (float.fromhex(v) for v in out[1 + t].split())
        print(t, out[1 + t], float(e_ref[t]).hex())
        assert row == step == float(e_ref[t]), t
    if rho == 0.0:  # white noise, value for value
        assert np.array_equal(e_ref, z)


# ---- C ABI without a device

def test_abi_null_handle_is_an_argument_error():
    from mppi_hip import _lib as L
    lib = L.load()
    s = (ctypes.c_float * 4)(1, 1, 1, 1)
    rho, active = ctypes.c_float(), ctypes.c_int()
    assert lib.mppi_set_noise_model(None, None, 0.0) == L.MPPI_E_ARG
    assert b"mppi_set_noise_model" in lib.mppi_last_error()
    assert lib.mppi_set_noise_model(None, s, 0.5) == L.MPPI_E_ARG
    assert lib.mppi_get_noise_model(None, s, ctypes.byref(rho), ctypes.byref(active)) == L.MPPI_E_ARG
    assert b"mppi_get_noise_model" in lib.mppi_last_error()
    assert lib.mppi_get_noise_model(None, None, None, None) == L.MPPI_E_ARG
