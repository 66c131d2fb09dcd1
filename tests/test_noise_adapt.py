"""The device's adaptation rule on the host: csrc/noise_adapt.h through g++ against its numpy float32 restatement
(mppi_hip.stats.adapt_noise_model_f32) and the float64 rule (adapt_noise_model), the NULL-handle paths of the three C
entries, and MPPIModel(adapt_on="device") against a recording engine (no GPU needed)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import PKG, REPO

HARNESS = r"""
#include <stdio.h>
#include <stdlib.h>
#include "noise_adapt.h"
// argv: B nu rate sigma_min sigma_max rho_max rho | sigma_u[nu] | n_finite[B] | m2[B][nu] | m11[B][nu]  (hex floats)
int main(int argc, char** argv) {
  int i = 1;
  const int B = atoi(argv[i++]), nu = atoi(argv[i++]);
  NoiseAdapt a;
  a.rate = strtof(argv[i++], 0);
  a.sigma_min = strtof(argv[i++], 0);
  a.sigma_max = strtof(argv[i++], 0);
  a.rho_max = strtof(argv[i++], 0);
  float rho = strtof(argv[i++], 0), c = -1.0f;
  float s[32], m2[8 * 32], m11[8 * 32];
  int nf[8];
  if (B > 8 || nu > 32 || argc != 8 + nu + B + 2 * B * nu) return 2;
  for (int u = 0; u < nu; ++u) s[u] = strtof(argv[i++], 0);
  for (int b = 0; b < B; ++b) nf[b] = atoi(argv[i++]);
  for (int j = 0; j < B * nu; ++j) m2[j] = strtof(argv[i++], 0);
  for (int j = 0; j < B * nu; ++j) m11[j] = strtof(argv[i++], 0);
  const int moved = noise_adapt_step(a, s, &rho, &c, m2, m11, nf, 1, B, nu);
  printf("%d %a %a\n", moved, rho, c);
  for (int u = 0; u < nu; ++u) printf("%a\n", s[u]);
  return 0;
}
"""


@pytest.fixture(scope="module")
def rule(tmp_path_factory):
    """noise_adapt.h compiled with g++ into a small program; rule(law, moments, settings) runs one step through it."""
    d = tmp_path_factory.mktemp("noise_adapt")
    src, exe = str(d / "h.cpp"), str(d / "h")
    open(src, "w").write(HARNESS)
    r = subprocess.run(["g++", "-O2", "-I", os.path.join(PKG, "csrc"), src, "-o", exe], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.fail(r.stderr)

    def run(sigma_u, rho, m2, m11, rate, lo, hi, rho_max, n_finite=None):
        m2 = np.asarray(m2, np.float32)
        B, nu = m2.shape
        nf = [1] * B if n_finite is None else list(n_finite)
        hx = lambda v: float(np.float32(v)).hex()
        args = [str(B), str(nu), hx(rate), hx(lo), hx(hi), hx(rho_max), hx(rho)] + [hx(v) for v in sigma_u] + \
               [str(int(v)) for v in nf] + [hx(v) for v in m2.ravel()] + \
               [hx(v) for v in np.asarray(m11, np.float32).ravel()]
        out = subprocess.run([exe, *args], capture_output=True, text=True, check=True).stdout.split("\n")
        moved, rho_new, c = out[0].split()
        s = np.array([float.fromhex(v) for v in out[1:1 + nu]], np.float32)
        return int(moved), s, np.float32(float.fromhex(rho_new)), np.float32(float.fromhex(c))

    return run


def _case(rs, B, nu, H1=False):
    """Seeded law and moments of the sizes a solve produces: sigma_u in (0.05, 2), m2 around sigma^2, |m11| <= m2."""
    s = (0.05 + 1.95 * rs.rand(nu)).astype(np.float32)
    m2 = ((s * s)[None] * (0.2 + 1.6 * rs.rand(B, nu))).astype(np.float32)
    m11 = np.zeros_like(m2) if H1 else (m2 * (1.8 * rs.rand(B, nu) - 0.8)).astype(np.float32)
    return s, np.float32(0.9 * rs.rand()), m2, m11


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _check(rule, s, rho, m2, m11, rate, lo, hi, rho_max, n_finite=None):
    """g++ == numpy float32 bit for bit (sigma_u, rho, and c = sqrtf(1 - rho * rho)), and both within the fp32 bound of
    the float64 rule.  Returns the float32 result."""
    from mppi_hip.stats import adapt_noise_model, adapt_noise_model_f32
    B, nu = np.asarray(m2).shape
    moved, s_c, rho_c, c_c = rule(s, rho, m2, m11, rate, lo, hi, rho_max, n_finite)
    s_n, rho_n = adapt_noise_model_f32(s, rho, m2, m11, rate, lo, hi, rho_max, n_finite=n_finite)
    assert s_n.dtype == np.float32 and isinstance(rho_n, np.float32)
    assert np.array_equal(_bits(s_c), _bits(s_n)), (s_c, s_n)
    assert _bits(rho_c) == _bits(rho_n), (rho_c, rho_n)
    if n_finite is not None and 0 in list(n_finite):
        assert moved == 0 and np.array_equal(_bits(s_c), _bits(s)) and _bits(rho_c) == _bits(rho)
        return s_n, rho_n
    assert moved == 1
    assert _bits(c_c) == _bits(np.sqrt(np.float32(1.0) - rho_n * rho_n, dtype=np.float32))
    # float64 rule on the same (float32-valued) inputs.  The bound counts the fp32 roundings of the rule: B - 1 adds and
    # a divide per mean, nu - 1 adds per sum over u, and the handful of products, the fma, the square root and the
    # quotient: (nu + B + 8) 2^-24 relative for sigma.  rho is a blend of rho (<= 1) and the quotient num / den, whose
    # ABSOLUTE error is that figure times sum|m11bar| / sum m2bar when the terms of num cancel, hence the factor; rho
    # itself is below 1, so the figure is taken absolutely.
    s64, rho64 = adapt_noise_model(s.astype(np.float64), float(rho), m2.astype(np.float64), m11.astype(np.float64),
                                   float(np.float32(rate)), float(np.float32(lo)), float(np.float32(hi)),
                                   float(np.float32(rho_max)))
    fig = (nu + B + 8) * 2.0 ** -24
    m2bar, m11bar = m2.astype(np.float64).mean(0), m11.astype(np.float64).mean(0)
    amp = max(1.0, np.abs(m11bar).sum() / m2bar.sum()) if m2bar.sum() > 0 else 1.0
    err_s = float(np.max(np.abs(s_n - s64) / np.maximum(s64, 1e-300)))
    err_r = abs(float(rho_n) - rho64)
    print(f"B={B} nu={nu}: sigma rel err {err_s:.3e} (bound {fig:.3e}), rho err {err_r:.3e} (bound {fig * amp:.3e})")
    np.testing.assert_allclose(s_n, s64, rtol=fig, atol=0.0)
    assert err_r <= fig * amp
    return s_n, rho_n


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("nu", [1, 3, 21, 32])
def test_header_equals_numpy_f32_and_stays_within_the_fp32_bound_of_the_f64_rule(rule, B, nu):
    """Bit for bit: x86-64's sqrtss / divss and glibc's fmaf are correctly rounded, as numpy's float32 sqrt and divide
    and the exact-rational fma of adapt_noise_model_f32 are (0 ulp found)."""
    rs = np.random.RandomState(100 * B + nu)
    for i in range(6):
        s, rho, m2, m11 = _case(rs, B, nu)
        rate = [0.3, 1.0, 0.05, 0.5, 0.7, 2.0 ** -10][i]
        s_n, rho_n = _check(rule, s, rho, m2, m11, rate, 1e-3, 10.0, 0.95)
        assert not np.array_equal(s_n, s) and rho_n != rho  # (no clip binds: the law moved)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("nu", [1, 3, 21, 32])
def test_every_clip_binds_exactly(rule, B, nu):
    rs = np.random.RandomState(7 + 100 * B + nu)
    s, rho, m2, m11 = _case(rs, B, nu)
    s_n, _ = _check(rule, s, rho, m2, m11, 0.5, 5.0, 10.0, 0.95)  # sigma_min above every sigma
    assert np.all(s_n == np.float32(5.0))
    s_n, _ = _check(rule, s, rho, m2, m11, 0.5, 1e-3, 0.01, 0.95)  # sigma_max below every sigma
    assert np.all(s_n == np.float32(0.01))
    _, rho_n = _check(rule, s, np.float32(0.8), m2, 0.9 * m2, 1.0, 1e-3, 10.0, 0.1)  # rho_hat = 0.9 > rho_max
    assert rho_n == np.float32(0.1)
    _, rho_n = _check(rule, s, np.float32(0.8), m2, -0.5 * m2, 1.0, 1e-3, 10.0, 0.95)  # rho_hat < 0 -> 0
    assert rho_n == np.float32(0.0)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("nu", [1, 3, 21, 32])
def test_zero_denominator_h1_moments_frozen_actuator_and_nonfinite_batch(rule, B, nu):
    rs = np.random.RandomState(13 + 100 * B + nu)
    s, rho, m2, m11 = _case(rs, B, nu)
    z = np.zeros_like(m2)
    s_n, rho_n = _check(rule, s, rho, z, z, 0.25, 1e-3, 10.0, 0.95)  # den = 0: rho_hat = 0
    assert rho_n == np.float32(np.float32(0.75) * rho)
    s, rho, m2, m11 = _case(rs, B, nu, H1=True)  # H = 1: m11 = 0
    _, rho_n = _check(rule, s, rho, m2, m11, 0.25, 1e-3, 10.0, 0.95)
    assert rho_n == np.float32(np.float32(0.75) * rho)
    s0 = s.copy()
    s0[0] = 0.0  # a frozen actuator with no noise moment: clipped up to sigma_min, kept at 0 by sigma_min = 0
    m2[:, 0] = 0.0
    s_n, _ = _check(rule, s0, rho, m2, m11, 0.5, 1e-3, 10.0, 0.95)
    assert s_n[0] == np.float32(1e-3)
    s_n, _ = _check(rule, s0, rho, m2, m11, 0.5, 0.0, 10.0, 0.95)
    assert s_n[0] == 0.0
    nf = [5] * B
    nf[B - 1] = 0  # one solve of the batch without a finite cost: the law is unchanged
    s_n, rho_n = _check(rule, s, rho, m2, m11, 0.5, 1e-3, 10.0, 0.95, n_finite=nf)
    assert np.array_equal(s_n, s) and rho_n == rho


def test_nonfinite_moments_leave_their_entry(rule):
    s = np.array([0.5, 0.7], np.float32)
    m2 = np.array([[np.inf, 0.3]], np.float32)
    m11 = np.array([[0.1, 0.1]], np.float32)
    from mppi_hip.stats import adapt_noise_model_f32
    moved, s_c, rho_c, _ = rule(s, 0.4, m2, m11, 0.5, 1e-3, 10.0, 0.95)
    s_n, rho_n = adapt_noise_model_f32(s, 0.4, m2, m11, 0.5, 1e-3, 10.0, 0.95)
    assert moved == 1 and np.array_equal(_bits(s_c), _bits(s_n)) and _bits(rho_c) == _bits(rho_n)
    assert s_n[0] == np.float32(0.5) and s_n[1] != np.float32(0.7)  # var = inf: entry 0 stays
    m11[0, 0] = np.nan  # rho_hat = nan: rho stays
    _, s_c, rho_c, _ = rule(s, 0.4, np.array([[0.2, 0.3]], np.float32), m11, 0.5, 1e-3, 10.0, 0.95)
    _, rho_n = adapt_noise_model_f32(s, 0.4, [[0.2, 0.3]], m11, 0.5, 1e-3, 10.0, 0.95)
    assert rho_c == rho_n == np.float32(0.4)


# ---- C ABI without a device

def test_header_declares_and_the_binding_binds_the_three_entries():
    from mppi_hip import _lib as L
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "mppi.h")).read(), flags=re.S)
    assert re.search(r"#define\s+MPPI_ABI_VERSION\s+4\b", src)
    protos = {
        "mppi_set_noise_adapt": r"int mppi_set_noise_adapt\(mppi_handle\* h, float rate, float sigma_min, "
                                r"float sigma_max, float rho_max\);",
        "mppi_get_noise_adapt": r"int mppi_get_noise_adapt\(mppi_handle\* h, float\* rate, float\* sigma_min, "
                                r"float\* sigma_max, float\* rho_max\);",
        "mppi_get_noise_law": r"int mppi_get_noise_law\(mppi_handle\* h, int step, float\* sigma_u, float\* rho\);",
    }
    lib = L.load()
    for name, pat in protos.items():
        assert re.search(pat, src), name
        assert name in L.EXPORTED and hasattr(lib, name)
    jl = open(os.path.join(PKG, "julia", "MPPIHip.jl")).read()
    for name in protos:
        assert ":" + name in jl, name


def test_abi_null_handle_is_an_argument_error():
    from mppi_hip import _lib as L
    lib = L.load()
    f = [ctypes.c_float() for _ in range(4)]
    s = (ctypes.c_float * 4)()
    assert lib.mppi_set_noise_adapt(None, 0.3, 1e-3, 10.0, 0.95) == L.MPPI_E_ARG
    assert b"mppi_set_noise_adapt" in lib.mppi_last_error()
    assert lib.mppi_set_noise_adapt(None, 0.0, 0.0, 0.0, 0.0) == L.MPPI_E_ARG
    assert lib.mppi_get_noise_adapt(None, *(ctypes.byref(x) for x in f)) == L.MPPI_E_ARG
    assert b"mppi_get_noise_adapt" in lib.mppi_last_error()
    assert lib.mppi_get_noise_adapt(None, None, None, None, None) == L.MPPI_E_ARG
    assert lib.mppi_get_noise_law(None, 0, s, ctypes.byref(f[0])) == L.MPPI_E_ARG
    assert b"mppi_get_noise_law" in lib.mppi_last_error()
    assert lib.mppi_get_noise_law(None, 0, None, None) == L.MPPI_E_ARG


# ---- MPPIModel(adapt_on="device") against a recording engine

class _Recorder:
    """Stands in for Engine: records every call, answers solve / noise_model with fixed values."""

    def __init__(self, config, device=0):
        self.config = config
        self.calls = []
        self.law = (np.full(config.nu, 0.25, np.float32), 0.5, True)

    def _rec(self, name, *a, **kw):
        self.calls.append((name, a, kw))
        return self

    def load_dynamics(self, *a, **kw):
        return self._rec("load_dynamics")

    def set_cost(self, *a, **kw):
        return self._rec("set_cost")

    def set_noise_model(self, *a, **kw):
        return self._rec("set_noise_model", *a, **kw)

    def set_noise_adapt(self, *a, **kw):
        return self._rec("set_noise_adapt", *a, **kw)

    def noise_model(self):
        self._rec("noise_model")
        return self.law

    def solve(self, x0, U, **kw):
        from mppi_hip.engine import SolveResult
        self._rec("solve", **kw)
        c = self.config
        return SolveResult(U=np.asarray(U, np.float32), costs=np.zeros(c.K, np.float32),
                           weights=np.zeros(c.K, np.float32), u0=np.zeros(c.nu, np.float32), status=0, stats=None)

    def close(self):
        pass


def test_model_adapting_on_the_device_sets_no_law_and_requests_no_stats_per_step(monkeypatch):
    import mppi_hip.controller as C
    monkeypatch.setattr(C, "Engine", _Recorder)
    m = C.MPPIModel("cartpole_py", K=64, adapt_noise=0.3, adapt_on="device", noise_rho=0.4,
                    adapt_limits=(0.01, 5.0, 0.9))
    names = [c[0] for c in m.engine.calls]
    assert names.count("set_noise_model") == 1 and names.index("set_noise_model") < names.index("set_noise_adapt")
    assert [c for c in m.engine.calls if c[0] == "set_noise_adapt"][0][1] == (0.3, 0.01, 5.0, 0.9)
    n0 = len(m.engine.calls)
    data = C.SimData(qpos=np.zeros(2), qvel=np.zeros(2), ctrl=np.zeros(1))
    for _ in range(3):
        C.mppi_step(m, data)
        C.mppi_controller(m, data)
    steps = m.engine.calls[n0:]
    assert [c[0] for c in steps] == ["solve"] * 6
    assert all("stats" not in c[2] for c in steps)
    # the law is the engine's
    assert np.array_equal(m.noise_sigma, np.full(1, 0.25)) and m.noise_rho == 0.5
    # ... and the host mode is what it was: stats requested, the law set per step
    h = C.MPPIModel("cartpole_py", K=64, adapt_noise=0.3, noise_rho=0.4)
    assert "set_noise_adapt" not in [c[0] for c in h.engine.calls]
    assert h.noise_sigma is None and h.noise_rho == 0.4
    with pytest.raises(ValueError):
        C.MPPIModel("cartpole_py", K=64, adapt_on="gpu")
