"""Horizon-basis sampling noise on the host: mppi_hip.noise.basis_filter / colored_basis, the header csrc/noise_basis.h
through g++ (bitwise), and the NULL-handle paths of the C ABI (no GPU needed)."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

from basis_cases import BIG, GRID, TAIL, bits, table
from conftest import PKG
from philox_ref import device_noise

U24 = 2.0 ** -24  # the relative size of one rounding to fp32


def _tables(H, R):
    """the tables of one shape: random normals and, where R allows it, the coloured basis of beta = 1"""
    from mppi_hip.noise import colored_basis
    out = [table(H, R)]
    if R == H or R % 2 == 1:
        out.append(colored_basis(H, 1.0, R))
    return out


# ---- 1. the header, through g++

HARNESS = r"""
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "noise_basis.h"
// argv: H R sigma, then z[0..R) and M [H][R] on stdin as hex floats   ->   the row
int main(int argc, char** argv) {
  if (argc != 4) return 2;
  const int H = atoi(argv[1]), R = atoi(argv[2]);
  const float sigma = strtof(argv[3], 0);
  if (!basis_law_valid(H, R) || R > kMaxBasis) return 2;
  std::vector<float> z(R), M((size_t)H * R), eps(H);
  char tok[64];
  for (int r = 0; r < R; ++r) {
    if (scanf("%63s", tok) != 1) return 3;
    z[r] = strtof(tok, 0);
  }
  for (size_t i = 0; i < M.size(); ++i) {
    if (scanf("%63s", tok) != 1) return 3;
    M[i] = strtof(tok, 0);
  }
  if (!basis_table_finite(M.data(), H, R)) return 4;
  basis_row(sigma, z.data(), R, M.data(), eps.data(), H);
  for (int t = 0; t < H; ++t) printf("%a\n", eps[t]);
  return 0;
}
"""


@pytest.fixture(scope="module")
def harness():
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "b.cpp")
        with open(src, "w") as f:
            f.write(HARNESS)
        exe = os.path.join(d, "b")
        r = subprocess.run(["g++", "-O2", "-I", os.path.join(PKG, "csrc"), src, "-o", exe], capture_output=True,
                           text=True)
        if r.returncode != 0:
            pytest.fail(r.stderr)
        yield exe


def _run(harness, H, R, sigma, z, M):
    text = " ".join(float(v).hex() for v in list(z[:R]) + list(np.asarray(M, np.float32).ravel()))
    return subprocess.run([harness, str(H), str(R), float(sigma).hex()], input=text, capture_output=True, text=True)


@pytest.mark.parametrize("H,R", GRID + list(BIG) + [TAIL])
def test_header_matches_basis_filter_bitwise(harness, H, R):
    from mppi_hip.noise import basis_filter
    sigma = np.float32(0.7)
    z = device_noise(0xBA5150 + 256 * H + R, 1, 1, H, 4, 1.0)[0, 0, :, 1].astype(np.float32)  # [H]
    for M in _tables(H, R):
        out = _run(harness, H, R, sigma, z, M)
        assert out.returncode == 0, out.stderr
        got = np.array([float.fromhex(v) for v in out.stdout.split()], np.float32)
        ref = basis_filter(z.reshape(1, H, 1), M, sigma)[0, :, 0]
        assert ref.dtype == np.float32 and got.shape == ref.shape
        assert np.array_equal(bits(got), bits(ref)), (got, ref)


def test_header_refuses_bad_laws(harness):
    z = np.ones(8, np.float32)
    assert _run(harness, 7, 0, 1.0, z, np.zeros((7, 0))).returncode == 2
    assert _run(harness, 7, 8, 1.0, z, np.zeros((7, 8))).returncode == 2
    bad = np.ones((7, 2), np.float32)
    bad[3, 1] = np.inf
    assert _run(harness, 7, 2, 1.0, z, bad).returncode == 4
    bad[3, 1] = np.nan
    assert _run(harness, 7, 2, 1.0, z, bad).returncode == 4


# ---- 2. identities of the filter

@pytest.mark.parametrize("H,R", GRID)
def test_basis_filter_identities(H, R):
    from mppi_hip.noise import basis_filter
    z = np.random.RandomState(H * 16 + R).randn(2, 3, H, 5).astype(np.float32)
    sig = np.float32([0.7, 0.2, 1.3])
    M = table(H, R)
    out = basis_filter(z, M, sig)
    assert out.dtype == np.float32 and out.shape == z.shape
    zz = z.copy()
    zz[..., R:, :] = np.nan  # only the first R rows are read
    assert np.array_equal(bits(basis_filter(zz, M, sig)), bits(out))
    # the chain against float64: R roundings in the chain and one of the scale, 2^-24 each relative to sum |M z| (and
    # one more for the terms of second order)
    ref = sig[:, None, None].astype(np.float64) * np.einsum("tr,...rk->...tk", M.astype(np.float64),
                                                            z[..., :R, :].astype(np.float64))
    mag = sig[:, None, None].astype(np.float64) * np.einsum("tr,...rk->...tk", np.abs(M).astype(np.float64),
                                                            np.abs(z[..., :R, :]).astype(np.float64))
    assert np.all(np.abs(out - ref) <= (R + 2) * U24 * mag)
    if R == H:  # M = I: sigma * z, bitwise
        assert np.array_equal(bits(basis_filter(z, np.eye(H, dtype=np.float32), sig)), bits(sig[:, None, None] * z))
        assert np.array_equal(bits(basis_filter(z, np.eye(H, dtype=np.float32))), bits(z))
    for bad in (np.zeros((H + 1, 1)), np.zeros((H, H + 1)), np.zeros((H, 0)), np.zeros(H)):
        with pytest.raises(ValueError):
            basis_filter(z, bad)
    with pytest.raises(ValueError):
        basis_filter(z, M, np.ones(2))


@pytest.mark.parametrize("order", (0, 1))
@pytest.mark.parametrize("H,P", GRID)
def test_the_densified_knot_table_is_the_knot_law(H, P, order):
    """rho = 0: a knot table of order 0 or 1 written out as a dense [H, P] matrix (duplicate taps add to the same
    column, zero elsewhere) gives knot_filter's values.  (Order 3 is not claimed: its clamped ends repeat an index.)"""
    from mppi_hip.noise import basis_filter, knot_filter, knot_table
    idx, w = knot_table(H, P, order)
    M = np.zeros((H, P), np.float32)
    for t in range(H):
        for i in range(4):
            M[t, idx[t, i]] += w[t, i]
    z = np.random.RandomState(H * 16 + P).randn(2, 3, H, 5).astype(np.float32)
    sig = np.float32([0.7, 0.2, 1.3])
    assert np.array_equal(basis_filter(z, M, sig), knot_filter(z, P, order, 0.0, sig))


# ---- 3. the coloured basis

@pytest.mark.parametrize("beta", (0.0, 1.0, 2.0))
@pytest.mark.parametrize("H", (1, 7, 8, 9, 64, 128))
def test_colored_basis_in_fp32_has_unit_rows(H, beta):
    """one rounding of relative size 2^-24 per entry and Cauchy-Schwarz on unit rows: the bounds of 4 * 2^-24"""
    from mppi_hip.noise import colored_basis
    M = colored_basis(H, beta)
    assert M.shape == (H, H) and M.dtype == np.float32 and np.all(np.isfinite(M))
    assert np.array_equal(bits(M), bits(colored_basis(H, beta, dtype=np.float64).astype(np.float32)))
    G = M.astype(np.float64) @ M.astype(np.float64).T
    err = float(np.abs(np.diag(G) - 1.0).max())
    print(f"H {H} beta {beta}: max |row norm^2 - 1| = {err:.3e}")
    assert err <= 4 * U24
    if beta == 0.0:
        err = float(np.abs(G - np.eye(H)).max())
        print(f"H {H}: max |M M^T - I| = {err:.3e}")
        assert err <= 4 * U24
    if H == 1:
        assert np.array_equal(M, np.ones((1, 1), np.float32))


@pytest.mark.parametrize("beta", (0.0, 1.0, 2.0))
@pytest.mark.parametrize("H", (8, 9, 64))
def test_colored_basis_in_float64_has_the_power_law_spectrum(H, beta):
    from mppi_hip.noise import colored_basis
    M = colored_basis(H, beta, dtype=np.float64)
    assert M.dtype == np.float64
    G = M @ M.T
    first = G[0]
    for t in range(H):  # circulant
        np.testing.assert_allclose(G[t], np.roll(first, t), rtol=0, atol=1e-12)
    lam = np.fft.fft(first)
    assert np.abs(lam.imag).max() <= 1e-12 * H
    lam = lam.real
    np.testing.assert_allclose(lam[0], lam[1], rtol=1e-9)
    j = np.arange(1, H // 2 + 1)
    np.testing.assert_allclose(lam[j] / lam[1], j.astype(np.float64) ** -beta, rtol=1e-9)


def test_colored_basis_truncation():
    from mppi_hip.noise import colored_basis
    M = colored_basis(9, 1.0, 5)
    assert M.shape == (9, 5) and M.dtype == np.float32
    assert np.linalg.matrix_rank(M.astype(np.float64)) == 5
    assert np.abs((M.astype(np.float64) ** 2).sum(axis=1) - 1.0).max() <= 4 * U24
    full = colored_basis(9, 1.0, dtype=np.float64)
    low = colored_basis(9, 1.0, 5, dtype=np.float64)
    np.testing.assert_allclose(low / low[0, 0], full[:, :5] / full[0, 0], rtol=1e-14, atol=1e-15)  # the first columns
    assert colored_basis(8, 1.0, 8).shape == (8, 8)  # (n_basis == H may be even)
    for H, R in ((9, 4), (9, 2), (8, 6), (9, 0), (9, 10), (1, 2)):
        with pytest.raises(ValueError):
            colored_basis(H, 1.0, R)
    with pytest.raises(ValueError):
        colored_basis(0, 1.0)


# ---- 4. C ABI without a device

def test_abi_null_handle_is_an_argument_error():
    from mppi_hip import _lib as L
    lib = L.load()
    n = ctypes.c_int()
    buf = (ctypes.c_float * 64)()
    assert lib.mppi_set_noise_basis(None, 3, buf) == L.MPPI_E_ARG
    assert b"mppi_set_noise_basis" in lib.mppi_last_error()
    assert lib.mppi_set_noise_basis(None, 0, None) == L.MPPI_E_ARG
    assert lib.mppi_set_noise_basis(None, 3, None) == L.MPPI_E_ARG
    assert lib.mppi_get_noise_basis(None, ctypes.byref(n), None) == L.MPPI_E_ARG
    assert b"mppi_get_noise_basis" in lib.mppi_last_error()
    assert lib.mppi_get_noise_basis(None, None, None) == L.MPPI_E_ARG
    for name in ("mppi_set_noise_basis", "mppi_get_noise_basis"):
        assert name in L.EXPORTED


# ---- 5. MPPIModel(noise_basis=...) against a recording engine

class _Recorder:
    """Stands in for Engine: records the setters."""

    def __init__(self, config, device=0):
        self.config = config
        self.calls = []

    def _rec(self, name, *a):
        self.calls.append((name, a))
        return self

    def load_dynamics(self, *a, **kw):
        return self._rec("load_dynamics")

    def set_cost(self, *a, **kw):
        return self._rec("set_cost")

    def set_noise_model(self, *a):
        return self._rec("set_noise_model", *a)

    def set_noise_knots(self, n_knots, order=1):
        return self._rec("set_noise_knots", n_knots, order)

    def noise_knots(self):
        return (0, 0, None, None)

    def set_noise_basis(self, M):
        return self._rec("set_noise_basis", M)

    def close(self):
        pass


def test_model_sets_the_basis_law_and_samples_it_in_numpy_mode(monkeypatch):
    import mppi_hip.controller as C
    from mppi_hip.noise import basis_filter, colored_basis
    monkeypatch.setattr(C, "Engine", _Recorder)
    sig = [0.3]
    m = C.MPPIModel("cartpole_py", K=64, noise="numpy", noise_basis=("colored", 1.0), noise_sigma=sig)
    c = m.config
    names = [call[0] for call in m.engine.calls]
    assert names.index("set_noise_model") < names.index("set_noise_basis")
    want = colored_basis(c.H, 1.0)
    assert np.array_equal(bits(m.engine.calls[names.index("set_noise_basis")][1][0]), bits(want))
    assert np.array_equal(bits(m.noise_basis), bits(want))
    np.random.seed(5)
    z = np.random.randn(c.nu, c.H, c.K)
    np.random.seed(5)
    eps = m.draw_noise()
    assert eps.shape == (c.nu, c.H, c.K) and eps.dtype == np.float64
    assert np.array_equal(eps, basis_filter(z, want, sig).astype(np.float64))
    M3 = table(c.H, 3)  # an array, assigned: a law of rank 3, scaled by the preset's sigma
    m = C.MPPIModel("cartpole_py", K=64, noise="numpy")
    m.noise_basis = M3
    assert m.engine.calls[-1][0] == "set_noise_basis" and np.array_equal(m.engine.calls[-1][1][0], M3)
    np.random.seed(6)
    z = np.random.randn(c.nu, c.H, c.K)
    np.random.seed(6)
    eps = m.draw_noise()
    assert np.array_equal(eps, basis_filter(z, M3, c.sigma).astype(np.float64))
    assert np.linalg.matrix_rank(eps[0].astype(np.float32)) == 3
    m.noise_basis = ("colored", 2.0, 5)
    assert np.array_equal(bits(m.noise_basis), bits(colored_basis(c.H, 2.0, 5)))
    m.noise_basis = None
    assert m.engine.calls[-1] == ("set_noise_basis", (None,)) and m.noise_basis is None
    np.random.seed(7)
    z = np.random.randn(c.nu, c.H, c.K)
    np.random.seed(7)
    assert np.array_equal(m.draw_noise(), z * c.sigma)  # the default law again
    plain = C.MPPIModel("cartpole_py", K=64)  # the default asks for nothing
    assert plain.noise_basis is None and "set_noise_basis" not in [call[0] for call in plain.engine.calls]
    for kw in (dict(noise_knots=3), dict(noise_rho=0.5), dict(adapt_noise=0.3), dict(control_cost=0.5)):
        with pytest.raises(ValueError):
            C.MPPIModel("cartpole_py", K=64, noise_basis=M3, **kw)
    for bad in (np.zeros((c.H + 1, 2)), np.zeros((c.H, c.H + 1)), np.zeros(c.H)):
        with pytest.raises(ValueError):
            C.MPPIModel("cartpole_py", K=64, noise_basis=bad)
