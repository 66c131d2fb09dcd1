"""Knot-parameterised sampling noise on the host: mppi_hip.noise.knot_table / knot_filter, the header
csrc/noise_knots.h through g++ (bitwise), and the NULL-handle paths of the C ABI (no GPU needed)."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import PKG
from knot_cases import GRID, ORDERS, RHOS, TABLE_GRID, bits
from philox_ref import device_noise

EPS32 = float(np.finfo(np.float32).eps)  # one ulp of fp32 at 1


# ---- 1. the table

@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("H,P", TABLE_GRID)
def test_knot_table_properties(H, P, order):
    from mppi_hip.noise import knot_table
    idx, w = knot_table(H, P, order)
    assert idx.shape == (H, 4) and idx.dtype == np.int32 and w.shape == (H, 4) and w.dtype == np.float32
    assert idx.min() >= 0 and idx.max() <= P - 1
    assert np.all(np.diff(idx[:, 0]) >= 0)
    assert np.all(idx[:, 0] == idx.min(axis=1)) and np.all(idx.max(axis=1) - idx[:, 0] <= 3)  # a window of four knots
    row_sum = w.astype(np.float64).sum(axis=1)
    print("max |sum w - 1|", float(np.abs(row_sum - 1.0).max()))
    assert np.all(np.abs(row_sum - 1.0) <= EPS32)
    if order == 0:
        assert np.array_equal(idx[:, 0], (np.arange(H) * P) // H)
        assert np.array_equal(w, np.tile(np.float32([1, 0, 0, 0]), (H, 1)))
    if order == 1:
        assert np.all(w >= 0.0) and np.all(w <= 1.0)
    if order in (1, 3):  # the ends reproduce the first and the last knot exactly
        for t, knot in ((0, 0), (H - 1, P - 1)):
            on = idx[t] == knot
            assert float(w[t][on].sum()) == 1.0 and np.count_nonzero(w[t]) == 1 and np.all(w[t][~on] == 0.0)
    if P == H and order in (0, 1):  # the identity: weight 1 on knot t, 0 elsewhere
        for t in range(H):
            on = idx[t] == t
            assert np.count_nonzero(w[t]) == 1 and float(w[t][on].sum()) == 1.0 and np.all(w[t][~on] == 0.0)


def test_knot_table_refuses_bad_laws():
    from mppi_hip.noise import knot_table
    for H, P, order in ((7, 0, 1), (7, 8, 1), (7, 3, 2), (7, -1, 0), (7, 3, 4)):
        with pytest.raises(ValueError):
            knot_table(H, P, order)


# ---- 2. the header, through g++

HARNESS = r"""
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "noise_knots.h"
// argv: H P order rho sigma z[0..P)   ->   the table, then the row
int main(int argc, char** argv) {
  const int H = atoi(argv[1]), P = atoi(argv[2]), order = atoi(argv[3]);
  const float rho = strtof(argv[4], 0), sigma = strtof(argv[5], 0);
  if (!knot_law_valid(H, P, order) || argc != 6 + P) return 2;
  std::vector<float> z(P), kn(P), eps(H), w(4 * H);
  std::vector<int32_t> idx(4 * H);
  for (int j = 0; j < P; ++j) z[j] = strtof(argv[6 + j], 0);
  knot_table(H, P, order, idx.data(), w.data());
  knot_row(rho, ar1_innovation_scale(rho), sigma, z.data(), P, idx.data(), w.data(), kn.data(), eps.data(), H);
  for (int t = 0; t < H; ++t)
    printf("%d %d %d %d %a %a %a %a %a\n", idx[4 * t], idx[4 * t + 1], idx[4 * t + 2], idx[4 * t + 3], w[4 * t],
           w[4 * t + 1], w[4 * t + 2], w[4 * t + 3], eps[t]);
  return 0;
}
"""


@pytest.fixture(scope="module")
def harness():
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "k.cpp")
        with open(src, "w") as f:
            f.write(HARNESS)
        exe = os.path.join(d, "k")
        r = subprocess.run(["g++", "-O2", "-I", os.path.join(PKG, "csrc"), src, "-o", exe], capture_output=True,
                           text=True)
        if r.returncode != 0:
            pytest.fail(r.stderr)
        yield exe


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("H,P", TABLE_GRID)
def test_header_matches_numpy_restatements_bitwise(harness, H, P, order):
    from mppi_hip.noise import knot_filter, knot_table
    idx, w = knot_table(H, P, order)
    sigma = np.float32(0.7)
    z = device_noise(0xABCDEF + 64 * H + P, 1, 1, H, 4, 1.0)[0, 0, :, 1].astype(np.float32)  # [H]
    for rho in RHOS:
        args = [str(H), str(P), str(order), float(np.float32(rho)).hex(), float(sigma).hex()]
        args += [float(v).hex() for v in z[:P]]
        out = subprocess.run([harness, *args], capture_output=True, text=True, check=True).stdout.split("\n")
        got_idx = np.array([[int(v) for v in out[t].split()[:4]] for t in range(H)], np.int32)
        got_w = np.array([[float.fromhex(v) for v in out[t].split()[4:8]] for t in range(H)], np.float32)
        got_eps = np.array([float.fromhex(out[t].split()[8]) for t in range(H)], np.float32)
        assert np.array_equal(got_idx, idx)
        assert np.array_equal(bits(got_w), bits(w))
        ref = knot_filter(z.reshape(1, H, 1), P, order, rho, sigma)[0, :, 0]
        assert ref.dtype == np.float32
        assert np.array_equal(bits(got_eps), bits(ref)), (rho, got_eps, ref)


# ---- 3. identities of the filter

@pytest.mark.parametrize("H,P", GRID)
def test_knot_filter_identities(H, P):
    from mppi_hip.noise import ar1_filter, ar1_filter_f32, knot_filter
    z = np.random.RandomState(H * 16 + P).randn(2, 3, H, 5).astype(np.float32)
    sig = np.float32([0.7, 0.2, 1.3])
    for rho in RHOS:
        for order in ORDERS:
            out = knot_filter(z, P, order, rho, sig)
            assert out.dtype == np.float32 and out.shape == z.shape
            zz = z.copy()
            zz[..., P:, :] = 123.0  # only the first P rows are read
            assert np.array_equal(knot_filter(zz, P, order, rho, sig), out)
            if P == 1:  # one knot: constant in t
                assert np.array_equal(out, np.broadcast_to(out[..., :1, :], out.shape))
            if P == H and order in (0, 1):  # the handle's AR(1) / white noise value for value
                want = sig[:, None, None] * ar1_filter_f32(z, rho)
                assert np.array_equal(out, want)
                if rho == 0.0:  # (ar1_filter is float64: its product of two fp32 values is exact, rounded once here)
                    assert np.array_equal(out, sig[:, None, None] * z)
                    assert np.array_equal(out, ar1_filter(z, 0.0, sig).astype(np.float32))
                # ... and the float64 ar1_filter to fp32 rounding: about 1 / (1 - rho) = 10 roundings of 2^-24
                np.testing.assert_allclose(out, ar1_filter(z, rho, sig), rtol=0, atol=2e-6 * float(np.abs(out).max()))
    with pytest.raises(ValueError):
        knot_filter(z, P, 2)
    with pytest.raises(ValueError):
        knot_filter(z, H + 1, 1)


def test_fma_emulation_is_correctly_rounded():
    """_fma32 against exact rational arithmetic, on random operands, on sums that cancel, and on exact fp32 ties that
    only the product's low bits break (where rounding the float64 sum again would go wrong)."""
    from fractions import Fraction
    from mppi_hip.noise import _fma32
    rs = np.random.RandomState(0)
    a, b, c = (rs.randn(600).astype(np.float32) for _ in range(3))
    c[200:400] = -(a[200:400] * b[200:400]) * np.float32(1 + 2.0 ** -12)
    t = np.arange(100, dtype=np.float32)
    # a * b = 2^-24 - 2^-54: c + a * b lies just below the tie between c and its successor, which float64 cannot hold
    a[400:500], b[400:500] = np.float32(1 + 2.0 ** -15), np.float32((1 - 2.0 ** -15) * 2.0 ** -24)
    c[400:500] = np.float32(1.0) + t * np.float32(2.0 ** -23)
    a[500:600], b[500:600], c[500:600] = -a[400:500], b[400:500], c[400:500]
    got = _fma32(a, b, c)
    for i in range(600):
        v = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        f = np.float32(float(v))
        best = None
        for cand in (f, np.nextafter(f, np.float32(np.inf)), np.nextafter(f, np.float32(-np.inf))):
            d = abs(Fraction(float(cand)) - v)
            even = (int(np.float32(cand).view(np.uint32)) & 1) == 0
            if best is None or d < best[0] or (d == best[0] and even and not best[2]):
                best = (d, np.float32(cand), even)
        assert got[i] == best[1], (i, a[i], b[i], c[i])


# ---- 4. C ABI without a device

def test_abi_null_handle_is_an_argument_error():
    from mppi_hip import _lib as L
    lib = L.load()
    n, order = ctypes.c_int(), ctypes.c_int()
    buf = (ctypes.c_float * 64)()
    assert lib.mppi_set_noise_knots(None, 3, 1) == L.MPPI_E_ARG
    assert b"mppi_set_noise_knots" in lib.mppi_last_error()
    assert lib.mppi_set_noise_knots(None, 0, 0) == L.MPPI_E_ARG
    assert lib.mppi_get_noise_knots(None, ctypes.byref(n), ctypes.byref(order), None, None) == L.MPPI_E_ARG
    assert b"mppi_get_noise_knots" in lib.mppi_last_error()
    assert lib.mppi_get_noise_knots(None, None, None, None, None) == L.MPPI_E_ARG
    assert lib.mppi_noise_eval(None, 1, ctypes.c_uint64(1), buf) == L.MPPI_E_ARG
    assert b"mppi_noise_eval" in lib.mppi_last_error()
    assert lib.mppi_noise_eval(None, 1, ctypes.c_uint64(1), None) == L.MPPI_E_ARG


# ---- 5. MPPIModel(noise_knots=...) against a recording engine

class _Recorder:
    """Stands in for Engine: records the setters, keeps the knot law it was given."""

    def __init__(self, config, device=0):
        self.config = config
        self.calls = []
        self.knots = (0, 0)

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
        self.knots = (n_knots, order) if n_knots else (0, 0)
        return self._rec("set_noise_knots", n_knots, order)

    def noise_knots(self):
        return self.knots + (None, None)

    def close(self):
        pass


def test_model_sets_the_knot_law_and_samples_it_in_numpy_mode(monkeypatch):
    import mppi_hip.controller as C
    from mppi_hip.noise import knot_filter
    monkeypatch.setattr(C, "Engine", _Recorder)
    m = C.MPPIModel("cartpole_py", K=64, noise="numpy", noise_knots=(3, 3), noise_rho=0.4)
    names = [c[0] for c in m.engine.calls]
    assert names.index("set_noise_model") < names.index("set_noise_knots")
    assert ("set_noise_knots", (3, 3)) in m.engine.calls and m.noise_knots == (3, 3)
    c = m.config
    np.random.seed(5)
    z = np.random.randn(c.nu, c.H, c.K)
    np.random.seed(5)
    eps = m.draw_noise()
    assert eps.shape == (c.nu, c.H, c.K)
    assert np.array_equal(eps, knot_filter(z, 3, 3, rho=0.4, sigma_u=c.sigma).astype(np.float64))
    assert np.linalg.matrix_rank(eps[0].astype(np.float32)) == 3
    m.noise_knots = 5  # a bare count is linear
    assert m.engine.calls[-1] == ("set_noise_knots", (5, 1)) and m.noise_knots == (5, 1)
    m.noise_knots = None
    assert m.engine.calls[-1] == ("set_noise_knots", (0, 0)) and m.noise_knots is None
    assert C.MPPIModel("cartpole_py", K=64).noise_knots is None  # the default asks for nothing
    assert "set_noise_knots" not in [c[0] for c in C.MPPIModel("cartpole_py", K=64).engine.calls]
    for kw in (dict(adapt_noise=0.3), dict(control_cost=0.5)):
        with pytest.raises(ValueError):
            C.MPPIModel("cartpole_py", K=64, noise_knots=3, **kw)
