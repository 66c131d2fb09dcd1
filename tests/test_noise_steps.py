"""The per-step sampling scale on the host: csrc/step_moments.h and csrc/step_law.h through g++ against their numpy
float32 restatements (mppi_hip.stats.step_moments_f32, adapt_noise_steps_f32), those against the float64 definitions,
noise.steps_filter against ar1_filter, the NULL-handle paths of the six C entries, and MPPIModel(noise_steps=...,
adapt_steps=...) against a recording engine (no GPU needed)."""
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
#include <vector>
#include "step_law.h"
#include "step_moments.h"
// argv: in out.  in: int32 {mode, B, nu, H, Kp, centred, shift}, then float32 data; out: float32 results.
//   mode 0: w [B][Kp], noise [B][nu][H][Kp]                                   -> m1, m2 [B][nu][H]
//   mode 1: rate, sigma_min, sigma_max, fill[nu], n_finite[B] (as floats), S, m1, m2 [B][nu][H]  -> S [B][nu][H]
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  int hd[7];
  if (fread(hd, 4, 7, f) != 7) return 4;
  const int mode = hd[0], B = hd[1], nu = hd[2], H = hd[3], Kp = hd[4], centred = hd[5], shift = hd[6];
  const size_t n = (size_t)B * nu * H;
  auto rd = [&](std::vector<float>& v, size_t m) {
    v.resize(m);
    if (fread(v.data(), 4, m, f) != m) exit(5);
  };
  FILE* o = fopen(argv[2], "wb");
  if (mode == 0) {
    std::vector<float> w, e, m1(n), m2(n);
    rd(w, (size_t)B * Kp);
    rd(e, n * Kp);
    step_moments_host(w.data(), e.data(), B, nu, H, Kp, m1.data(), m2.data());
    fwrite(m1.data(), 4, n, o);
    fwrite(m2.data(), 4, n, o);
  } else {
    std::vector<float> p, fill, nf, S, m1, m2;
    rd(p, 3);
    rd(fill, nu);
    rd(nf, B);
    rd(S, n);
    rd(m1, n);
    rd(m2, n);
    const StepAdapt a = {p[0], p[1], p[2], centred};
    for (int b = 0; b < B; ++b)
      for (int u = 0; u < nu; ++u) {
        const size_t r = ((size_t)b * nu + u) * H;
        step_law_row(a, S.data() + r, m1.data() + r, m2.data() + r, H, shift != 0, fill[u], nf[b] != 0.0f);
      }
    fwrite(S.data(), 4, n, o);
  }
  fclose(o);
  fclose(f);
  return 0;
}
"""


@pytest.fixture(scope="module")
def native(tmp_path_factory):
    """step_law.h and step_moments.h compiled with g++ into a small program of their own."""
    d = tmp_path_factory.mktemp("noise_steps")
    src, exe = str(d / "h.cpp"), str(d / "h")
    open(src, "w").write(HARNESS)
    r = subprocess.run(["g++", "-O2", "-I", os.path.join(PKG, "csrc"), src, "-o", exe], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.fail(r.stderr)

    def run(header, arrays, n_out, shape):
        fin, fout = str(d / "in.bin"), str(d / "out.bin")
        with open(fin, "wb") as f:
            f.write(np.asarray(header, np.int32).tobytes())
            for a in arrays:
                f.write(np.ascontiguousarray(a, np.float32).tobytes())
        subprocess.run([exe, fin, fout], check=True)
        out = np.fromfile(fout, np.float32)
        return [out[i * int(np.prod(shape)):(i + 1) * int(np.prod(shape))].reshape(shape) for i in range(n_out)]

    return run


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def _weights(rs, B, K, lam):
    """Normalised softmin weights of seeded costs, float32 as the device holds them."""
    from mppi_hip.stats import softmin_weights_ref
    costs = 5.0 + 3.0 * rs.randn(B, K)
    return softmin_weights_ref(costs, lam).astype(np.float32)


def _pad(a, Kp):
    out = np.zeros(a.shape[:-1] + (Kp,), np.float32)
    out[..., :a.shape[-1]] = a
    return out


def _moments_native(native, w, e):
    B, nu, H, K = e.shape
    Kp = (K + 63) // 64 * 64
    return native([0, B, nu, H, Kp, 0, 0], [_pad(w, Kp), _pad(e, Kp)], 2, (B, nu, H))


# ---------------------------------------------------------------------------------- 1. headers == numpy float32

@pytest.mark.parametrize("K", [130, 300])
@pytest.mark.parametrize("H", [1, 7, 19])
def test_headers_equal_the_numpy_f32_restatements_bit_for_bit(native, H, K):
    """Moments: K = 130 is one partial wave-chunk, K = 300 (Kp = 320) two, the second partial.  Refit: both centred
    values, with and without the shift, a dead solve, cells whose m2 - m1^2 is negative by rounding, and both clamps
    binding."""
    from mppi_hip.stats import adapt_noise_steps_f32, step_moments_f32
    rs = np.random.RandomState(1000 * H + K)
    B, nu = 3, 3
    w = _weights(rs, B, K, 1.0)
    e = (rs.randn(B, nu, H, K) * np.array([0.05, 0.5, 2.0])[None, :, None, None]).astype(np.float32)
    m1, m2 = step_moments_f32(w, e)
    c1, c2 = _moments_native(native, w, e)
    assert np.array_equal(_bits(c1), _bits(m1)) and np.array_equal(_bits(c2), _bits(m2))
    assert np.all(m2 > 0)
    # the refit's inputs: the moments above, then cells made to take each branch
    S = (0.05 + 1.5 * rs.rand(B, nu, H)).astype(np.float32)
    fill = np.array([0.2, 0.5, 0.8], np.float32)
    a1, a2 = m1.copy(), m2.copy()
    # solve 1, actuator 0: m2 one ulp below m1^2 rounded -- the centred difference is negative, max(., 0) is taken
    a1[1, 0] = (0.3 + rs.rand(H)).astype(np.float32)
    a2[1, 0] = np.nextafter((a1[1, 0] * a1[1, 0]).astype(np.float32), np.float32(0.0))
    neg = a2[1, 0].astype(np.float64) - a1[1, 0].astype(np.float64) ** 2
    assert np.all(neg < 0.0)
    a2[1, 1] = np.float32(1e6)   # sigma_max binds
    a2[1, 2] = np.float32(0.0)   # with a1 = 0 and a small S: sigma_min binds
    a1[1, 2] = np.float32(0.0)
    S[1, 2] = np.float32(1e-3)
    a2[0, 0, 0] = np.float32(np.inf)  # a non-finite moment leaves its cell
    nf = np.array([K, K, 0], np.float32)  # solve 2 is dead: only shifted
    lo, hi = 0.01, 3.0
    for centred in (0, 1):
        for shift in (0, 1):
            for rate in (0.3, 1.0):
                want = adapt_noise_steps_f32(S, a1, a2, rate, lo, hi, centred=bool(centred), shift=bool(shift),
                                             fill=fill, n_finite=nf)
                got, = native([1, B, nu, H, 0, centred, shift], [np.float32([rate, lo, hi]), fill, nf, S, a1, a2], 1,
                              (B, nu, H))
                assert want.dtype == np.float32
                assert np.array_equal(_bits(got), _bits(want)), (centred, shift, rate)
                # the branches were taken: un-shift the result and look at the cells
                core = want[..., :H - 1] if shift else want
                old = S[..., 1:] if shift else S
                if core.size:
                    assert np.all(core[1, 1] == np.float32(hi)) and np.all(core[1, 2] == np.float32(lo))
                    assert np.array_equal(_bits(core[2]), _bits(old[2]))  # the dead solve's cells as they were
                    if centred:  # v clipped to 0: sqrt((1 - rate) S^2), clamped
                        keep = np.float32(1.0) - np.float32(rate)
                        ref = np.clip(np.sqrt(keep * (old[1, 0] * old[1, 0])), np.float32(lo), np.float32(hi))
                        assert np.array_equal(_bits(core[1, 0]), _bits(ref))
                    if not shift:
                        assert _bits(want[0, 0, 0]) == _bits(S[0, 0, 0])  # the non-finite moment's cell
                if shift:
                    assert np.array_equal(want[..., H - 1], np.broadcast_to(fill, (B, nu)))  # H == 1: the fill alone


def test_refit_agrees_with_the_float64_rule():
    from mppi_hip.stats import adapt_noise_steps, adapt_noise_steps_f32
    rs = np.random.RandomState(5)
    B, nu, H = 2, 3, 7
    S = (0.05 + 1.5 * rs.rand(B, nu, H)).astype(np.float32)
    m1 = (0.2 * rs.randn(B, nu, H)).astype(np.float32)
    m2 = (m1 * m1 + 0.5 * rs.rand(B, nu, H)).astype(np.float32)
    for centred in (False, True):
        for shift in (False, True):
            a = adapt_noise_steps_f32(S, m1, m2, 0.3, 1e-3, 10.0, centred, shift, fill=0.5, n_finite=[3, 0])
            b = adapt_noise_steps(S, m1, m2, float(np.float32(0.3)), 1e-3, 10.0, centred, shift, fill=0.5,
                                  n_finite=[3, 0])
            # (a product, a difference, the fma, the square root: a handful of roundings)
            np.testing.assert_allclose(a, b, rtol=8 * 2.0 ** -24, atol=0.0)
    with pytest.raises(ValueError):
        adapt_noise_steps(S, m1, m2, 1.5)
    with pytest.raises(ValueError):
        adapt_noise_steps(S, m1, m2, 0.3, 0.0, 1.0)
    with pytest.raises(ValueError):
        adapt_noise_steps(S, m1, m2, 0.3, shift=True)


# ---------------------------------------------------------------------------------- 2. float32 against float64

@pytest.mark.parametrize("K", [130, 300])
def test_f32_moments_stay_within_the_bound_of_an_fp32_sum_of_k_positive_terms(K):
    """m2 within relative K 2^-24 and m1 within K 2^-24 sqrt(m2) of the float64 sums over the same float32 weights and
    noise: the bound of an fp32 sum of K positive terms (sequential sums, the worst order, stay below 1e-6 here).  The
    two moments are compared separately, never their cancelling difference."""
    from mppi_hip.stats import step_moments_f32, step_moments_ref
    B, nu, H = 2, 3, 7
    bound = K * 2.0 ** -24
    worst = [0.0, 0.0]
    for lam in (0.05, 1.0, 1e6):
        for sigma in (0.05, 0.5, 2.0):
            rs = np.random.RandomState(int(K + 10 * sigma + 7))
            w = _weights(rs, B, K, lam)
            e = (sigma * rs.randn(B, nu, H, K)).astype(np.float32)
            m1, m2 = step_moments_f32(w, e)
            r1, r2 = step_moments_ref(None, e, w=w)
            e2 = float(np.max(np.abs(m2 - r2) / r2))
            e1 = float(np.max(np.abs(m1 - r1) / np.sqrt(r2)))
            worst = [max(worst[0], e1), max(worst[1], e2)]
            assert e2 <= bound and e1 <= bound, (lam, sigma, e1, e2)
    print(f"K={K}: m1 err {worst[0]:.3e}, m2 rel err {worst[1]:.3e}, bound {bound:.3e}")


def test_ref_from_costs_uses_the_statistics_weights():
    from mppi_hip.stats import softmin_weights_ref, step_moments_ref
    rs = np.random.RandomState(2)
    costs, e = rs.rand(2, 40) * 4, rs.randn(2, 3, 5, 40)
    w = softmin_weights_ref(costs, 0.7)
    a1, a2 = step_moments_ref(costs, e, lam=0.7)
    np.testing.assert_allclose(a1, np.einsum("bk,buhk->buh", w, e))
    np.testing.assert_allclose(a2, np.einsum("bk,buhk->buh", w, e * e))


# ---------------------------------------------------------------------------------- 3. the law

@pytest.mark.parametrize("rho", [0.0, 0.9])
def test_a_table_of_sigma_u_broadcast_is_the_ar1_law_bit_for_bit(rho):
    from mppi_hip.noise import ar1_filter, ar1_filter_f32, steps_filter
    rs = np.random.RandomState(3)
    nu, H, K = 3, 19, 33
    z = rs.randn(2, nu, H, K)
    sig = np.array([0.2, 0.5, 0.8])
    table = np.broadcast_to(sig[:, None], (nu, H))
    got = steps_filter(z, table, rho)
    assert got.dtype == np.float64 and np.array_equal(got, ar1_filter(z, rho, sig))
    # float32 normals: the device's operations
    z32 = z.astype(np.float32)
    got = steps_filter(z32, table, rho)
    want = (sig.astype(np.float32)[:, None, None] * ar1_filter_f32(z32, rho)).astype(np.float32)
    assert got.dtype == np.float32 and np.array_equal(_bits(got), _bits(want))
    # one table per solve, varying along the horizon
    per = (0.1 + rs.rand(2, nu, H)).astype(np.float32)
    got = steps_filter(z32, per, rho)
    assert np.array_equal(_bits(got[1, 2, 5]), _bits(per[1, 2, 5] * ar1_filter_f32(z32, rho)[1, 2, 5]))
    for bad in (np.ones((nu, H + 1)), -np.ones((nu, H)), np.full((nu, H), np.nan), np.ones((3, nu, H))):
        with pytest.raises(ValueError):
            steps_filter(z, bad, rho)
    with pytest.raises(ValueError):
        steps_filter(z, table, 1.0)


# ---------------------------------------------------------------------------------- C ABI without a device

ENTRIES = {
    "mppi_set_noise_steps": r"int mppi_set_noise_steps\(mppi_handle\* h, int B, const float\* sigma\s*\);",
    "mppi_get_noise_steps": r"int mppi_get_noise_steps\(mppi_handle\* h, int B, float\* sigma\s*, int\* active\);",
    "mppi_set_noise_steps_adapt": r"int mppi_set_noise_steps_adapt\(mppi_handle\* h, float rate, float sigma_min, "
                                  r"float sigma_max, int centred\);",
    "mppi_get_noise_steps_adapt": r"int mppi_get_noise_steps_adapt\(mppi_handle\* h, float\* rate, float\* sigma_min, "
                                  r"float\* sigma_max, int\* centred\);",
    "mppi_get_step_moments": r"int mppi_get_step_moments\(mppi_handle\* h, int B, int step, float\* m1, "
                             r"float\* m2\s*\);",
    "mppi_step_moments_eval": r"int mppi_step_moments_eval\(mppi_handle\* h, int B, const float\* costs, "
                              r"const float\* noise, float\* m1, float\* m2\);",
}


def test_header_declares_and_the_bindings_bind_the_entries():
    from mppi_hip import _lib as L
    raw = open(os.path.join(REPO, "include", "mppi.h")).read()
    assert re.search(r"#define\s+MPPI_FLAG_STEP_MOMENTS\s+0x800\b", raw) and L.FLAG_STEP_MOMENTS == 0x800
    assert re.search(r"#define\s+MPPI_ABI_VERSION\s+4\b", raw)
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    lib = L.load()
    jl = open(os.path.join(PKG, "julia", "MPPIHip.jl")).read()
    for name, pat in ENTRIES.items():
        assert re.search(pat, src), name
        assert name in L.EXPORTED and hasattr(lib, name)
    for name in ("mppi_set_noise_steps", "mppi_get_noise_steps", "mppi_set_noise_steps_adapt", "mppi_get_step_moments"):
        assert ":" + name in jl, name
    for fn in ("set_noise_steps!", "noise_steps", "set_noise_steps_adapt!", "step_moments"):
        assert "function " + fn + "(" in jl, fn


def test_abi_null_handle_is_an_argument_error():
    from mppi_hip import _lib as L
    lib = L.load()
    buf = (ctypes.c_float * 8)()
    f = [ctypes.c_float() for _ in range(3)]
    i = ctypes.c_int()
    calls = {
        "mppi_set_noise_steps": lambda: lib.mppi_set_noise_steps(None, 1, buf),
        "mppi_get_noise_steps": lambda: lib.mppi_get_noise_steps(None, 1, buf, ctypes.byref(i)),
        "mppi_set_noise_steps_adapt": lambda: lib.mppi_set_noise_steps_adapt(None, 0.3, 1e-3, 10.0, 1),
        "mppi_get_noise_steps_adapt": lambda: lib.mppi_get_noise_steps_adapt(None, *(ctypes.byref(x) for x in f),
                                                                             ctypes.byref(i)),
        "mppi_get_step_moments": lambda: lib.mppi_get_step_moments(None, 1, 0, buf, buf),
        "mppi_step_moments_eval": lambda: lib.mppi_step_moments_eval(None, 1, buf, buf, buf, buf),
    }
    for name, call in calls.items():
        assert call() == L.MPPI_E_ARG, name
        assert name.encode() in lib.mppi_last_error(), name
    assert lib.mppi_set_noise_steps(None, 0, None) == L.MPPI_E_ARG


# ---------------------------------------------------------------------------------- MPPIModel against a recorder

class _Recorder:
    """Stands in for Engine: records every call."""

    def __init__(self, config, device=0):
        self.config = config
        self.calls = []
        self.table = None

    def _rec(self, name, *a, **kw):
        self.calls.append((name, a, kw))
        return self

    def load_dynamics(self, *a, **kw):
        return self._rec("load_dynamics")

    def set_cost(self, *a, **kw):
        return self._rec("set_cost")

    def set_noise_model(self, *a, **kw):
        return self._rec("set_noise_model", *a, **kw)

    def set_elites(self, *a, **kw):
        return self._rec("set_elites", *a, **kw)

    def set_noise_steps(self, S):
        self.table = np.asarray(S, np.float32)[None]
        return self._rec("set_noise_steps", S)

    def set_noise_steps_adapt(self, *a, **kw):
        return self._rec("set_noise_steps_adapt", *a, **kw)

    def noise_steps(self, B=1):
        self._rec("noise_steps")
        return self.table

    def noise_knots(self):
        return 0, 0, None, None

    def set_noise_knots(self, *a, **kw):
        return self._rec("set_noise_knots", *a, **kw)

    def set_control_cost(self, *a, **kw):
        return self._rec("set_control_cost", *a, **kw)

    def solve(self, x0, U, **kw):
        from mppi_hip.engine import SolveResult
        self._rec("solve", **kw)
        c = self.config
        return SolveResult(U=np.asarray(U, np.float32), costs=np.zeros(c.K, np.float32),
                           weights=np.zeros(c.K, np.float32), u0=np.zeros(c.nu, np.float32), status=0, stats=None)

    def close(self):
        pass


def test_model_sets_the_table_and_the_refit_once_and_requests_nothing_per_step(monkeypatch):
    import mppi_hip.controller as C
    monkeypatch.setattr(C, "Engine", _Recorder)
    H = 100
    table = np.linspace(0.2, 1.0, H, dtype=np.float32)[None]
    m = C.MPPIModel("cartpole_py", K=64, noise_steps=table, adapt_steps=0.3, noise_rho=0.4, n_elite=8,
                    adapt_limits=(0.01, 5.0, 0.9))
    names = [c[0] for c in m.engine.calls]
    assert names.count("set_noise_steps") == 1 and names.index("set_noise_steps") < names.index("set_noise_steps_adapt")
    assert names.index("set_noise_model") < names.index("set_noise_steps")
    assert [c for c in m.engine.calls if c[0] == "set_noise_steps_adapt"][0][1] == (0.3, 0.01, 5.0)
    n0 = len(m.engine.calls)
    data = C.SimData(qpos=np.zeros(2), qvel=np.zeros(2), ctrl=np.zeros(1))
    for _ in range(3):
        C.mppi_controller(m, data)
    steps = m.engine.calls[n0:]
    assert [c[0] for c in steps] == ["solve"] * 3 and all("stats" not in c[2] for c in steps)
    assert np.array_equal(m.noise_steps, table[0].reshape(1, H))
    # the numpy noise mode samples the same law from the live table
    h = C.MPPIModel("cartpole_py", K=64, noise="numpy", noise_steps=table)
    np.random.seed(0)
    eps = h.draw_noise()
    np.random.seed(0)
    z = np.random.randn(1, H, 64)
    assert np.array_equal(eps, C.steps_filter(z, table, 0.0))
    off = C.MPPIModel("cartpole_py", K=64)
    assert off.noise_steps is None and "set_noise_steps" not in [c[0] for c in off.engine.calls]
    for kw in (dict(adapt_steps=0.3), dict(noise_steps=table, adapt_steps=1.5), dict(noise_steps=table, noise_knots=4),
               dict(noise_steps=table, adapt_noise=0.3), dict(noise_steps=table, control_cost=1.0)):
        with pytest.raises(ValueError):
            C.MPPIModel("cartpole_py", K=64, **kw)
