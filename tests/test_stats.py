"""Solve diagnostics on the host: mppi_hip.stats.solve_stats_ref (the float64 statement of include/mppi.h's
definitions) against explicit loops, adapt_noise_model, and the parts of the C ABI that need no GPU."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from conftest import REPO
from philox_ref import device_noise

INF, NAN = float("inf"), float("nan")


def _loops(c, eps, lam, norm_eps):
    """One solve, as explicit Python loops over k, u and t: (dict of the struct's fields, m2 [nu], m11 [nu])."""
    K = len(c)
    F = [k for k in range(K) if math.isfinite(c[k])]
    nu, H = (len(eps), len(eps[0])) if eps is not None else (0, 0)
    if not F:
        st = dict(cost_min=INF, cost_max=INF, cost_mean=INF, free_energy=INF, cost_std=0.0, cost_weighted=0.0, ess=0.0,
                  entropy=0.0, n_finite=0, k_best=-1)
        return st, [0.0] * nu, [0.0] * nu
    beta = min(c[k] for k in F)
    wt = [math.exp(-(c[k] - beta) / lam) if k in F else 0.0 for k in range(K)]
    S = sum(wt)
    w = [v / (S + norm_eps) for v in wt]
    mean = sum(c[k] for k in F) / len(F)
    ent = 0.0
    for k in F:
        p = wt[k] / S
        if p > 0.0:
            ent -= p * math.log(p)
    st = dict(cost_min=beta, cost_max=max(c[k] for k in F), cost_mean=mean,
              cost_std=math.sqrt(sum((c[k] - mean) ** 2 for k in F) / len(F)),
              cost_weighted=sum(w[k] * c[k] for k in F), ess=S * S / sum(v * v for v in wt), entropy=ent,
              free_energy=beta - lam * math.log(S / len(F)), n_finite=len(F),
              k_best=min(k for k in F if c[k] == beta))
    m2, m11 = [], []
    for u in range(nu):
        a = sum(w[k] * eps[u][t][k] ** 2 for t in range(H) for k in range(K)) / H
        b = sum(w[k] * eps[u][t][k] * eps[u][t - 1][k] for t in range(1, H) for k in range(K)) / (H - 1) if H > 1 \
            else 0.0
        m2.append(a)
        m11.append(b)
    return st, m2, m11


def test_solve_stats_ref_matches_explicit_loops():
    """[B, nu, H, K] = [2, 3, 5, 7] with a NaN, a +inf, a -inf and a tie for the minimum (the lower k wins)."""
    from mppi_hip.stats import FIELDS, solve_stats_ref
    rs = np.random.RandomState(1)
    costs = 100.0 + 5.0 * rs.randn(2, 7)
    costs[0, 0], costs[0, 3], costs[0, 6] = NAN, INF, -INF
    costs[0, 5] = costs[0, 2] = costs[0].copy()[np.isfinite(costs[0])].min() - 1.0  # tie: k = 2 and k = 5
    costs[1, 4] = costs[1, 1] = costs[1].min() - 0.5                                 # tie: k = 1 and k = 4
    noise = rs.randn(2, 3, 5, 7)
    lam, eps = 2.5, 1e-3
    got = solve_stats_ref(costs, noise, lam, eps)
    assert got["k_best"].tolist() == [2, 1] and got["n_finite"].tolist() == [4, 7]
    for b in range(2):
        st, m2, m11 = _loops(costs[b].tolist(), noise[b].tolist(), lam, eps)
        for n in FIELDS:
            assert got[n][b] == pytest.approx(st[n], rel=1e-13, abs=1e-15), n
        np.testing.assert_allclose(got["eps_m2"][b], m2, rtol=1e-13)
        np.testing.assert_allclose(got["eps_m11"][b], m11, rtol=1e-12, atol=1e-15)
        assert 1.0 <= got["ess"][b] <= got["n_finite"][b]
        assert 0.0 <= got["entropy"][b] <= math.log(got["n_finite"][b])
    # a single solve, no noise, H = 1
    one = solve_stats_ref(costs[1], None, lam, eps)
    assert one["k_best"] == 1 and "eps_m2" not in one
    h1 = solve_stats_ref(costs, noise[:, :, :1], lam, eps)
    assert np.all(h1["eps_m11"] == 0.0) and h1["eps_m2"].shape == (2, 3)


def test_solve_stats_ref_without_a_finite_cost():
    from mppi_hip.stats import solve_stats_ref
    costs = np.array([[NAN, INF, -INF, NAN], [1.0, 2.0, 3.0, 4.0]])
    got = solve_stats_ref(costs, np.ones((2, 2, 3, 4)), 1.0, 0.0)
    assert got["n_finite"][0] == 0 and got["k_best"][0] == -1
    for n in ("ess", "entropy", "cost_std", "cost_weighted"):
        assert got[n][0] == 0.0, n
    for n in ("cost_min", "cost_max", "cost_mean", "free_energy"):
        assert got[n][0] == INF, n
    assert np.all(got["eps_m2"][0] == 0.0) and np.all(got["eps_m11"][0] == 0.0)
    assert got["n_finite"][1] == 4 and np.all(got["eps_m2"][1] > 0.0)  # ... and the other solve is untouched by it


def test_uniform_weights_have_full_ess_and_entropy():
    from mppi_hip.stats import solve_stats_ref
    got = solve_stats_ref(np.full((1, 30), 7.0), None, 1.0, 0.0)
    assert got["ess"][0] == 30.0 and got["entropy"][0] == pytest.approx(math.log(30.0), rel=1e-15)
    assert got["k_best"][0] == 0 and got["free_energy"][0] == 7.0 and got["cost_std"][0] == 0.0


# ---- adapt_noise_model

def _uniform_moments(eps):
    """eps [nu, H, K] -> (m2, m11) [nu] with uniform weights 1 / K."""
    H = eps.shape[1]
    return (eps ** 2).mean(axis=2).sum(axis=1) / H, (eps[:, 1:] * eps[:, :-1]).mean(axis=2).sum(axis=1) / (H - 1)


def test_adapt_rate_zero_is_the_identity():
    from mppi_hip.stats import adapt_noise_model
    s, rho = adapt_noise_model([0.5, 2.0], 0.3, [[9.0, 9.0]], [[1.0, 1.0]], 0.0)
    assert np.array_equal(s, [0.5, 2.0]) and rho == 0.3


def test_adapt_rate_one_recovers_the_law_of_the_device_normals():
    """Uniform-weight moments of AR(1) noise over N = 64 * 4096 values per actuator: the estimators' standard error is
    near 1 / sqrt(N) = 0.002, so 0.02 is ten of them (tests/test_noise_model.py's bars)."""
    from mppi_hip.noise import ar1_filter
    from mppi_hip.stats import adapt_noise_model, solve_stats_ref
    rho, sig = 0.8, np.array([0.5, 2.0])
    eps = ar1_filter(device_noise(0x1234, 1, 2, 64, 4096, 1.0), rho, sig)
    m2, m11 = _uniform_moments(eps[0])
    ref = solve_stats_ref(np.zeros((1, 4096)), eps, 1.0, 0.0)  # equal costs: the same uniform weights
    np.testing.assert_allclose(ref["eps_m2"][0], m2, rtol=1e-12)
    np.testing.assert_allclose(ref["eps_m11"][0], m11, rtol=1e-12)
    s, r = adapt_noise_model([1.0, 1.0], 0.0, m2[None], m11[None], 1.0)
    print("sigma", s, "rho", r)
    assert np.all(np.abs(s / sig - 1.0) < 0.02)
    assert abs(r - rho) < 0.02
    # half way: the variances and rho are averaged, batch rows are averaged first
    s2, r2 = adapt_noise_model([1.0, 1.0], 0.0, np.stack([m2, m2]), np.stack([m11, m11]), 0.5)
    np.testing.assert_allclose(s2, np.sqrt(0.5 + 0.5 * m2), rtol=1e-14)
    assert r2 == pytest.approx(0.5 * r, rel=1e-14)


def test_adapt_clips():
    from mppi_hip.stats import adapt_noise_model
    s, r = adapt_noise_model([1.0, 1.0], 0.5, [1e-8, 1e4], [1e-8, 1e4], 1.0, sigma_min=0.1, sigma_max=3.0, rho_max=0.9)
    assert s.tolist() == [0.1, 3.0] and r == 0.9  # m11 / m2 = 1 -> rho_max
    s, r = adapt_noise_model([1.0], 0.5, [1.0], [-0.4], 1.0)
    assert r == 0.0  # a negative lag product is no AR(1) correlation the engine can sample
    s, r = adapt_noise_model([1.0], 0.5, [0.0], [0.0], 1.0, sigma_min=0.25)
    assert s.tolist() == [0.25] and r == 0.0  # every winner had zero noise


@pytest.mark.parametrize("kw", [dict(rate=-0.1), dict(rate=1.5), dict(rate=NAN), dict(rho=1.0), dict(rho=-0.1),
                                dict(rho_max=1.0), dict(sigma_min=2.0, sigma_max=1.0), dict(sigma_min=-1.0),
                                dict(sigma_u=[1.0, -1.0]), dict(sigma_u=[1.0, NAN]), dict(eps_m2=[1.0, NAN]),
                                dict(eps_m2=[1.0, -1.0]), dict(eps_m11=[INF, 0.0]), dict(eps_m2=[1.0, 1.0, 1.0]),
                                dict(eps_m11=[[0.1, 0.1]])])
def test_adapt_refuses_bad_arguments(kw):
    from mppi_hip.stats import adapt_noise_model
    args = dict(sigma_u=[1.0, 1.0], rho=0.5, eps_m2=[1.0, 1.0], eps_m11=[0.1, 0.1], rate=0.5, sigma_min=1e-3,
                sigma_max=10.0, rho_max=0.95)
    adapt_noise_model(**args)
    args.update(kw)
    with pytest.raises(ValueError):
        adapt_noise_model(**args)


# ---- C ABI without a device

def test_struct_is_40_bytes_and_mirrors_the_header():
    from mppi_hip import _lib as L
    assert ctypes.sizeof(L.mppi_solve_stats) == 40
    assert np.dtype(L.STATS_DTYPE).itemsize == 40
    src = open(os.path.join(REPO, "include", "mppi.h")).read()
    body = re.search(r"typedef struct mppi_solve_stats \{(.*?)\} mppi_solve_stats;", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for ctype, decl in re.findall(r"\b(float|int32_t)\s+([^;]+);", body):
        names += [(n.strip(), ctype) for n in decl.split(",")]
    want = [(n, "float" if t is ctypes.c_float else "int32_t") for n, t in L.mppi_solve_stats._fields_]
    assert names == want
    from mppi_hip.stats import FIELDS
    assert list(FIELDS) == [n for n, _ in want]


def test_header_declares_what_the_binding_binds():
    from mppi_hip import _lib as L
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "mppi.h")).read(), flags=re.S)
    assert re.search(r"#define\s+MPPI_FLAG_STATS\s+0x200\b", src) and L.FLAG_STATS == 0x200
    assert re.search(r"#define\s+MPPI_ABI_VERSION\s+4\b", src)
    protos = {
        "mppi_get_stats": r"int mppi_get_stats\(mppi_handle\* h, int B, int step, mppi_solve_stats\* stats, "
                          r"float\* eps_m2, float\* eps_m11\);",
        "mppi_device_stats": r"int mppi_device_stats\(mppi_handle\* h, void\*\* d_stats, void\*\* d_m2, "
                             r"void\*\* d_m11\);",
        "mppi_stats_eval": r"int mppi_stats_eval\(mppi_handle\* h, int B, const float\* costs, const float\* noise, "
                           r"mppi_solve_stats\* stats,\s+float\* eps_m2, float\* eps_m11\);",
    }
    lib = L.load()
    for name, pat in protos.items():
        assert re.search(pat, src), name
        assert name in L.EXPORTED and hasattr(lib, name)
    assert len(lib.mppi_get_stats.argtypes) == 6 and len(lib.mppi_stats_eval.argtypes) == 7
    assert len(lib.mppi_device_stats.argtypes) == 4


def test_abi_null_handle_is_an_argument_error():
    from mppi_hip import _lib as L
    lib = L.load()
    st = L.mppi_solve_stats()
    m = (ctypes.c_float * 4)()
    c = (ctypes.c_float * 4)(1, 2, 3, 4)
    p = ctypes.c_void_p()
    assert lib.mppi_get_stats(None, 1, 0, ctypes.byref(st), m, m) == L.MPPI_E_ARG
    assert b"mppi_get_stats" in lib.mppi_last_error()
    assert lib.mppi_get_stats(None, 1, 0, None, None, None) == L.MPPI_E_ARG
    assert lib.mppi_device_stats(None, ctypes.byref(p), None, None) == L.MPPI_E_ARG
    assert b"mppi_device_stats" in lib.mppi_last_error()
    assert lib.mppi_stats_eval(None, 1, c, None, ctypes.byref(st), None, None) == L.MPPI_E_ARG
    assert b"mppi_stats_eval" in lib.mppi_last_error()
