"""The control-rate cost term on the host (mppi_set_rate_cost; no GPU needed): the float64 reference's exact cases and
edge rules, the six C entries' prototypes and NULL-handle paths, MPPIModel's argument check, and the host form of the
fp32 rule (csrc/rate_cost.h) as a stand-alone program built with g++, held to the bound the kernel is held to
(tests/test_gpu_rate_cost.py): with u = 2^-24 and n = nu (H - t0) summands, all non-negative,
|term_f32 - term_f64| <= (n + 4) u / (1 - (n + 4) u) * term_f64 -- one rounding for d, one for q = r d, one per fma,
in any summation order; v = U + eps is formed in fp32 on both sides, so it carries no error."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import PKG, REPO

CXX = shutil.which("g++") or shutil.which("c++")
U32 = 2.0 ** -24
ENTRIES = ("mppi_set_rate_cost", "mppi_get_rate_cost", "mppi_set_prev_control", "mppi_get_prev_control",
           "mppi_get_rate_term", "mppi_rate_term_eval")


def bound(n, term64):
    g = (n + 4) * U32
    return g / (1.0 - g) * term64


# ------------------------------------------------------------------------------------------ the float64 reference

def test_reference_exact_cases():
    from mppi_hip.stats import rate_term_ref
    U = np.full((2, 3, 5), 0.75, np.float32)
    assert np.all(rate_term_ref(U, np.zeros((2, 3, 5, 4), np.float32), [1.0, 2.0, 0.5]) == 0.0)  # constant U, no anchor
    U2, e2 = np.zeros((1, 2), np.float32), np.array([[[0.0], [3.0]]], np.float32)  # nu = 1, H = 2, K = 1
    assert rate_term_ref(U2, e2, 2.0).tolist() == [18.0]
    assert rate_term_ref(U2, e2, 2.0, u_prev=[1.0]).tolist() == [20.0]
    assert rate_term_ref(U2, e2, 2.0, ctrl_clamp=1.0).tolist() == [2.0]  # v = [0, 1]
    assert rate_term_ref(U2, e2, 2.0, u_prev=[1.0], ctrl_clamp=1.0).tolist() == [4.0]  # u_prev is not clamped again
    assert np.all(rate_term_ref(np.ones((3, 1)), np.random.RandomState(0).randn(3, 1, 6), [1.0, 2.0, 3.0]) == 0.0)  # H = 1
    one = rate_term_ref(np.ones((3, 1)), np.zeros((3, 1, 6)), [1.0, 2.0, 3.0], u_prev=[0.0, 1.0, 3.0])
    assert one.tolist() == [1.0 + 0.0 + 12.0] * 6  # H = 1 with the anchor: r (U - u_prev)^2


def test_reference_definition_edge_rules_and_argument_errors():
    from mppi_hip.stats import rate_term_ref
    rs = np.random.RandomState(3)
    B, nu, H, K = 2, 3, 7, 11
    U, e = rs.randn(B, nu, H).astype(np.float32), rs.randn(B, nu, H, K).astype(np.float32)
    r, up = np.array([0.5, 0.0, 2.0]), rs.randn(B, nu).astype(np.float32)
    for clamp in (0.0, 0.8):
        v = (U[..., None] + e).astype(np.float32)
        v = (np.clip(v, -clamp, clamp) if clamp > 0 else v).astype(np.float64)
        d = np.diff(v, axis=2)
        free = np.einsum("u,buhk->bk", r, d * d)
        np.testing.assert_allclose(rate_term_ref(U, e, r, ctrl_clamp=clamp), free, rtol=1e-13)
        d0 = v[:, :, 0] - up.astype(np.float64)[:, :, None]
        np.testing.assert_allclose(rate_term_ref(U, e, r, u_prev=up, ctrl_clamp=clamp),
                                   free + np.einsum("u,buk->bk", r, d0 * d0), rtol=1e-13)
    t1 = rate_term_ref(U[0], e[0], 0.5)  # one solve, a scalar weight
    assert t1.shape == (K,)
    np.testing.assert_allclose(t1, rate_term_ref(U[:1], e[:1], [0.5] * 3)[0], rtol=1e-15)
    # a non-finite entry makes ITS sample's term non-finite: on an r == 0 row, at an unanchored t = 0, under a clamp
    bad = e.copy()
    bad[:, 1, 2, 4], bad[0, 0, 0, 3], bad[1, 2, 6, 9] = np.inf, np.nan, -np.inf
    hit = np.zeros((B, K), bool)
    hit[:, 4], hit[0, 3], hit[1, 9] = True, True, True
    for kw in ({}, {"ctrl_clamp": 0.8}, {"u_prev": up}, {"u_prev": up, "ctrl_clamp": 0.8}):
        t_bad, t_ok = rate_term_ref(U, bad, r, **kw), rate_term_ref(U, e, r, **kw)
        assert not np.isfinite(t_bad[hit]).any() and np.array_equal(t_bad[~hit], t_ok[~hit]), kw
    h1 = e[:, :, :1].copy()  # H = 1 without the anchor: 0 -- and still non-finite for a non-finite row
    h1[0, 1, 0, 2] = np.inf
    th1 = rate_term_ref(U[:, :, :1], h1, r)
    assert np.isnan(th1[0, 2]) and np.all(np.delete(th1.ravel(), 2) == 0.0)
    nan, inf = float("nan"), float("inf")
    for args in ((U, e, [0.5, -1.0, 2.0]), (U, e, [0.5, nan, 2.0]), (U, e, [0.5, inf, 2.0]), (U, e, [0.5, 2.0]),
                 (U, e[:, :, :3], r), (U, e[0], r), (U[0, 0], e[0, 0], r)):
        with pytest.raises(ValueError):
            rate_term_ref(*args)
    with pytest.raises(ValueError):
        rate_term_ref(U, e, r, u_prev=np.zeros((B, nu + 1)))


# ------------------------------------------------------------------------------------------ the ABI

def test_ctypes_prototypes_and_null_handles():
    from mppi_hip import _lib as L
    lib = L.load()
    for name, nargs in zip(ENTRIES, (3, 4, 3, 3, 3, 6)):
        assert name in L.EXPORTED
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == nargs, name
    out = np.zeros(4, np.float32)
    p, fp = out.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(L._fp)
    calls = (lambda: lib.mppi_set_rate_cost(None, fp, 1), lambda: lib.mppi_get_rate_cost(None, fp, None, None),
             lambda: lib.mppi_set_prev_control(None, 1, p), lambda: lib.mppi_get_prev_control(None, 1, p),
             lambda: lib.mppi_get_rate_term(None, 1, p), lambda: lib.mppi_rate_term_eval(None, 1, p, p, None, p))
    for name, call in zip(ENTRIES, calls):
        assert call() == L.MPPI_E_ARG, name
        assert name.encode() in lib.mppi_last_error(), name
    assert lib.mppi_abi_version() == 4  # additive


def test_header_declares_the_entries_and_the_engine_wraps_them():
    text = open(os.path.join(REPO, "include", "mppi.h")).read()
    for name in ENTRIES:
        assert f"int {name}(mppi_handle*" in text, name
    assert "#define MPPI_ABI_VERSION 4" in text and '"rate_cost"' in text
    from mppi_hip import Engine, rate_term_ref  # noqa: F401  (exported)
    for name in ("set_rate_cost", "rate_cost", "set_prev_control", "prev_control", "rate_term", "rate_term_eval"):
        assert callable(getattr(Engine, name))
    jl = open(os.path.join(PKG, "julia", "MPPIHip.jl")).read()
    for name in ENTRIES:
        assert f":{name}" in jl, name


# ------------------------------------------------------------------------------------------ MPPIModel

class _Recorder:
    """Stands in for Engine: records the calls MPPIModel and the controller functions make."""
    calls = []

    def __init__(self, config, device=0):
        self.config = config
        type(self).calls = []

    def solve(self, x0, U, **kw):
        from mppi_hip.engine import SolveResult
        type(self).calls.append(("solve", ()))
        c = self.config
        U = np.asarray(U, np.float32).reshape(c.nu, c.H)
        return SolveResult(U=U, u0=np.full(c.nu, 0.25, np.float32), costs=np.zeros(c.K, np.float32),
                           weights=np.zeros(c.K, np.float32), status=0, stats=None)

    def __getattr__(self, name):
        def call(*a, **kw):
            type(self).calls.append((name, a))
            return self
        return call


def _named(name):
    return [c for c in _Recorder.calls if c[0] == name]


def test_mppimodel_argument_checks_and_the_previous_control(monkeypatch):
    from mppi_hip import controller
    monkeypatch.setattr(controller.Config, "preset", classmethod(lambda cls, name, **kw: cls(nx=4, nu=2, H=8, K=16)))
    made = []
    real_init = _Recorder.__init__
    monkeypatch.setattr(_Recorder, "__init__", lambda self, *a, **kw: (made.append(1), real_init(self, *a, **kw))[1])
    monkeypatch.setattr(controller, "Engine", _Recorder)
    nan, inf = float("nan"), float("inf")
    for bad in (-0.1, nan, inf, 0.0, [0.0, 0.0], [1.0, -1.0], [1.0, nan], [1.0, 2.0, 3.0], [], "x"):
        with pytest.raises(ValueError):
            controller.MPPIModel(rate_cost=bad)
    assert not made, "every refusal comes ahead of the engine's creation"
    data = controller.SimData(qpos=np.zeros(2), qvel=np.zeros(2), ctrl=np.array([0.5, -0.5]))
    m = controller.MPPIModel()  # the default asks for nothing, before a solve and around it
    assert m.rate_cost is None and not _named("set_rate_cost")
    controller.mppi_step(m, data)
    controller.mppi_controller(m, data)
    assert [c[0] for c in _Recorder.calls if c[0] in ("set_rate_cost", "set_prev_control", "solve")] == ["solve"] * 2
    m = controller.MPPIModel(rate_cost=0.75)  # a scalar broadcasts, the anchor defaults to on
    (_, (r, anchor)), = _named("set_rate_cost")
    assert np.asarray(r).tolist() == [0.75, 0.75] and anchor is True
    data.ctrl[:] = [0.5, -0.5]
    controller.mppi_controller(m, data)  # data.ctrl, as the environment applied it, goes in ahead of the solve
    order = [c for c in _Recorder.calls if c[0] in ("set_prev_control", "solve")]
    assert [c[0] for c in order] == ["set_prev_control", "solve"]
    assert np.asarray(order[0][1][0]).tolist() == [0.5, -0.5] and np.asarray(order[0][1][0]).dtype == np.float32
    assert data.ctrl.tolist() == [0.25, 0.25]
    controller.mppi_step(m, data)
    assert np.asarray(_named("set_prev_control")[-1][1][0]).tolist() == [0.25, 0.25]
    m = controller.MPPIModel(rate_cost=[0.0, 2.0], rate_anchor=False)  # no anchor: no previous control is passed
    (_, (r, anchor)), = _named("set_rate_cost")
    assert np.asarray(r).tolist() == [0.0, 2.0] and anchor is False
    controller.mppi_controller(m, data)
    assert not _named("set_prev_control")


# ------------------------------------------------------------------------------------------ the fp32 rule on the host

@pytest.fixture(scope="module")
def host_rule(tmp_path_factory):
    """tests/native/rate_cost_host.cpp (its own main; includes csrc/rate_cost.h) built with g++ and run directly.
    host_rule(U [nu, H], eps [nu, H, K], r [nu], u_prev [nu] or None, clamp) -> term [K] f32."""
    if not CXX:
        pytest.skip("no C++ compiler")
    d = tmp_path_factory.mktemp("rate_cost")
    exe = str(d / "rate_cost_host")
    cmd = [CXX, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", f"-I{PKG}/csrc",
           os.path.join(REPO, "tests", "native", "rate_cost_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    count = [0]

    def run(U, eps, r, u_prev=None, clamp=0.0):
        U, eps = np.ascontiguousarray(U, np.float32), np.ascontiguousarray(eps, np.float32)
        nu, H, K = eps.shape
        up = np.zeros(nu, np.float32) if u_prev is None else np.asarray(u_prev, np.float32)
        count[0] += 1
        path = d / f"in_{count[0]}.f32"
        np.concatenate([U.ravel(), np.asarray(r, np.float32).ravel(), up.ravel(), eps.ravel()]).tofile(path)
        p = subprocess.run([exe, str(path), str(nu), str(H), str(K), str(int(u_prev is not None)),
                            float(np.float32(clamp)).hex()], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, (p.returncode, (p.stdout + p.stderr)[-3000:])
        out = np.array([np.float32(float.fromhex(x)) for x in p.stdout.split()], np.float32)
        assert out.shape == (K,)
        return out
    return run


def test_host_form_exact_cases(host_rule):
    U = np.full((3, 5), 0.75, np.float32)
    assert np.all(host_rule(U, np.zeros((3, 5, 4)), [1.0, 2.0, 0.5]) == 0.0)      # constant U, zero noise, no anchor
    U2, e2 = np.zeros((1, 2), np.float32), np.array([[[0.0], [3.0]]], np.float32)
    assert host_rule(U2, e2, [2.0]).tolist() == [18.0]                            # r (3 - 0)^2
    assert host_rule(U2, e2, [2.0], u_prev=[1.0]).tolist() == [20.0]              # + r (0 - 1)^2
    assert host_rule(U2, e2, [2.0], clamp=1.0).tolist() == [2.0]                  # v = [0, 1]
    e1 = np.random.RandomState(0).randn(3, 1, 6)
    assert np.all(host_rule(np.ones((3, 1)), e1, [1.0, 2.0, 3.0]) == 0.0)         # H = 1 without the anchor
    assert not np.any(np.signbit(host_rule(np.ones((3, 1)), e1, [1.0, 2.0, 3.0])))


@pytest.mark.parametrize("H", [1, 2, 7, 17])
def test_host_form_of_the_rule_meets_the_derived_bound(host_rule, H):
    """Random U, eps and u_prev of mixed scale, r with a zero entry, anchor on and off, ctrl_clamp off and binding on
    about a third of the elements; and the header's non-finite rule."""
    from mppi_hip.stats import rate_term_ref
    worst = 0.0
    for nu in (1, 3, 32):
        rs = np.random.RandomState(100 * H + nu)
        K = 9
        U = rs.randn(nu, H).astype(np.float32)
        eps = (rs.randn(nu, H, K) * 10.0 ** rs.uniform(-2, 1, (nu, 1, 1))).astype(np.float32)
        r = (0.2 + rs.rand(nu)).astype(np.float32)
        if nu > 1:
            r[1] = 0.0
        up = rs.randn(nu).astype(np.float32)
        clamp = float(np.float32(np.quantile(np.abs(U[..., None] + eps), 2.0 / 3.0)))
        for anchor in (False, True):
            for cl in (0.0, clamp):
                got = host_rule(U, eps, r, up if anchor else None, cl)
                want = rate_term_ref(U, eps, r.astype(np.float64), up if anchor else None, cl)
                n = nu * (H - (0 if anchor else 1))
                err = np.abs(got.astype(np.float64) - want)
                assert np.all(err <= bound(n, want)), (H, nu, anchor, cl, float((err / bound(n, want)).max()))
                if n == 0:
                    assert np.all(got == 0.0)
                elif np.any(want > 0):
                    worst = max(worst, float((err[want > 0] / bound(n, want)[want > 0]).max()))
        if H > 1 or nu > 1:  # a non-finite eps on any row: that sample alone
            bad = eps.copy()
            bad[min(1, nu - 1), 0, 2], bad[0, H - 1, 5] = np.inf, np.nan
            for cl in (0.0, clamp):
                got, ok = host_rule(U, bad, r, None, cl), host_rule(U, eps, r, None, cl)
                hit = np.zeros(K, bool)
                hit[[2, 5]] = True
                assert not np.isfinite(got[hit]).any(), (H, nu, cl)
                assert np.array_equal(got[~hit].view(np.uint32), ok[~hit].view(np.uint32)), (H, nu, cl)
    print(f"H={H}: worst |term_f32 - term_f64| / bound = {worst:.3g}")
