"""The control-cost term on the host (mppi_set_control_cost; no GPU needed): the float64 reference's precision matrix
and edge rules, the four C entries' prototypes and NULL-handle paths, MPPIModel's argument check, and the host form of
the fp32 rule for lin (csrc/control_cost.h) as a stand-alone program under AddressSanitizer +
UndefinedBehaviorSanitizer, held to the bound the kernel is held to (tests/test_gpu_control_cost.py):
|lin_f32 - lin_f64| <= 8 u A with u = 2^-24 and A the absolute-value majorant of lin."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import PKG, REPO

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
U32 = 2.0 ** -24
ENTRIES = ("mppi_set_control_cost", "mppi_get_control_cost", "mppi_get_control_term", "mppi_control_term_eval")
HS, RHOS, SIGMAS = (1, 2, 7, 17), (0.0, 0.3, 0.6, 0.95), (0.0, 0.2, 1.0, 3.0)


# ------------------------------------------------------------------------------------------ the float64 reference

@pytest.mark.parametrize("H", HS)
def test_precision_matrix_inverts_the_ar1_covariance(H):
    from mppi_hip.stats import ar1_precision
    t = np.arange(H)
    for rho in RHOS:
        C = rho ** np.abs(t[:, None] - t[None, :]) if rho > 0.0 else np.eye(H)
        P = ar1_precision(H, rho)
        assert np.max(np.abs(P @ C - np.eye(H))) <= 1e-13, (H, rho)
        np.testing.assert_allclose(P, np.linalg.inv(C), rtol=0.0, atol=1e-12 * np.abs(P).max())
        assert np.array_equal(P, np.triu(np.tril(P, 1), -1))  # tridiagonal
    assert ar1_precision(1, 0.6).tolist() == [[1.0]]
    for bad in ((0, 0.5), (3, 1.0), (3, -0.1), (3, float("nan"))):
        with pytest.raises(ValueError):
            ar1_precision(*bad)


def test_reference_edge_rules_and_argument_errors():
    from mppi_hip.stats import ar1_precision, control_term_ref
    rs = np.random.RandomState(3)
    B, nu, H, K = 2, 3, 7, 11
    U, e = rs.randn(B, nu, H), rs.randn(B, nu, H, K)
    sig = np.array([0.5, 2.0, 0.25])
    term, lin, A = control_term_ref(U, e, sig, 0.0, 1.5)  # rho = 0: gamma U / sigma^2
    np.testing.assert_allclose(lin, 1.5 * U / sig[None, :, None] ** 2, rtol=1e-15)
    np.testing.assert_allclose(A, np.abs(lin), rtol=1e-15)
    np.testing.assert_allclose(term, np.einsum("buh,buhk->bk", lin, e), rtol=1e-13)
    term, lin, A = control_term_ref(U, e, sig, 0.6, 1.5)  # the definition, row by row
    P = ar1_precision(H, 0.6)
    for b in range(B):
        for u in range(nu):
            np.testing.assert_allclose(lin[b, u], 1.5 / sig[u] ** 2 * (P @ U[b, u]), rtol=1e-13)
            np.testing.assert_allclose(A[b, u], 1.5 / sig[u] ** 2 * (np.abs(P) @ np.abs(U[b, u])), rtol=1e-13)
    assert np.all(np.abs(lin) <= A * (1 + 1e-15))
    term0, lin0, A0 = control_term_ref(U, e, [0.5, 0.0, 0.25], 0.6, 1.5)  # a frozen actuator: lin 0, no NaN
    assert np.all(lin0[:, 1] == 0.0) and np.all(A0[:, 1] == 0.0) and np.all(np.isfinite(term0))
    assert np.array_equal(lin0[:, 0], lin[:, 0]) and np.array_equal(lin0[:, 2], lin[:, 2])
    e_bad = e.copy()  # a non-finite noise entry makes ITS sample's term non-finite, on a lin == 0 row too (0 * inf)
    e_bad[:, 1, 2, 4], e_bad[0, 0, 1, 3] = np.inf, np.inf
    t_bad = control_term_ref(U, e_bad, [0.5, 0.0, 0.25], 0.6, 1.5)[0]
    hit = np.zeros((B, K), bool)
    hit[:, 4], hit[0, 3] = True, True
    assert not np.isfinite(t_bad[hit]).any() and np.array_equal(t_bad[~hit], term0[~hit])
    t1, l1, _ = control_term_ref(U[0], e[0], 0.5, 0.6, 1.5)  # one solve, a scalar sigma
    assert t1.shape == (K,) and l1.shape == (nu, H)
    np.testing.assert_allclose(l1, control_term_ref(U[:1], e[:1], [0.5] * 3, 0.6, 1.5)[1][0], rtol=1e-15)
    assert np.all(control_term_ref(U, e, sig, 0.6, 0.0)[0] == 0.0)  # gamma = 0
    tH1, lH1, _ = control_term_ref(U[:, :, :1], e[:, :, :1], sig, 0.9, 2.0)  # H = 1: P = [1] whatever rho is
    np.testing.assert_allclose(lH1, 2.0 * U[:, :, :1] / sig[None, :, None] ** 2, rtol=1e-15)
    nan, inf = float("nan"), float("inf")
    for bad in ((U, e, sig, 0.6, -1.0), (U, e, sig, 0.6, nan), (U, e, sig, 0.6, inf), (U, e, sig, 1.0, 1.0),
                (U, e, sig, -0.1, 1.0), (U, e, sig, nan, 1.0), (U, e, [0.5, -1.0, 0.25], 0.6, 1.0),
                (U, e, [0.5, nan, 0.25], 0.6, 1.0), (U, e, [0.5, 0.25], 0.6, 1.0), (U, e[:, :, :3], sig, 0.6, 1.0),
                (U, e[0], sig, 0.6, 1.0), (U[0, 0], e[0, 0], sig, 0.6, 1.0)):
        with pytest.raises(ValueError):
            control_term_ref(*bad)


# ------------------------------------------------------------------------------------------ the ABI

def test_ctypes_prototypes_and_null_handles():
    from mppi_hip import _lib as L
    lib = L.load()
    for name, nargs in zip(ENTRIES, (2, 2, 4, 6)):
        assert name in L.EXPORTED
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == nargs, name
    out = np.zeros(4, np.float32)
    p = out.ctypes.data_as(ctypes.c_void_p)
    calls = (lambda: lib.mppi_set_control_cost(None, ctypes.c_float(1.0)), lambda: lib.mppi_get_control_cost(None, None),
             lambda: lib.mppi_get_control_term(None, 1, p, p), lambda: lib.mppi_control_term_eval(None, 1, p, p, p, p))
    for name, call in zip(ENTRIES, calls):
        assert call() == L.MPPI_E_ARG, name
        assert name.encode() in lib.mppi_last_error(), name
    assert lib.mppi_abi_version() == 4  # additive


def test_header_declares_the_entries_and_the_engine_wraps_them():
    text = open(os.path.join(REPO, "include", "mppi.h")).read()
    for name in ENTRIES:
        assert f"int {name}(mppi_handle*" in text, name
    assert "#define MPPI_ABI_VERSION 4" in text and '"ctrl_cost"' in text
    from mppi_hip import Engine, control_term_ref  # noqa: F401  (exported)
    for name in ("set_control_cost", "control_cost", "control_term", "control_term_eval"):
        assert callable(getattr(Engine, name))
    jl = open(os.path.join(PKG, "julia", "MPPIHip.jl")).read()
    for name in ENTRIES:
        assert f":{name}" in jl, name


# ------------------------------------------------------------------------------------------ MPPIModel

class _Recorder:
    """Stands in for Engine: records the calls MPPIModel's constructor makes."""
    calls = []

    def __init__(self, config, device=0):
        self.config = config
        type(self).calls = []

    def __getattr__(self, name):
        def call(*a, **kw):
            type(self).calls.append((name, a))
            return self
        return call


def test_mppimodel_argument_checks(monkeypatch):
    from mppi_hip import controller
    monkeypatch.setattr(controller.Config, "preset", classmethod(lambda cls, name, **kw: cls(nx=4, nu=1, H=8, K=16)))
    monkeypatch.setattr(controller, "Engine", _Recorder)
    for bad in (-0.1, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError):
            controller.MPPIModel(control_cost=bad)
    controller.MPPIModel()  # the default asks for nothing
    assert not [c for c in _Recorder.calls if c[0] == "set_control_cost"]
    m = controller.MPPIModel(control_cost=0.75)
    assert [c for c in _Recorder.calls if c[0] == "set_control_cost"] == [("set_control_cost", (0.75,))]
    assert m.control_cost == 0.75


# ------------------------------------------------------------------------------------------ the fp32 rule on the host

@pytest.fixture(scope="module")
def host_rule(tmp_path_factory):
    """tests/native/control_cost_host.cpp (its own main; includes csrc/control_cost.h) built host-only with ASan +
    UBSan and run directly, as tests/test_ess_target.py builds ess_target_host.cpp.
    host_rule(U [rows, H] f32, gamma, sigma, rho) -> lin [rows, H] f32."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    d = tmp_path_factory.mktemp("control_cost")
    exe = str(d / "control_cost_host")
    cmd = [HIPCC, "-x", "hip", "--offload-host-only", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address",
           "-Xarch_host", "-fsanitize=undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           f"-I{REPO}/include", f"-I{PKG}/csrc", os.path.join(REPO, "tests", "native", "control_cost_host.cpp"),
           "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    count = [0]

    def run(U, gamma, sigma, rho):
        U = np.ascontiguousarray(U, np.float32)
        count[0] += 1
        path = d / f"U_{count[0]}.f32"
        U.tofile(path)
        r = subprocess.run([exe, str(path), str(U.shape[0]), str(U.shape[1])] +
                           [float(np.float32(v)).hex() for v in (gamma, sigma, rho)],
                           capture_output=True, text=True, timeout=240, env=env)
        assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
        rows = [[np.float32(float.fromhex(x)) for x in ln.split()] for ln in r.stdout.strip().splitlines()]
        assert len(rows) == U.shape[0] and all(len(x) == U.shape[1] for x in rows)
        return np.array(rows, np.float32)
    return run


@pytest.mark.parametrize("H", HS)
def test_host_form_of_the_rule_under_asan_ubsan(host_rule, H):
    """lin on the (H, rho, sigma) grid against float64 at 8 u A, with U rows of mixed sign and scale (the
    cancellation inside P U), rows of one value (the interior of P U nearly cancels at rho near 1) and a zero row."""
    from mppi_hip.stats import control_term_ref
    rs = np.random.RandomState(100 + H)
    U = np.concatenate([rs.randn(6, H), 1e3 * rs.randn(2, H), np.ones((1, H)), np.zeros((1, H)),
                        rs.randn(2, H) * 10.0 ** rs.uniform(-3, 3, (2, H))]).astype(np.float32)
    gamma = np.float32(0.7)
    e = np.zeros(U.shape + (1,))
    worst = 0.0
    for rho in RHOS:
        for sigma in SIGMAS:
            got = host_rule(U, gamma, sigma, rho)
            s64, r64 = float(np.float32(sigma)), float(np.float32(rho))
            _, want, A = control_term_ref(U[:, None, :], e[:, None], s64, r64, float(gamma))
            want, A = want[:, 0], A[:, 0]
            if sigma == 0.0:
                assert np.all(got == 0.0) and not np.any(np.signbit(got) & (got != 0))
                continue
            assert np.all(np.isfinite(got))
            err = np.abs(got.astype(np.float64) - want)
            assert np.all(err <= 8 * U32 * A), (H, rho, sigma, float((err / np.maximum(A, 1e-300)).max() / U32))
            worst = max(worst, float((err[A > 0] / A[A > 0]).max() / U32)) if np.any(A > 0) else worst
            assert np.all(got[A == 0.0] == 0.0)
    print(f"H={H}: worst |lin_f32 - lin_f64| / (u A) = {worst:.3g} (bound 8)")


def test_host_form_edge_rules(host_rule):
    U = np.array([[1.0, -2.0, 3.0]], np.float32)
    np.testing.assert_array_equal(host_rule(U, 2.0, 0.5, 0.0), np.float32(8.0) * U)  # rho = 0: gamma U / sigma^2, exact here
    assert np.all(host_rule(U, 0.0, 0.5, 0.6) == 0.0)                                # gamma = 0
    assert np.all(host_rule(U, 2.0, 1e-30, 0.6) == 0.0)                              # sigma^2 underflows: no coefficient
    one = host_rule(np.array([[3.0]], np.float32), 2.0, 0.5, 0.9)                    # H = 1: P = [1]
    assert one.tolist() == [[24.0]]
