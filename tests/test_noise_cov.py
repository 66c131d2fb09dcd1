"""The cross-actuator sampling covariance on the host (mppi_set_noise_cov; no GPU needed): mppi_hip.noise.cov_factor /
cov_mix / cov_filter against the header csrc/noise_cov.h through g++ (bitwise), the law's empirical covariance, the
control-cost coefficients under the law (csrc/control_cost.h ctrl_lin_cov_entry) against their float64 restatement, the
NULL-handle paths of the C ABI, and tests/native/noise_cov_host.cpp as a stand-alone program under AddressSanitizer +
UndefinedBehaviorSanitizer."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import PKG, REPO
from cov_cases import B, HS, K, NUS, RHOS, bits, sigma_of
from philox_ref import device_noise

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
U32 = 2.0 ** -24
SRC = os.path.join(REPO, "tests", "native", "noise_cov_host.cpp")
ENTRIES = ("mppi_set_noise_cov", "mppi_get_noise_cov")


def _rows(lines, n):
    return np.array([[float.fromhex(x) for x in ln.split()] for ln in lines[:n]], np.float64).astype(np.float32)


class _Host:
    """the program's three modes on numpy arrays"""

    def __init__(self, exe, d, env=None):
        self.exe, self.d, self.env, self.n = exe, d, env, 0

    def _file(self, a):
        self.n += 1
        path = str(self.d / f"a{self.n}.f32")
        np.ascontiguousarray(a, np.float32).tofile(path)
        return path

    def _run(self, *args):
        r = subprocess.run([self.exe, *[str(a) for a in args]], capture_output=True, text=True, timeout=240,
                           env=self.env)
        assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
        return r.stdout.strip().splitlines()

    def factor(self, S):
        """-> (L, Sinv, sigma_u) float32, or None where the header refuses Sigma"""
        nu = S.shape[0]
        out = self._run("factor", nu, self._file(S))
        if out[0] != "ok":
            assert out[0] == "refused"
            return None
        return _rows(out[1:], nu), _rows(out[1 + nu:], nu), _rows(out[1 + 2 * nu:], 1)[0]

    def mix(self, L, e):
        """e [nu, n] -> eps [nu, n]"""
        nu, n = e.shape
        return _rows(self._run("mix", nu, n, self._file(L), self._file(e)), nu)

    def lin(self, Sinv, U, gamma, rho):
        """U [nu, H] -> lin [nu, H]"""
        nu, H = U.shape
        args = [float(np.float32(gamma)).hex(), float(np.float32(rho)).hex()]
        return _rows(self._run("lin", nu, H, *args, self._file(Sinv), self._file(U)), nu)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """tests/native/noise_cov_host.cpp through g++ (as tests/test_noise_knots.py builds its harness)"""
    d = tmp_path_factory.mktemp("noise_cov")
    exe = str(d / "noise_cov_host")
    r = subprocess.run(["g++", "-O2", "-I", os.path.join(PKG, "csrc"), SRC, "-o", exe], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.fail(r.stderr)
    return _Host(exe, d)


# ---- 1. the factor

@pytest.mark.parametrize("nu", NUS)
def test_cov_factor_matches_the_header_bitwise(host, nu):
    from mppi_hip.noise import cov_factor
    S = sigma_of(nu)
    L = cov_factor(S)
    got_L, got_Sinv, got_sig = host.factor(S)
    assert L.dtype == np.float32 and L.shape == (nu, nu)
    assert np.array_equal(bits(got_L), bits(L))
    assert not np.any(np.triu(L, 1)) and not np.any(np.signbit(np.triu(L, 1)))  # exactly +0 above the diagonal
    L64, S64 = L.astype(np.float64), S.astype(np.float64)
    err = float(np.abs(L64 @ L64.T - S64).max())
    print(f"nu {nu}: max |L L^T - Sigma| = {err:.3g} (bound {1e-6 * np.abs(S64).max():.3g})")
    assert err <= 1e-6 * np.abs(S64).max()
    assert np.array_equal(bits(got_sig), bits(np.sqrt(np.diag(S64)).astype(np.float32)))
    inv = np.linalg.inv(S64)
    assert np.array_equal(got_Sinv, got_Sinv.T)
    assert np.abs(got_Sinv - inv).max() <= 1e-5 * np.linalg.cond(S64) * np.abs(inv).max()


def test_cov_factor_refuses_what_the_header_refuses(host):
    from mppi_hip.noise import cov_factor
    S = sigma_of(3)
    bad = []
    for i, v in (((2, 2), np.nan), ((0, 0), np.inf), ((1, 1), 0.0), ((0, 0), -S[0, 0])):
        M = S.copy()
        M[i] = v
        bad.append(M)
    M = S.copy()
    M[0, 1] = np.nextafter(M[0, 1], np.float32(10))  # asymmetric by one ulp
    bad.append(M)
    bad.append(np.float32([[1, 2, 0], [2, 1, 0], [0, 0, 1]]))  # indefinite
    bad.append(np.float32([[1, 1], [1, 1]]))                     # semidefinite: the second pivot is 0
    for M in bad:
        assert host.factor(M) is None, M
        with pytest.raises(ValueError):
            cov_factor(M)
    with pytest.raises(ValueError):
        cov_factor(np.ones((2, 3), np.float32))


# ---- 2. the mix

@pytest.mark.parametrize("nu", NUS)
def test_cov_mix_matches_the_header_bitwise(host, nu):
    from mppi_hip.noise import cov_factor, cov_mix
    rs = np.random.RandomState(40 + nu)
    n = 96
    e = (rs.randn(nu, n) * 10.0 ** rs.uniform(-2, 2, (nu, n))).astype(np.float32)
    L = cov_factor(sigma_of(nu))
    want = cov_mix(e.reshape(nu, 1, n), L).reshape(nu, n)
    assert want.dtype == np.float32
    assert np.array_equal(bits(host.mix(L, e)), bits(want))
    if nu == 1:
        assert np.array_equal(bits(want), bits(L[0, 0] * e))
    eye = np.eye(nu, dtype=np.float32)
    assert np.array_equal(cov_mix(e.reshape(nu, 1, n), eye).reshape(nu, n), e)
    assert np.array_equal(host.mix(eye, e), e)
    # a batch axis in front, and only the lower triangle is read
    e4 = rs.randn(2, nu, 3, 5).astype(np.float32)
    full = cov_mix(e4, L)
    assert np.array_equal(bits(full[1]), bits(cov_mix(e4[1], L)))
    assert np.array_equal(bits(cov_mix(e4, L + np.triu(np.ones_like(L), 1))), bits(full))


def test_cov_filter_is_the_mix_of_the_ar1_rows():
    from mppi_hip.noise import ar1_filter_f32, cov_factor, cov_filter, cov_mix
    rs = np.random.RandomState(5)
    z = rs.randn(2, 3, 7, 11).astype(np.float32)
    S = sigma_of(3)
    L = cov_factor(S)
    for rho in RHOS:
        want = cov_mix(ar1_filter_f32(z, rho), L)
        assert np.array_equal(bits(cov_filter(z, S, rho)), bits(want))  # Sigma: factored
        assert np.array_equal(bits(cov_filter(z, L, rho)), bits(want))  # lower-triangular: the factor itself
    assert np.array_equal(cov_filter(z, np.eye(3, dtype=np.float32), 0.0), z)
    D = np.diag(np.float32([0.25, 4.0, 0.0625]))  # a diagonal matrix reads as L unless told otherwise
    assert np.array_equal(cov_filter(z, D, 0.0), np.float32([0.25, 4.0, 0.0625])[:, None, None] * z)
    assert np.array_equal(cov_filter(z, D, 0.0, is_factor=False), np.float32([0.5, 2.0, 0.25])[:, None, None] * z)
    with pytest.raises(ValueError):
        cov_filter(z, S, 1.0)
    with pytest.raises(ValueError):
        cov_filter(z, np.ones((3, 2), np.float32))


# ---- 3. the law is the law

def _worst_deviation(eps, S):
    """max over (u, v) of |C[u][v] - Sigma[u][v]| in standard deviations sqrt((S_uu S_vv + S_uv^2) / N) of the
    empirical second moment C of N zero-mean draws; eps [B, nu, H, K]"""
    nu = eps.shape[1]
    x = np.moveaxis(np.asarray(eps, np.float64), 1, 0).reshape(nu, -1)
    N = x.shape[1]
    C = x @ x.T / N
    S = np.asarray(S, np.float64)
    d = np.diag(S)
    sd = np.sqrt((d[:, None] * d[None, :] + S * S) / N)
    return float((np.abs(C - S) / sd).max()), N


@pytest.mark.parametrize("nu", NUS)
def test_the_law_has_the_covariance_it_was_given(nu):
    from mppi_hip.noise import cov_factor, cov_filter
    H = 9
    z = device_noise(0xC0FFEE + nu, B, nu, H, K, 1.0).astype(np.float32)  # the Philox normals the device draws
    S = sigma_of(nu)
    L = cov_factor(S)
    worst, N = _worst_deviation(cov_filter(z, S, 0.0, is_factor=False), S)
    print(f"nu {nu}: worst |C - Sigma| = {worst:.2f} standard deviations (bound 6; N = {N})")
    assert N == 2340 and worst <= 6.0
    if nu > 1:  # a transposed factor has another covariance: the same check must catch it
        wrong = np.einsum("vu,bvtk->butk", L.astype(np.float64), z.astype(np.float64))
        flipped, _ = _worst_deviation(wrong, S)
        print(f"nu {nu}: with L^T {flipped:.1f} standard deviations")
        assert flipped > 6.0


# ---- 4. the control-cost coefficients under the law

@pytest.mark.parametrize("nu", NUS)
def test_lin_in_cov_form_against_float64(host, nu):
    from mppi_hip.stats import control_term_ref
    S = sigma_of(nu)
    _, Sinv, _ = host.factor(S)  # the fp32 inverse both sides use
    gamma = np.float32(0.7)
    rs = np.random.RandomState(300 + nu)
    worst = 0.0
    for H in HS + (17,):
        U = np.concatenate([rs.randn(nu, H)[None], (rs.randn(nu, H) * 10.0 ** rs.uniform(-3, 3, (nu, H)))[None],
                            np.ones((1, nu, H))]).astype(np.float32)
        e = np.zeros(U.shape + (1,))
        for rho in RHOS + (0.3,):
            r64 = float(np.float32(rho))
            _, want, A = control_term_ref(U, e, None, r64, float(gamma), Sinv=Sinv)
            for b in range(U.shape[0]):
                got = host.lin(Sinv, U[b], gamma, rho)
                assert np.all(np.isfinite(got))
                err = np.abs(got.astype(np.float64) - want[b])
                ratio = float((err[A[b] > 0] / A[b][A[b] > 0]).max() / U32)
                worst = max(worst, ratio)
                assert np.all(err <= (nu + 8) * U32 * A[b]), (nu, H, rho, b, ratio)
    print(f"nu {nu}: worst |lin_f32 - lin_f64| / (u A) = {worst:.3g} (bound {nu + 8})")


def test_lin_reference_with_a_diagonal_inverse_is_the_per_actuator_form():
    from mppi_hip.stats import control_term_ref
    rs = np.random.RandomState(8)
    Bn, nu, H, Kn = 2, 3, 7, 5
    U, e = rs.randn(Bn, nu, H), rs.randn(Bn, nu, H, Kn)
    sig = np.array([0.5, 0.25, 2.0])
    for rho in (0.0, 0.6):
        t0, l0, a0 = control_term_ref(U, e, sig, rho, 1.5)
        t1, l1, a1 = control_term_ref(U, e, None, rho, 1.5, Sinv=np.diag(1.0 / sig ** 2))
        np.testing.assert_allclose(l1, l0, rtol=1e-14, atol=0)
        np.testing.assert_allclose(a1, a0, rtol=1e-14, atol=0)
        np.testing.assert_allclose(t1, t0, rtol=1e-12, atol=1e-12)
    t0, l0, a0 = control_term_ref(U, e, sig, 0.6, 1.5)  # the default is today's behaviour, exactly
    t2, l2, a2 = control_term_ref(U, e, sig, 0.6, 1.5, Sinv=None)
    assert np.array_equal(l0, l2) and np.array_equal(a0, a2) and np.array_equal(t0, t2)
    for bad in (np.eye(2), np.full((3, 3), np.nan)):
        with pytest.raises(ValueError):
            control_term_ref(U, e, sig, 0.6, 1.5, Sinv=bad)


# ---- 5. the C ABI without a device

def test_ctypes_prototypes_and_null_handles():
    from mppi_hip import _lib as L
    lib = L.load()
    for name, nargs in zip(ENTRIES, (2, 5)):
        assert name in L.EXPORTED
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == nargs, name
    buf = np.eye(3, dtype=np.float32)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    active = ctypes.c_int(7)
    assert lib.mppi_set_noise_cov(None, p) == L.MPPI_E_ARG
    assert b"mppi_set_noise_cov" in lib.mppi_last_error()
    assert lib.mppi_set_noise_cov(None, None) == L.MPPI_E_ARG
    assert lib.mppi_get_noise_cov(None, p, p, p, ctypes.byref(active)) == L.MPPI_E_ARG
    assert b"mppi_get_noise_cov" in lib.mppi_last_error()
    assert lib.mppi_get_noise_cov(None, None, None, None, None) == L.MPPI_E_ARG
    assert active.value == 7 and np.array_equal(buf, np.eye(3, dtype=np.float32))
    assert lib.mppi_abi_version() == 4  # additive


def test_header_declares_the_entries_and_the_wrappers_exist():
    text = open(os.path.join(REPO, "include", "mppi.h")).read()
    for name in ENTRIES:
        assert f"int {name}(mppi_handle*" in text, name
    assert "#define MPPI_ABI_VERSION 4" in text
    from mppi_hip import Engine
    for name in ("set_noise_cov", "noise_cov"):
        assert callable(getattr(Engine, name))
    jl = open(os.path.join(PKG, "julia", "MPPIHip.jl")).read()
    for name in ENTRIES:
        assert f":{name}" in jl, name


# ---- the stand-alone program under the sanitizers

def test_host_program_under_asan_ubsan(tmp_path):
    """tests/native/noise_cov_host.cpp (its own main) built host-only with ASan + UBSan and run directly, as
    tests/test_control_cost.py builds control_cost_host.cpp: its own checks of the factor, the mix and lin on the shared
    cases, and one call of every mode the bitwise tests use."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "noise_cov_host")
    cmd = [HIPCC, "-x", "hip", "--offload-host-only", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address",
           "-Xarch_host", "-fsanitize=undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           f"-I{REPO}/include", f"-I{PKG}/csrc", SRC, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, "self"], capture_output=True, text=True, timeout=240, env=env)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.stdout + r.stderr)[-3000:]
    from mppi_hip.noise import cov_factor, cov_mix
    san = _Host(exe, tmp_path, env)
    for nu in NUS:  # clang's host build gives the bits of the numpy restatements too
        S = sigma_of(nu)
        L, Sinv, _ = san.factor(S)
        assert np.array_equal(bits(L), bits(cov_factor(S)))
        e = np.random.RandomState(nu).randn(nu, 7).astype(np.float32)
        assert np.array_equal(bits(san.mix(L, e)), bits(cov_mix(e.reshape(nu, 1, 7), L).reshape(nu, 7)))
        assert san.lin(Sinv, e, 0.7, 0.9).shape == (nu, 7)
    assert san.factor(np.float32([[1, 2], [2, 1]])) is None
