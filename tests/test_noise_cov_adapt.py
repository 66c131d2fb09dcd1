"""The covariance adapted from the cross moments, on the host (mppi_set_noise_cov_adapt; no GPU needed):
mppi_hip.stats.adapt_noise_cov_f32 against the header csrc/noise_cov_adapt.h through g++ (bitwise), the header's factor
against cov_factor of csrc/noise_cov.h (bitwise), the properties of the rule, its float64 statement, the NULL-handle
paths of the three entries, and tests/native/cross_adapt_host.cpp as a stand-alone program under AddressSanitizer +
UndefinedBehaviorSanitizer."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import PKG, REPO
from cross_cases import B, NUS, SRC, bits, build_host, case, host_cross, moments_like, rows, sigma_of

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
U32 = 2.0 ** -24
ENTRIES = ("mppi_set_noise_cov_adapt", "mppi_get_noise_cov_adapt", "mppi_get_noise_cov_law")
WIDE = (1e-3, 10.0)  # limits no case below reaches


class _Host:
    """the program's adapt and factor modes on numpy arrays"""

    def __init__(self, exe, d, env=None):
        self.exe, self.d, self.env = exe, d, env

    def _run(self, *args):
        r = subprocess.run([self.exe, *[str(a) for a in args]], capture_output=True, text=True, timeout=240,
                           env=self.env)
        return r.returncode, r.stdout.strip().splitlines(), r.stderr

    def adapt(self, S, mx, rate, lo, hi, n_finite=None):
        """-> (status word, Sigma, L, Sinv, sigma_u) as they stand after the step"""
        nu = S.shape[0]
        mx = np.ascontiguousarray(mx, np.float32).reshape(-1, nu, nu)
        nf = np.full(mx.shape[0], 5, np.int32) if n_finite is None else np.asarray(n_finite, np.int32)
        np.ascontiguousarray(S, np.float32).tofile(self.d / "S.f32")
        mx.tofile(self.d / "mx.f32")
        nf.tofile(self.d / "nf.i32")
        rc, out, err = self._run("adapt", mx.shape[0], nu, *(float(np.float32(v)).hex() for v in (rate, lo, hi)),
                                 self.d / "S.f32", self.d / "mx.f32", self.d / "nf.i32")
        assert rc == 0, err[-3000:]
        return (out[0], rows(out[1:], nu), rows(out[1 + nu:], nu), rows(out[1 + 2 * nu:], nu),
                rows(out[1 + 3 * nu:], 1)[0])

    def factor(self, S):
        """-> (L, Sinv, sigma_u), or None where both statements refuse; fails where they disagree"""
        nu = S.shape[0]
        np.ascontiguousarray(S, np.float32).tofile(self.d / "F.f32")
        rc, out, err = self._run("factor", nu, self.d / "F.f32")
        assert rc == 0, f"cov_factor and the adaptation's factor disagree (rc {rc}) {err[-2000:]}"
        if out[0] == "refused":
            return None
        return rows(out[1:], nu), rows(out[1 + nu:], nu), rows(out[1 + 2 * nu:], 1)[0]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("noise_cov_adapt")
    return _Host(build_host(d), d)


STATUS = {1: "moved", 0: "unchanged", -1: "rejected"}


def _same_step(got, want):
    """(status, Sigma, L, Sinv, sigma_u) of the harness against adapt_noise_cov_f32's tuple, bit for bit"""
    S, L, Sinv, sig, status = want
    assert got[0] == STATUS[status]
    for a, b, name in zip(got[1:], (S, L, Sinv, sig), ("Sigma", "L", "Sinv", "sigma_u")):
        assert np.array_equal(bits(a), bits(b)), name


# ---- 1. the numpy restatement and the factor against the headers

@pytest.mark.parametrize("nu", NUS)
def test_adapt_f32_equals_the_header_bitwise(host, nu):
    from mppi_hip.stats import adapt_noise_cov_f32
    S = sigma_of(nu)
    s = np.sqrt(np.diag(S).astype(np.float64))
    for i, (rate, lo, hi) in enumerate(((0.3,) + WIDE, (1.0,) + WIDE, (0.5, float(np.median(s)), float(np.median(s)) * 1.2),
                                        (1.0 / 3.0, 1e-3, float(s.min())))):
        mx = moments_like(nu, 100 * nu + i, Bn=3)
        want = adapt_noise_cov_f32(S, mx, rate, lo, hi)
        assert want[4] == 1
        _same_step(host.adapt(S, mx, rate, lo, hi), want)
        # ... and a second step from the adapted law (the blend of a blend)
        mx2 = moments_like(nu, 100 * nu + i + 50, Bn=1)
        _same_step(host.adapt(want[0], mx2, rate, lo, hi), adapt_noise_cov_f32(want[0], mx2, rate, lo, hi))


@pytest.mark.parametrize("nu", NUS)
def test_the_adaptations_factor_is_cov_factor_bitwise(host, nu):
    """on sigma_of(nu) and on blended matrices (the S2 of a step): the header's column-by-column element functions,
    cov_factor of csrc/noise_cov.h (the harness compares the two and fails on one bit) and mppi_hip.noise.cov_factor"""
    from mppi_hip.noise import cov_factor
    from mppi_hip.stats import adapt_noise_cov_f32
    S = sigma_of(nu)
    mats = [S] + [adapt_noise_cov_f32(S, moments_like(nu, 7 * nu + i), r, *WIDE)[0] for i, r in enumerate((0.3, 0.9, 1.0))]
    for Mx in mats:
        L, Sinv, sig = host.factor(Mx)
        assert np.array_equal(bits(L), bits(cov_factor(Mx)))
        assert np.array_equal(bits(Sinv), bits(Sinv.T))
        assert np.array_equal(bits(sig), bits(np.sqrt(np.diag(Mx).astype(np.float64)).astype(np.float32)))
    if nu > 1:  # both statements refuse the same matrices
        bad = S.copy()
        bad[0, 1] = bad[1, 0] = np.float32(2.0) * np.sqrt(S[0, 0] * S[1, 1])
        assert host.factor(bad) is None
        semi = np.float32([[0.25, 0.25], [0.25, 0.25]])
        assert host.factor(semi) is None


# ---- 2. the rule

@pytest.mark.parametrize("nu", NUS)
def test_rate_one_without_clamps_gives_the_batch_mean(nu):
    from mppi_hip.stats import adapt_noise_cov_f32
    mx = moments_like(nu, 31 * nu, Bn=3)
    acc = np.zeros((nu, nu), np.float32)
    for b in range(3):
        acc = acc + mx[b]
    mbar = acc / np.float32(3)
    S2, L, Sinv, sig, status = adapt_noise_cov_f32(sigma_of(nu), mx, 1.0, *WIDE)
    assert status == 1 and np.array_equal(bits(S2), bits(mbar))


@pytest.mark.parametrize("nu", (3, 21, 32))
def test_clamps_land_and_keep_the_correlations(nu):
    """limits that clamp the small scales up and the large ones down and leave the middle alone.  A clamped diagonal
    is c_u * c_u exactly; a pair of unclamped actuators keeps its entry, hence its correlation, exactly (the issue's
    bar: 4 * 2^-24 relative); a pair with a clamped member keeps its correlation to 8 * 2^-24 relative: two roundings
    in the product (S1 g_u) g_v, one in each gain, one in each s_u the gains divide by, and half of one per clamped
    diagonal c_u * c_u under the square root -- at most 2 + 2 + 2 + 1 = 7 half-ulps of 2^-24, so 8 holds with room."""
    from mppi_hip.stats import adapt_noise_cov_f32
    S = sigma_of(nu)
    mx = moments_like(nu, 900 + nu, Bn=2)
    rate = 0.4
    free = adapt_noise_cov_f32(S, mx, rate, *WIDE)[0]  # = S1: no clamp binds
    s = np.sqrt(np.diag(free)).astype(np.float32)
    lo, hi = np.float32(np.sort(s)[nu // 3]), np.float32(np.sort(s)[-1 - nu // 3])
    S2, L, Sinv, sig, status = adapt_noise_cov_f32(S, mx, rate, lo, hi)
    assert status == 1
    c = np.minimum(np.maximum(s, lo), hi)
    clamped = c != s
    assert clamped.any() and (~clamped).any()
    assert np.array_equal(bits(np.diag(S2)[clamped]), bits((c * c)[clamped]))
    assert np.array_equal(bits(np.diag(S2)[~clamped]), bits(np.diag(free)[~clamped]))
    both = ~clamped[:, None] & ~clamped[None, :]
    assert np.array_equal(bits(S2[both]), bits(free[both]))
    f1, f2 = free.astype(np.float64), S2.astype(np.float64)
    corr1 = f1 / np.sqrt(np.outer(np.diag(f1), np.diag(f1)))
    corr2 = f2 / np.sqrt(np.outer(np.diag(f2), np.diag(f2)))
    off = ~np.eye(nu, dtype=bool)
    rel = np.abs(corr2 / corr1 - 1.0)
    print(f"nu {nu}: {int(clamped.sum())} clamped; max rel change of a correlation: unclamped pairs "
          f"{rel[both & off].max(initial=0.0) / U32:.2f}, others {rel[~both & off].max() / U32:.2f} (x 2^-24)")
    assert rel[both & off].max(initial=0.0) <= 4 * U32
    assert rel[~both & off].max() <= 8 * U32
    # the standard deviations the law reports are the clamped ones, to one rounding of the square and one of the root
    np.testing.assert_allclose(sig[clamped], c[clamped], rtol=2 * U32, atol=0.0)
    assert np.linalg.eigvalsh(f2).min() > 0.0


def _pm_half_noise(nu, H, K, repeat):
    """noise of +-0.5 entries (row `repeat[1]` a copy of row `repeat[0]`) with uniform weights 1 / K, K a power of two:
    every second moment is a sum of exactly representable terms, so the diagonal is 0.25 and the repeated pair's
    entry 0.25 to the bit -- the second pivot of that pair is then exactly 0, not a rounding's worth above it"""
    rs = np.random.RandomState(5)
    noise = np.where(rs.rand(B, nu, H, K) < 0.5, np.float32(-0.5), np.float32(0.5)).astype(np.float32)
    noise[:, repeat[1]] = noise[:, repeat[0]]
    return np.full((B, K), 1.0 / K, np.float32), noise


def test_zero_and_rank_deficient_moments_are_rejected_whole(host):
    """rate = 1: the law becomes the moments.  All-zero noise (every s_u = 0) and one repeated row (a zero pivot) are
    rejected and leave Sigma, L, Sinv and sigma_u untouched; so is a non-finite moment."""
    from mppi_hip.stats import adapt_noise_cov_f32, cross_moments_f32
    nu, H, K = 3, 7, 128
    S = sigma_of(nu)
    keep = adapt_noise_cov_f32(S, np.zeros((B, nu, nu), np.float32), 1.0, *WIDE, n_finite=[0, 0])
    assert keep[4] == 0  # (the law as it stands, factored: what "untouched" is compared with)
    w, noise = _pm_half_noise(nu, H, K, (0, 1))
    zero = cross_moments_f32(w, np.zeros_like(noise))
    assert not np.any(zero)
    twin = cross_moments_f32(w, noise)
    assert twin[0, 0, 0] == 0.25 and np.array_equal(bits(twin[:, 0]), bits(twin[:, 1]))
    assert np.array_equal(bits(twin), bits(host_cross(host.exe, host.d, w, noise)))
    nan = moments_like(nu, 3)
    nan[1, 2, 1] = nan[1, 1, 2] = np.nan
    inf = moments_like(nu, 4)
    inf[0, 0, 0] = np.inf
    for name, mx in (("zero", zero), ("twin", twin), ("nan", nan), ("inf", inf)):
        got = adapt_noise_cov_f32(S, mx, 1.0, *WIDE)
        assert got[4] == -1, name
        for a, b in zip(got[:4], keep[:4]):
            assert np.array_equal(bits(a), bits(b)), name
        _same_step(host.adapt(S, mx, 1.0, *WIDE), got)
    # the same moments blended at a small rate leave a positive definite matrix: accepted
    assert adapt_noise_cov_f32(S, twin, 0.25, *WIDE)[4] == 1
    assert adapt_noise_cov_f32(S, zero, 0.25, *WIDE)[4] == 1


def test_a_solve_without_a_finite_cost_changes_nothing(host):
    from mppi_hip.stats import adapt_noise_cov_f32
    for nu in (1, 21):
        S, mx = sigma_of(nu), moments_like(nu, 60 + nu)
        got = adapt_noise_cov_f32(S, mx, 0.5, *WIDE, n_finite=[130, 0])
        assert got[4] == 0 and np.array_equal(bits(got[0]), bits(S))
        _same_step(host.adapt(S, mx, 0.5, *WIDE, n_finite=[130, 0]), got)
        assert adapt_noise_cov_f32(S, mx, 0.5, *WIDE, n_finite=[130, 1])[4] == 1


@pytest.mark.parametrize("nu", NUS)
def test_float64_rule_within_the_counted_bound(nu):
    """adapt_noise_cov (float64) against the f32 step, entry by entry.  The roundings of an entry: Bn - 1 additions and
    one division for the mean, 1 - rate, its product with S, the fma, and then the square root, the gain (each of the
    two actuators') and the two products of the congruence: Bn + 3 + 2 * 2 + 2 = Bn + 9 half-ulps at most, each
    relative to a quantity bounded by T = g_u g_v ((1 - rate) |S| + rate mean_b |mx|) -- the blend may cancel, its
    terms do not.  Bound: (Bn + 9) 2^-24 T (as tests/test_noise_adapt.py counts its rule's)."""
    from mppi_hip.stats import adapt_noise_cov, adapt_noise_cov_f32
    Bn = 3
    S = sigma_of(nu)
    s0 = np.sqrt(np.diag(S).astype(np.float64))
    for i, (rate, lo, hi) in enumerate(((0.3,) + WIDE, (1.0,) + WIDE, (0.6, float(np.median(s0)), float(s0.max())))):
        mx = moments_like(nu, 300 + 10 * nu + i, Bn=Bn)
        got = adapt_noise_cov_f32(S, mx, rate, lo, hi)[0].astype(np.float64)
        ref = adapt_noise_cov(S, mx, rate, lo, hi)
        S1 = (1.0 - rate) * S.astype(np.float64) + rate * mx.astype(np.float64).mean(0)
        s = np.sqrt(np.diag(S1))
        g = np.clip(s, lo, hi) / s
        T = np.outer(g, g) * ((1.0 - rate) * np.abs(S.astype(np.float64)) + rate * np.abs(mx.astype(np.float64)).mean(0))
        ratio = float((np.abs(got - ref) / ((Bn + 9) * U32 * T)).max())
        print(f"nu {nu} rate {rate}: max |f32 - f64| / bound = {ratio:.3f}")
        assert ratio <= 1.0
        assert np.array_equal(ref, ref.T)


def test_float64_rule_refuses_bad_input():
    from mppi_hip.stats import adapt_noise_cov, adapt_noise_cov_f32
    S, mx = sigma_of(3), moments_like(3, 1)
    for fn in (adapt_noise_cov, adapt_noise_cov_f32):
        for args in ((-0.1, 1e-3, 10.0), (1.5, 1e-3, 10.0), (0.3, 0.0, 10.0), (0.3, 2.0, 1.0), (0.3, 1e-3, np.inf),
                     (0.3, np.nan, 10.0)):
            with pytest.raises(ValueError):
                fn(S, mx, *args)
    with pytest.raises(ValueError):
        adapt_noise_cov(S, np.zeros((2, 2)), 0.3)
    with pytest.raises(ValueError):
        adapt_noise_cov(S, np.zeros((3, 3)), 1.0)  # a zero diagonal
    np.testing.assert_allclose(adapt_noise_cov(S, mx, 0.0), S.astype(np.float64), rtol=1e-15)


# ---- 3. the C ABI without a device

def test_ctypes_prototypes_and_null_handles():
    from mppi_hip import _lib as L
    lib = L.load()
    for name, nargs in zip(ENTRIES, (4, 5, 3)):
        assert name in L.EXPORTED
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == nargs, name
    buf = np.eye(3, dtype=np.float32)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    f = ctypes.c_float
    assert lib.mppi_set_noise_cov_adapt(None, f(0.3), f(1e-3), f(10.0)) == L.MPPI_E_ARG
    assert b"mppi_set_noise_cov_adapt" in lib.mppi_last_error()
    r = ctypes.c_uint64(7)
    assert lib.mppi_get_noise_cov_adapt(None, None, None, None, ctypes.byref(r)) == L.MPPI_E_ARG
    assert b"mppi_get_noise_cov_adapt" in lib.mppi_last_error() and r.value == 7
    assert lib.mppi_get_noise_cov_law(None, 0, p) == L.MPPI_E_ARG
    assert b"mppi_get_noise_cov_law" in lib.mppi_last_error()
    assert np.array_equal(buf, np.eye(3, dtype=np.float32))
    assert lib.mppi_abi_version() == 4  # additive


def test_header_declares_the_entries_and_the_wrappers_exist():
    text = open(os.path.join(REPO, "include", "mppi.h")).read()
    for name in ENTRIES:
        assert f"int {name}(mppi_handle*" in text, name
    assert "#define MPPI_ABI_VERSION 4" in text
    from mppi_hip import Engine
    for name in ("set_noise_cov_adapt", "noise_cov_adapt", "noise_cov_law"):
        assert callable(getattr(Engine, name))
    jl = open(os.path.join(PKG, "julia", "MPPIHip.jl")).read()
    for name in ENTRIES:
        assert f":{name}" in jl, name


# ---- the stand-alone program under the sanitizers

def test_host_program_under_asan_ubsan(tmp_path):
    """tests/native/cross_adapt_host.cpp (its own main) built host-only with ASan + UBSan and run directly, as
    tests/test_noise_cov.py builds its harness: its self mode at nu = 1 and nu = 32 (every mode on generated data, the
    two factors compared inside), and one call of each mode the bitwise tests use -- clang's host build gives the
    bits of the numpy restatements too."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "cross_adapt_host")
    cmd = [HIPCC, "-x", "hip", "--offload-host-only", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address",
           "-Xarch_host", "-fsanitize=undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           f"-I{REPO}/include", f"-I{PKG}/csrc", SRC, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    for nu in (1, 32):
        r = subprocess.run([exe, "self", str(nu)], capture_output=True, text=True, timeout=240, env=env)
        words = [ln for ln in r.stdout.splitlines() if ln in ("ok", "moved", "unchanged", "rejected")]
        assert r.returncode == 0 and words == ["ok", "moved", "moved", "unchanged", "rejected"], \
            (r.stdout[-1000:] + r.stderr)[-3000:]
    from mppi_hip.stats import adapt_noise_cov_f32, cross_moments_f32, softmin_weights_ref
    san = _Host(exe, tmp_path, env)
    for nu in (1, 32):
        costs, noise = case(nu, 7, 130)
        w = softmin_weights_ref(costs).astype(np.float32)
        assert np.array_equal(bits(host_cross(exe, tmp_path, w, noise, env)), bits(cross_moments_f32(w, noise)))
        S, mx = sigma_of(nu), moments_like(nu, 11 * nu)
        _same_step(san.adapt(S, mx, 0.3, *WIDE), adapt_noise_cov_f32(S, mx, 0.3, *WIDE))
        assert san.factor(S) is not None
