"""ESS targeting on the host (mppi_set_ess_target; no GPU needed): the float64 reference's end rules and monotonicity,
the four C entries' prototypes and NULL-handle paths, MPPIModel's argument checks, and the host form of the fp32 rule
(csrc/ess_target.h) as a stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer, held to the float64
conditions the kernel is held to (tests/test_gpu_ess_target.py)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import PKG, REPO
from ess_cases import BOUNDS, FAMILIES, FRACS, N_TIES, check_row, family

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


# ------------------------------------------------------------------------------------------ the float64 reference

def test_reference_end_rules():
    from mppi_hip.stats import ess_lambda_ref, ess_ref, ess_target_ref
    lo, hi = BOUNDS
    ties = family("ties", 75)
    assert ess_target_ref(ties[0], 0.02) == 1.5 and N_TIES >= 1.5
    assert ess_lambda_ref(ties, 0.02, lo, hi).tolist() == [lo, lo]      # ties at the minimum cover the target
    assert np.all(ess_lambda_ref(ties, 0.5, lo, hi) > lo)               # ... and do not cover 37.5
    gaps = family("gaps", 2500)
    assert ess_ref(gaps[0], hi) < 250.0
    assert ess_lambda_ref(gaps, 0.1, lo, hi).tolist() == [hi, hi]       # the target is out of reach below lambda_max
    assert ess_lambda_ref(np.full(40, 3.0), 1.0, lo, hi) == lo          # all costs equal: ESS = n at every lambda
    assert ess_lambda_ref([7.0], 0.5, lo, hi) == lo                     # K = 1
    nan_row = np.full((2, 30), np.nan)
    nan_row[1] = family("gauss", 30)[0]
    got = ess_lambda_ref(nan_row, 0.1, lo, hi, lam_default=2.5)
    assert got[0] == 2.5 and lo < got[1] < hi                           # no finite cost: the configured lambda
    assert ess_ref(nan_row[0], 1.0) == 0.0
    c = family("nan", 75)[0]                                            # non-finite costs carry no weight
    assert ess_lambda_ref(c, 0.1, lo, hi) == ess_lambda_ref(c[np.isfinite(c)], 0.1, lo, hi)
    assert ess_lambda_ref(c, 0.1, 3.0, 3.0) == 3.0                      # lambda_min == lambda_max
    for bad in ((0.0, lo, hi), (1.5, lo, hi), (float("nan"), lo, hi), (0.1, 0.0, hi), (0.1, 2.0, 1.0),
                (0.1, lo, float("inf")), (0.1, float("nan"), hi)):
        with pytest.raises(ValueError):
            ess_lambda_ref(c, *bad)


@pytest.mark.parametrize("name", FAMILIES)
def test_reference_hits_the_target_and_is_monotone_in_ess_frac(name):
    from mppi_hip.stats import ess_lambda_ref, ess_ref, ess_target_ref
    lo, hi = BOUNDS
    c = family(name, 300)
    prev = np.full(2, lo)
    for frac in (0.01, 0.02, 0.1, 0.3, 0.5, 0.9, 1.0):
        lam = ess_lambda_ref(c, frac, lo, hi)
        assert np.all(lam >= prev), (name, frac)  # a larger target never takes a smaller lambda
        prev = lam
        for b in range(2):
            if lo < lam[b] < hi:
                T = ess_target_ref(c[b], frac)
                assert abs(ess_ref(c[b], lam[b]) - T) <= 1e-9 * T, (name, frac, b)


# ------------------------------------------------------------------------------------------ the ABI

def test_ctypes_prototypes_and_null_handles():
    from mppi_hip import _lib as L
    lib = L.load()
    f = ctypes.c_float
    for name, nargs in (("mppi_set_ess_target", 4), ("mppi_get_ess_target", 4), ("mppi_get_lambda", 4),
                        ("mppi_lambda_eval", 4)):
        assert name in L.EXPORTED
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == nargs, name
    assert lib.mppi_set_ess_target(None, f(0.1), f(1e-3), f(1e3)) == L.MPPI_E_ARG
    assert b"mppi_set_ess_target" in lib.mppi_last_error()
    assert lib.mppi_get_ess_target(None, None, None, None) == L.MPPI_E_ARG
    out = np.zeros(1, np.float32)
    assert lib.mppi_get_lambda(None, 1, 0, out.ctypes.data_as(ctypes.c_void_p)) == L.MPPI_E_ARG
    assert lib.mppi_lambda_eval(None, 1, out.ctypes.data_as(ctypes.c_void_p),
                                out.ctypes.data_as(ctypes.c_void_p)) == L.MPPI_E_ARG
    assert lib.mppi_abi_version() == 4  # additive


def test_header_declares_the_entries_and_the_engine_wraps_them():
    text = open(os.path.join(REPO, "include", "mppi.h")).read()
    for name in ("mppi_set_ess_target", "mppi_get_ess_target", "mppi_get_lambda", "mppi_lambda_eval"):
        assert f"int {name}(mppi_handle*" in text, name
    from mppi_hip import Engine
    for name in ("set_ess_target", "ess_target", "lambdas", "lambda_eval"):
        assert callable(getattr(Engine, name))
    jl = open(os.path.join(PKG, "julia", "MPPIHip.jl")).read()
    for name in ("mppi_set_ess_target", "mppi_get_ess_target", "mppi_get_lambda", "mppi_lambda_eval"):
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
    nan, inf = float("nan"), float("inf")
    for kw in (dict(ess_target=-0.1), dict(ess_target=1.5), dict(ess_target=nan),
               dict(ess_target=0.1, lambda_limits=(0.0, 1.0)), dict(ess_target=0.1, lambda_limits=(2.0, 1.0)),
               dict(ess_target=0.1, lambda_limits=(1.0, inf)), dict(ess_target=0.1, lambda_limits=(nan, 1.0)),
               dict(ess_target=0.1, lambda_limits=(1.0,)), dict(lambda_limits=3.0)):
        with pytest.raises(ValueError):
            controller.MPPIModel(**kw)
    controller.MPPIModel()  # the default asks for nothing
    assert not [c for c in _Recorder.calls if c[0] == "set_ess_target"]
    m = controller.MPPIModel(ess_target=0.25, lambda_limits=(0.5, 20))
    assert [c for c in _Recorder.calls if c[0] == "set_ess_target"] == [("set_ess_target", (0.25, 0.5, 20.0))]
    assert m.ess_target == 0.25 and m.lambda_limits == (0.5, 20.0)


# ------------------------------------------------------------------------------------------ the fp32 rule on the host

@pytest.fixture(scope="module")
def host_rule(tmp_path_factory):
    """tests/native/ess_target_host.cpp (its own main; includes csrc/ess_target.h) built host-only with ASan + UBSan,
    as tests/test_sanitizers.py builds blob_fuzz.cpp.  host_rule(costs [B, K], frac, lo, hi, cfg_lambda) ->
    (lambda of the 15-candidate search [B], lambda of plain bisection [B], passes [B, 2])."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    d = tmp_path_factory.mktemp("ess_target")
    exe = str(d / "ess_target_host")
    cmd = [HIPCC, "-x", "hip", "--offload-host-only", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address",
           "-Xarch_host", "-fsanitize=undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           f"-I{REPO}/include", f"-I{PKG}/csrc", os.path.join(REPO, "tests", "native", "ess_target_host.cpp"),
           "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    count = [0]

    def run(costs, frac, lo, hi, cfg_lambda=1.0):
        costs = np.ascontiguousarray(costs, np.float32)
        count[0] += 1
        path = d / f"costs_{count[0]}.f32"
        costs.tofile(path)
        r = subprocess.run([exe, str(path), str(costs.shape[0]), str(costs.shape[1])] +
                           [float(np.float32(v)).hex() for v in (frac, lo, hi, cfg_lambda)],
                           capture_output=True, text=True, timeout=240, env=env)
        assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
        rows = [ln.split() for ln in r.stdout.strip().splitlines()]
        assert len(rows) == costs.shape[0]
        f32 = lambda s: np.float32(float.fromhex(s))
        return (np.array([f32(x[0]) for x in rows]), np.array([f32(x[1]) for x in rows]),
                np.array([[int(x[2]), int(x[3])] for x in rows]))
    return run


@pytest.mark.parametrize("K", [30, 75, 2500, 32768])
def test_host_form_of_the_rule_under_asan_ubsan(host_rule, K):
    """Both arms of the search (15 candidates per pass, plain bisection) on the five families: the two float64
    conditions on every row, and the pass counts the header states."""
    lo, hi = BOUNDS
    worst = 0.0
    for name in FAMILIES:
        c = family(name, K)
        for frac in (FRACS if K < 32768 else FRACS[1:2]):
            l15, l1, passes = host_rule(c, frac, lo, hi)
            for b in range(c.shape[0]):
                for lam in (l15[b], l1[b]):
                    err = check_row(c[b], lam, frac, lo, hi)
                    worst = max(worst, err or 0.0)
                assert passes[b, 0] <= 8 and passes[b, 1] <= 30, (name, frac, passes[b])
            if name == "ties" and N_TIES >= frac * K:
                assert l15.tolist() == [np.float32(lo)] * 2 and l1.tolist() == [np.float32(lo)] * 2
            if name == "gaps" and K == 2500 and frac == 0.1:
                assert l15.tolist() == [np.float32(hi)] * 2 and l1.tolist() == [np.float32(hi)] * 2
    print(f"K={K}: worst |ESS64(lambda) - T| / T at an interior lambda = {worst:.3g}")
    assert worst <= 1e-4


def test_host_form_end_rules(host_rule):
    lo, hi = BOUNDS
    c = family("gauss", 30)
    c[0] = np.nan  # no finite cost: the configured lambda
    l15, l1, passes = host_rule(c, 0.1, lo, hi, cfg_lambda=2.5)
    assert l15[0] == np.float32(2.5) and l1[0] == np.float32(2.5) and passes[0].tolist() == [0, 0]
    assert lo < l15[1] < hi
    l15, l1, _ = host_rule(np.array([[7.0], [np.inf]], np.float32), 0.5, lo, hi, cfg_lambda=2.5)  # K = 1
    assert l15.tolist() == [np.float32(lo), np.float32(2.5)] and l1.tolist() == l15.tolist()
    l15, l1, passes = host_rule(family("lognormal", 75), 0.1, 3.0, 3.0)  # lambda_min == lambda_max: the ends decide
    assert l15.tolist() == [3.0, 3.0] and l1.tolist() == [3.0, 3.0] and passes.max() <= 2
    l15, _, _ = host_rule(np.full((2, 40), 3.0, np.float32), 1.0, lo, hi)  # all equal: ESS = n at lambda_min
    assert l15.tolist() == [np.float32(lo)] * 2
