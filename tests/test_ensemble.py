"""Dynamics-model ensembles on the host (mppi_set_ensemble; no GPU needed): the header and the library's exports, the
numpy restatement of the combining rule on rows written out by hand, the host form of the rule (csrc/ensemble.h) as a
stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer held EXACTLY to the restatement on the hand
cases and the grid of tests/ensemble_cases.py, the entries' NULL-handle paths, the Engine / MPPIModel wrappers'
argument checks, and train_mlp_ensemble on the quadruped logs."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import PKG, REPO, golden
from ensemble_cases import MODES, assert_hand, bits, grid, hand_cases, same_bits

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
ENTRIES = (("mppi_load_member", 5), ("mppi_set_ensemble", 5), ("mppi_get_ensemble", 6), ("mppi_get_member_costs", 4),
           ("mppi_get_ensemble_spread", 3), ("mppi_ensemble_eval", 8))
MACROS = (("MPPI_ENS_MAX", 8), ("MPPI_ENS_MEAN", 0), ("MPPI_ENS_MEAN_STD", 1), ("MPPI_ENS_WORST", 2))


# ------------------------------------------------------------------------------------------ the ABI

def test_header_declares_the_entries_and_the_library_exports_them():
    text = open(os.path.join(REPO, "include", "mppi.h")).read()
    for name, _ in ENTRIES:
        assert f"int {name}(mppi_handle*" in text, name
    for name, value in MACROS:
        assert f"#define {name} {value}" in text, name
    assert '"ensemble"' in text  # the kernel time name
    assert "#define MPPI_ABI_VERSION 4" in text  # additive
    from mppi_hip import _lib as L
    lib = L.load()
    for name, nargs in ENTRIES:
        assert name in L.EXPORTED
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == nargs, name
    assert lib.mppi_abi_version() == 4


def test_null_handles_and_arguments_return_codes_without_a_gpu():
    from mppi_hip import _lib as L
    lib = L.load()
    out = np.zeros(8, np.float32)
    p = out.ctypes.data_as(ctypes.c_void_p)
    n = ctypes.c_int(-7)
    r = ctypes.byref(n)
    f = ctypes.c_float(-7.0)
    for name, call in (("mppi_load_member", lambda: lib.mppi_load_member(None, 1, 1, None, 0)),
                       ("mppi_set_ensemble", lambda: lib.mppi_set_ensemble(None, 2, 0, 0.0, 0)),
                       ("mppi_get_ensemble", lambda: lib.mppi_get_ensemble(None, r, r, ctypes.byref(f), r, r)),
                       ("mppi_get_member_costs", lambda: lib.mppi_get_member_costs(None, 1, 0, p)),
                       ("mppi_get_ensemble_spread", lambda: lib.mppi_get_ensemble_spread(None, 1, p)),
                       ("mppi_ensemble_eval", lambda: lib.mppi_ensemble_eval(None, 1, 2, 0, 0.0, p, p, p))):
        assert call() == L.MPPI_E_ARG, name
        assert name.encode() in lib.mppi_last_error(), name
    assert n.value == -7 and f.value == -7.0 and not out.any()


def test_every_layer_wraps_the_entries():
    import mppi_hip
    for name in ("load_member", "set_ensemble", "ensemble", "member_costs", "ensemble_spread", "ensemble_eval"):
        assert callable(getattr(mppi_hip.Engine, name)), name
    assert callable(mppi_hip.ensemble_combine_f32) and "ensemble_combine_f32" in mppi_hip.__all__
    from mppi_hip import training
    assert callable(training.train_mlp_ensemble)
    jl = open(os.path.join(PKG, "julia", "MPPIHip.jl")).read()
    for name in ("mppi_load_member", "mppi_set_ensemble", "mppi_get_ensemble", "mppi_get_member_costs",
                 "mppi_get_ensemble_spread"):
        assert f":{name}" in jl, name
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "mppi_set_ensemble" in open(os.path.join(REPO, doc)).read(), doc


# ------------------------------------------------------------------------------------------ the numpy restatement

@pytest.mark.parametrize("case", hand_cases(), ids=[c[0] for c in hand_cases()])
def test_restatement_on_hand_written_rows(case):
    from mppi_hip.stats import ensemble_combine_f32
    name, members, mode, kappa, want_cost, want_sd = case
    m = np.array(members, np.float32)
    keep = m.copy()
    cost, sd = ensemble_combine_f32(m, mode, kappa)
    assert cost.dtype == np.float32 and sd.dtype == np.float32 and cost.shape == sd.shape == m.shape[1:]
    assert_hand(name, cost, sd, want_cost, want_sd)
    assert same_bits(m, keep)  # the input is not written
    # a batch axis gives the same rows
    c2, s2 = ensemble_combine_f32(np.stack([m, m], axis=1), mode, kappa)
    assert same_bits(c2[0], cost) and same_bits(c2[1], cost) and same_bits(s2[0], sd) and same_bits(s2[1], sd)


def test_restatement_rejects_bad_arguments():
    from mppi_hip.stats import ensemble_combine_f32
    m = np.ones((3, 2, 5), np.float32)
    for bad in (m[:1], np.ones((9, 4), np.float32), np.float32(1.0)):
        with pytest.raises(ValueError):
            ensemble_combine_f32(bad)
    for mode in ("median", 3, -1, True, None):
        with pytest.raises(ValueError):
            ensemble_combine_f32(m, mode)
    for kappa in (np.inf, -np.inf, np.nan):
        with pytest.raises(ValueError):
            ensemble_combine_f32(m, "mean_std", kappa)
    for i, mode in enumerate(MODES):  # the ABI's integers name the modes too
        a, b = ensemble_combine_f32(m, mode, 0.5), ensemble_combine_f32(m, i, 0.5)
        assert same_bits(a[0], b[0]) and same_bits(a[1], b[1])


def test_restatement_properties_on_the_grid():
    """What the rule promises whatever the numbers: a non-finite member gives (+inf, +inf); everything returned is
    finite or +inf and sd >= 0; the maximum is one of the members; identical members give the member itself and
    sd = +0 for every n and in every mode -- where the sums as written would not (n = 3: a third of these costs)."""
    from mppi_hip.stats import ensemble_combine_f32
    for name, n, mode, kappa, m in grid():
        cost, sd = ensemble_combine_f32(m, mode, kappa)
        bad = ~np.isfinite(m).all(axis=0)
        assert bad.any() and np.all(cost[bad] == np.inf) and np.all(sd[bad] == np.inf), name
        assert not np.isnan(cost).any() and not np.isnan(sd).any() and not (cost == -np.inf).any(), name
        assert (sd >= 0).all(), name
        if mode == "worst":
            ok = ~bad
            assert np.array_equal(cost[ok], m.max(axis=0)[ok]), name
    rs = np.random.RandomState(0)
    c = (50.0 + 10.0 * rs.randn(4096)).astype(np.float32)
    for n in range(2, 9):
        for mode in MODES:
            cost, sd = ensemble_combine_f32(np.stack([c] * n), mode, -0.75)
            assert same_bits(cost, c) and not bits(sd).any(), (n, mode)
    s3 = ((c + c).astype(np.float32) + c).astype(np.float32)
    assert ((s3 * (np.float32(1) / np.float32(3))).astype(np.float32) != c).mean() > 0.2  # the sums alone would miss
    # one member a bit apart is not identical: the spread is one ulp-sized number, not +0
    m = np.stack([c] * 3)
    m[2] = np.nextafter(c, np.float32(np.inf))
    cost, sd = ensemble_combine_f32(m, "worst")
    assert same_bits(cost, m[2]) and (sd > 0).all()


# ------------------------------------------------------------------------------------------ Engine / MPPIModel

def test_engine_argument_checks_ahead_of_the_library():
    """The wrappers' own checks raise ValueError before any C call."""
    from mppi_hip.engine import Config, Engine

    class _Lib:
        def __getattr__(self, name):
            raise AssertionError(f"{name} reached the library")

    e = Engine.__new__(Engine)
    e.lib, e._h, e.config = _Lib(), None, Config(nx=4, nu=2, H=5, K=8)
    for bad in ("median", 3, -1, True, None, 1.0):
        with pytest.raises(ValueError):
            e.set_ensemble(2, bad)
        with pytest.raises(ValueError):
            e.ensemble_eval(np.zeros((2, 1, 8)), bad)
    for bad in (np.zeros((2, 1, 7)), np.zeros((2, 1, 1, 8)), np.zeros(8)):
        with pytest.raises(ValueError):
            e.ensemble_eval(bad)
    e._h = None


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


def test_mppimodel_loads_the_members_and_sets_the_rule(monkeypatch):
    from mppi_hip import controller
    from mppi_hip.nets import synthetic_mlp
    monkeypatch.setattr(controller.Config, "preset", classmethod(lambda cls, name, **kw: cls(nx=10, nu=3, H=8, K=16)))
    monkeypatch.setattr(controller, "Engine", _Recorder)
    sds = [synthetic_mlp(10, 3, seed=e) for e in range(3)]
    m = controller.MPPIModel(dynamics=("mlp_ensemble", sds), cost="quad_est", ensemble_mode="mean_std",
                             ensemble_kappa=0.5)
    names = [c[0] for c in _Recorder.calls]
    assert names[:4] == ["load_dynamics", "load_member", "load_member", "set_ensemble"]
    assert [c[1][0] for c in _Recorder.calls[1:3]] == [1, 2]
    assert _Recorder.calls[3][1] == (3, "mean_std", 0.5)
    assert (m.ensemble_mode, m.ensemble_kappa) == ("mean_std", 0.5)
    blobs = [_Recorder.calls[0][1][1], _Recorder.calls[1][1][2], _Recorder.calls[2][1][2]]
    assert len({len(b) for b in blobs}) == 1 and len(set(blobs)) == 3  # three different nets of one shape
    controller.MPPIModel(dynamics=("mlp", sds[0]), cost="quad_est")  # a single net asks for nothing
    assert not [c for c in _Recorder.calls if c[0] in ("load_member", "set_ensemble")]
    for bad in ("median", 1, None):
        with pytest.raises(ValueError):
            controller.MPPIModel(dynamics=("mlp_ensemble", sds), cost="quad_est", ensemble_mode=bad)
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError):
            controller.MPPIModel(dynamics=("mlp_ensemble", sds), cost="quad_est", ensemble_kappa=bad)
    for bad in (sds[:1], sds * 3):
        with pytest.raises(ValueError):
            controller.MPPIModel(dynamics=("mlp_ensemble", bad), cost="quad_est")


# ------------------------------------------------------------------------------------------ training

def test_train_mlp_ensemble_gives_members_that_differ_and_pack_alike():
    from mppi_hip import training as T
    g = golden("quad_logs.npz")
    X, Y = T.log_pairs(g["states0"], g["actions0"])
    sds = T.train_mlp_ensemble(X[:256], Y[:256], 2, 37, 12, hidden_dim=16, hidden_layers=1, epochs=1, device="cpu",
                               log=None)
    assert len(sds) == 2 and sorted(sds[0]) == sorted(sds[1])
    assert all(not np.array_equal(sds[0][k], sds[1][k]) for k in sds[0])
    blobs = [T.export_mlp_blob(sd, 37, 12, 16, 1)[1] for sd in sds]
    assert len(blobs[0]) == len(blobs[1]) and blobs[0] != blobs[1] and blobs[0][:4] == b"MPPW"
    # member i is train_mlp with seed i on the resample default_rng(i) draws
    idx = np.random.default_rng(1).integers(0, 256, size=256)
    m1, _ = T.train_mlp(X[:256][idx], Y[:256][idx], 37, 12, 16, 1, epochs=1, device="cpu", seed=1, log=None)
    want = T.state_dict_numpy(m1)
    assert all(np.array_equal(want[k], sds[1][k]) for k in want)
    # without the resample the members are apart by their seeds alone
    plain = T.train_mlp_ensemble(X[:256], Y[:256], 2, 37, 12, hidden_dim=16, hidden_layers=1, epochs=1, device="cpu",
                                 bootstrap=False, log=None)
    assert all(not np.array_equal(plain[0][k], plain[1][k]) for k in plain[0])
    assert any(not np.array_equal(plain[1][k], sds[1][k]) for k in plain[1])
    for bad in (1, 9):
        with pytest.raises(ValueError):
            T.train_mlp_ensemble(X[:8], Y[:8], bad, 37, 12, device="cpu", log=None)


# ------------------------------------------------------------------------------------------ the rule on the host

@pytest.fixture(scope="module")
def host_rule(tmp_path_factory):
    """tests/native/ensemble_host.cpp (its own main; includes csrc/ensemble.h) built host-only with ASan + UBSan, as
    tests/test_iterations.py builds its program.  host_rule(members [n, rows, K], mode, kappa) -> (cost, sd)."""
    assert os.path.exists(HIPCC), "hipcc is needed to build the host form of the rule"
    d = tmp_path_factory.mktemp("ensemble")
    exe = str(d / "ensemble_host")
    cmd = [HIPCC, "-x", "hip", "--offload-host-only", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address",
           "-Xarch_host", "-fsanitize=undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           f"-I{REPO}/include", f"-I{PKG}/csrc", os.path.join(REPO, "tests", "native", "ensemble_host.cpp"),
           "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    src, dst = d / "in.bin", d / "out.bin"

    def run(members, mode, kappa):
        m = np.ascontiguousarray(np.asarray(members, np.float32))
        n, rows, K = m.shape
        m.tofile(src)
        r = subprocess.run([exe, str(src), str(n), str(rows), str(K), str(MODES.index(mode)),
                            repr(float(np.float32(kappa))), str(dst)], capture_output=True, text=True, timeout=240, env=env)
        assert r.returncode == 0, (r.returncode, (r.stdout + r.stderr)[-3000:])
        raw = np.fromfile(dst, np.float32)
        assert raw.size == 2 * rows * K
        return raw[:rows * K].reshape(rows, K), raw[rows * K:].reshape(rows, K)
    return run


def test_host_form_on_the_hand_written_rows(host_rule):
    from mppi_hip.stats import ensemble_combine_f32
    for name, members, mode, kappa, want_cost, want_sd in hand_cases():
        m = np.array(members, np.float32)[:, None, :]
        cost, sd = host_rule(m, mode, kappa)
        assert_hand(name, cost[0], sd[0], want_cost, want_sd)
        ref = ensemble_combine_f32(m, mode, kappa)
        assert same_bits(cost, ref[0]) and same_bits(sd, ref[1]), name


def test_host_form_equals_the_restatement_exactly(host_rule):
    """ensemble_row on the whole grid -- every n in 2..8, the three modes, kappa of both signs -- at K = 130 and K = 4:
    bitwise costs and spread against the numpy restatement."""
    from mppi_hip.stats import ensemble_combine_f32
    n_cases = 0
    for K in (130, 4):
        for name, n, mode, kappa, m in grid(K):
            cost, sd = host_rule(m, mode, kappa)
            ref = ensemble_combine_f32(m, mode, kappa)
            assert same_bits(cost, ref[0]), (name, K, "cost")
            assert same_bits(sd, ref[1]), (name, K, "sd")
            n_cases += 1
    assert n_cases == 2 * 7 * 3
