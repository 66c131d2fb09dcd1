"""Elite truncation on the host (mppi_set_elites; no GPU needed): the numpy reference on rows written out by hand, the
four C entries' prototypes and NULL-handle paths, the Engine / MPPIModel wrappers and their argument checks, and the
host form of the rule (csrc/elite_select.h) as a stand-alone program under AddressSanitizer +
UndefinedBehaviorSanitizer, held EXACTLY to the numpy reference on the grid of tests/elite_cases.py."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import PKG, REPO
from elite_cases import FAMILIES, KS, family, hand_rows, n_elites

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
ENTRIES = (("mppi_set_elites", 2), ("mppi_get_elites", 2), ("mppi_get_elite_set", 5), ("mppi_elites_eval", 7))


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


# ------------------------------------------------------------------------------------------ the numpy reference

@pytest.mark.parametrize("case", hand_rows(), ids=[c[0] for c in hand_rows()])
def test_reference_on_hand_written_rows(case):
    from mppi_hip.stats import elite_select_ref
    _, row, n_elite, idx, count, tau, ecost = case
    c = np.array(row, np.float32)
    got_idx, got_count, got_tau, got_ecost = elite_select_ref(c, n_elite)
    assert got_idx.dtype == np.int32 and got_idx.tolist() == idx
    assert int(got_count) == count
    assert np.array_equal(_bits(got_tau), _bits(np.float32(tau))), (got_tau, tau)  # (+0.0 for a zero, bit for bit)
    want = np.array([np.inf if v is None else v for v in ecost], np.float32)
    assert np.array_equal(_bits(got_ecost), _bits(want)), (got_ecost, want)         # (-0.0 stays -0.0)
    # the batched form gives each row its own answer
    two = elite_select_ref(np.stack([c, c[::-1]]), n_elite)
    assert two[0][0].tolist() == idx and int(two[1][0]) == count
    assert np.array_equal(_bits(two[3][0]), _bits(want))


def test_reference_consequences():
    from mppi_hip.stats import elite_select_ref, solve_stats_ref
    for name in FAMILIES:
        c = family(name, 300)
        n = np.isfinite(c).sum(axis=1)
        for n_elite in (1, 7, 150, 300):
            idx, count, tau, ecost = elite_select_ref(c, n_elite)
            for b in range(2):
                m = min(n_elite, n[b])
                assert count[b] == m and np.isfinite(ecost[b]).sum() == m
                mem = idx[b, :m]
                assert np.all(np.diff(mem) > 0) and np.all(idx[b, m:] == -1)          # ascending k, -1 behind
                assert np.array_equal(_bits(ecost[b, mem]), _bits(c[b, mem]))         # the cost bit for bit
                off = np.setdiff1d(np.arange(300), mem)
                assert np.all(np.isposinf(ecost[b, off]))
                assert c[b, mem].max() == tau[b]
                fin_off = off[np.isfinite(c[b, off])]
                assert fin_off.size == 0 or c[b, fin_off].min() >= tau[b]             # nothing better was left out
                k_best = int(np.flatnonzero(c[b] == np.nanmin(np.where(np.isfinite(c[b]), c[b], np.nan)))[0])
                assert k_best in mem                                                  # the statistics' k_best is elite
                assert solve_stats_ref(ecost[b], lam=1.0)["k_best"] == k_best
        full = elite_select_ref(c, 300)[3]  # n_elite >= n: the weighted set is the finite set
        assert np.array_equal(np.isfinite(full), np.isfinite(c))
    for bad in (0, -1, 301):
        with pytest.raises(ValueError):
            elite_select_ref(family("gauss", 300), bad)


# ------------------------------------------------------------------------------------------ the ABI

def test_ctypes_prototypes_and_null_handles():
    from mppi_hip import _lib as L
    lib = L.load()
    for name, nargs in ENTRIES:
        assert name in L.EXPORTED
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == nargs, name
    out = np.zeros(4, np.float32)
    p = out.ctypes.data_as(ctypes.c_void_p)
    n = ctypes.c_int(-7)
    for name, call in (("mppi_set_elites", lambda: lib.mppi_set_elites(None, 3)),
                       ("mppi_get_elites", lambda: lib.mppi_get_elites(None, ctypes.byref(n))),
                       ("mppi_get_elite_set", lambda: lib.mppi_get_elite_set(None, 1, p, p, p)),
                       ("mppi_elites_eval", lambda: lib.mppi_elites_eval(None, 1, p, p, p, p, p))):
        assert call() == L.MPPI_E_ARG, name
        assert name.encode() in lib.mppi_last_error(), name
    assert n.value == -7
    assert lib.mppi_abi_version() == 4  # additive


def test_header_declares_the_entries_and_every_layer_wraps_them():
    text = open(os.path.join(REPO, "include", "mppi.h")).read()
    jl = open(os.path.join(PKG, "julia", "MPPIHip.jl")).read()
    for name, _ in ENTRIES:
        assert f"int {name}(mppi_handle*" in text, name
        assert f":{name}" in jl, name
    assert '"elites"' in text  # the kernel time name
    import mppi_hip
    for name in ("set_elites", "elites", "elite_set", "elites_eval"):
        assert callable(getattr(mppi_hip.Engine, name))
    assert callable(mppi_hip.elite_select_ref)
    from mppi_hip.distributed import combine_k_shards
    assert "elites_eval" in combine_k_shards.__doc__


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
    for bad in (-1, 17, 2.5, float("nan"), "3", None, True):
        with pytest.raises(ValueError):
            controller.MPPIModel(n_elite=bad)
    controller.MPPIModel()  # the default asks for nothing
    assert not [c for c in _Recorder.calls if c[0] == "set_elites"]
    controller.MPPIModel(n_elite=0)
    assert not [c for c in _Recorder.calls if c[0] == "set_elites"]
    for n in (1, 16, np.int64(5)):
        m = controller.MPPIModel(n_elite=n)
        assert [c for c in _Recorder.calls if c[0] == "set_elites"] == [("set_elites", (int(n),))]
        assert m.n_elite == int(n)


# ------------------------------------------------------------------------------------------ the rule on the host

@pytest.fixture(scope="module")
def host_rule(tmp_path_factory):
    """tests/native/elite_select_host.cpp (its own main; includes csrc/elite_select.h) built host-only with ASan +
    UBSan, as tests/test_ess_target.py builds its program.  host_rule(costs [B, K], n_elite) -> (idx, count, tau,
    ecost, key)."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    d = tmp_path_factory.mktemp("elites")
    exe = str(d / "elite_select_host")
    cmd = [HIPCC, "-x", "hip", "--offload-host-only", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address",
           "-Xarch_host", "-fsanitize=undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           f"-I{REPO}/include", f"-I{PKG}/csrc", os.path.join(REPO, "tests", "native", "elite_select_host.cpp"),
           "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    src, dst = d / "costs.f32", d / "out.bin"

    def run(costs, n_elite):
        costs = np.ascontiguousarray(costs, np.float32)
        B, K = costs.shape
        costs.tofile(src)
        r = subprocess.run([exe, str(src), str(B), str(K), str(n_elite), str(dst)], capture_output=True, text=True,
                           timeout=240, env=env)
        assert r.returncode == 0, (r.returncode, (r.stdout + r.stderr)[-3000:])
        raw = np.fromfile(dst, np.uint32)
        assert raw.size == B * n_elite + 2 * B + 2 * B * K
        parts = np.split(raw, np.cumsum([B * n_elite, B, B, B * K]))
        return (parts[0].view(np.int32).reshape(B, n_elite), parts[1].view(np.int32), parts[2].view(np.float32),
                parts[3].view(np.float32).reshape(B, K), parts[4].reshape(B, K))
    return run


def _assert_exact(got, want, msg):
    for name, g, w in zip(("idx", "count"), got[:2], want[:2]):
        assert np.array_equal(g, w), (msg, name)
    for name, g, w in zip(("tau", "ecost"), got[2:4], want[2:4]):
        assert np.array_equal(_bits(g), _bits(w)), (msg, name)


@pytest.mark.parametrize("K", KS)
def test_host_form_equals_the_reference_exactly(host_rule, K):
    """elite_select_row on every family x the n_elite grid: integer indices and bitwise tau / ecost against the numpy
    reference; elite_key orders the finite costs as the stable sort does."""
    from mppi_hip.stats import elite_select_ref
    for name in FAMILIES:
        c = family(name, K)
        grid = n_elites(c) if K < 32768 else [K // 10, K]
        for n_elite in grid:
            got = host_rule(c, n_elite)
            _assert_exact(got, elite_select_ref(c, n_elite), (name, K, n_elite))
        key = got[4]
        for b in range(c.shape[0]):
            fin = np.flatnonzero(np.isfinite(c[b]))
            assert np.all(key[b, ~np.isfinite(c[b])] == 0xFFFFFFFF) and np.all(key[b, fin] < 0xFF800000)
            assert np.array_equal(np.argsort(key[b, fin], kind="stable"), np.argsort(c[b, fin], kind="stable"))


def test_host_form_on_the_hand_written_rows(host_rule):
    for name, row, n_elite, idx, count, tau, ecost in hand_rows():
        c = np.array([row], np.float32)
        got = host_rule(c, n_elite)
        want = (np.array([idx], np.int32), np.array([count], np.int32), np.array([tau], np.float32),
                np.array([[np.inf if v is None else v for v in ecost]], np.float32))
        _assert_exact(got, want, name)
    # the key: -0.0 and +0.0 alike, denormals apart and in order, the sign boundary
    den = np.float32(1e-45)
    c = np.array([[-np.float32(3e38), -1.0, -den, -0.0, 0.0, den, 2 * den, 1.0, np.float32(3e38)]], np.float32)
    key = host_rule(c, 1)[4][0]
    assert key[3] == key[4] == 0x80000000
    assert np.all(np.diff(key[[0, 1, 2, 3]].astype(np.int64)) > 0) and np.all(np.diff(key[4:].astype(np.int64)) > 0)
