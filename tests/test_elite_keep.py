"""Keep / shift elites on the host (mppi_set_elite_keep; no GPU needed): the numpy references on rows written out by
hand, the consequence U + inject(store) == v within one ulp, the six C entries' prototypes and NULL-handle paths, the
Engine / MPPIModel wrappers and their argument checks, and the host form of the rule (csrc/elite_keep.h) as a
stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer, held EXACTLY to the numpy references on the
grid of tests/keep_cases.py."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import PKG, REPO
from keep_cases import bits, grid, hand_cases, hand_inject_cases, inputs, same_bits

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
ENTRIES = (("mppi_set_elite_keep", 2), ("mppi_get_elite_keep", 2), ("mppi_get_kept", 7), ("mppi_set_kept", 5),
           ("mppi_keep_store_eval", 11), ("mppi_keep_inject_eval", 8))


# ------------------------------------------------------------------------------------------ the numpy references

@pytest.mark.parametrize("case", hand_cases(), ids=[c[0] for c in hand_cases()])
def test_store_reference_on_hand_written_rows(case):
    from mppi_hip.stats import keep_store_ref
    _, U, eps, costs, n_keep, shift, clamp, v, kcost, idx, count, steps = case
    got = keep_store_ref(np.array(U, np.float32), np.array(eps, np.float32), np.array(costs, np.float32), n_keep,
                         shift=bool(shift), ctrl_clamp=clamp)
    assert got[0].dtype == np.float32 and got[1].dtype == np.float32
    assert got[2].dtype == np.int32 and got[3].dtype == np.int32 and got[4].dtype == np.int32
    assert np.array_equal(bits(got[0]), bits(np.array(v, np.float32)))  # (-0.0 and +0.0 told apart)
    assert np.array_equal(bits(got[1]), bits(np.array(kcost, np.float32)))
    assert np.array_equal(got[2], np.array(idx, np.int32))
    assert int(got[3]) == count and int(got[4]) == steps


@pytest.mark.parametrize("case", hand_inject_cases(), ids=[c[0] for c in hand_inject_cases()])
def test_inject_reference_on_hand_written_rows(case):
    from mppi_hip.stats import keep_inject_ref
    _, U, eps, v, count, steps, out = case
    eps = np.array(eps, np.float32)
    before = eps.copy()
    got = keep_inject_ref(np.array(U, np.float32), eps, np.array(v, np.float32), count, steps)
    assert got.dtype == np.float32 and same_bits(got, np.array(out, np.float32))
    assert same_bits(eps, before)  # the input is not written
    # the batched form gives the same rows
    got2 = keep_inject_ref(np.array([U, U], np.float32), np.array([before, before]), np.array([v, v], np.float32),
                           [count, count], [steps, steps])
    assert same_bits(got2[0], got) and same_bits(got2[1], got)


def test_references_reject_bad_arguments():
    from mppi_hip.stats import keep_inject_ref, keep_store_ref
    U, eps = inputs(2, 3, 4, 6)
    c = np.ones((2, 6), np.float32)
    for n in (0, 7, -1):
        with pytest.raises(ValueError):
            keep_store_ref(U, eps, c, n)
    with pytest.raises(ValueError):
        keep_store_ref(U, eps[:, :, :3], c, 2)
    with pytest.raises(ValueError):
        keep_store_ref(U, eps, c[:, :5], 2)
    v = np.zeros((2, 3, 4, 2), np.float32)
    for count, steps in (([3, 0], [4, 4]), ([-1, 0], [4, 4]), ([2, 2], [5, 0]), ([2, 2], [0, -1]), ([2], [4])):
        with pytest.raises(ValueError):
            keep_inject_ref(U, eps, v, count, steps)


@pytest.mark.parametrize("clamp", (0.0, 1.25))
def test_nominal_plus_injected_is_the_stored_control_within_one_ulp(clamp):
    """U unchanged and shift 0: U + inject(store) equals v within one ulp of max(|U|, |v|), column by column (the
    stored control is carried with at most one rounding), and equals what the rollout's own U + eps' would clamp to."""
    from mppi_hip.stats import keep_inject_ref, keep_store_ref
    B, nu, H, K, n_keep = 2, 3, 8, 130, 17
    U, eps = inputs(B, nu, H, K, seed=3)
    costs = np.random.RandomState(5).randn(B, K).astype(np.float32)
    v, kcost, idx, count, steps = keep_store_ref(U, eps, costs, n_keep, ctrl_clamp=clamp)
    assert (count == n_keep).all() and (steps == H).all()
    fresh = inputs(B, nu, H, K, seed=4)[1]
    out = keep_inject_ref(U, fresh, v, count, steps)
    assert same_bits(out[..., n_keep:], fresh[..., n_keep:])
    back = (U[..., None] + out[..., :n_keep]).astype(np.float32)
    ulp = np.spacing(np.maximum(np.abs(U[..., None]), np.abs(v)).astype(np.float32))
    assert np.all(np.abs(back.astype(np.float64) - v.astype(np.float64)) <= ulp)
    if clamp > 0:
        assert np.abs(v).max() <= clamp
        # beyond the clamp by at most that one rounding; the rollout clamps it back onto v
        assert np.all(np.abs(np.clip(back, -clamp, clamp).astype(np.float64) - v) <= ulp)


def test_store_reference_consequences():
    from mppi_hip.stats import elite_select_ref, keep_store_ref
    B, nu, H, K = 2, 3, 8, 130
    U, eps = inputs(B, nu, H, K)
    costs = np.random.RandomState(1).randn(B, K).astype(np.float32)
    costs[0, 5] = np.nan
    for n_keep in (1, 17, 70, K):
        v0, kc0, idx0, cnt0, st0 = keep_store_ref(U, eps, costs, n_keep, shift=False)
        v1, kc1, idx1, cnt1, st1 = keep_store_ref(U, eps, costs, n_keep, shift=True)
        want = elite_select_ref(costs, n_keep)
        assert np.array_equal(idx0, want[0]) and np.array_equal(cnt0, want[1])
        assert np.array_equal(idx1, idx0) and same_bits(kc1, kc0)  # the shift moves v alone
        assert (st0 == H).all() and (st1 == H - 1).all()
        assert same_bits(v1[:, :, :-1], v0[:, :, 1:]) and not v1[:, :, -1].any()
        for b in range(B):
            m = int(cnt0[b])
            assert same_bits(kc0[b, :m], costs[b, idx0[b, :m]]) and np.isposinf(kc0[b, m:]).all()
            assert np.array_equal(bits(v0[b, :, :, m:]), np.zeros_like(bits(v0[b, :, :, m:])))
    assert cnt0[0] == K - 1 and cnt0[1] == K  # the NaN is never kept


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
    for name, call in (("mppi_set_elite_keep", lambda: lib.mppi_set_elite_keep(None, 3)),
                       ("mppi_get_elite_keep", lambda: lib.mppi_get_elite_keep(None, ctypes.byref(n))),
                       ("mppi_get_kept", lambda: lib.mppi_get_kept(None, 1, p, p, p, p, p)),
                       ("mppi_set_kept", lambda: lib.mppi_set_kept(None, 1, p, p, p)),
                       ("mppi_keep_store_eval", lambda: lib.mppi_keep_store_eval(None, 1, p, p, p, 0, p, p, p, p, p)),
                       ("mppi_keep_inject_eval", lambda: lib.mppi_keep_inject_eval(None, 1, p, p, p, p, p, p))):
        assert call() == L.MPPI_E_ARG, name
        assert name.encode() in lib.mppi_last_error(), name
    assert n.value == -7
    assert lib.mppi_abi_version() == 4  # additive


def test_header_declares_the_entries_and_every_layer_wraps_them():
    text = open(os.path.join(REPO, "include", "mppi.h")).read()
    jl = open(os.path.join(PKG, "julia", "MPPIHip.jl")).read()
    for name, _ in ENTRIES:
        assert f"int {name}(mppi_handle*" in text, name
    for name in ("mppi_set_elite_keep", "mppi_get_elite_keep", "mppi_get_kept"):
        assert f":{name}" in jl, name
    for name in ("set_elite_keep!", "elite_keep", "kept"):
        assert f"function {name}(c::Controller" in jl, name
    assert '"keep"' in text  # the kernel time name
    import mppi_hip
    for name in ("set_elite_keep", "elite_keep", "kept", "set_kept", "keep_store_eval", "keep_inject_eval"):
        assert callable(getattr(mppi_hip.Engine, name))
    assert callable(mppi_hip.keep_store_ref) and callable(mppi_hip.keep_inject_ref)
    assert "keep_store_ref" in mppi_hip.__all__ and "keep_inject_ref" in mppi_hip.__all__


# ------------------------------------------------------------------------------------------ Engine / MPPIModel

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
            controller.MPPIModel(n_keep=bad)
    controller.MPPIModel()  # the default asks for nothing
    assert not [c for c in _Recorder.calls if c[0] == "set_elite_keep"]
    controller.MPPIModel(n_keep=0)
    assert not [c for c in _Recorder.calls if c[0] == "set_elite_keep"]
    for n in (1, 16, np.int64(5)):
        m = controller.MPPIModel(n_keep=n)
        assert [c for c in _Recorder.calls if c[0] == "set_elite_keep"] == [("set_elite_keep", (int(n),))]
        assert m.n_keep == int(n)
    m = controller.MPPIModel(n_keep=4, n_elite=4)  # both: each its own setter
    assert [c[0] for c in _Recorder.calls if c[0] in ("set_elites", "set_elite_keep")] == ["set_elites", "set_elite_keep"]


def test_engine_argument_checks_ahead_of_the_library():
    """The wrappers' own shape checks raise ValueError before any C call (a stand-in library that must not be reached
    beyond mppi_get_elite_keep)."""
    from mppi_hip.engine import Config, Engine

    class _Lib:
        def mppi_get_elite_keep(self, h, ref):
            ref._obj.value = 3
            return 0

        def __getattr__(self, name):
            raise AssertionError(f"{name} reached the library")

    e = Engine.__new__(Engine)
    e.lib, e._h, e.config = _Lib(), None, Config(nx=4, nu=2, H=5, K=8)
    assert e.elite_keep() == 3
    v = np.zeros((1, 2, 5, 3), np.float32)
    with pytest.raises(ValueError):
        e.set_kept(np.zeros((1, 2, 5, 4), np.float32), B=1)
    with pytest.raises(ValueError):
        e.set_kept(v, count=[1, 2])
    with pytest.raises(ValueError):
        e.set_kept(v, steps=[1, 2])
    with pytest.raises(ValueError):
        e.keep_inject_eval(np.zeros((1, 2, 5)), np.zeros((1, 2, 5, 8)), v[..., :2], [1], [1])
    with pytest.raises(ValueError):
        e.keep_inject_eval(np.zeros((1, 2, 5)), np.zeros((1, 2, 5, 8)), v, [1, 1], [1])
    e._h = None


# ------------------------------------------------------------------------------------------ the rule on the host

@pytest.fixture(scope="module")
def host_rule(tmp_path_factory):
    """tests/native/elite_keep_host.cpp (its own main; includes csrc/elite_keep.h) built host-only with ASan + UBSan, as
    tests/test_elites.py builds its program.  host_rule(U, eps, costs, U2, eps2, n_keep, shift, clamp) -> (v, kcost,
    idx, count, steps, eps2 after the injection)."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    d = tmp_path_factory.mktemp("elite_keep")
    exe = str(d / "elite_keep_host")
    cmd = [HIPCC, "-x", "hip", "--offload-host-only", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address",
           "-Xarch_host", "-fsanitize=undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           f"-I{REPO}/include", f"-I{PKG}/csrc", os.path.join(REPO, "tests", "native", "elite_keep_host.cpp"),
           "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    src, dst = d / "in.f32", d / "out.bin"

    def run(U, eps, costs, U2, eps2, n_keep, shift, clamp):
        B, nu, H, K = eps.shape
        np.concatenate([np.asarray(a, np.float32).ravel() for a in (U, eps, costs, U2, eps2)]).tofile(src)
        r = subprocess.run([exe, str(src), str(B), str(nu), str(H), str(K), str(n_keep), str(int(shift)), repr(clamp),
                            str(dst)], capture_output=True, text=True, timeout=240, env=env)
        assert r.returncode == 0, (r.returncode, (r.stdout + r.stderr)[-3000:])
        raw = np.fromfile(dst, np.uint32)
        nV, nK, nN = B * nu * H * n_keep, B * n_keep, B * nu * H * K
        assert raw.size == nV + 2 * nK + 2 * B + nN
        p = np.split(raw, np.cumsum([nV, nK, nK, B, B]))
        return (p[0].view(np.float32).reshape(B, nu, H, n_keep), p[1].view(np.float32).reshape(B, n_keep),
                p[2].view(np.int32).reshape(B, n_keep), p[3].view(np.int32), p[4].view(np.int32),
                p[5].view(np.float32).reshape(B, nu, H, K))
    return run


def _assert_exact(got, want, msg):
    for name, g, w in zip(("v", "kcost"), got[:2], want[:2]):
        assert same_bits(g, w), (msg, name)
    for name, g, w in zip(("idx", "count", "steps"), got[2:5], want[2:5]):
        assert np.array_equal(g, w), (msg, name)


def test_host_form_equals_the_references_exactly(host_rule):
    """keep_store_row and keep_inject_row on the whole grid: bitwise v, kcost and injected noise, integer idx, count
    and steps against the numpy references; the injection runs against another nominal than the store's."""
    from mppi_hip.stats import keep_inject_ref, keep_store_ref
    for name, B, nu, H, K, n_keep, shift, clamp, costs in grid():
        U, eps = inputs(B, nu, H, K)
        U2, eps2 = inputs(B, nu, H, K, seed=1)
        eps2[0, 0, 0, 0] = np.nan  # (a column the injection overwrites, or leaves: both must agree)
        got = host_rule(U, eps, costs, U2, eps2, n_keep, shift, clamp)
        want = keep_store_ref(U, eps, costs, n_keep, shift=bool(shift), ctrl_clamp=clamp)
        _assert_exact(got, want, name)
        assert same_bits(got[5], keep_inject_ref(U2, eps2, want[0], want[3], want[4])), (name, "inject")


def test_host_form_on_the_hand_written_rows(host_rule):
    for name, U, eps, costs, n_keep, shift, clamp, v, kcost, idx, count, steps in hand_cases():
        U, eps = np.array([U], np.float32), np.array([eps], np.float32)
        got = host_rule(U, eps, np.array([costs], np.float32), U, eps, n_keep, shift, clamp)
        want = (np.array([v], np.float32), np.array([kcost], np.float32), np.array([idx], np.int32),
                np.array([count], np.int32), np.array([steps], np.int32))
        for g, w, what in zip(got[:2], want[:2], ("v", "kcost")):
            assert np.array_equal(bits(g), bits(w)), (name, what)
        for g, w, what in zip(got[2:5], want[2:], ("idx", "count", "steps")):
            assert np.array_equal(g, w), (name, what)
