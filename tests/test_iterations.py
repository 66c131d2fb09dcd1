"""Inner iterations per control step on the host (mppi_set_iterations; no GPU needed): the numpy reference of the
best-sample tracking on rows written out by hand, the four C entries' prototypes and NULL-handle paths, the Engine /
MPPIModel wrappers and their argument checks, and the host form of the rule (csrc/iter_best.h) as a stand-alone program
under AddressSanitizer + UndefinedBehaviorSanitizer, held EXACTLY to the numpy reference on the grid of
tests/iter_cases.py."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import PKG, REPO
from iter_cases import bits, grid, hand_cases, inputs, same_bits, stored_for

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
ENTRIES = (("mppi_set_iterations", 4), ("mppi_get_iterations", 4), ("mppi_get_best", 6), ("mppi_iter_best_eval", 11))


def _stored(st):
    if st is None:
        return None
    v, cost, k, it = st
    return np.array(v, np.float32), np.float32(cost), np.int32(k), np.int32(it)


def _assert_best(got, want, msg):
    assert got[0].dtype == np.float32 and got[1].dtype == np.float32, msg
    assert got[2].dtype == np.int32 and got[3].dtype == np.int32, msg
    assert same_bits(got[0], want[0]), (msg, "v")
    assert np.array_equal(bits(got[1]), bits(want[1])), (msg, "cost")  # (-0.0 and +0.0 told apart)
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3]), (msg, "k / iter")


# ------------------------------------------------------------------------------------------ the numpy reference

@pytest.mark.parametrize("case", hand_cases(), ids=[c[0] for c in hand_cases()])
def test_reference_on_hand_written_rows(case):
    from mppi_hip.stats import iter_best_ref
    name, U, eps, costs, clamp, stored, it, want = case
    U, eps, costs = np.array(U, np.float32), np.array(eps, np.float32), np.array(costs, np.float32)
    st = _stored(stored)
    keep = None if st is None else [np.array(a).copy() for a in st]
    got = iter_best_ref(U, eps, costs, it=it, stored=st, ctrl_clamp=clamp)
    w = (np.array(want[0], np.float32), np.float32(want[1]), np.int32(want[2]), np.int32(want[3]))
    _assert_best([np.asarray(g) for g in got], w, name)
    if st is not None:  # the stored best carried in is not written
        for a, b in zip(st, keep):
            assert np.array_equal(np.asarray(a), b)
    # the batched form gives the same rows
    st2 = None if st is None else tuple(np.array([a, a]) for a in st)
    got2 = iter_best_ref(np.array([U, U]), np.array([eps, eps]), np.array([costs, costs]), it=it, stored=st2,
                         ctrl_clamp=clamp)
    for b in range(2):
        _assert_best([np.asarray(g[b]) for g in got2], w, (name, b))


def test_reference_rejects_bad_shapes():
    from mppi_hip.stats import iter_best_ref
    U, eps = inputs(2, 3, 4, 6)
    c = np.ones((2, 6), np.float32)
    with pytest.raises(ValueError):
        iter_best_ref(U, eps[:, :, :3], c)
    with pytest.raises(ValueError):
        iter_best_ref(U, eps, c[:, :5])
    with pytest.raises(ValueError):
        iter_best_ref(U[0], eps, c)


def test_reference_folded_over_iterations_never_rises():
    """Folding the rule over a step's iterations: the stored cost is the running minimum of the iterations' minima,
    iter names the first iteration that attained it."""
    from mppi_hip.stats import iter_best_ref
    B, nu, H, K = 2, 3, 7, 130
    rs = np.random.RandomState(3)
    st, mins = None, []
    for it in range(4):
        U, eps = inputs(B, nu, H, K, seed=it)
        c = rs.randn(B, K).astype(np.float32)
        if it == 2:
            c[:] = st[1][:, None]  # every sample reproduces the stored cost: nothing is replaced
        mins.append(c.min(axis=1))
        new = iter_best_ref(U, eps, c, it=it, stored=st, ctrl_clamp=0.0)
        if st is not None:
            assert np.all(new[1] <= st[1])
        st = new
    run = np.minimum.accumulate(np.array(mins), axis=0)
    assert np.array_equal(st[1], run[-1])
    assert np.array_equal(st[3], np.argmax(np.array(mins) == run[-1][None], axis=0).astype(np.int32))
    assert (st[3] != 2).all()


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
    r = ctypes.byref(n)
    for name, call in (("mppi_set_iterations", lambda: lib.mppi_set_iterations(None, 2, 0, 0)),
                       ("mppi_get_iterations", lambda: lib.mppi_get_iterations(None, r, r, r)),
                       ("mppi_get_best", lambda: lib.mppi_get_best(None, 1, p, p, p, p)),
                       ("mppi_iter_best_eval", lambda: lib.mppi_iter_best_eval(None, 1, p, p, p, 1, 0, p, p, p, p))):
        assert call() == L.MPPI_E_ARG, name
        assert name.encode() in lib.mppi_last_error(), name
    assert n.value == -7
    assert lib.mppi_abi_version() == 4  # additive


def test_header_declares_the_entries_and_every_layer_wraps_them():
    text = open(os.path.join(REPO, "include", "mppi.h")).read()
    jl = open(os.path.join(PKG, "julia", "MPPIHip.jl")).read()
    for name, _ in ENTRIES:
        assert f"int {name}(mppi_handle*" in text, name
    for name in ("mppi_set_iterations", "mppi_get_iterations", "mppi_get_best"):
        assert f":{name}" in jl, name
    for name in ("set_iterations!", "iterations", "best"):
        assert f"function {name}(c::Controller" in jl, name
    assert '"iter"' in text  # the kernel time name
    import mppi_hip
    for name in ("set_iterations", "iterations", "best", "iter_best_eval"):
        assert callable(getattr(mppi_hip.Engine, name))
    assert callable(mppi_hip.iter_best_ref) and "iter_best_ref" in mppi_hip.__all__
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "mppi_set_iterations" in open(os.path.join(REPO, doc)).read(), doc


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
    for bad in (0, -1, 17, 2.5, float("nan"), "3", None, True):
        with pytest.raises(ValueError):
            controller.MPPIModel(n_iter=bad)
    for bad in (1, "yes", None):
        with pytest.raises(ValueError):
            controller.MPPIModel(return_best=bad)
        with pytest.raises(ValueError):
            controller.MPPIModel(add_mean=bad)
    with pytest.raises(ValueError):
        controller.MPPIModel(n_iter=2, noise="numpy")  # one injected array cannot serve two iterations
    with pytest.raises(ValueError):
        controller.MPPIModel(n_iter=2, u0_before=True)
    with pytest.raises(ValueError):
        controller.MPPIModel(return_best=True, u0_before=True)
    controller.MPPIModel()  # the default asks for nothing
    assert not [c for c in _Recorder.calls if c[0] == "set_iterations"]
    controller.MPPIModel(n_iter=1, return_best=False, add_mean=False)
    assert not [c for c in _Recorder.calls if c[0] == "set_iterations"]
    for args in ((3, False, False), (1, True, False), (1, False, True), (np.int64(16), True, True)):
        m = controller.MPPIModel(n_iter=args[0], return_best=args[1], add_mean=args[2])
        want = ("set_iterations", (int(args[0]), args[1], args[2]))
        assert [c for c in _Recorder.calls if c[0] == "set_iterations"] == [want]
        assert (m.n_iter, m.return_best, m.add_mean) == (int(args[0]), args[1], args[2])
    # iteration i of a step draws key seed + i: consecutive steps' by-value seeds are n_iter apart
    m = controller.MPPIModel(n_iter=3, seed=5)
    s0, s1 = m.next_seed(), m.next_seed()
    assert s1 - s0 == 3 and s0 >> 32 == 5
    m = controller.MPPIModel(seed=5)
    assert m.next_seed() == (5 << 32) ^ 1 and m.next_seed() == (5 << 32) ^ 2  # as before


def test_engine_argument_checks_ahead_of_the_library():
    """The wrappers' own checks raise ValueError before any C call."""
    from mppi_hip.engine import Config, Engine

    class _Lib:
        def __getattr__(self, name):
            raise AssertionError(f"{name} reached the library")

    e = Engine.__new__(Engine)
    e.lib, e._h, e.config = _Lib(), None, Config(nx=4, nu=2, H=5, K=8)
    for bad in (2, "x", None):
        with pytest.raises(ValueError):
            e.set_iterations(2, return_best=bad)
        with pytest.raises(ValueError):
            e.set_iterations(2, add_mean=bad)
    with pytest.raises(ValueError):
        e.iter_best_eval(np.zeros((1, 2, 5)), np.zeros((1, 2, 5, 7)), np.zeros((1, 8)))
    with pytest.raises(ValueError):
        e.iter_best_eval(np.zeros((1, 2, 5)), np.zeros((1, 2, 5, 8)), np.zeros((1, 7)))
    with pytest.raises(ValueError):
        e.iter_best_eval(np.zeros((1, 2, 5)), np.zeros((1, 2, 5, 8)), np.zeros((1, 8)),
                         stored=(np.zeros((1, 2, 4)), [0.0], [0], [0]))
    e._h = None


# ------------------------------------------------------------------------------------------ the rule on the host

@pytest.fixture(scope="module")
def host_rule(tmp_path_factory):
    """tests/native/iter_best_host.cpp (its own main; includes csrc/iter_best.h) built host-only with ASan + UBSan, as
    tests/test_elite_keep.py builds its program.  host_rule(U, eps, costs, clamp, stored or None, it) -> (v, cost, k,
    iter)."""
    assert os.path.exists(HIPCC), "hipcc is needed to build the host form of the rule"
    d = tmp_path_factory.mktemp("iter_best")
    exe = str(d / "iter_best_host")
    cmd = [HIPCC, "-x", "hip", "--offload-host-only", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address",
           "-Xarch_host", "-fsanitize=undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           f"-I{REPO}/include", f"-I{PKG}/csrc", os.path.join(REPO, "tests", "native", "iter_best_host.cpp"),
           "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    src, dst = d / "in.bin", d / "out.bin"

    def run(U, eps, costs, clamp, stored, it):
        B, nu, H, K = eps.shape
        if stored is None:
            st = (np.full((B, nu, H), 5.0, np.float32), np.full(B, -3.0, np.float32), np.full(B, 77, np.int32),
                  np.full(B, 66, np.int32))  # (garbage a reset must not read)
        else:
            st = stored
        parts = [np.asarray(a, np.float32).ravel().view(np.uint32) for a in (U, eps, costs, st[0], st[1])]
        parts += [np.asarray(a, np.int32).ravel().view(np.uint32) for a in st[2:]]
        np.concatenate(parts).tofile(src)
        r = subprocess.run([exe, str(src), str(B), str(nu), str(H), str(K), repr(clamp), str(int(stored is None)),
                            str(it), str(dst)], capture_output=True, text=True, timeout=240, env=env)
        assert r.returncode == 0, (r.returncode, (r.stdout + r.stderr)[-3000:])
        raw = np.fromfile(dst, np.uint32)
        assert raw.size == B * nu * H + 3 * B
        p = np.split(raw, np.cumsum([B * nu * H, B, B]))
        return (p[0].view(np.float32).reshape(B, nu, H), p[1].view(np.float32), p[2].view(np.int32),
                p[3].view(np.int32))
    return run


def test_host_form_equals_the_reference_exactly(host_rule):
    """iter_best_row on the whole grid, with reset and with a stored best carried in: bitwise v and cost, integer k and
    iter against the numpy reference."""
    from mppi_hip.stats import iter_best_ref
    n_take = 0
    for name, B, nu, H, K, clamp, costs, reset in grid():
        U, eps = inputs(B, nu, H, K)
        eps[0, 0, 0, 0] = np.nan  # (a control that is not finite is stored as such)
        st = None if reset else stored_for(U, eps, costs)
        got = host_rule(U, eps, costs, clamp, st, 2)
        want = iter_best_ref(U, eps, costs, it=2, stored=st, ctrl_clamp=clamp)
        _assert_best(got, want, name)
        n_take += int((want[3] == 2).sum())
        if st is not None and B > 1 and np.isfinite(costs[1]).any():
            assert want[3][1] == 0 and want[2][1] == st[2][1]  # strictness: solve 1's equal cost stayed
    assert n_take > 0


def test_host_form_on_the_hand_written_rows(host_rule):
    for name, U, eps, costs, clamp, stored, it, want in hand_cases():
        U, eps = np.array([U], np.float32), np.array([eps], np.float32)
        st = _stored(stored)
        st = None if st is None else tuple(np.array([a]) for a in st)
        got = host_rule(U, eps, np.array([costs], np.float32), clamp, st, it)
        w = (np.array([want[0]], np.float32), np.array([want[1]], np.float32), np.array([want[2]], np.int32),
             np.array([want[3]], np.int32))
        _assert_best(got, w, name)
