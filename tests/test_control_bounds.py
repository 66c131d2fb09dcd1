"""Per-actuator control bounds on the host (mppi_set_control_bounds; no GPU needed): the numpy reference's edge rules,
the four C entries' prototypes and NULL-handle paths, MPPIModel's argument check, and the host form of the rule
(csrc/ctrl_bounds.h) as a stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer, which must equal
mppi_hip.stats.project_noise_ref BITWISE, values and counts: the rule is a select and one subtract."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from bounds_cases import EDGE_KINDS, MAIN_SHAPES, bits, edge_case, main_case, share_ok
from conftest import PKG, REPO

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
ENTRIES = ("mppi_set_control_bounds", "mppi_get_control_bounds", "mppi_get_bound_counts", "mppi_bounds_eval")
INF = np.float32(np.inf)


# ------------------------------------------------------------------------------------------ the numpy reference

def test_reference_inside_the_box_is_untouched_and_uncounted():
    from mppi_hip.stats import project_noise_ref
    rs = np.random.RandomState(1)
    U, e = rs.randn(2, 3, 5).astype(np.float32), rs.randn(2, 3, 5, 9).astype(np.float32)
    out, n = project_noise_ref(U, e, -100.0, 100.0)
    assert out.dtype == np.float32 and n.dtype == np.uint32 and n.shape == (2, 3)
    assert np.array_equal(bits(out), bits(e)) and not n.any()
    out, n = project_noise_ref(U, e)  # the fully infinite box: count 0 and an identical array
    assert np.array_equal(bits(out), bits(e)) and not n.any()
    out, n = project_noise_ref(U, e, [-INF] * 3, [INF] * 3)
    assert np.array_equal(bits(out), bits(e)) and not n.any()
    s = (U[..., None] + e).astype(np.float32)  # a box that touches the extreme samples: s == lo / s == hi are inside
    out, n = project_noise_ref(U, e, s.min(axis=(0, 2, 3)), s.max(axis=(0, 2, 3)))
    assert np.array_equal(bits(out), bits(e)) and not n.any()
    o1, n1 = project_noise_ref(U[0], e[0], -100.0, 100.0)  # one solve
    assert o1.shape == e[0].shape and n1.shape == (3,)


def test_reference_projects_to_the_bound_minus_U():
    from mppi_hip.stats import project_noise_ref
    U = np.array([[[0.5, -1.0]]], np.float32)  # B = 1, nu = 1, H = 2
    e = np.array([[[[0.1, 2.0, -3.0], [0.2, 1.6, -0.5]]]], np.float32)
    out, n = project_noise_ref(U, e, [-1.5], [1.0])
    want = np.array([[[[0.1, np.float32(1.0) - np.float32(0.5), np.float32(-1.5) - np.float32(0.5)],
                       [0.2, 1.6, -0.5]]]], np.float32)  # row 1: s = -0.8, 0.6, -1.5 (== lo: inside)
    assert np.array_equal(bits(out), bits(want)) and n.tolist() == [[2]]
    out, n = project_noise_ref(U, e, [-2.8], [-0.9])  # a box that excludes zero
    s = np.clip((U[..., None] + e).astype(np.float32), np.float32(-2.8), np.float32(-0.9))
    moved = ((U[..., None] + e).astype(np.float32) != s)
    assert np.array_equal(out[moved], (s - U[..., None]).astype(np.float32)[moved]) and n.tolist() == [[int(moved.sum())]]
    assert np.array_equal(bits(out[~moved]), bits(e[~moved]))
    out, n = project_noise_ref(U, e, [0.25], [0.25])  # lo == hi pins the actuator
    assert np.array_equal(out, np.broadcast_to((np.float32(0.25) - U)[..., None], e.shape)) and n.tolist() == [[6]]
    pin = np.array([[[[np.float32(0.25) - np.float32(0.5)]]]], np.float32)  # s == lo == hi is inside: untouched
    out, n = project_noise_ref(U[:, :, :1], pin, [0.25], [0.25])
    assert np.array_equal(bits(out), bits(pin)) and n.tolist() == [[0]]
    out, n = project_noise_ref(U, e, None, [0.1])  # one-sided
    assert n.tolist() == [[3]] and np.array_equal(out[0, 0, :, 2], e[0, 0, :, 2])
    out, n = project_noise_ref(U, e, [0.0], None)
    assert n.tolist() == [[3]] and np.array_equal(out[0, 0, :, 1], e[0, 0, :, 1])


def test_reference_nonfinite_noise_and_U_outside_the_box():
    from mppi_hip.stats import project_noise_ref
    nan = np.float32(np.nan)
    U = np.array([[[0.5]]], np.float32)
    e = np.array([[[[nan, INF, -INF, 0.0]]]], np.float32)
    out, n = project_noise_ref(U, e, [-1.0], [1.0])
    assert np.array_equal(bits(out[..., 0]), bits(e[..., 0]))  # NaN untouched, bit for bit, and uncounted
    assert out[0, 0, 0, 1:].tolist() == [0.5, -1.5, 0.0] and n.tolist() == [[2]]  # +inf -> hi - U, -inf -> lo - U
    out, n = project_noise_ref(U, e, None, None)
    assert np.array_equal(bits(out), bits(e)) and n.tolist() == [[0]]
    Uo = np.full((2, 1, 3), 5.0, np.float32)  # U outside the box projects every element of that row
    eo = np.random.RandomState(2).randn(2, 1, 3, 30).astype(np.float32)
    out, n = project_noise_ref(Uo, eo, [-1.0], [1.0])
    assert n.tolist() == [[90], [90]] and np.all(out == np.float32(-4.0))
    Un = np.array([[[nan]]], np.float32)  # a NaN nominal: s is a NaN everywhere, nothing moves
    out, n = project_noise_ref(Un, e, [-1.0], [1.0])
    assert np.array_equal(bits(out), bits(e)) and n.tolist() == [[0]]


def test_reference_argument_errors():
    from mppi_hip.stats import project_noise_ref
    U, e = np.zeros((2, 3, 4), np.float32), np.zeros((2, 3, 4, 5), np.float32)
    nan = float("nan")
    for bad in ((U, e, [0.0, 1.0, 0.0], [1.0, 0.5, 1.0]), (U, e, nan, 1.0), (U, e, [0.0, nan, 0.0], None),
                (U, e, None, [1.0, nan, 1.0]), (U, e, [0.0, 0.0], [1.0, 1.0, 1.0]), (U, e, 1.0, 0.0),
                (U, e[:, :, :3], 0.0, 1.0), (U, e[0], 0.0, 1.0), (U[0, 0], e[0, 0], 0.0, 1.0)):
        with pytest.raises(ValueError):
            project_noise_ref(*bad)


@pytest.mark.parametrize("shape", MAIN_SHAPES, ids=lambda s: "B%d-nu%d-H%d-K%d" % s)
def test_main_cases_bind_on_a_fixed_share(shape):
    """The condition the GPU tests rest on, checked where no GPU is needed: every actuator of every main case projects
    between 5 % and 60 % of its elements, and some on each side of the box."""
    from mppi_hip.stats import project_noise_ref
    B, nu, H, K = shape
    U, e, lo, hi = main_case(B, nu, H, K)
    out, n = project_noise_ref(U, e, lo, hi)
    assert share_ok(n, H, K), (n / (H * K)).round(3)
    s = (U[..., None] + e).astype(np.float32)
    assert (s < lo[None, :, None, None]).any() and (s > hi[None, :, None, None]).any()
    s2 = (U[..., None] + out).astype(np.float32)  # within one rounding of the box (ctrl_bounds.h says why not inside)
    tol = np.spacing(np.maximum(np.abs(U), np.maximum(np.abs(lo), np.abs(hi))[None, :, None]))[..., None]
    assert np.all(s2 >= lo[None, :, None, None] - tol) and np.all(s2 <= hi[None, :, None, None] + tol)


# ------------------------------------------------------------------------------------------ the ABI

def test_ctypes_prototypes_and_null_handles():
    from mppi_hip import _lib as L
    lib = L.load()
    for name, nargs in zip(ENTRIES, (3, 4, 3, 6)):
        assert name in L.EXPORTED
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == nargs, name
    out = np.zeros(4, np.float32)
    p, fp = out.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(L._fp)
    calls = (lambda: lib.mppi_set_control_bounds(None, fp, fp), lambda: lib.mppi_get_control_bounds(None, None, None, None),
             lambda: lib.mppi_get_bound_counts(None, 1, p), lambda: lib.mppi_bounds_eval(None, 1, p, p, p, p))
    for name, call in zip(ENTRIES, calls):
        assert call() == L.MPPI_E_ARG, name
        assert name.encode() in lib.mppi_last_error(), name
    assert lib.mppi_abi_version() == 4  # additive


def test_header_declares_the_entries_and_the_engine_wraps_them():
    text = open(os.path.join(REPO, "include", "mppi.h")).read()
    for name in ENTRIES:
        assert f"int {name}(mppi_handle*" in text, name
    assert "#define MPPI_ABI_VERSION 4" in text and '"bounds"' in text
    from mppi_hip import Engine, project_noise_ref  # noqa: F401  (exported)
    for name in ("set_control_bounds", "control_bounds", "bound_counts", "bounds_eval"):
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
    monkeypatch.setattr(controller.Config, "preset", classmethod(lambda cls, name, **kw: cls(nx=4, nu=3, H=8, K=16)))
    monkeypatch.setattr(controller, "Engine", _Recorder)
    nan = float("nan")
    for bad in (dict(u_min=1.0, u_max=0.0), dict(u_min=nan), dict(u_max=[1.0, nan, 1.0]), dict(u_min=[0.0, 2.0, 0.0],
                u_max=[1.0, 1.0, 1.0]), dict(u_min=[0.0, 0.0]), dict(u_max=[1.0] * 4), dict(u_min="low"),
                dict(u_min=[0.0, 0.0], u_max=[1.0, 1.0, 1.0]), dict(u_min=[])):
        with pytest.raises(ValueError):
            controller.MPPIModel(**bad)
    controller.MPPIModel()  # the default asks for nothing
    assert not [c for c in _Recorder.calls if c[0] == "set_control_bounds"]
    m = controller.MPPIModel(u_min=-1.0, u_max=[1.0, 2.0, 3.0])  # a scalar spreads over the actuators
    (call,) = [c for c in _Recorder.calls if c[0] == "set_control_bounds"]
    assert call[1][0].tolist() == [-1.0] * 3 and call[1][1].tolist() == [1.0, 2.0, 3.0]
    assert m.u_min.tolist() == [-1.0] and m.u_max.tolist() == [1.0, 2.0, 3.0]
    controller.MPPIModel(u_max=0.5)  # one side only
    (call,) = [c for c in _Recorder.calls if c[0] == "set_control_bounds"]
    assert call[1][0] is None and call[1][1].tolist() == [0.5] * 3
    controller.MPPIModel(u_min=[-2.8, -1.0, 0.0], u_max=[-0.9, 1.0, 0.0])  # excluding zero, pinned: allowed


# ------------------------------------------------------------------------------------------ the rule on the host

@pytest.fixture(scope="module")
def host_rule(tmp_path_factory):
    """tests/native/ctrl_bounds_host.cpp (its own main; includes csrc/ctrl_bounds.h) built host-only with ASan + UBSan
    and run directly, as tests/test_control_cost.py builds control_cost_host.cpp.
    host_rule(U [B, nu, H], eps [B, nu, H, K], lo [nu], hi [nu]) -> (eps' [B, nu, H, K] f32, counts [B, nu] u32);
    with check=False it returns the program's exit status instead of asserting on it."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    d = tmp_path_factory.mktemp("ctrl_bounds")
    exe = str(d / "ctrl_bounds_host")
    cmd = [HIPCC, "-x", "hip", "--offload-host-only", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address",
           "-Xarch_host", "-fsanitize=undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           f"-I{REPO}/include", f"-I{PKG}/csrc", os.path.join(REPO, "tests", "native", "ctrl_bounds_host.cpp"),
           "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    count = [0]

    def run(U, eps, lo, hi, check=True):
        U, eps = np.ascontiguousarray(U, np.float32), np.ascontiguousarray(eps, np.float32)
        B, nu, H, K = eps.shape
        box = np.broadcast_to(np.stack([np.asarray(lo, np.float32), np.asarray(hi, np.float32)], axis=1)[None],
                              (B, nu, 2))
        count[0] += 1
        paths = [str(d / f"{n}_{count[0]}.f32") for n in ("U", "eps", "box", "out")]
        for a, p in zip((U, eps, np.ascontiguousarray(box)), paths):
            a.tofile(p)
        r = subprocess.run([exe] + paths + [str(B * nu), str(H), str(K)], capture_output=True, text=True, timeout=240,
                           env=env)
        if not check:
            return r.returncode
        assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
        n = np.array([int(x) for x in r.stdout.split()], np.uint32).reshape(B, nu)
        return np.fromfile(paths[3], np.float32).reshape(eps.shape), n
    return run


@pytest.mark.parametrize("shape", MAIN_SHAPES, ids=lambda s: "B%d-nu%d-H%d-K%d" % s)
def test_host_form_equals_the_reference_bitwise_main(host_rule, shape):
    from mppi_hip.stats import project_noise_ref
    U, e, lo, hi = main_case(*shape)
    want, n_want = project_noise_ref(U, e, lo, hi)
    assert share_ok(n_want, shape[2], shape[3])
    got, n_got = host_rule(U, e, lo, hi)
    assert np.array_equal(bits(got), bits(want)) and np.array_equal(n_got, n_want)


@pytest.mark.parametrize("first", range(len(EDGE_KINDS)))
def test_host_form_equals_the_reference_bitwise_edges(host_rule, first):
    """Every edge box on every actuator position (nu = 3 windows of the 7 kinds, and nu = 1), with a NaN, a +inf and a
    -inf in every row."""
    from mppi_hip.stats import project_noise_ref
    for B, nu, H, K in ((2, 3, 2, 30), (1, 1, 5, 7)):
        U, e, lo, hi, kinds = edge_case(B, nu, H, K, first)
        want, n_want = project_noise_ref(U, e, lo, hi)
        got, n_got = host_rule(U, e, lo, hi)
        assert np.array_equal(bits(got), bits(want)) and np.array_equal(n_got, n_want), kinds
        for u, kind in enumerate(kinds):
            if kind in ("wide", "infinite"):
                fin = np.isfinite(e[:, u]) if kind == "wide" else np.ones(e[:, u].shape, bool)
                assert np.array_equal(bits(got[:, u][fin]), bits(e[:, u][fin])), kind
            if kind == "infinite":
                assert not n_got[:, u].any()
            if kind == "U_outside":
                assert np.all(n_got[:, u] == H * K - H)  # all but the row's NaN


def test_host_form_rejects_a_bad_box(host_rule):
    U, e = np.zeros((1, 2, 2), np.float32), np.zeros((1, 2, 2, 3), np.float32)
    assert host_rule(U, e, [0.0, 0.0], [1.0, 1.0], check=False) == 0
    assert host_rule(U, e, [0.0, 2.0], [1.0, 1.0], check=False) == 3
    assert host_rule(U, e, [0.0, np.nan], [1.0, 1.0], check=False) == 3
    assert host_rule(U, e, [0.0, 0.0], [1.0, np.nan], check=False) == 3
