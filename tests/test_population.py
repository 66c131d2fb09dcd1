"""Population-size decay on the host (mppi_set_population; no GPU needed): the rule's one header (csrc/population.h) as a
stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer -- iCEM's schedule held EXACTLY to the numpy
mirror on a grid, every invalid table refused, and the two-pitch reduce + generate pass restated as a plain loop with
the kernel's predicates -- plus the C entries' prototypes, the handle-free helper through ctypes and the wrappers."""
import ctypes
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import PKG, REPO

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
KS = (1, 33, 130, 1024, 32768)
GAMMAS = (1.0, 1.25, 1.3, 2.0, 3.0)
PITCHES = (64, 128, 192, 256, 1152)
# population.h PopError
OK, COUNT, FIRST, RANGE, ELITE, KEEP, MEAN = range(7)


def _grid():
    for K, g in itertools.product(KS, GAMMAS):
        for k_min in sorted({1, 26, K}):  # (26 > K: both sides refuse)
            for n in range(1, 17):
                yield K, n, g, k_min


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """tests/native/population_host.cpp (its own main; includes csrc/population.h) built host-only with ASan + UBSan, as
    tests/test_iterations.py builds its program.  host(*args) -> the lines it prints."""
    assert os.path.exists(HIPCC), "hipcc is needed to build the host form of the rule"
    d = tmp_path_factory.mktemp("population")
    exe = str(d / "population_host")
    cmd = [HIPCC, "-x", "hip", "--offload-host-only", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address",
           "-Xarch_host", "-fsanitize=undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           f"-I{REPO}/include", f"-I{PKG}/csrc", os.path.join(REPO, "tests", "native", "population_host.cpp"),
           "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")

    def run(*args):
        r = subprocess.run([exe] + [repr(a) if isinstance(a, float) else str(a) for a in args], capture_output=True,
                           text=True, timeout=240, env=env)
        assert r.returncode == 0, (args[:8], r.returncode, (r.stdout + r.stderr)[-3000:])
        return r.stdout.strip().split("\n")
    return run


# ------------------------------------------------------------------------------------------ iCEM's schedule

def test_numpy_mirror_by_hand():
    from mppi_hip.stats import icem_population
    got = icem_population(1024, 4, 2.0, 100)
    assert got.dtype == np.int32 and got.tolist() == [1024, 512, 256, 128]
    assert icem_population(130, 3, 1.25, 26).tolist() == [130, 104, 83]  # 130 / 1.5625 = 83.2
    assert icem_population(130, 5, 3.0, 26).tolist() == [130, 43, 26, 26, 26]
    assert icem_population(7, 3, 1.0, 1).tolist() == [7, 7, 7]
    assert icem_population(1, 2, 2.0, 1).tolist() == [1, 1]
    for bad in ((130, 3, 0.99, 1), (130, 3, float("nan"), 1), (130, 3, 2.0, 0), (130, 3, 2.0, 131), (130, 0, 2.0, 1),
                (130, 17, 2.0, 1), (0, 1, 2.0, 1)):
        with pytest.raises(ValueError):
            icem_population(*bad)


def test_host_schedule_equals_the_mirror_exactly(host):
    from mppi_hip.stats import icem_population
    cases = list(_grid())
    assert len(cases) >= 5 * 5 * 2 * 16 and any(c[3] > c[0] for c in cases)
    lines = host("icem", *[v for c in cases for v in c])
    assert len(lines) == len(cases)
    for c, line in zip(cases, lines):
        got = [int(v) for v in line.split()]
        if c[3] > c[0]:
            assert got == [1], c
            with pytest.raises(ValueError):
                icem_population(*c)
            continue
        want = icem_population(*c)
        assert got[0] == 0 and got[1:] == want.tolist(), (c, got, want)
        K, n, g, k_min = c
        assert want[0] == K and (np.diff(want) <= 0).all() and want.min() >= k_min
    for bad in ((130, 3, 0.5, 1), (130, 3, float("nan"), 1), (130, 3, 2.0, 0), (130, 3, 2.0, 131), (130, 0, 2.0, 1),
                (130, 17, 2.0, 1), (0, 1, 2.0, 1)):
        assert host("icem", *bad) == ["1"], bad


def test_c_helper_through_ctypes_equals_the_mirror():
    """mppi_population_icem needs no handle (and no GPU): the library's own answer on the grid."""
    from mppi_hip import _lib as L
    from mppi_hip.stats import icem_population
    lib = L.load()
    for c in _grid():
        tab = np.full(16, -1, np.int32)
        if c[3] > c[0]:
            assert lib.mppi_population_icem(c[0], c[1], c[2], c[3], tab.ctypes.data_as(ctypes.c_void_p)) == L.MPPI_E_ARG
            continue
        assert lib.mppi_population_icem(c[0], c[1], c[2], c[3], tab.ctypes.data_as(ctypes.c_void_p)) == L.MPPI_OK
        assert tab[: c[1]].tolist() == icem_population(*c).tolist() and (tab[c[1]:] == -1).all(), c
    tab = np.full(16, -1, np.int32)
    p = tab.ctypes.data_as(ctypes.c_void_p)
    for bad in ((130, 3, 0.5, 1), (130, 3, float("nan"), 1), (130, 3, 2.0, 0), (130, 3, 2.0, 131), (130, 0, 2.0, 1),
                (130, 17, 2.0, 1)):
        assert lib.mppi_population_icem(bad[0], bad[1], bad[2], bad[3], p) == L.MPPI_E_ARG, bad
        assert b"mppi_population_icem" in lib.mppi_last_error()
    assert lib.mppi_population_icem(130, 3, 2.0, 1, None) == L.MPPI_E_ARG
    assert (tab == -1).all()


# ------------------------------------------------------------------------------------------ the table's validity

def test_host_validation(host):
    def v(K, n_iter, n_elite, n_keep, add_mean, tab):
        return int(host("validate", K, n_iter, n_elite, n_keep, add_mean, len(tab), *tab)[0])
    assert v(130, 3, 0, 0, 0, (130, 70, 33)) == OK
    assert v(130, 3, 33, 33, 0, (130, 70, 33)) == OK
    assert v(130, 3, 33, 32, 1, (130, 70, 33)) == OK
    assert v(130, 3, 0, 0, 0, (130, 130, 130)) == OK
    assert v(130, 1, 0, 0, 0, (130,)) == OK
    assert v(130, 3, 0, 0, 0, (130, 33, 70)) == OK  # (not required to shrink)
    # n differs from the handle's n_iter
    assert v(130, 3, 0, 0, 0, (130, 70)) == COUNT
    assert v(130, 2, 0, 0, 0, (130, 70, 33)) == COUNT
    assert v(130, 1, 0, 0, 0, (130, 70, 33)) == COUNT
    assert v(130, 17, 0, 0, 0, (130,) * 17) == COUNT
    assert v(130, 0, 0, 0, 0, ()) == COUNT
    # K_it[0] != cfg.K
    assert v(130, 3, 0, 0, 0, (129, 70, 33)) == FIRST
    assert v(130, 3, 0, 0, 0, (131, 70, 33)) == FIRST
    # an entry outside [1, cfg.K]
    assert v(130, 3, 0, 0, 0, (130, 0, 33)) == RANGE
    assert v(130, 3, 0, 0, 0, (130, 70, -5)) == RANGE
    assert v(130, 3, 0, 0, 0, (130, 131, 33)) == RANGE
    # n_elite, n_keep, n_keep + 1 with add_mean
    assert v(130, 3, 34, 0, 0, (130, 70, 33)) == ELITE
    assert v(130, 3, 0, 34, 0, (130, 70, 33)) == KEEP
    assert v(130, 3, 0, 33, 1, (130, 70, 33)) == MEAN
    assert v(130, 3, 0, 33, 0, (130, 70, 33)) == OK
    assert v(130, 3, 71, 0, 0, (130, 70, 130)) == ELITE  # (any entry, not the last alone)
    # off / pitch
    assert host("off", 130, 3, 130, 130, 130) == ["1"] and host("off", 130, 3, 130, 129, 130) == ["0"]
    for K_i, Kp in ((1, 64), (33, 64), (64, 64), (65, 128), (70, 128), (130, 192), (200, 256), (1100, 1152),
                    (32768, 32768)):
        assert host("pitch", K_i) == [str(Kp)]


# ------------------------------------------------------------------------------------------ the two-pitch pass

@pytest.mark.parametrize("Kp", PITCHES)
def test_two_pitch_walk_writes_and_reads_every_quad_once(host, Kp):
    """The kernel's loop over (q0, j) with its predicates: every quad of the next row written exactly once, every quad
    of the read row consumed exactly once, in exactly the one-pitch loop's per-lane order (on which the sums' bits
    rest), in ceil(max(nq, nq_next) / 256) tiles."""
    for Kp_next in PITCHES:
        wmin, wmax, rmin, rmax, order, tiles = (int(x) for x in host("walk", Kp, Kp_next)[0].split())
        assert (wmin, wmax) == (1, 1), (Kp, Kp_next, "next-row quads written", wmin, wmax)
        assert (rmin, rmax) == (1, 1), (Kp, Kp_next, "read quads consumed", rmin, rmax)
        assert order == 1, (Kp, Kp_next)
        assert tiles == (max(Kp, Kp_next) // 4 + 255) // 256, (Kp, Kp_next, tiles)


# ------------------------------------------------------------------------------------------ the ABI and the wrappers

def test_ctypes_prototypes_and_null_handles():
    from mppi_hip import _lib as L
    lib = L.load()
    for name, nargs, res in (("mppi_set_population", 3, ctypes.c_int), ("mppi_get_population", 3, ctypes.c_int),
                             ("mppi_population_icem", 5, ctypes.c_int),
                             ("mppi_iter_rollout_kernel", 2, ctypes.c_char_p)):
        assert name in L.EXPORTED
        fn = getattr(lib, name)
        assert fn.restype is res and len(fn.argtypes) == nargs, name
    tab = np.array([130, 70, 33], np.int32)
    n = ctypes.c_int(-7)
    assert lib.mppi_set_population(None, tab.ctypes.data_as(ctypes.c_void_p), 3) == L.MPPI_E_ARG
    assert b"mppi_set_population" in lib.mppi_last_error()
    assert lib.mppi_get_population(None, None, ctypes.byref(n)) == L.MPPI_E_ARG and n.value == -7
    assert lib.mppi_iter_rollout_kernel(None, 0) == b""
    assert lib.mppi_abi_version() == 4  # additive


def test_header_declares_the_entries_and_every_layer_wraps_them():
    text = open(os.path.join(REPO, "include", "mppi.h")).read()
    for proto in ("int mppi_set_population(mppi_handle* h, const int32_t* K_it",
                  "int mppi_get_population(mppi_handle* h, int32_t* K_it",
                  "int mppi_population_icem(int K, int n_iter, double gamma, int k_min, int32_t* K_it",
                  "const char* mppi_iter_rollout_kernel(mppi_handle* h, int it)"):
        assert proto in text, proto
    import mppi_hip
    from mppi_hip import stats
    for name in ("set_population", "population", "iter_rollout_kernel"):
        assert callable(getattr(mppi_hip.Engine, name))
    assert callable(stats.icem_population)
    jl = open(os.path.join(PKG, "julia", "MPPIHip.jl")).read()
    for name in ("mppi_set_population", "mppi_get_population"):
        assert f":{name}" in jl, name
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "mppi_set_population" in open(os.path.join(REPO, doc)).read(), doc
    rule = open(os.path.join(PKG, "csrc", "population.h")).read()
    for name in ("pop_validate", "pop_pitch", "pop_icem", "pop_walk"):  # the rule in one header
        assert name in rule


def test_engine_wrappers_pass_the_table_through():
    from mppi_hip.engine import Config, Engine

    class _Lib:
        def __init__(self):
            self.calls = []

        def mppi_set_population(self, h, p, n):
            tab = None if p is None else np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_int32)), (n,)).copy()
            self.calls.append((None if tab is None else tab.tolist(), n))
            return 0

    e = Engine.__new__(Engine)
    e.lib, e._h, e.config = _Lib(), None, Config(nx=4, nu=2, H=5, K=130)
    assert e.set_population([130, 70, 33]) is e and e.set_population(np.array([130, 130])) is e
    assert e.set_population(None) is e
    assert e.lib.calls == [([130, 70, 33], 3), ([130, 130], 2), (None, 0)]
    with pytest.raises(ValueError):
        e.set_population([130, 2**40])
    e._h = None
