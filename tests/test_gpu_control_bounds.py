"""Per-actuator control bounds on the device (mppi_set_control_bounds): the projection kernel against its numpy
restatement BITWISE (the rule of csrc/ctrl_bounds.h is a select and one subtract), a bounded solve against an unbounded
one fed the projected noise, the contract lo <= U, u0 <= hi, the consumers of the projected noise at the bars their own
tests use, every stream form against a loop of plain solves, the launches per solve and the state rules of the four
entries.

The main cases (tests/bounds_cases.py) cut each actuator's box from the sampled controls themselves; every test that
relies on them first asserts, from project_noise_ref's counts, that every (solve, actuator) projects between 5 % and
60 % of its elements: the bounds neither never bind nor always bind."""
import ctypes

import numpy as np
import pytest

from bounds_cases import EDGE_KINDS, bits, edge_case, main_case, share_ok
from test_gpu_control_cost import _check_kernels, _env, _setup, _snap
from test_gpu_stats import _check_against_ref

pytestmark = pytest.mark.gpu

MLP_NU = 3
# the projection's forms, each forced in turn (read per launch): cached / nontemporal loads, quad / line stores, and the
# rows a wave takes -- 1, 2, 4 or 8 (the launcher picks by the size of the solve, and these small shapes alone would
# only ever reach the first two)
KNOBS = (dict(MPPI_BOUNDS_NT="0"), dict(MPPI_BOUNDS_NT="1"), dict(MPPI_BOUNDS_STORE="quad"),
         dict(MPPI_BOUNDS_STORE="line")) + tuple(dict(MPPI_BOUNDS_ROWS=str(r)) for r in (1, 2, 4, 8)) + (
             dict(MPPI_BOUNDS_ROWS="8", MPPI_BOUNDS_STORE="quad", MPPI_BOUNDS_NT="1"),)
FRAC, LIMITS = 0.25, (1e-3, 1e3)


@pytest.fixture(scope="module")
def M(gpu_available):
    import mppi_hip
    return mppi_hip


def _same(a, b, msg=""):
    assert np.array_equal(bits(a), bits(b)), (msg, a, b)


def _box(U0, e, lo_pct=15.0, hi_pct=80.0):
    """lo, hi [nu] cut from the sampled controls U0 + e (as bounds_cases.main_case cuts them)."""
    s = (U0[..., None] + e).astype(np.float32)
    nu = U0.shape[1]
    return (np.array([np.percentile(s[:, u], lo_pct) for u in range(nu)], np.float32),
            np.array([np.percentile(s[:, u], hi_pct) for u in range(nu)], np.float32))


def _inside(a, lo, hi):
    """every entry of a [B, nu, ...] inside [lo[u], hi[u]], exactly"""
    a = np.asarray(a)
    shape = (1, -1) + (1,) * (a.ndim - 2)
    return bool(np.all(a >= lo.reshape(shape)) and np.all(a <= hi.reshape(shape)))


# ------------------------------------------------------------------------------------------ 1. the projection kernel

@pytest.mark.parametrize("K", [30, 75, 1100])
def test_bounds_eval_equals_the_reference_bitwise(M, K):
    """No rollout: bounds_eval at K below a chunk with pad lanes / ragged / five 256-k chunks with a ragged last one,
    H in {1, 2, 17} (one row, two, more than a wave's eight), nu in {1, 3, 32}, B in {1, 3}: values and counts equal
    project_noise_ref exactly, under the default routing and every forced form of KNOBS (with H = 17 a wave's rows
    straddle two actuators and the last wave's tile is short: 17, 51 or 544 rows per solve), and the input is not
    written."""
    from mppi_hip.stats import project_noise_ref
    for H in (1, 2, 17):
        for nu in (1, 3, 32):
            eng = M.Engine(M.Config(nx=4, nu=nu, H=H, K=K, max_batch=3))
            for B in (1, 3):
                msg = (K, H, nu, B)
                U, e, lo, hi = main_case(B, nu, H, K)
                keep = e.copy()
                want, n_want = project_noise_ref(U, e, lo, hi)
                assert share_ok(n_want, H, K), (msg, n_want / (H * K))
                eng.set_control_bounds(lo, hi)
                got, n_got = eng.bounds_eval(U, e)
                _same(got, want, msg)
                assert n_got.dtype == np.uint32 and np.array_equal(n_got, n_want), (msg, n_got, n_want)
                for knob in KNOBS:
                    with _env(**knob):
                        g2, n2 = eng.bounds_eval(U, e)
                    _same(g2, want, (msg, knob))
                    assert np.array_equal(n2, n_want), (msg, knob)
                _same(e, keep, (msg, "the caller's noise"))
            eng.close()


@pytest.mark.parametrize("first", range(len(EDGE_KINDS)))
def test_bounds_eval_edge_boxes(M, first):
    """Every edge box of csrc/ctrl_bounds.h on every actuator position, a NaN, a +inf and a -inf in every row: a wide
    box and the infinite one leave the array as it is, a box excluding zero, a pinned actuator, one-sided boxes, and a
    nominal outside the box, bitwise the reference's."""
    from mppi_hip.stats import project_noise_ref
    for B, nu, H, K in ((3, 3, 2, 30), (1, 1, 17, 75), (2, 32, 1, 1100)):
        U, e, lo, hi, kinds = edge_case(B, nu, H, K, first)
        want, n_want = project_noise_ref(U, e, lo, hi)
        eng = M.Engine(M.Config(nx=4, nu=nu, H=H, K=K, max_batch=B))
        eng.set_control_bounds(lo, hi)
        for knob in ({},) + KNOBS:
            with _env(**knob):
                got, n_got = eng.bounds_eval(U, e)
            _same(got, want, (kinds, knob))
            assert np.array_equal(n_got, n_want), (kinds, knob, n_got, n_want)
        for u, kind in enumerate(kinds):
            if kind == "infinite":
                _same(got[:, u], e[:, u], kind)
                assert not n_got[:, u].any()
            if kind == "U_outside":
                assert np.all(n_got[:, u] == H * K - H)  # all but the row's NaN
        eng.close()


def test_pad_lanes_are_never_counted(M):
    """K = 30 (Kp = 64) with U wholly outside the box: every one of the H K elements projects and the count is H K -- a
    kernel that counted the 34 pad lanes of each row would say H Kp.  After a solve too, whose pads the generators
    fill."""
    from mppi_hip.stats import project_noise_ref
    B, nu, H, K = 3, 3, 17, 30
    rs = np.random.RandomState(4)
    U = np.full((B, nu, H), 50.0, np.float32)  # (far outside: no sample comes back into the box)
    e = rs.randn(B, nu, H, K).astype(np.float32)
    eng = M.Engine(M.Config(nx=4, nu=nu, H=H, K=K, max_batch=B))
    eng.set_control_bounds(-1.0, [1.0, 2.0, 0.5])
    for nt in ("0", "1"):
        with _env(MPPI_BOUNDS_NT=nt):
            got, n = eng.bounds_eval(U, e)
        assert np.all(n == H * K), n
        _same(got, project_noise_ref(U, e, -1.0, [1.0, 2.0, 0.5])[0])
    eng.close()
    eng, x0, U0 = _setup(M, "mlp", K, 7, 2)  # device noise: the chained form's generators write the pads too
    eng.set_control_bounds(-1.0, 1.0)
    eng.set_U(np.full_like(U0, 5.0))
    import torch
    dev = torch.device("cuda")
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    tx, tu0 = torch.from_numpy(x0).to(dev), torch.zeros(2, MLP_NU, device=dev)
    for _ in range(2):  # without the shift U stays at the clipped bound, 1: U + eps is outside about half the time
        eng.solve_device(2, tx.data_ptr(), None, None, seed=3, u0_ptr=tu0.data_ptr(), resident_U=True, chain=True)
        n = eng.bound_counts(2)
        assert np.all(n <= 7 * K), n
    eng.set_U(np.full_like(U0, 5.0))
    eng.solve_device(2, tx.data_ptr(), None, None, seed=3, u0_ptr=tu0.data_ptr(), resident_U=True, chain=True)
    assert np.all(eng.bound_counts(2) == 7 * K)
    eng.close()


# ------------------------------------------------------------------------------------------ 2. a bounded solve

@pytest.mark.parametrize("mode", [0, 1], ids=["add", "replace"])
@pytest.mark.parametrize("shift", [False, True], ids=["noshift", "shift"])
@pytest.mark.parametrize("H", [7, 1])
@pytest.mark.parametrize("kind", ["cartpole", "mlp"])
def test_a_bounded_solve_is_the_unbounded_solve_of_the_projected_noise(M, kind, H, shift, mode):
    """One handle has bounds and gets injected noise e; a second has none and gets project_noise_ref(U, e): costs and
    weights bitwise equal, U and u0 of the first np.clip of the second's, the same rollout kernel; the caller's e is not
    written; the counts are the reference's."""
    from mppi_hip.stats import project_noise_ref
    K, B = 130, 2
    eng, x0, U0 = _setup(M, kind, K, H, B, update_mode=mode)
    ref, _, _ = _setup(M, kind, K, H, B, update_mode=mode)
    nu = U0.shape[1]
    e = (eng.config.sigma * np.random.RandomState(5).randn(B, nu, H, K)).astype(np.float32)
    keep = e.copy()
    lo, hi = _box(U0, e)
    ep, n_want = project_noise_ref(U0, e, lo, hi)
    assert share_ok(n_want, H, K), n_want / (H * K)
    eng.set_control_bounds(lo, hi)
    got = eng.solve(x0, U0, noise=e, want_weights=True, shift=shift)
    want = ref.solve(x0, U0, noise=ep, want_weights=True, shift=shift)
    _same(got.costs, want.costs, "costs")
    _same(got.weights, want.weights, "weights")
    _same(got.U, np.clip(want.U, lo[None, :, None], hi[None, :, None]), "U")
    _same(got.u0, np.clip(want.u0, lo[None, :], hi[None, :]), "u0")
    assert eng.rollout_kernel() == ref.rollout_kernel() != ""
    assert np.array_equal(eng.bound_counts(B), n_want)
    _same(e, keep, "the caller's noise")
    assert _inside(got.U, lo, hi) and _inside(got.u0, lo, hi)
    assert not np.array_equal(bits(got.costs), bits(ref.solve(x0, U0, noise=e).costs))  # the box binds
    # a box that never binds: bit for bit the solve without bounds
    eng.set_control_bounds(-1e3, 1e3)
    wide, plain = eng.solve(x0, U0, noise=e, want_weights=True, shift=shift), ref.solve(x0, U0, noise=e,
                                                                                      want_weights=True, shift=shift)
    for name in ("costs", "weights", "U", "u0"):
        _same(getattr(wide, name), getattr(plain, name), name)
    assert not eng.bound_counts(B).any()
    # disabling restores the handle
    eng.set_control_bounds(None, None)
    off = eng.solve(x0, U0, noise=e, want_weights=True, shift=shift)
    for name in ("costs", "weights", "U", "u0"):
        _same(getattr(off, name), getattr(plain, name), name)
    for h in (eng, ref):
        h.close()


# ------------------------------------------------------------------------------------------ 3. the contract

def _solve_raw(eng, B, x0_ptr, U_ptr, u0_ptr, seed, flags):
    from mppi_hip import _lib as L
    io = L.mppi_io(x0_ptr, U_ptr, None, None, None, u0_ptr, None)
    return L.check(eng.lib.mppi_solve_ex(eng._h, B, ctypes.byref(io), ctypes.c_uint64(seed), flags))


@pytest.mark.parametrize("before", [False, True], ids=["u0_after", "u0_before"])
@pytest.mark.parametrize("mode", [0, 1], ids=["add", "replace"])
@pytest.mark.parametrize("kind", ["cartpole", "mlp"])
def test_U_and_u0_stay_inside_the_box(M, kind, mode, before):
    """A box that excludes zero on one actuator, shift_fill = 0 (the shift fills the last column with 0, outside that
    box) and U starting outside: after each of 6 shifted solves with device noise every entry of the resident U, of its
    device mirror (io.U with MPPI_FLAG_RESIDENT_U) and of u0 is inside the box exactly -- with MPPI_FLAG_U0_BEFORE too,
    whose u0 is the nominal the solve started from."""
    import torch
    from mppi_hip import _lib as L
    K, H, B = 130, 7, 2
    eng, x0, U0 = _setup(M, kind, K, H, B, update_mode=mode, shift_fill=0.0)
    nu = U0.shape[1]
    lo = np.array([0.2] if nu == 1 else [-0.3, -2.8, 0.1], np.float32)
    hi = np.array([0.9] if nu == 1 else [0.4, -0.9, 0.1], np.float32)  # (the third actuator pinned)
    assert not _inside(U0, lo, hi)
    eng.set_control_bounds(lo, hi)
    eng.set_U(U0)
    dev = torch.device("cuda")
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    tx, tU = torch.from_numpy(x0).to(dev), torch.zeros(B, nu, H, device=dev)
    tu0 = torch.zeros(B, nu, device=dev)
    flags = (L.FLAG_DEVICE | L.FLAG_SHIFT | L.FLAG_RESIDENT_U | L.FLAG_SEED_COUNTER | L.FLAG_ENV_STEP |
             (L.FLAG_U0_BEFORE if before else 0))
    for i in range(6):
        _solve_raw(eng, B, tx.data_ptr(), tU.data_ptr(), tu0.data_ptr(), 7, flags)
        Ures = eng.get_U(B)
        mirror, u0 = _snap(torch, tU, tu0)
        assert _inside(Ures, lo, hi), (i, Ures)
        _same(mirror, Ures, (i, "the mirror is the resident U"))
        assert _inside(u0, lo, hi), (i, u0)
        n = eng.bound_counts(B)
        assert np.all(n > 0) and np.all(n <= H * K), (i, n)
    eng.close()


# ------------------------------------------------------------------------------------------ 4. tied to what exists

@pytest.mark.parametrize("H", [7, 1])
def test_symmetric_bounds_at_zero_nominal_are_ctrl_clamp(M, H):
    """Cartpole, U = 0, bounds [-a, a], device noise: the costs are bitwise those of a handle without bounds and with
    cfg.ctrl_clamp = a and the same seed -- with U = 0 both evaluate exactly +-a where the noise is beyond it."""
    K, B, a, seed = 130, 2, 0.8, 12
    eng, x0, U0 = _setup(M, "cartpole", K, H, B)
    ref, _, _ = _setup(M, "cartpole", K, H, B, ctrl_clamp=a)
    Uz = np.zeros_like(U0)
    eng.set_control_bounds(-a, a)
    got, want = eng.solve(x0, Uz, seed=seed), ref.solve(x0, Uz, seed=seed)
    _same(got.costs, want.costs)
    n = eng.bound_counts(B)
    assert share_ok(n, H, K), n / (H * K)  # sigma = 1: about 42 % of the noise is beyond 0.8
    for h in (eng, ref):
        h.close()


# ------------------------------------------------------------------------------------------ 5. the consumers

@pytest.mark.parametrize("kind", ["cartpole", "mlp"])
def test_consumers_read_the_projected_noise(M, kind):
    """MPPI_FLAG_STATS' moments meet solve_stats_ref on the projected noise at tests/test_gpu_stats.py's bars, and
    with the control-cost term on mppi_get_control_term meets control_term_ref(U, project_noise_ref(U, e)) at the
    bounds of tests/test_gpu_control_cost.py; both differ from what the raw noise gives."""
    from mppi_hip.stats import project_noise_ref, solve_stats_ref
    K, H, B, gamma = 130, 7, 2, 0.7
    eng, x0, U0 = _setup(M, kind, K, H, B)
    nu, sigma = U0.shape[1], eng.config.sigma
    e = (sigma * np.random.RandomState(6).randn(B, nu, H, K)).astype(np.float32)
    lo, hi = _box(U0, e)
    ep, n = project_noise_ref(U0, e, lo, hi)
    assert share_ok(n, H, K)
    eng.set_control_bounds(lo, hi)
    res = eng.solve(x0, U0, noise=e, stats=True)
    ref = solve_stats_ref(res.costs, ep, eng.config.lambda_, eng.config.norm_eps)
    _check_against_ref(res.stats, ref)
    raw = solve_stats_ref(res.costs, e, eng.config.lambda_, eng.config.norm_eps)
    assert np.all(np.abs(raw["eps_m2"] - ref["eps_m2"]) > 1e-3 * ref["eps_m2"])  # (the raw noise would miss the bar)
    eng.set_control_cost(gamma)
    eng.solve(x0, U0, noise=e)
    term, lin = eng.control_term(B)
    _check_kernels(lin, term, U0, ep, np.full(nu, sigma), 0.0, gamma, kind)
    with pytest.raises(AssertionError):
        _check_kernels(lin, term, U0, e, np.full(nu, sigma), 0.0, gamma, kind)
    _same(term, eng.control_term_eval(U0, ep)[0], "the term of the projected noise")
    eng.close()


# ------------------------------------------------------------------------------------------ 6. streams

def _bounds_for(kind):
    return (np.array([-0.7], np.float32), np.array([0.8], np.float32)) if kind == "cartpole" else \
        (np.array([-0.4, -0.3, 0.05], np.float32), np.array([0.5, 0.6, 0.9], np.float32))


def _configure(eng, kind, full):
    eng.set_control_bounds(*_bounds_for(kind))
    if full:
        eng.set_noise_model(*(([0.6], 0.7) if kind == "cartpole" else ([0.2, 0.5, 0.8], 0.7)))
        eng.set_noise_adapt(0.3)
        eng.set_ess_target(FRAC, *LIMITS)
        eng.set_control_cost(0.5)


def _run_form(M, torch, kind, form, n, seed, full):
    """One stream form, n steps (device noise, seed counter, shift + env step) with bounds on (full: with
    set_noise_adapt, set_ess_target and set_control_cost too)."""
    from mppi_hip.trajectory import run_stream
    K, H, B = 130, 8, 2
    dev = torch.device("cuda")
    eng, x0, U0 = _setup(M, kind, K, H, B)
    _configure(eng, kind, full)
    out = {}
    if form == "traj":
        states, actions, U_end = run_stream(eng, x0, U0, n, seed=seed)
        out["traj"] = (states, actions)
        out["U"] = U_end
    else:
        eng.set_stream(torch.cuda.current_stream().cuda_stream)
        tx, tU = torch.from_numpy(x0).to(dev), torch.from_numpy(U0).to(dev)
        tu0 = torch.zeros(B, U0.shape[1], device=dev)
        if form == "graph":
            eng.graph_capture(B, n, tx.data_ptr(), tU.data_ptr(), tu0.data_ptr(), seed=seed)
            eng.graph_launch(sync=True)
        else:
            out["x_before"], out["u0_steps"] = [], []
            for i in range(n):
                if form == "plain":
                    out["x_before"].append(_snap(torch, tx)[0])
                eng.solve_device(B, tx.data_ptr(), tU.data_ptr(), None, seed=seed, u0_ptr=tu0.data_ptr(), shift=True,
                                 env_step=True, seed_counter=form == "plain", chain=form != "plain")
                if form == "plain":
                    out["u0_steps"].append(_snap(torch, tu0)[0])
        out["x"], out["U"], out["u0"] = _snap(torch, tx, tU, tu0)
    out["counts"] = eng.bound_counts(B)
    out["law"] = eng.noise_model() if full else None
    out["ctr"] = eng.get_seed_counter()
    eng.close()
    return out


@pytest.mark.parametrize("kind", ["cartpole", "mlp"])
@pytest.mark.parametrize("full", [False, True], ids=["bounds", "bounds+adapt+ess+term"])
def test_stream_forms_agree_bitwise(M, kind, full):
    """Plain counter solves, chained solves, one captured graph and graph_capture_traj via run_stream, five steps with
    SHIFT | ENV_STEP: bitwise equal U, u0 and states, the last solve's counts, the final law (full) and seed counter 5."""
    import torch
    n, seed, B = 5, 9, 2
    outs = {f: _run_form(M, torch, kind, f, n, seed, full) for f in ("plain", "chain", "graph", "traj")}
    want = outs["plain"]
    lo, hi = _bounds_for(kind)
    assert np.all(want["counts"] > 0) and np.all(want["counts"] < 8 * 130), want["counts"]  # the box binds, not always
    for form, got in outs.items():
        assert got["ctr"] == n, form
        _same(got["U"], want["U"], (form, "U"))
        assert _inside(got["U"], lo, hi), form
        if form != "traj":
            _same(got["x"], want["x"], (form, "x"))
            _same(got["u0"], want["u0"], (form, "u0"))
        assert np.array_equal(got["counts"], want["counts"]), (form, got["counts"], want["counts"])
        if full:
            _same(got["law"][0], want["law"][0], (form, "sigma_u"))
            assert got["law"][1] == want["law"][1] and got["law"][2] == want["law"][2], form
    states, actions = outs["traj"]["traj"]
    _same(states, np.stack(want["x_before"]), "logged states")
    _same(actions, np.stack(want["u0_steps"]), "logged controls")
    assert _inside(np.moveaxis(actions, 0, -1), lo, hi)


# ------------------------------------------------------------------------------------------ 7. launches per solve

@pytest.mark.parametrize("kind", ["cartpole", "mlp"])
def test_launches_per_solve(M, kind):
    """Bounds off: the counts of tests/test_gpu_control_cost.py's test_launches_per_solve, and "bounds" 0.  Bounds on:
    the same counts plus "bounds" once per solve -- the cartpole keeps its fused form (one rollout launch, no reduce);
    off again: as at first."""
    K, H, B = 130, 7, 2
    eng, x0, U0 = _setup(M, kind, K, H, B)
    names = ("noise", "rollout", "ctrl_cost", "lambda", "reduce", "stats", "bounds")

    def counts():
        eng.profile(True)  # (resets the counters)
        eng.solve(x0, U0, seed=3)
        got = {k: eng.kernel_time(k)[0] for k in names}
        ms = eng.kernel_time("bounds")[1]
        eng.profile(False)
        return got, ms

    fused = kind == "cartpole"
    off = dict(noise=1, rollout=1, ctrl_cost=0, reduce=0 if fused else 1, stats=0, bounds=0, **{"lambda": 0})
    assert counts() == (off, 0.0)
    eng.set_control_bounds(*_bounds_for(kind))
    got, ms = counts()
    assert got == dict(off, bounds=1) and ms > 0.0
    eng.set_control_cost(0.5)
    eng.set_ess_target(FRAC, *LIMITS)
    assert counts()[0] == dict(noise=1, rollout=1, ctrl_cost=1, reduce=1, stats=0, bounds=1, **{"lambda": 1})
    eng.set_ess_target(0.0)
    eng.set_control_cost(0.0)
    assert counts()[0] == dict(off, bounds=1)
    eng.set_control_bounds(None, None)
    assert counts() == (off, 0.0)
    eng.close()


# ------------------------------------------------------------------------------------------ 8. state and arguments

def test_state_and_argument_errors(M):
    from mppi_hip import _lib as L
    eng = M.Engine(M.Config(nx=4, nu=2, H=3, K=30, max_batch=2))
    U, nz = np.ones((2, 2, 3), np.float32), np.ones((2, 2, 3, 30), np.float32)
    lo, hi, active = eng.control_bounds()
    assert not active and np.all(lo == -np.inf) and np.all(hi == np.inf)
    with pytest.raises(M.MPPIError) as ei:  # the bounds are off
        eng.bounds_eval(U, nz)
    assert ei.value.code == L.MPPI_E_STATE
    with pytest.raises(M.MPPIError) as ei:  # no bounded solve has run
        eng.bound_counts(1)
    assert ei.value.code == L.MPPI_E_STATE
    eng.set_control_bounds([-0.5, 0.0], None)  # one side only
    lo, hi, active = eng.control_bounds()
    assert active and lo.tolist() == [-0.5, 0.0] and np.all(hi == np.inf)
    eng.set_control_bounds([-0.5, 0.0], [1.5, 0.25])
    out, n = eng.bounds_eval(U, nz)  # s = 2: beyond both upper bounds
    assert np.all(out[:, 0] == 0.5) and np.all(out[:, 1] == -0.75) and np.all(n == 90)
    with pytest.raises(M.MPPIError) as ei:
        eng.bounds_eval(np.ones((3, 2, 3), np.float32), np.ones((3, 2, 3, 30), np.float32))  # beyond max_batch
    assert ei.value.code == L.MPPI_E_ARG
    with pytest.raises(M.MPPIError) as ei:  # an evaluation is no solve
        eng.bound_counts(1)
    assert ei.value.code == L.MPPI_E_STATE
    nan = float("nan")
    fp = lambda v: np.asarray(v, np.float32).ctypes.data_as(L._fp)
    for blo, bhi in (([0.0, 2.0], [1.0, 1.0]), ([nan, 0.0], [1.0, 1.0]), ([0.0, 0.0], [1.0, nan])):  # refused, and
        # nothing changes
        assert eng.lib.mppi_set_control_bounds(eng._h, fp(blo), fp(bhi)) == L.MPPI_E_ARG, (blo, bhi)
        assert b"mppi_set_control_bounds" in eng.lib.mppi_last_error()
        lo, hi, active = eng.control_bounds()
        assert active and lo.tolist() == [-0.5, 0.0] and hi.tolist() == [1.5, 0.25]
    assert eng.lib.mppi_set_control_bounds(eng._h, fp([nan, 0.0]), None) == L.MPPI_E_ARG  # a NaN with one side NULL
    assert eng.control_bounds()[1].tolist() == [1.5, 0.25]
    with pytest.raises(ValueError):
        eng.set_control_bounds([0.0, 0.0, 0.0], None)  # not nu entries
    eng.set_control_bounds(None, None)
    assert not eng.control_bounds()[2]
    with pytest.raises(M.MPPIError) as ei:
        eng.bounds_eval(U, nz)
    assert ei.value.code == L.MPPI_E_STATE
    eng.close()
    big = M.Engine(M.Config(nx=4, nu=33, H=2, K=30))  # the box travels as a kernel argument
    with pytest.raises(M.MPPIError) as ei:
        big.set_control_bounds(-1.0, 1.0)
    assert ei.value.code == L.MPPI_E_UNSUPPORTED
    big.set_control_bounds(None, None)  # nothing to disable: fine at any nu
    assert not big.control_bounds()[2]
    big.close()


def test_set_control_bounds_destroys_graphs_and_keeps_the_prefetched_noise(M):
    import torch
    from mppi_hip import _lib as L
    K, H, B, n, seed = 130, 8, 2, 3, 21
    dev = torch.device("cuda")
    box1, box2 = _bounds_for("mlp"), (np.array([-0.2, -0.2, -0.2], np.float32), np.array([0.3, 0.3, 0.3], np.float32))

    def start():
        eng, x0, U0 = _setup(M, "mlp", K, H, B)
        eng.set_stream(torch.cuda.current_stream().cuda_stream)
        tx, tU = torch.from_numpy(x0).to(dev), torch.from_numpy(U0).to(dev)
        return eng, tx, tU, torch.zeros(B, MLP_NU, device=dev)

    def chain(eng, tx, tU, tu0, steps):
        for _ in range(steps):
            eng.solve_device(B, tx.data_ptr(), tU.data_ptr(), None, seed=seed, u0_ptr=tu0.data_ptr(), shift=True,
                             env_step=True, chain=True)
        return _snap(torch, tx, tU, tu0)

    def plain(eng, tx, tU, tu0):
        eng.solve_device(B, tx.data_ptr(), tU.data_ptr(), None, seed=seed, u0_ptr=tu0.data_ptr(), shift=True,
                         env_step=True, seed_counter=True)

    def refused(eng):
        with pytest.raises(M.MPPIError) as ei:
            eng.graph_launch(sync=True)
        assert ei.value.code == L.MPPI_E_STATE and "mppi_graph_capture first" in str(ei.value)

    eng, tx, tU, tu0 = start()
    capture = lambda: eng.graph_capture(B, n, tx.data_ptr(), tU.data_ptr(), tu0.data_ptr(), seed=seed)
    capture()
    eng.graph_launch(sync=True)  # leaves a prefetched noise: the device counter is one ahead
    assert eng.get_seed_counter() == n
    eng.set_control_bounds(None, None)  # off -> off: nothing to destroy
    eng.graph_launch(sync=True)
    eng.set_control_bounds(*box1)  # enabling destroys the graph, keeps the key sequence
    assert eng.get_seed_counter() == 2 * n
    refused(eng)
    with pytest.raises(M.MPPIError) as ei:  # enabling alone is no bounded solve
        eng.bound_counts(B)
    assert ei.value.code == L.MPPI_E_STATE
    capture()
    eng.graph_launch(sync=True)
    assert eng.get_seed_counter() == 3 * n
    eng.bound_counts(B)
    for bad in (B + 1, 0):
        with pytest.raises(M.MPPIError) as ei:
            eng.bound_counts(bad)
        assert ei.value.code == L.MPPI_E_ARG
    eng.set_control_bounds(*box1)  # the bounds in effect: a no-op, the graph stays
    eng.graph_launch(sync=True)
    eng.set_control_bounds(*box2)  # a change destroys it
    refused(eng)
    capture()
    eng.set_control_bounds(None, None)  # ... and so does disabling
    refused(eng)
    eng.close()

    # a prefetched noise survives set_control_bounds: a chain whose box changes after two steps goes on with the noise it
    # would have drawn -- what plain counter solves with the same switch draw; re-setting the box in effect (step 3)
    # disturbs nothing
    a = start()
    a[0].set_control_bounds(*box1)
    chain(*a, 2)
    a[0].set_control_bounds(*box2)
    chain(*a, 1)
    a[0].set_control_bounds(*box2)
    got = chain(*a, 1)
    assert a[0].get_seed_counter() == 4
    b = start()
    b[0].set_control_bounds(*box1)
    for i in range(4):
        if i == 2:
            b[0].set_control_bounds(*box2)
        plain(*b)
    want = _snap(torch, *b[1:])
    for x, y in zip(got, want):
        _same(x, y)
    assert np.array_equal(a[0].bound_counts(B), b[0].bound_counts(B))
    # ... and bounds_eval drops it with the key sequence unchanged, its counts in a slot of their own
    n_solve = a[0].bound_counts(B)
    U1, nz1 = np.ones((B, MLP_NU, H), np.float32), np.ones((B, MLP_NU, H, K), np.float32)
    assert np.all(a[0].bounds_eval(U1, nz1)[1] == H * K)
    assert np.array_equal(a[0].bound_counts(B), n_solve)
    assert a[0].get_seed_counter() == 4
    got = chain(*a, 1)
    plain(*b)
    for x, y in zip(got, _snap(torch, *b[1:])):
        _same(x, y)
    for e in (a[0], b[0]):
        e.close()
