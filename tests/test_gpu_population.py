"""Population-size decay on the device (mppi_set_population): a table of cfg.K throughout is the handle that never called
the setter; with a table on, iteration i of a control step is, bit for bit, the solve of a handle created with cfg.K =
K_it[i] -- the defining loop, driven over one handle per sample count with the state handed over -- in every stream
form, bare and under the CEM stack; the two-pitch form of the fused reduce + generate against that loop and against the
overlap stream; the best sample against the numpy reference folded over the loop; the per-iteration routes; and the
state rules of the entries.  Every comparison is bitwise.

The defining loop hands over, from handle to handle: U and x0 (shared device tensors, or host arrays), the kept set
(kept / set_kept), the per-step scale table (noise_steps / set_noise_steps), u_prev (prev_control / set_prev_control)
and the seed counter (set_seed_counter).  The stacks are bare and cem as _stack defines them; the adapted per-actuator
law (set_noise_adapt) and the adapted covariance (set_noise_cov_adapt) have no setter for their device state and are
not part of either stack, so they are left out."""
import ctypes
import os

import numpy as np
import pytest

from conftest import REPO
from iter_cases import bits, same_bits

pytestmark = pytest.mark.gpu

K0, B0, SEED = 130, 2, 7  # Kp = 192: the pads are live
TABLE = (130, 70, 33)     # Kp 192, 128, 64
MLP_NX, MLP_NU = 10, 3
KERNELS = ("noise", "rollout", "reduce", "update", "stats", "lambda", "ctrl_cost", "bounds", "rate_cost", "elites",
           "keep", "cross", "cov_adapt", "step_mom", "step_adapt")
BOX = 0.3
H_OF = {"mlp": 7, "ca": 5, "cartpole": 9}


@pytest.fixture(scope="module")
def M(gpu_available):
    import mppi_hip
    return mppi_hip


def _setup(M, kind, H, K=K0, B=B0, **kw):
    """(engine, x0 [B, nx] f32, U0 [B, nu, H] f32): the seeded synthetic MLP (nx 10, nu 3, fp32, quad_est), the golden
    CrossAttention humanoid at bf16 (precision= overrides), or the cartpole preset.  x0 and U0 do not depend on K."""
    rs = np.random.RandomState(11)
    if kind == "ca":
        sd = M.load_npz(os.path.join(REPO, "tests", "golden", "ca_humanoid_weights.npz"))
        kw.setdefault("precision", 1)
        eng = M.Engine(M.Config.preset("humanoid_v3", K=K, H=H, max_batch=B, **kw))
        eng.load_dynamics(*M.cross_attention_blob(sd)).set_cost("humanoid_v3")
        x0 = np.load(os.path.join(REPO, "tests", "golden", "g5_ca_humanoid_fwd.npz"))["x0_stride20"][:B]
    elif kind == "cartpole":
        eng = M.Engine(M.Config.preset("cartpole_py", K=K, H=H, max_batch=B, **kw))
        eng.load_dynamics(1).set_cost("cartpole")
        x0 = np.stack([[0.0, 0.2 + 0.3 * b, 0.0, 0.0] for b in range(B)])
    else:
        from mppi_hip.nets import mlp_blob, synthetic_mlp
        cfg = dict(nx=MLP_NX, nu=MLP_NU, H=H, K=K, max_batch=B, lambda_=1.0, sigma=0.5, precision=0)
        cfg.update(kw)
        eng = M.Engine(M.Config(**cfg))
        eng.load_dynamics(*mlp_blob(synthetic_mlp(MLP_NX, MLP_NU, seed=0), MLP_NX, MLP_NU))
        eng.set_cost("quad_est")
        x0 = 0.3 * rs.randn(B, MLP_NX)
    U0 = 0.1 * rs.randn(B, eng.config.nu, H)
    return eng, np.ascontiguousarray(x0, np.float32), U0.astype(np.float32)


def _stack(eng, kind, stack, B=B0):
    """bare: nothing (the cartpole pinned to its unfused form on both sides: the iterations take it there, and the fused
    one-launch form differs from reduce_kernel in the last bits).
    cem: elites, kept elites, the per-step scale table with its refit, bounds that bind, the anchored rate term and the
    ESS-targeted temperature."""
    c = eng.config
    if stack == "cem":
        sig = (0.2 + 0.6 * np.arange(c.nu) / max(c.nu - 1, 1)).astype(np.float32)
        eng.set_elites(13)
        eng.set_elite_keep(5)
        eng.set_noise_model(sig, 0.5)
        eng.set_noise_steps((0.1 + 0.9 * np.random.RandomState(3).rand(B, c.nu, c.H)).astype(np.float32))
        eng.set_noise_steps_adapt(0.5, 0.01, 3.0, centred=True)
        eng.set_control_bounds(-BOX, BOX)
        eng.set_rate_cost(0.05, anchor=True)
        eng.set_ess_target(0.2)
    elif kind == "cartpole":
        eng.set_ess_target(0.25, c.lambda_, c.lambda_)
    return eng


def _has_lambda(kind, stack):
    return stack == "cem" or kind == "cartpole"


def _eq(a, b, msg):
    """Bitwise: floats by their bits (a NaN equals a NaN), everything else by value; tuples and dicts member by member."""
    if isinstance(a, dict):
        assert a.keys() == b.keys(), msg
        for k in a:
            _eq(a[k], b[k], (msg, k))
    elif isinstance(a, (tuple, list)):
        assert len(a) == len(b), msg
        for i, (x, y) in enumerate(zip(a, b)):
            _eq(x, y, (msg, i))
    elif a is None or b is None:
        assert a is None and b is None, msg
    else:
        a, b = np.asarray(a), np.asarray(b)
        assert a.shape == b.shape and a.dtype == b.dtype, (msg, a.shape, b.shape, a.dtype, b.dtype)
        if a.dtype == np.float32:
            assert same_bits(a, b), (msg, a, b)
        else:
            assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), (msg, a, b)


def _readouts(eng, stack, B=B0):
    out = {"ctr": eng.get_seed_counter()}
    if stack == "cem":
        out["kept"] = eng.kept(B)
        out["steps"] = eng.noise_steps(B)
        out["uprev"] = eng.prev_control(B)
    return out


def _slot(eng, kind, stack, step, B=B0):
    """What one iteration leaves in its per-step slot: its statistics and, where a search ran, its lambdas."""
    return {"stats": eng.stats(B, step), "lam": eng.lambdas(B, step) if _has_lambda(kind, stack) else None}


def _snap(torch, *ts):
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in ts)


def _tensors(torch, eng, x0, U0, K=None):
    dev = torch.device("cuda")
    c = eng.config
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    return (torch.from_numpy(x0).to(dev), torch.from_numpy(U0).to(dev), torch.zeros(x0.shape[0], c.nu, device=dev),
            torch.full((x0.shape[0], c.K if K is None else K), -1.0, device=dev))


def _state(eng, stack, B):
    """What a cem iteration leaves for the next one beyond U and x0 (None for bare)."""
    if stack != "cem":
        return None
    return dict(kept=eng.kept(B), steps=eng.noise_steps(B), uprev=eng.prev_control(B))


def _hand_over(eng, state):
    if state is None:
        return
    v, _, _, count, steps = state["kept"]
    eng.set_kept(v, count, steps)
    eng.set_noise_steps(state["steps"])
    eng.set_prev_control(state["uprev"])


# ------------------------------------------------------------------------------------------ the defining loop

_LOOPS = {}


def _loop(M, torch, kind, table, stack, steps=3, B=B0, H=None, chained=False):
    """The defining loop on device pointers: one handle per K_it[i] at n_iter = 1, driven in turn on the seed counter
    with the state handed over; `steps` control steps, shift and env step on each step's last iteration.  Cached: the
    device forms share it.
    chained: the handles' solves are chained solves (the definition's "same stream form").  Up to 512 samples a plain
    solve and a chained one agree bitwise (tests/test_gpu_iterations.py holds the streams to the plain loop) and the
    plain loop serves every form; beyond, the plain reduce's 512 threads and the stream forms' 1024 partition the
    softmin sum differently, so a stream form is held to the loop of chained solves."""
    H = H_OF[kind] if H is None else H
    key = (kind, tuple(table), stack, steps, B, H, chained)
    if key in _LOOPS:
        return _LOOPS[key]
    n = len(table)
    engs, x0, U0 = [], None, None
    for k in table:
        e, x0, U0 = _setup(M, kind, H, K=k, B=B)
        engs.append(_stack(e, kind, stack, B))
    tx, tU, tu0, _ = _tensors(torch, engs[0], x0, U0)
    tcs = []
    for e, k in zip(engs, table):
        e.set_stream(torch.cuda.current_stream().cuda_stream)
        tcs.append(torch.zeros(B, k, device=torch.device("cuda")))
    out = {"x_before": [], "u0": [], "state": [], "slots": [], "read": [], "kernels": [None] * n}
    state, ctr = None, 0
    for s in range(steps):
        out["x_before"].append(_snap(torch, tx)[0])
        slots = []
        for i, e in enumerate(engs):
            last = i == n - 1
            _hand_over(e, state)
            e.set_seed_counter(ctr)
            e.solve_device(B, tx.data_ptr(), tU.data_ptr(), None, seed=SEED, u0_ptr=tu0.data_ptr(),
                           costs_ptr=tcs[i].data_ptr(), shift=last, env_step=last, seed_counter=True,
                           asynchronous=False, stats=True, chain=chained)
            slots.append(_slot(e, kind, stack, 0, B))
            out["kernels"][i] = e.rollout_kernel()
            ctr = e.get_seed_counter()
            state = _state(e, stack, B)
        out["slots"].append(slots)
        out["state"].append(_snap(torch, tx, tU, tu0, tcs[-1]))
        out["u0"].append(out["state"][-1][2])
        out["read"].append(_readouts(engs[-1], stack, B))
    for e in engs:
        e.close()
    _LOOPS[key] = out
    return out


def _decayed(M, kind, table, stack, B=B0, H=None, **kw):
    eng, x0, U0 = _setup(M, kind, H_OF[kind] if H is None else H, K=table[0], B=B, **kw)
    _stack(eng, kind, stack, B).set_iterations(len(table))
    eng.set_population(table)
    assert eng.population() == (None if all(k == table[0] for k in table) else tuple(table))
    return eng, x0, U0


def _host_form(M, kind, table, stack):
    """Two control steps on host pointers (by-value seeds: iteration i of step s draws key SEED + s n + i)."""
    n, KL = len(table), table[-1]
    eng, x0, U0 = _decayed(M, kind, table, stack)
    got, U = [], U0
    for s in range(2):
        res = eng.solve(x0, U, seed=SEED + s * n, shift=True, stats=True, want_weights=True)
        U = res.U
        got.append(((res.U, res.u0, res.costs[:, :KL], res.weights[:, :KL]),
                    [_slot(eng, kind, stack, i) for i in range(n)], _readouts(eng, stack)))
    eng.close()
    refs = []
    for k in table:
        e, _, _ = _setup(M, kind, H_OF[kind], K=k)
        refs.append(_stack(e, kind, stack))
    want, U, state = [], U0, None
    for s in range(2):
        slots = []
        for i, e in enumerate(refs):
            _hand_over(e, state)
            r = e.solve(x0, U, seed=SEED + s * n + i, shift=i == n - 1, stats=True, want_weights=True)
            U = r.U
            slots.append(_slot(e, kind, stack, 0))
            state = _state(e, stack, B0)
        want.append(((r.U, r.u0, r.costs, r.weights), slots, _readouts(refs[-1], stack)))
    for e in refs:
        e.close()
    _eq(got, want, ("host pointers", kind, table, stack))


def _device_form(M, torch, kind, table, stack, form, B=B0, H=None, steps=None, expect_route=None, chained=False):
    """async: two steps of ASYNC device solves on the counter; chain: two chained steps; graph / traj: a captured graph
    of three steps (with the trajectory log) -- against the defining loop."""
    n, KL = len(table), table[-1]
    steps = (3 if form in ("graph", "traj") else 2) if steps is None else steps
    want = _loop(M, torch, kind, table, stack, 3, B, H, chained)
    eng, x0, U0 = _decayed(M, kind, table, stack, B, H)
    tx, tU, tu0, tc = _tensors(torch, eng, x0, U0)
    msg = (form, kind, table, stack)
    if form in ("async", "chain"):
        for s in range(steps):
            eng.solve_device(B, tx.data_ptr(), tU.data_ptr(), None, seed=SEED, u0_ptr=tu0.data_ptr(),
                             costs_ptr=tc.data_ptr(), shift=True, env_step=True, chain=form == "chain",
                             seed_counter=True, asynchronous=True, stats=True)
            _eq([_slot(eng, kind, stack, i, B) for i in range(n)], want["slots"][s], (msg, "slots of step", s))
            x, U, u0, c = _snap(torch, tx, tU, tu0, tc)
            _eq((x, U, u0, c[:, :KL]), want["state"][s], (msg, "state behind step", s))
            if form == "chain" and expect_route:
                assert eng.gen_route() == expect_route, (msg, eng.gen_route())
    else:
        dev = torch.device("cuda")
        trx = torch.zeros(steps, B, eng.config.nx, device=dev)
        tru = torch.zeros(steps, B, eng.config.nu, device=dev)
        traj = dict(traj_x_ptr=trx.data_ptr(), traj_u_ptr=tru.data_ptr()) if form == "traj" else {}
        eng.graph_capture_traj(B, steps, tx.data_ptr(), tU.data_ptr(), tu0.data_ptr(), costs_ptr=tc.data_ptr(),
                               seed=SEED, stats=True, **traj)
        if expect_route:
            assert eng.gen_route() == expect_route, (msg, eng.gen_route())
        eng.graph_launch(sync=True)
        _eq([[_slot(eng, kind, stack, s * n + i, B) for i in range(n)] for s in range(steps)], want["slots"][:steps],
            (msg, "slots of the launch"))
        if form == "traj":  # one row per control step
            sx, su = _snap(torch, trx, tru)
            _eq(sx, np.stack(want["x_before"][:steps]), (msg, "traj_x"))
            _eq(su, np.stack(want["u0"][:steps]), (msg, "traj_u"))
    x, U, u0, c = _snap(torch, tx, tU, tu0, tc)
    _eq((x, U, u0, c[:, :KL]), want["state"][steps - 1], (msg, "final state"))
    if KL < table[0]:  # the rest of each row is left untouched
        assert (c[:, KL:] == -1.0).all(), (msg, "io.costs beyond K_last")
    _eq(_readouts(eng, stack, B), want["read"][steps - 1], (msg, "read-outs"))
    assert eng.get_seed_counter() == steps * n
    for i in range(n):
        assert eng.iter_rollout_kernel(i) == want["kernels"][i], (msg, i)
    eng.close()
    return (x, U, u0, c[:, :KL])


# ------------------------------------------------------------------------------------------ 1. off is off

def test_a_table_of_K_throughout_is_the_handle_that_never_called_the_setter(M):
    """Never set / set and cleared / the all-K table: the same outputs, seed counter, per-kernel launch counts and
    gen_route over a solve, two chained solves and a 3-solve graph (MLP, K = 130, B = 2, H = 7, n_iter = 3)."""
    import torch
    outs = []
    for touch in ("never", "cleared", "all-K"):
        eng, x0, U0 = _setup(M, "mlp", 7)
        eng.set_iterations(3)
        if touch == "cleared":
            eng.set_population(TABLE)
            assert eng.population() == TABLE
            eng.set_population(None)
        elif touch == "all-K":
            eng.set_population((K0, K0, K0))
        assert eng.population() is None
        eng.profile(True)
        res = eng.solve(x0, U0, seed=SEED, shift=True, want_weights=True, stats=True)
        host = ((res.U, res.u0, res.costs, res.weights), [eng.stats(B0, i) for i in range(3)])
        tx, tU, tu0, tc = _tensors(torch, eng, x0, res.U)
        routes = []
        for _ in range(2):
            eng.solve_device(B0, tx.data_ptr(), tU.data_ptr(), None, seed=SEED, u0_ptr=tu0.data_ptr(),
                             costs_ptr=tc.data_ptr(), shift=True, env_step=True, chain=True)
            routes.append(eng.gen_route())
        chained = _snap(torch, tx, tU, tu0, tc)
        eng.profile(False)
        counts = {k: eng.kernel_time(k)[0] for k in KERNELS + ("iter",)}
        eng.graph_capture(B0, 3, tx.data_ptr(), tU.data_ptr(), tu0.data_ptr(), costs_ptr=tc.data_ptr(), seed=SEED)
        routes.append(eng.gen_route())
        eng.graph_launch(sync=True)
        graph = _snap(torch, tx, tU, tu0, tc)
        kernels = [eng.iter_rollout_kernel(i) for i in range(3)]
        outs.append((host, chained, graph, eng.get_seed_counter(), counts, routes, kernels))
        eng.close()
    for o, name in zip(outs[1:], ("set and cleared", "the all-K table")):
        _eq(o[:4], outs[0][:4], ("never set vs " + name))
        assert o[4] == outs[0][4] and o[5] == outs[0][5] and o[6] == outs[0][6], (name, o[4:], outs[0][4:])
    # (the host solve draws by-value keys: the counter counts the 2 chained and the 3 captured steps' iterations)
    assert outs[0][3] == 2 * 3 + 3 * 3 and outs[0][4]["rollout"] == 3 + 2 * 3 and outs[0][6][0] == outs[0][6][2] != ""


# ------------------------------------------------------------------------------------------ 2. the defining loop

@pytest.mark.parametrize("stack", ["bare", "cem"])
@pytest.mark.parametrize("form", ["host", "async", "chain", "graph", "traj"])
@pytest.mark.parametrize("kind", ["mlp", "ca", "cartpole"])
def test_an_iteration_is_the_solve_of_a_handle_of_its_sample_count(M, kind, form, stack):
    """Table (130, 70, 33) -- Kp 192, 128, 64 -- at B = 2, H = 7 / 5 / 9: U, u0, the last iteration's costs and weights
    (their first K_last entries), every per-iteration statistics and lambda slot, the kept set, the scale table, u_prev
    and the seed counter against the loop over three handles of K = 130, 70, 33."""
    import torch
    if form == "host":
        _host_form(M, kind, TABLE, stack)
    else:
        _device_form(M, torch, kind, TABLE, stack, form)


@pytest.mark.parametrize("form", ["host", "chain", "graph"])
@pytest.mark.parametrize("table", [(130, 100, 70), (130, 130, 64)], ids=["equal-pitch", "equal-neighbour"])
def test_the_loop_at_equal_pitches_and_equal_neighbours(M, table, form):
    """(130, 100, 70): iterations 1 and 2 share the pitch 128 with different K (the one-pitch kernel at that boundary);
    (130, 130, 64): equal neighbours, then a shrink."""
    import torch
    if form == "host":
        _host_form(M, "mlp", table, "cem")
    else:
        _device_form(M, torch, "mlp", table, "cem", form)


# ------------------------------------------------------------------------------------------ 3. the two-pitch generator

@pytest.mark.parametrize("form", ["chain", "graph"])
def test_the_fused_generator_at_two_pitches(M, form, monkeypatch):
    """MLP, B = 1, H = 3, table (1100, 200): Kp 1152 and 256, three control steps.  The shrink crosses the 1024-sample
    wave tile; the growth at every step boundary generates 288 quads per row while reading 64.  The loop's handles run
    chained solves (_loop: the same stream form; K = 1100 is past where a plain solve equals a chained one).  MPPI_GEN_OVERLAP=0, the
    plain i.i.d. law: every next noise is drawn inside the reduce (gen_route "fused", no generator launch behind
    any reduce).  Equal to the defining loop, and to the same run with the overlap stream forced."""
    import torch
    table = (1100, 200)
    monkeypatch.setenv("MPPI_GEN_OVERLAP", "0")
    fused = _device_form(M, torch, "mlp", table, "bare", form, B=1, H=3, steps=3, expect_route="fused", chained=True)
    if form == "chain":
        eng, x0, U0 = _decayed(M, "mlp", table, "bare", B=1, H=3)
        tx, tU, tu0, tc = _tensors(torch, eng, x0, U0)
        eng.profile(True)
        for s in range(3):
            eng.solve_device(1, tx.data_ptr(), tU.data_ptr(), None, seed=SEED, u0_ptr=tu0.data_ptr(),
                             costs_ptr=tc.data_ptr(), shift=True, env_step=True, chain=True)
        torch.cuda.synchronize()
        eng.profile(False)
        # (no generator launch behind any reduce: "noise" counts those; the prime ahead of the first solve is not timed)
        assert eng.kernel_time("noise")[0] == 0 and eng.kernel_time("reduce")[0] == 6
        eng.close()
        monkeypatch.setenv("MPPI_GEN_OVERLAP", "1")
        over = _device_form(M, torch, "mlp", table, "bare", form, B=1, H=3, steps=3, expect_route="overlap",
                            chained=True)
        _eq(fused, over, "fused at two pitches vs the overlap stream")
        # the A/B knob: the next noise from a launch of its own behind the (read-only, same block) reduce
        monkeypatch.setenv("MPPI_GEN_OVERLAP", "0")
        monkeypatch.setenv("MPPI_GEN_TWO_PITCH", "0")
        sep = _device_form(M, torch, "mlp", table, "bare", form, B=1, H=3, steps=3, expect_route="fused", chained=True)
        _eq(fused, sep, "fused at two pitches vs the separate launch")


@pytest.mark.parametrize("form", ["chain", "graph"])
def test_the_fused_generator_at_two_pitches_with_statistics(M, form, monkeypatch):
    """B = 2, table (130, 33): Kp 192 -> 64 -> 192, with MPPI_FLAG_STATS (the statistics read the noise the two-pitch
    pass has just read, ahead of the next generator)."""
    import torch
    monkeypatch.setenv("MPPI_GEN_OVERLAP", "0")
    _device_form(M, torch, "mlp", (130, 33), "bare", form, steps=3, expect_route="fused")


# ------------------------------------------------------------------------------------------ 4. the best sample

def test_the_best_sample_is_the_reference_folded_over_the_loop(M):
    """return_best and add_mean on table (130, 70, 33) under the cem stack, one host step: best() equals iter_best_ref
    folded over the defining loop's (U ahead of the iteration, the noise as its rollout saw it, the costs its selection
    read); u0 is its first control; the add_mean column count[b] lies inside K_last."""
    from mppi_hip.stats import iter_best_ref
    n, KL = len(TABLE), TABLE[-1]
    eng, x0, U0 = _decayed(M, "mlp", TABLE, "cem")
    eng.set_iterations(n, True, True)
    assert eng.population() == TABLE  # (the table admits the change: it stays)
    res = eng.solve(x0, U0, seed=SEED, shift=True)
    got = eng.best(B0)
    eng.close()
    refs = []
    for k in TABLE:
        e, _, _ = _setup(M, "mlp", H_OF["mlp"], K=k)
        refs.append(_stack(e, "mlp", "cem"))
    refs[-1].set_iterations(1, False, True)  # the step's last iteration enters the mean
    st, U, state, j0 = None, U0, None, None
    for i, e in enumerate(refs):
        last = i == n - 1
        _hand_over(e, state)
        nz = e.noise_eval(B0, SEED + i)
        if state is not None:
            v, _, _, count, steps = state["kept"]
            nz = e.keep_inject_eval(U, nz, v, count, steps)
        if last:
            j0 = state["kept"][3]
            for b in range(B0):
                nz[b, :, :, j0[b]] = 0.0
        nz = e.bounds_eval(U, nz)[0]
        r = e.solve(x0, U, seed=SEED + i, shift=last)
        sel = (r.costs + e.rate_term(B0)).astype(np.float32)  # the unmasked end of the chain: costs + rate term
        st = iter_best_ref(U, nz, sel, it=i, stored=st, ctrl_clamp=e.config.ctrl_clamp)
        U, state = r.U, _state(e, "cem", B0)
    for e in refs:
        e.close()
    _eq(res.U, r.U, "U")
    assert same_bits(got[0], st[0]), ("v", got[0], st[0])
    assert np.array_equal(bits(got[1]), bits(st[1])), ("cost", got[1], st[1])
    assert np.array_equal(got[2], st[2]) and np.array_equal(got[3], st[3]), ("k / iter", got[2:], st[2:])
    assert (got[2] >= 0).all() and (got[2] < np.array(TABLE)[got[3]]).all()  # k* indexes its own iteration's samples
    _eq(res.u0, np.clip(got[0][:, :, 0], -BOX, BOX), "u0 is the best sample's first control")
    assert (j0 >= 0).all() and (j0 < KL).all(), j0


# ------------------------------------------------------------------------------------------ 5. routes

def test_every_iteration_is_routed_on_its_own_shape(M):
    """The CA fixture in the split mode (precision 2) at B = 2: iter_rollout_kernel(i) is rollout_kernel() of the
    K = K_it[i] handle."""
    eng, x0, U0 = _decayed(M, "ca", TABLE, "bare", precision=2)
    eng.solve(x0, U0, seed=SEED, shift=True)
    got = [eng.iter_rollout_kernel(i) for i in range(len(TABLE))]
    assert eng.rollout_kernel() == got[-1] and eng.iter_rollout_kernel(3) == "" and eng.iter_rollout_kernel(-1) == ""
    eng.close()
    want = []
    for k in TABLE:
        ref, _, _ = _setup(M, "ca", H_OF["ca"], K=k, precision=2)
        ref.solve(x0, U0, seed=SEED)
        want.append(ref.rollout_kernel())
        ref.close()
    print("routes of", TABLE, ":", got)
    assert got == want and all(got), (got, want)


# ------------------------------------------------------------------------------------------ 6. state rules

def test_state_and_argument_errors(M):
    import torch
    L = M._lib
    eng, x0, U0 = _setup(M, "mlp", 7)

    def code(fn):
        with pytest.raises(M.MPPIError) as ei:
            fn()
        return ei.value

    def refused(fn, what):
        e = code(fn)
        assert e.code == L.MPPI_E_ARG, (what, e)
        return e

    # the setter's refusals: nothing changed
    refused(lambda: eng.set_population(TABLE), "n != n_iter (1)")
    eng.set_iterations(3)
    refused(lambda: eng.set_population((130, 70)), "n != n_iter (3)")
    refused(lambda: eng.set_population((129, 70, 33)), "K_it[0] != K")
    refused(lambda: eng.set_population((130, 0, 33)), "an entry below 1")
    refused(lambda: eng.set_population((130, 131, 33)), "an entry above K")
    assert eng.lib.mppi_set_population(eng._h, None, 3) == L.MPPI_E_ARG
    assert eng.population() is None
    # ... against the other settings, in this order
    eng.set_elites(34)
    refused(lambda: eng.set_population(TABLE), "n_elite > K_it[2]")
    eng.set_elites(33).set_elite_keep(34)
    refused(lambda: eng.set_population(TABLE), "n_keep > K_it[2]")
    eng.set_elite_keep(33).set_iterations(3, False, True)
    refused(lambda: eng.set_population(TABLE), "add_mean: n_keep + 1 > K_it[2]")
    assert eng.population() is None
    eng.set_iterations(3, False, False).set_population(TABLE)
    assert eng.population() == TABLE
    # ... and in the other order: the other setters refuse while the table is on, nothing changed
    assert "mppi_set_population" in str(refused(lambda: eng.set_iterations(2), "n_iter away from the table's"))
    refused(lambda: eng.set_iterations(1), "n_iter = 1")
    refused(lambda: eng.set_iterations(3, False, True), "add_mean with n_keep = 33")
    refused(lambda: eng.set_elites(34), "n_elite above K_it[2]")
    refused(lambda: eng.set_elite_keep(34), "n_keep above K_it[2]")
    assert eng.iterations() == (3, False, False) and eng.elites() == 33 and eng.elite_keep() == 33
    eng.set_iterations(3, True, False).set_elites(13).set_elite_keep(5).set_iterations(3, True, True)  # admitted
    assert eng.population() == TABLE
    # injected noise
    nz = np.zeros((B0, MLP_NU, 7, K0), np.float32)
    e = code(lambda: eng.solve(x0, U0, noise=nz))
    assert e.code == L.MPPI_E_UNSUPPORTED and "mppi_set_population" in str(e)
    # K-sharding
    from mppi_hip import distributed
    e = code(lambda: distributed.solve_k_sharded(lambda x, U: None, x0[0], U0[0], 1.0, engine=eng))
    assert e.code == L.MPPI_E_UNSUPPORTED
    # off again: the other setters are free, injected noise is n_iter's business alone
    eng.set_population(None)
    eng.set_iterations(1).set_elites(100).set_elite_keep(0).set_elites(0)
    eng.solve(x0, U0, noise=nz)

    # a change destroys captured graphs and drops a prefetched noise with the counter unchanged; a no-op keeps both
    tx, tU, tu0, tc = _tensors(torch, eng, x0, U0)
    eng.set_iterations(3).set_population(TABLE)
    eng.set_seed_counter(0)
    eng.graph_capture(B0, 2, tx.data_ptr(), tU.data_ptr(), tu0.data_ptr(), seed=SEED)
    eng.graph_launch(sync=True)
    assert eng.get_seed_counter() == 6
    eng.set_population(TABLE)  # in effect: the graph and the prefetched noise stay
    eng.set_population(np.array(TABLE, np.int64))
    eng.graph_launch(sync=True)
    assert eng.get_seed_counter() == 12
    eng.set_population((130, 70, 34))
    assert eng.get_seed_counter() == 12  # the prefetch was dropped, the counter stepped back: no key skipped
    assert code(lambda: eng.graph_launch(sync=True)).code == L.MPPI_E_STATE
    eng.graph_capture(B0, 2, tx.data_ptr(), tU.data_ptr(), tu0.data_ptr(), seed=SEED)
    eng.graph_launch(sync=True)
    assert eng.get_seed_counter() == 18
    eng.set_population(None)  # a change too
    assert eng.get_seed_counter() == 18
    assert code(lambda: eng.graph_launch(sync=True)).code == L.MPPI_E_STATE
    # the all-K table on a handle with the feature off is the table in effect
    eng.graph_capture(B0, 2, tx.data_ptr(), tU.data_ptr(), tu0.data_ptr(), seed=SEED)
    eng.set_population((K0, K0, K0))
    eng.graph_launch(sync=True)
    assert eng.get_seed_counter() == 24 and eng.population() is None
    eng.close()


def test_the_read_outs_hold_the_last_iterations_samples(M):
    """The [B][K] read-outs without per-step slots under a table: rows of cfg.K whose first K_last entries are the last
    iteration's (the K = K_last handle's of the defining loop, by the rate term), the rest left untouched."""
    n, KL = len(TABLE), TABLE[-1]
    eng, x0, U0 = _decayed(M, "mlp", TABLE, "cem")
    res = eng.solve(x0, U0, seed=SEED, shift=True)
    term = np.full((B0, K0), -7.0, np.float32)
    M._lib.check(eng.lib.mppi_get_rate_term(eng._h, B0, term.ctypes.data_as(ctypes.c_void_p)))
    eng.close()
    refs = []
    for k in TABLE:
        e, _, _ = _setup(M, "mlp", H_OF["mlp"], K=k)
        refs.append(_stack(e, "mlp", "cem"))
    U, state = U0, None
    for i, e in enumerate(refs):
        _hand_over(e, state)
        r = e.solve(x0, U, seed=SEED + i, shift=i == n - 1)
        U, state = r.U, _state(e, "cem", B0)
    want = refs[-1].rate_term(B0)
    for e in refs:
        e.close()
    _eq(term[:, :KL], want, "the rate term's first K_last entries")
    assert (term[:, KL:] == -7.0).all()
    _eq(res.costs[:, :KL], r.costs, "io.costs")
