"""Inner iterations per control step on the device (mppi_set_iterations): a handle set to (1, 0, 0) is the handle that
never called the setter; a control step of n_iter iterations is, bit for bit, the defining loop of n_iter = 1 solves in
every stream form, bare and under the CEM stack; the tracking kernel against its numpy reference, exactly; the stored
best of a step against the reference folded over the loop; return_best, add_mean; and the state rules of the four
entries.  Every comparison is bitwise."""
import os

import numpy as np
import pytest

from conftest import REPO
from iter_cases import bits, grid, hand_cases, inputs, same_bits, stored_for

pytestmark = pytest.mark.gpu

K0, B0, SEED = 130, 2, 7  # Kp = 192: the pads are live
MLP_NX, MLP_NU = 10, 3
KERNELS = ("noise", "rollout", "reduce", "update", "stats", "lambda", "ctrl_cost", "bounds", "rate_cost", "elites",
           "keep", "cross", "cov_adapt", "step_mom", "step_adapt")
BOX = 0.3


@pytest.fixture(scope="module")
def M(gpu_available):
    import mppi_hip
    return mppi_hip


def _setup(M, kind, H, K=K0, B=B0, **kw):
    """(engine, x0 [B, nx] f32, U0 [B, nu, H] f32): the seeded synthetic MLP (nx 10, nu 3, fp32, quad_est), the golden
    CrossAttention humanoid at bf16, or the cartpole preset."""
    rs = np.random.RandomState(11)
    if kind == "ca":
        sd = M.load_npz(os.path.join(REPO, "tests", "golden", "ca_humanoid_weights.npz"))
        eng = M.Engine(M.Config.preset("humanoid_v3", K=K, H=H, precision=1, max_batch=B, **kw))
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
    """bare: nothing (the cartpole pinned to its unfused form on both sides, as tests/test_gpu_elites.py compares it:
    the feature takes it there, and the fused one-launch form differs from reduce_kernel in the last bits).
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


def _tensors(torch, eng, x0, U0):
    dev = torch.device("cuda")
    c = eng.config
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    return (torch.from_numpy(x0).to(dev), torch.from_numpy(U0).to(dev), torch.zeros(x0.shape[0], c.nu, device=dev),
            torch.zeros(x0.shape[0], c.K, device=dev))


# ------------------------------------------------------------------------------------------ 1. off is off

def test_one_iteration_without_options_is_the_handle_that_never_called_the_setter(M):
    import torch
    outs = []
    for touch in (False, True):
        eng, x0, U0 = _setup(M, "mlp", 7)
        if touch:
            eng.set_iterations(3, True, True).set_iterations(1, False, False)
            assert eng.iterations() == (1, False, False)
        eng.profile(True)
        res = eng.solve(x0, U0, seed=SEED, shift=True, want_weights=True)
        tx, tU, tu0, tc = _tensors(torch, eng, x0, res.U)
        for _ in range(2):
            eng.solve_device(B0, tx.data_ptr(), tU.data_ptr(), None, seed=SEED, u0_ptr=tu0.data_ptr(),
                             costs_ptr=tc.data_ptr(), shift=True, env_step=True, chain=True)
        dev = _snap(torch, tx, tU, tu0, tc)
        eng.profile(False)
        counts = {k: eng.kernel_time(k)[0] for k in KERNELS + ("iter",)}
        outs.append(((res.U, res.u0, res.costs, res.weights), dev, eng.get_seed_counter(), counts))
        eng.close()
    _eq(outs[0][:3], outs[1][:3], "never set vs (1, 0, 0)")
    assert outs[0][3] == outs[1][3] and outs[1][3]["iter"] == 0 and outs[1][3]["rollout"] == 3, outs[1][3]


# ------------------------------------------------------------------------------------------ 2. the loop

_LOOPS = {}


def _loop(M, torch, kind, H, n, stack, steps):
    """The defining loop on a handle at n_iter = 1, plain device solves on the seed counter: `steps` control steps of n
    iterations, flags masked on all but the last.  Cached per case: forms (c), (d) and (e) share it."""
    key = (kind, H, n, stack, steps)
    if key in _LOOPS:
        return _LOOPS[key]
    eng, x0, U0 = _setup(M, kind, H)
    _stack(eng, kind, stack)
    tx, tU, tu0, tc = _tensors(torch, eng, x0, U0)
    out = {"x_before": [], "u0": [], "state": [], "slots": [], "read": []}
    for s in range(steps):
        out["x_before"].append(_snap(torch, tx)[0])
        slots = []
        for i in range(n):
            last = i == n - 1
            eng.solve_device(B0, tx.data_ptr(), tU.data_ptr(), None, seed=SEED, u0_ptr=tu0.data_ptr(),
                             costs_ptr=tc.data_ptr(), shift=last, env_step=last, seed_counter=True, asynchronous=False,
                             stats=True)
            slots.append(_slot(eng, kind, stack, 0))
        out["slots"].append(slots)
        out["state"].append(_snap(torch, tx, tU, tu0, tc))
        out["u0"].append(out["state"][-1][2])
        out["read"].append(_readouts(eng, stack))
    eng.close()
    _LOOPS[key] = out
    return out


def _host_form(M, kind, H, n, stack):
    eng, x0, U0 = _setup(M, kind, H)
    _stack(eng, kind, stack).set_iterations(n)
    res = eng.solve(x0, U0, seed=SEED, shift=True, stats=True, want_weights=True)
    got = ((res.U, res.u0, res.costs, res.weights), [_slot(eng, kind, stack, i) for i in range(n)],
           _readouts(eng, stack))
    _eq(res.stats, {k: v for k, v in got[1][-1]["stats"].items()}, "SolveResult.stats is the last iteration's")
    eng.close()
    ref, x0, U = _setup(M, kind, H)
    _stack(ref, kind, stack)
    slots = []
    for i in range(n):
        r = ref.solve(x0, U, seed=SEED + i, shift=i == n - 1, stats=True, want_weights=True)
        U = r.U
        slots.append(_slot(ref, kind, stack, 0))
    want = ((r.U, r.u0, r.costs, r.weights), slots, _readouts(ref, stack))
    ref.close()
    _eq(got, want, ("host pointers", kind, H, n, stack))


def _async_form(M, torch, kind, H, n, stack):
    outs = []
    for feature in (True, False):
        eng, x0, U0 = _setup(M, kind, H)
        _stack(eng, kind, stack).set_iterations(n if feature else 1)
        tx, tU, tu0, tc = _tensors(torch, eng, x0, U0)
        slots = []
        for i in range(1 if feature else n):
            last = feature or i == n - 1
            eng.solve_device(B0, tx.data_ptr(), tU.data_ptr(), None, seed=SEED + i, u0_ptr=tu0.data_ptr(),
                             costs_ptr=tc.data_ptr(), shift=last, env_step=last, asynchronous=True, stats=True)
            if not feature:
                slots.append(_slot(eng, kind, stack, 0))
        if feature:
            slots = [_slot(eng, kind, stack, i) for i in range(n)]
        outs.append((_snap(torch, tx, tU, tu0, tc), slots, _readouts(eng, stack)))
        eng.close()
    _eq(outs[0], outs[1], ("device pointers, ASYNC", kind, H, n, stack))


def _stream_form(M, torch, kind, H, n, stack, form):
    """(c) chained over 3 control steps, (d) a captured graph of 3 steps launched twice, (e) the trajectory-logging
    capture -- against the loop of plain counter solves."""
    steps = 6 if form == "graph" else 3
    want = _loop(M, torch, kind, H, n, stack, 6)
    eng, x0, U0 = _setup(M, kind, H)
    _stack(eng, kind, stack).set_iterations(n)
    tx, tU, tu0, tc = _tensors(torch, eng, x0, U0)
    msg = (form, kind, H, n, stack)
    if form == "chain":
        for s in range(steps):
            eng.solve_device(B0, tx.data_ptr(), tU.data_ptr(), None, seed=SEED, u0_ptr=tu0.data_ptr(),
                             costs_ptr=tc.data_ptr(), shift=True, env_step=True, chain=True, stats=True)
            _eq([_slot(eng, kind, stack, i) for i in range(n)], want["slots"][s], (msg, "slots of step", s))
            _eq(_snap(torch, tx, tU, tu0, tc), want["state"][s], (msg, "state behind step", s))
    else:
        dev = torch.device("cuda")
        trx = torch.zeros(3, B0, eng.config.nx, device=dev)
        tru = torch.zeros(3, B0, eng.config.nu, device=dev)
        traj = dict(traj_x_ptr=trx.data_ptr(), traj_u_ptr=tru.data_ptr()) if form == "traj" else {}
        eng.graph_capture_traj(B0, 3, tx.data_ptr(), tU.data_ptr(), tu0.data_ptr(), costs_ptr=tc.data_ptr(), seed=SEED,
                               stats=True, **traj)
        for _ in range(steps // 3):
            eng.graph_launch(sync=True)
        _eq([[_slot(eng, kind, stack, s * n + i) for i in range(n)] for s in range(3)], want["slots"][steps - 3:steps],
            (msg, "slots of the last launch"))
        if form == "traj":  # one row per control step
            sx, su = _snap(torch, trx, tru)
            _eq(sx, np.stack(want["x_before"][:3]), (msg, "traj_x"))
            _eq(su, np.stack(want["u0"][:3]), (msg, "traj_u"))
    _eq(_snap(torch, tx, tU, tu0, tc), want["state"][steps - 1], (msg, "final state"))
    _eq(_readouts(eng, stack), want["read"][steps - 1], (msg, "read-outs"))
    assert eng.get_seed_counter() == steps * n
    eng.close()


@pytest.mark.parametrize("stack", ["bare", "cem"])
@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("form", ["host", "async", "chain", "graph", "traj"])
def test_a_step_is_the_defining_loop_mlp(M, form, n, stack):
    import torch
    if form == "host":
        _host_form(M, "mlp", 7, n, stack)
    elif form == "async":
        _async_form(M, torch, "mlp", 7, n, stack)
    else:
        _stream_form(M, torch, "mlp", 7, n, stack, form)


@pytest.mark.parametrize("form", ["host", "graph"])
def test_a_step_is_the_defining_loop_at_horizon_one(M, form):
    """H = 1: a shifting step keeps no step of a carried sequence and refits a one-cell table."""
    import torch
    if form == "host":
        _host_form(M, "mlp", 1, 2, "cem")
    else:
        _stream_form(M, torch, "mlp", 1, 2, "cem", form)


@pytest.mark.parametrize("stack", ["bare", "cem"])
@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("form", ["host", "graph"])
@pytest.mark.parametrize("kind", ["ca", "cartpole"])
def test_a_step_is_the_defining_loop_ca_and_cartpole(M, kind, form, n, stack):
    import torch
    if form == "host":
        _host_form(M, kind, 7, n, stack)
    else:
        _stream_form(M, torch, kind, 7, n, stack, form)


# ------------------------------------------------------------------------------------------ 3. the kernel

def _assert_best(got, want, msg):
    assert same_bits(got[0], want[0]), (msg, "v", got[0], want[0])
    assert np.array_equal(bits(got[1]), bits(want[1])), (msg, "cost", got[1], want[1])
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3]), (msg, "k / iter", got[2:], want[2:])


def test_iter_best_eval_equals_the_reference_on_the_shared_cases(M):
    from mppi_hip.stats import iter_best_ref
    engines = {}
    for name, B, nu, H, K, clamp, costs, reset in grid():
        key = (nu, H, K, clamp)
        if key not in engines:
            engines[key] = M.Engine(M.Config(nx=4, nu=nu, H=H, K=K, max_batch=B, ctrl_clamp=clamp))
        U, eps = inputs(B, nu, H, K)
        eps[0, 0, 0, 0] = np.nan
        st = None if reset else stored_for(U, eps, costs)
        got = engines[key].iter_best_eval(U, eps, costs, it=2, stored=st)
        _assert_best(got, iter_best_ref(U, eps, costs, it=2, stored=st, ctrl_clamp=clamp), name)
    for e in engines.values():
        e.close()
    for name, U, eps, costs, clamp, stored, it, want in hand_cases():
        eps = np.array(eps, np.float32)
        eng = M.Engine(M.Config(nx=4, nu=eps.shape[0], H=eps.shape[1], K=eps.shape[2], max_batch=2, ctrl_clamp=clamp))
        st = None if stored is None else (np.array([stored[0]], np.float32), np.array([stored[1]], np.float32),
                                          np.array([stored[2]], np.int32), np.array([stored[3]], np.int32))
        got = eng.iter_best_eval(np.array([U], np.float32), eps[None], np.array([costs], np.float32), it=it, stored=st)
        w = (np.array([want[0]], np.float32), np.array([want[1]], np.float32), np.array([want[2]], np.int32),
             np.array([want[3]], np.int32))
        _assert_best(got, w, name)
        eng.close()


@pytest.mark.parametrize("K", [130, 300, 5000])
def test_iter_best_eval_at_both_forms_of_the_kernel(M, K):
    """K = 130 and 300 in whole waves, K = 5000 in the 1024-thread form; reset 1 and 0; a clamp that binds; two solves
    of a batch with different winners, the winner in the last wave's last lanes, and an all-non-finite row beside a
    normal one; two calls bitwise equal; the handle's own stored best untouched (none: mppi_get_best stays refused)."""
    from mppi_hip.stats import iter_best_ref
    H, nu, clamp = 7, 3, 1.25
    eng = M.Engine(M.Config(nx=4, nu=nu, H=H, K=K, max_batch=B0, ctrl_clamp=clamp))
    U, eps = inputs(B0, nu, H, K, scale=1.5)
    rs = np.random.RandomState(K)
    c = (50.0 + 10.0 * rs.randn(B0, K)).astype(np.float32)
    c[0, K - 1] = c[0].min() - 1.0  # the winner of solve 0: the last sample before the pads
    c[1, 3], c[1, K // 2] = np.nan, -np.inf
    for reset in (1, 0):
        st = None if reset else stored_for(U, eps, c)
        got = eng.iter_best_eval(U, eps, c, it=1, stored=st)
        want = iter_best_ref(U, eps, c, it=1, stored=st, ctrl_clamp=clamp)
        _assert_best(got, want, (K, reset))
        _assert_best(eng.iter_best_eval(U, eps, c, it=1, stored=st), got, "two calls")
        if reset:
            assert got[2][0] == K - 1 and got[2][1] == int(np.nanargmin(np.where(np.isfinite(c[1]), c[1], np.inf)))
            assert got[2][0] != got[2][1] and np.abs(got[0]).max() == np.float32(clamp)  # the clamp bound
    c[1] = np.array([np.nan, np.inf, -np.inf], np.float32)[np.arange(K) % 3]
    for reset in (1, 0):
        st = None if reset else stored_for(U, eps, c)
        _assert_best(eng.iter_best_eval(U, eps, c, stored=st), iter_best_ref(U, eps, c, stored=st, ctrl_clamp=clamp),
                     ("no finite cost beside a normal row", K, reset))
    with pytest.raises(M.MPPIError) as ei:
        eng.best(B0)
    assert ei.value.code == M._lib.MPPI_E_STATE
    eng.close()


# ------------------------------------------------------------------------------------------ 4. tracking through a solve

@pytest.mark.parametrize("bounds", [False, True], ids=["free", "bounded"])
def test_the_stored_best_is_the_reference_folded_over_the_loop(M, bounds):
    """n_iter = 3, no keep, a clamp that binds: iter_best_ref folded over the loop's per-iteration (U before the
    iteration, noise_eval(key_i) [through bounds_eval], costs) equals best()."""
    from mppi_hip.stats import iter_best_ref
    n, clamp = 3, 0.9
    eng, x0, U0 = _setup(M, "mlp", 7, ctrl_clamp=clamp)
    ref, _, _ = _setup(M, "mlp", 7, ctrl_clamp=clamp)
    for e in (eng, ref):
        if bounds:
            e.set_control_bounds(-BOX, [BOX, 2.0, BOX])
    eng.set_iterations(n)
    res = eng.solve(x0, U0, seed=SEED, shift=True)
    got = eng.best(B0)
    st, U = None, U0
    for i in range(n):
        nz = ref.noise_eval(B0, SEED + i)
        if bounds:
            nz = ref.bounds_eval(U, nz)[0]
        r = ref.solve(x0, U, seed=SEED + i, shift=i == n - 1)
        st = iter_best_ref(U, nz, r.costs, it=i, stored=st, ctrl_clamp=clamp)
        U = r.U
    _eq(res.U, r.U, "U")
    _assert_best(got, st, ("best() against the fold", bounds))
    assert (got[2] >= 0).all() and (got[3] >= 0).all()
    eng.close()
    ref.close()


def test_with_kept_elites_and_the_mean_the_best_cost_never_rises(M):
    """Keep on and add_mean, the same step at n_iter = 1, 2, 3 (no shift): the stored best cost is the running minimum
    of the iterations' own minima (each iteration's statistics slot), names the first iteration that attained it, is
    never above the cost of the nominal the last iteration entered (the column at the kept set's count) -- and does not
    rise from n_iter to n_iter + 1."""
    prev = None
    for n in (1, 2, 3):
        eng, x0, U0 = _setup(M, "mlp", 7)
        eng.set_elite_keep(5).set_iterations(n, False, True)
        res = eng.solve(x0, U0, seed=SEED, stats=True)
        v, cost, k, it = eng.best(B0)
        mins = np.stack([eng.stats(B0, i)["cost_min"] for i in range(n)])  # [n, B]
        print(f"n_iter {n}: best cost {cost.tolist()} at iteration {it.tolist()}, per-iteration minima {mins.T.tolist()}")
        run = np.minimum.accumulate(mins, axis=0)
        _eq(cost, run[-1], "the best cost is the running minimum")
        assert np.array_equal(it, np.argmax(mins == run[-1][None], axis=0).astype(np.int32))
        # the column the last iteration zeroed: the count of the set stored ahead of it -- none at n_iter = 1; behind
        # a store the count, which an unshifted store of the same n_keep leaves as the last iteration's own store does
        j0 = eng.kept(B0)[3] if n > 1 else np.zeros(B0, np.int32)
        assert n == 1 or j0.tolist() == [5, 5]
        assert np.all(cost <= res.costs[np.arange(B0), j0]), (j0, cost)
        if prev is not None:
            assert np.all(cost <= prev), (n, cost, prev)
        prev = cost
        eng.close()


# ------------------------------------------------------------------------------------------ 5. return_best

@pytest.mark.parametrize("bounds", [False, True], ids=["free", "bounded"])
def test_return_best_executes_the_best_samples_first_control(M, bounds):
    import torch
    n = 3
    outs = {}
    for rb in (False, True):
        eng, x0, U0 = _setup(M, "mlp", 7)
        eng.set_rate_cost(0.05, anchor=True)
        if bounds:
            eng.set_control_bounds(-0.05, 0.05)  # (tight: the best sample's first control lies outside for some u)
        eng.set_iterations(n, rb, False)
        res = eng.solve(x0, U0, seed=SEED, shift=True)
        v = eng.best(B0)[0]
        want = np.clip(v[:, :, 0], -0.05, 0.05) if bounds else v[:, :, 0]
        if rb:
            _eq(res.u0, want, "host: u0 is the best sample's first control")
            _eq(eng.prev_control(B0), want, "host: the anchor")
        else:
            assert not same_bits(res.u0, want)
        # the graph form, two steps with trajectory logging
        tx, tU, tu0, tc = _tensors(torch, eng, x0, U0)
        dev = torch.device("cuda")
        trx, tru = torch.zeros(2, B0, MLP_NX, device=dev), torch.zeros(2, B0, MLP_NU, device=dev)
        eng.graph_capture_traj(B0, 2, tx.data_ptr(), tU.data_ptr(), tu0.data_ptr(), seed=SEED, traj_x_ptr=trx.data_ptr(),
                               traj_u_ptr=tru.data_ptr())
        eng.graph_launch(sync=True)
        x, U, u0, sx, su = _snap(torch, tx, tU, tu0, trx, tru)
        outs[rb] = (res.U, U)
        if rb:
            v = eng.best(B0)[0]
            want = np.clip(v[:, :, 0], -0.05, 0.05) if bounds else v[:, :, 0]
            _eq(u0, want, "graph: u0")
            _eq(su[1], want, "graph: traj_u holds the executed control")
            _eq(eng.prev_control(B0), want, "graph: the anchor")
            # the state after the env step: a plain env step from it (a one-step handle fed zero noise keeps U)
            one, _, _ = _setup(M, "mlp", 1, K=64)
            t1x = torch.from_numpy(sx[1]).to(dev)
            t1U = torch.from_numpy(np.ascontiguousarray(want[:, :, None])).to(dev)
            t1u0, zero = torch.zeros(B0, MLP_NU, device=dev), torch.zeros(B0, MLP_NU, 1, 64, device=dev)
            one.set_stream(torch.cuda.current_stream().cuda_stream)
            one.solve_device(B0, t1x.data_ptr(), t1U.data_ptr(), zero.data_ptr(), u0_ptr=t1u0.data_ptr(),
                             env_step=True, asynchronous=False)
            x1, u1 = _snap(torch, t1x, t1u0)
            _eq(u1, want, "the one-step handle applied the same control")
            _eq(x, x1, "graph: the state after the env step")
            one.close()
        eng.close()
    _eq(outs[True][0], outs[False][0], "host: U is the return_best = 0 run's")
    if not bounds:  # (in the graph the second step starts from another state once the executed control differs)
        assert not same_bits(outs[True][1], outs[False][1])


# ------------------------------------------------------------------------------------------ 6. add_mean

@pytest.mark.parametrize("keep", [False, True], ids=["j0=0", "j0=count"])
def test_add_mean_enters_the_nominal_as_one_candidate(M, keep):
    eng, x0, U0 = _setup(M, "mlp", 7)
    ref, _, _ = _setup(M, "mlp", 7)
    if keep:
        eng.set_elite_keep(5)
    eng.set_iterations(1, False, True)
    seed, U, j0 = SEED, U0, np.zeros(B0, np.int32)
    nz = ref.noise_eval(B0, seed)
    if keep:  # a first solve stores a set: the second one's column is the one behind it
        U = eng.solve(x0, U0, seed=seed).U
        v, _, _, count, steps = eng.kept(B0)
        assert count.tolist() == [5, 5]
        seed, j0 = SEED + 1, count
        nz = eng.keep_inject_eval(U, ref.noise_eval(B0, seed), v, count, steps)
    got = eng.solve(x0, U, seed=seed)
    plain = ref.solve(x0, U, noise=nz)
    zeroed = nz.copy()
    for b in range(B0):
        zeroed[b, :, :, j0[b]] = 0.0
    want = ref.solve(x0, U, noise=zeroed)
    _eq(got.costs, want.costs, "costs: the zeroed column's solve")
    _eq(got.U, want.U, "U")
    for b in range(B0):
        other = np.arange(K0) != j0[b]
        _eq(got.costs[b, other], plain.costs[b, other], "every other column is unchanged")
        assert got.costs[b, j0[b]] != plain.costs[b, j0[b]]
    eng.close()
    ref.close()


# ------------------------------------------------------------------------------------------ 7. state rules

def test_state_and_argument_errors(M):
    import torch
    L = M._lib
    eng, x0, U0 = _setup(M, "mlp", 7)

    def code(fn):
        with pytest.raises(M.MPPIError) as ei:
            fn()
        return ei.value

    eng.set_iterations(2, True, False)
    for bad in ((0, 0, 0), (17, 0, 0), (-1, 0, 0), (2, 2, 0), (2, 0, -1)):
        assert eng.lib.mppi_set_iterations(eng._h, *bad) == L.MPPI_E_ARG, bad
        assert eng.iterations() == (2, True, False)  # the state is intact
    assert code(lambda: eng.best(B0)).code == L.MPPI_E_STATE  # no tracking solve yet
    nz = np.zeros((B0, MLP_NU, 7, K0), np.float32)
    e = code(lambda: eng.solve(x0, U0, noise=nz))
    assert e.code == L.MPPI_E_ARG and "noise" in str(e)
    e = code(lambda: eng.solve(x0, U0, u0_before=True))
    assert e.code == L.MPPI_E_UNSUPPORTED and "MPPI_FLAG_U0_BEFORE" in str(e) and "n_iter" in str(e)
    eng.set_iterations(1, True, False)
    e = code(lambda: eng.solve(x0, U0, u0_before=True))
    assert e.code == L.MPPI_E_UNSUPPORTED and "MPPI_FLAG_U0_BEFORE" in str(e) and "return_best" in str(e)
    eng.solve(x0, U0, noise=nz)  # one iteration takes injected noise
    assert eng.best(B0)[2].tolist() == [0, 0]  # (all samples alike: the lowest k)
    assert code(lambda: eng.best(B0 + 1)).code == L.MPPI_E_ARG
    eng.set_iterations(1, False, False)
    eng.solve(x0, U0, u0_before=True)  # off: as before
    # a change destroys captured graphs; the value in effect keeps them
    tx, tU, tu0, tc = _tensors(torch, eng, x0, U0)
    eng.set_iterations(2)
    eng.graph_capture(B0, 2, tx.data_ptr(), tU.data_ptr(), tu0.data_ptr(), seed=SEED)
    eng.graph_launch(sync=True)
    assert eng.get_seed_counter() == 4
    eng.set_iterations(2, False, False)
    eng.graph_launch(sync=True)
    assert eng.get_seed_counter() == 8
    eng.set_iterations(2, False, True)
    assert code(lambda: eng.graph_launch(sync=True)).code == L.MPPI_E_STATE
    eng.graph_capture(B0, 2, tx.data_ptr(), tU.data_ptr(), tu0.data_ptr(), seed=SEED)
    eng.graph_launch(sync=True)
    assert eng.get_seed_counter() == 12  # the prefetched noise was kept: no key skipped, none drawn twice
    eng.close()


def test_a_chained_stream_whose_setting_changes_draws_the_loops_keys(M):
    """Chained steps at n_iter = 1, 3, 2 on one stream (the prefetched noise survives each change): the state, U and the
    counter of the defining loop of plain counter solves."""
    import torch
    plan = (1, 3, 2)
    outs = []
    for feature in (True, False):
        eng, x0, U0 = _setup(M, "mlp", 7)
        tx, tU, tu0, tc = _tensors(torch, eng, x0, U0)
        for n in plan:
            if feature:
                eng.set_iterations(n)
            for i in range(1 if feature else n):
                last = feature or i == n - 1
                eng.solve_device(B0, tx.data_ptr(), tU.data_ptr(), None, seed=SEED, u0_ptr=tu0.data_ptr(),
                                 costs_ptr=tc.data_ptr(), shift=last, env_step=last, chain=feature,
                                 seed_counter=not feature, asynchronous=feature)
        outs.append((_snap(torch, tx, tU, tu0, tc), eng.get_seed_counter()))
        eng.close()
    assert outs[0][1] == sum(plan)
    _eq(outs[0], outs[1], "chained, the setting changing mid-stream")
