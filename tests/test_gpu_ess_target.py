"""ESS targeting on the device (mppi_set_ess_target): the search kernel against the float64 conditions of the rule, a
solve that updates with the lambda it chose, every stream form against a loop of plain solves, and the state rules of
the four entries."""
import ctypes

import numpy as np
import pytest

from ess_cases import BOUNDS, FAMILIES, FRACS, N_TIES, check_row, family

pytestmark = pytest.mark.gpu

MLP_NX, MLP_NU = 10, 3
FRAC, LIMITS = 0.25, (1e-3, 1e3)


@pytest.fixture(scope="module")
def M(gpu_available):
    import mppi_hip
    return mppi_hip


def _setup(M, kind, K, H, B, **kw):
    """(engine, x0 [B,nx] f32, U0 [B,nu,H] f32): the analytic cartpole, or a seeded MLP (nu = 3, fp32, quad_est) -- the
    setups of tests/test_gpu_noise_adapt.py."""
    rs = np.random.RandomState(11)
    if kind == "cartpole":
        eng = M.Engine(M.Config.preset("cartpole_py", K=K, H=H, max_batch=B, **kw))
        eng.load_dynamics(1).set_cost("cartpole")
        x0 = np.stack([[0.0, 0.2 + 0.3 * b, 0.0, 0.0] for b in range(B)])
        nu = 1
    else:
        from mppi_hip.nets import mlp_blob, synthetic_mlp
        sd = synthetic_mlp(MLP_NX, MLP_NU, seed=0)
        cfg = dict(nx=MLP_NX, nu=MLP_NU, H=H, K=K, max_batch=B, lambda_=1.0, sigma=0.5, precision=0)
        cfg.update(kw)
        eng = M.Engine(M.Config(**cfg))
        eng.load_dynamics(*mlp_blob(sd, MLP_NX, MLP_NU))
        eng.set_cost("quad_est")
        x0 = 0.3 * rs.randn(B, MLP_NX)
        nu = MLP_NU
    U0 = 0.1 * rs.randn(B, nu, H)
    return eng, x0.astype(np.float32), U0.astype(np.float32)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def _same(a, b, msg=""):
    assert np.array_equal(_bits(a), _bits(b)), (msg, a, b)


def _snap(torch, *ts):
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in ts)


# ------------------------------------------------------------------------------------------ 1. the rule

@pytest.mark.parametrize("K", [30, 75, 2500, 32768])
def test_lambda_eval_meets_the_float64_conditions_on_every_family(M, K):
    """No rollout: lambda_eval on five cost families x three targets at bounds (1e-4, 1e4), B = 2 -- K below a wave,
    ragged, several ragged costs per thread, and kMaxK (the 32-costs-per-thread form).  Both float64 conditions of
    ess_cases.check_row on every row, the end rules exactly, two calls bitwise equal, and the bisection arm
    (MPPI_LAMBDA_SEARCH=bisect) under the same conditions.
    Worst |ESS64(lambda) - T| / T at an interior lambda on an MI355X, K = 30 / 75 / 2500 / 32768: 9.9e-7, 2.9e-6,
    5.6e-6, 8.1e-6 with the default search; 2.0e-6, 3.5e-6, 5.8e-6, 1.1e-5 with bisection."""
    import os
    lo, hi = BOUNDS
    eng = M.Engine(M.Config(nx=4, nu=1, H=2, K=K, max_batch=2, lambda_=2.5))
    worst = {"default": 0.0, "bisect": 0.0}
    for name in FAMILIES:
        c = family(name, K)
        for frac in FRACS:
            eng.set_ess_target(frac, lo, hi)
            lam = eng.lambda_eval(c)
            _same(eng.lambda_eval(c), lam, "two calls")
            os.environ["MPPI_LAMBDA_SEARCH"] = "bisect"
            try:
                lam1 = eng.lambda_eval(c)
            finally:
                del os.environ["MPPI_LAMBDA_SEARCH"]
            for b in range(2):
                worst["default"] = max(worst["default"], check_row(c[b], lam[b], frac, lo, hi) or 0.0)
                worst["bisect"] = max(worst["bisect"], check_row(c[b], lam1[b], frac, lo, hi) or 0.0)
            if name == "ties" and N_TIES >= frac * K:
                _same(lam, np.full(2, lo, np.float32), "ties cover the target: lambda_min")
            if name == "gaps" and K == 2500 and frac == 0.1:
                _same(lam, np.full(2, hi, np.float32), "the target is out of reach: lambda_max")
    print(f"K={K}: worst |ESS64(lambda) - T| / T at an interior lambda:", worst)
    # a row without a finite cost keeps the configured lambda; its neighbour is searched as usual
    c = family("gauss", K)
    c[0] = np.nan
    lam = eng.lambda_eval(c)
    assert lam[0] == np.float32(2.5) and lo < lam[1] < hi
    check_row(c[1], lam[1], FRACS[-1], lo, hi)
    eng.close()


def test_lambda_eval_end_rules_at_k_1_and_needs_targeting(M):
    from mppi_hip import _lib as L
    eng = M.Engine(M.Config(nx=4, nu=1, H=2, K=1, max_batch=2, lambda_=2.5))
    with pytest.raises(M.MPPIError) as ei:  # targeting is off
        eng.lambda_eval(np.ones((2, 1), np.float32))
    assert ei.value.code == L.MPPI_E_STATE
    eng.set_ess_target(0.5, *BOUNDS)
    lam = eng.lambda_eval(np.array([[7.0], [np.inf]], np.float32))
    _same(lam, np.array([BOUNDS[0], 2.5], np.float32), "K = 1: lambda_min; no finite cost: cfg.lambda")
    with pytest.raises(M.MPPIError) as ei:
        eng.lambda_eval(np.ones((3, 1), np.float32))  # beyond max_batch
    assert ei.value.code == L.MPPI_E_ARG
    eng.close()


# ------------------------------------------------------------------------------------------ 2. a solve uses it

@pytest.mark.parametrize("kind", ["cartpole", "mlp"])
@pytest.mark.parametrize("H", [7, 1])
def test_a_solve_updates_with_the_lambda_it_chose(M, kind, H):
    from mppi_hip.stats import ess_ref, solve_stats_ref
    K, B = 130, 2
    eng, x0, U0 = _setup(M, kind, K, H, B)
    nu = U0.shape[1]
    nz = (eng.config.sigma * np.random.RandomState(5).randn(B, nu, H, K)).astype(np.float32)
    ref = eng.solve(x0, U0, noise=nz, want_weights=True, stats=True)  # the same solve without targeting
    eng.set_ess_target(FRAC, *LIMITS)
    assert eng.ess_target() == tuple(float(np.float32(v)) for v in (FRAC,) + LIMITS)
    res = eng.solve(x0, U0, noise=nz, want_weights=True, stats=True)
    lam = eng.lambdas(B)
    _same(res.costs, ref.costs, "targeting changes no cost")
    _same(lam, eng.lambda_eval(res.costs), "the solve's lambda is the kernel's on its costs")
    _same(eng.lambdas(B), lam, "lambda_eval leaves the solve's lambdas readable")
    assert np.all(lam > LIMITS[0]) and np.all(lam < LIMITS[1]) and not np.any(lam == np.float32(eng.config.lambda_))
    c64, e64 = res.costs.astype(np.float64), nz.astype(np.float64)
    for b in range(B):
        check_row(res.costs[b], lam[b], FRAC, *LIMITS)
        w = np.exp(-(c64[b] - c64[b].min()) / float(lam[b]))
        w /= w.sum()
        np.testing.assert_allclose(res.weights[b], w, rtol=0.0, atol=1e-5)
        np.testing.assert_allclose(res.U[b], U0[b] + np.einsum("k,uhk->uh", w, e64[b]), rtol=0.0, atol=1e-4)
        want = solve_stats_ref(res.costs[b], nz[b], lam=float(lam[b]))
        np.testing.assert_allclose(res.stats["ess"][b], ess_ref(res.costs[b], lam[b]), rtol=1e-4, atol=0.0)
        np.testing.assert_allclose(res.stats["free_energy"][b], want["free_energy"], rtol=1e-4, atol=0.0)
        other = solve_stats_ref(res.costs[b], lam=eng.config.lambda_)["free_energy"]  # ... and not cfg.lambda's
        if abs(want["free_energy"] - other) > 1e-3 * abs(want["free_energy"]):
            assert abs(res.stats["free_energy"][b] - want["free_energy"]) < abs(res.stats["free_energy"][b] - other)
        np.testing.assert_allclose(res.stats["entropy"][b], want["entropy"], rtol=1e-4, atol=0.0)
        np.testing.assert_allclose(res.stats["eps_m2"][b], want["eps_m2"], rtol=1e-4, atol=1e-6)
    # lambda_min == lambda_max == cfg.lambda: the update of a handle without targeting
    eng.set_ess_target(FRAC, eng.config.lambda_, eng.config.lambda_)
    pin = eng.solve(x0, U0, noise=nz, want_weights=True, stats=True)
    _same(eng.lambdas(B), np.full(B, eng.config.lambda_, np.float32))
    _same(pin.costs, ref.costs)
    if kind == "mlp":
        for name in ("U", "u0", "weights"):
            _same(getattr(pin, name), getattr(ref, name), name)
        for k, v in ref.stats.items():
            assert np.array_equal(pin.stats[k], v), k
    else:
        # the cartpole's unfused path (rollout, search, reduce_kernel) against its fused one-launch form, whose
        # online-softmin partials are combined block by block: the bits differ, so the cartpole's parity bars
        np.testing.assert_allclose(pin.weights, ref.weights, rtol=0.0, atol=1e-5)
        np.testing.assert_allclose(pin.U, ref.U, rtol=0.0, atol=1e-4)
        np.testing.assert_allclose(pin.u0, ref.u0, rtol=0.0, atol=1e-4)
    # disabling restores the handle: bitwise the first solve
    eng.set_ess_target(0.0)
    off = eng.solve(x0, U0, noise=nz, want_weights=True, stats=True)
    for name in ("costs", "U", "u0", "weights"):
        _same(getattr(off, name), getattr(ref, name), name)
    eng.close()


@pytest.mark.parametrize("kind", ["cartpole", "mlp"])
def test_launches_per_solve(M, kind):
    """A handle that never enables targeting launches what it launched before (the cartpole: its one fused launch, no
    reduce); with targeting the search sits between the rollout and the reduce, and the cartpole takes three launches."""
    K, H, B = 130, 7, 2
    eng, x0, U0 = _setup(M, kind, K, H, B)

    def counts():
        eng.profile(True)  # (resets the counters)
        eng.solve(x0, U0, seed=3)
        got = {k: eng.kernel_time(k)[0] for k in ("noise", "rollout", "lambda", "reduce", "stats")}
        eng.profile(False)
        return got

    fused = kind == "cartpole"
    assert counts() == dict(noise=1, rollout=1, reduce=0 if fused else 1, stats=0, **{"lambda": 0})
    eng.set_ess_target(FRAC, *LIMITS)
    assert counts() == dict(noise=1, rollout=1, reduce=1, stats=0, **{"lambda": 1})
    eng.set_ess_target(0.0)
    assert counts() == dict(noise=1, rollout=1, reduce=0 if fused else 1, stats=0, **{"lambda": 0})
    eng.close()


# ------------------------------------------------------------------------------------------ 3. streams

def _run_form(M, torch, kind, form, n, seed, adapt):
    """One stream form, two launches of n steps (shift + env step) with targeting on.  Returns snaps (x0, U, u0 after
    each launch), lam (the lambda of each of the 2n steps; None where the form cannot be asked per step), law (the law
    history, adapting runs), ctr."""
    from mppi_hip.trajectory import run_stream
    K, H, B = 130, 8, 2
    dev = torch.device("cuda")
    eng, x0, U0 = _setup(M, kind, K, H, B)
    eng.set_ess_target(FRAC, *LIMITS)
    if adapt:
        eng.set_noise_model(*(([0.6], 0.7) if kind == "cartpole" else ([0.2, 0.5, 0.8], 0.7)))
        eng.set_noise_adapt(0.3)
    law = lambda i: tuple(np.asarray(v, np.float32) for v in eng.noise_law(i)) if adapt else None
    out = dict(snaps=[], lam=[], law=[])
    if form == "traj":
        out["traj"] = run_stream(eng, x0, U0, n, seed=seed, launches=2)
        out["lam"] = [None] * n + [eng.lambdas(B, i) for i in range(n)]
        out["law"] = [None] * n + [law(i) for i in range(n)]
    else:
        eng.set_stream(torch.cuda.current_stream().cuda_stream)
        tx, tU = torch.from_numpy(x0).to(dev), torch.from_numpy(U0).to(dev)
        tu0 = torch.zeros(B, U0.shape[1], device=dev)
        out["x_before"], out["u0_steps"] = [], []
        if form == "graph":
            eng.graph_capture(B, n, tx.data_ptr(), tU.data_ptr(), tu0.data_ptr(), seed=seed)
            for _ in range(2):
                eng.graph_launch(sync=True)
                out["snaps"].append(_snap(torch, tx, tU, tu0))
                out["lam"] += [eng.lambdas(B, i) for i in range(n)]
                out["law"] += [law(i) for i in range(n)]
        else:
            for i in range(2 * n):
                if form == "plain":
                    out["x_before"].append(_snap(torch, tx)[0])
                eng.solve_device(B, tx.data_ptr(), tU.data_ptr(), None, seed=seed, u0_ptr=tu0.data_ptr(), shift=True,
                                 env_step=True, seed_counter=form == "plain", chain=form != "plain")
                out["lam"].append(eng.lambdas(B, 0))
                out["law"].append(law(0))
                if form == "plain":
                    out["u0_steps"].append(_snap(torch, tu0)[0])
                if i + 1 in (n, 2 * n):
                    out["snaps"].append(_snap(torch, tx, tU, tu0))
    out["ctr"] = eng.get_seed_counter()
    eng.close()
    return out


@pytest.mark.parametrize("kind", ["cartpole", "mlp"])
@pytest.mark.parametrize("adapt", [False, True], ids=["white", "adapting"])
def test_stream_forms_agree_bitwise(M, kind, adapt):
    """Plain counter solves, chained solves, one graph launched twice and graph_capture_traj via run_stream: bitwise
    equal x0, U, u0 and per-step lambda (with set_noise_model + set_noise_adapt on: the law history too), seed counter
    2n; get_lambda(step) after a graph launch returns each step's value."""
    import torch
    n, seed = 4, 9
    outs = {f: _run_form(M, torch, kind, f, n, seed, adapt) for f in ("plain", "chain", "graph", "traj")}
    want = outs["plain"]
    for form, got in outs.items():
        assert got["ctr"] == 2 * n, form
        for sa, sb in zip(got["snaps"], want["snaps"]):
            for a, b in zip(sa, sb):
                np.testing.assert_array_equal(a, b, err_msg=form)
        assert len(got["lam"]) == 2 * n
        for i, (a, b) in enumerate(zip(got["lam"], want["lam"])):
            if a is not None:
                _same(a, b, (form, "lambda of step", i))
        for i, (a, b) in enumerate(zip(got["law"], want["law"])):
            if a is not None:
                _same(a[0], b[0], (form, "sigma_u of step", i))
                _same(a[1], b[1], (form, "rho of step", i))
    states, actions, U_end = outs["traj"]["traj"]
    np.testing.assert_array_equal(states, np.stack(want["x_before"]))
    np.testing.assert_array_equal(actions, np.stack(want["u0_steps"]))
    np.testing.assert_array_equal(U_end, want["snaps"][1][1])
    # the stream moved, and so did lambda: the per-step values are each step's own
    lam = np.stack(want["lam"])
    assert len({tuple(_bits(v)) for v in lam}) == 2 * n
    assert np.all(lam > LIMITS[0]) and np.all(lam < LIMITS[1])


# ------------------------------------------------------------------------------------------ 4. state rules

def test_bad_arguments_are_refused_and_change_nothing(M):
    from mppi_hip import _lib as L
    eng = M.Engine(M.Config(nx=MLP_NX, nu=MLP_NU, H=4, K=16))
    lib = eng.lib
    nan, inf = float("nan"), float("inf")
    bad = [(-0.1, 1e-3, 1e3), (1.5, 1e-3, 1e3), (nan, 1e-3, 1e3), (0.1, 0.0, 1e3), (0.1, -1.0, 1e3), (0.1, 2.0, 1.0),
           (0.1, 1e-3, inf), (0.1, nan, 1e3), (0.1, 1e-3, nan), (0.0, 2.0, 1.0), (0.0, 0.0, 1.0)]
    for state in ("off", "on"):
        if state == "on":
            eng.set_ess_target(0.25, 0.01, 50.0)
        want = eng.ess_target()
        for args in bad:
            assert lib.mppi_set_ess_target(eng._h, *(ctypes.c_float(v) for v in args)) == L.MPPI_E_ARG, args
            assert b"mppi_set_ess_target" in lib.mppi_last_error()
            assert eng.ess_target() == want, args
    assert eng.ess_target() == tuple(float(np.float32(v)) for v in (0.25, 0.01, 50.0))
    eng.set_ess_target(1.0, 3.0, 3.0)  # the edges are allowed
    eng.set_ess_target(0.0, 0.5, 2.0)  # off: the limits are kept
    assert eng.ess_target() == (0.0, 0.5, 2.0)
    eng.close()


def test_set_ess_target_destroys_graphs_keeps_the_prefetched_noise_and_disabling_restores(M):
    import torch
    from mppi_hip import _lib as L
    K, H, B, n, seed = 130, 8, 2, 3, 21
    dev = torch.device("cuda")

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

    eng, tx, tU, tu0 = start()
    with pytest.raises(M.MPPIError) as ei:  # no targeting solve yet
        eng.lambdas(B)
    assert ei.value.code == L.MPPI_E_STATE
    eng.graph_capture(B, n, tx.data_ptr(), tU.data_ptr(), tu0.data_ptr(), seed=seed)
    eng.graph_launch(sync=True)  # leaves a prefetched noise: the device counter is one ahead
    assert eng.get_seed_counter() == n
    eng.set_ess_target(FRAC, *LIMITS)
    assert eng.get_seed_counter() == n  # the key sequence is unchanged
    with pytest.raises(M.MPPIError) as ei:
        eng.graph_launch(sync=True)
    assert ei.value.code == L.MPPI_E_STATE and "mppi_graph_capture first" in str(ei.value)
    with pytest.raises(M.MPPIError) as ei:  # enabling alone is no targeting solve
        eng.lambdas(B)
    assert ei.value.code == L.MPPI_E_STATE
    eng.graph_capture(B, n, tx.data_ptr(), tU.data_ptr(), tu0.data_ptr(), seed=seed)
    eng.graph_launch(sync=True)
    assert eng.get_seed_counter() == 2 * n
    eng.lambdas(B, n - 1)
    for args in ((B, n), (B, -1), (B + 1, 0), (0, 0)):  # beyond the graph / the batch
        with pytest.raises(M.MPPIError) as ei:
            eng.lambdas(*args)
        assert ei.value.code == L.MPPI_E_ARG, args
    eng.set_ess_target(FRAC, *LIMITS)  # the same settings: nothing changes, the graph stays
    eng.graph_launch(sync=True)
    eng.set_ess_target(0.5, *LIMITS)  # a change of the settings destroys it
    with pytest.raises(M.MPPIError) as ei:
        eng.graph_launch(sync=True)
    assert ei.value.code == L.MPPI_E_STATE
    eng.set_ess_target(0.0)  # ... and so does disabling
    eng.graph_capture(B, n, tx.data_ptr(), tU.data_ptr(), tu0.data_ptr(), seed=seed)
    eng.set_ess_target(0.0, 0.5, 2.0)  # off -> off: only the limits are kept, nothing to destroy
    eng.graph_launch(sync=True)
    eng.close()

    # a prefetched noise survives set_ess_target: a chain with the settings changed after two steps goes on with the
    # noise it would have drawn -- what plain counter solves with the same switch draw
    a = start()
    chain(*a, 2)
    a[0].set_ess_target(FRAC, *LIMITS)
    got = chain(*a, 2)
    assert a[0].get_seed_counter() == 4
    b = start()
    eng_b, bx, bU, bu0 = b
    for i in range(4):
        if i == 2:
            eng_b.set_ess_target(FRAC, *LIMITS)
        eng_b.solve_device(B, bx.data_ptr(), bU.data_ptr(), None, seed=seed, u0_ptr=bu0.data_ptr(), shift=True,
                           env_step=True, seed_counter=True)
    want = _snap(torch, bx, bU, bu0)
    for x, y in zip(got, want):
        np.testing.assert_array_equal(x, y)
    _same(a[0].lambdas(B), eng_b.lambdas(B))
    # disabling restores outputs bitwise equal to a fresh handle's
    a[0].set_ess_target(0.0)
    fresh, x0, U0 = _setup(M, "mlp", K, H, B)
    r1 = a[0].solve(x0, U0, seed=77, want_weights=True)
    r2 = fresh.solve(x0, U0, seed=77, want_weights=True)
    for name in ("costs", "U", "u0", "weights"):
        _same(getattr(r1, name), getattr(r2, name), name)
    for e in (a[0], eng_b, fresh):
        e.close()
