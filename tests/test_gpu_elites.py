"""Elite truncation on the device (mppi_set_elites): the selection kernel against the numpy reference, exactly; a solve
whose softmin weighs the elite set alone; the pass-through at n_elite = K; the composition with the cost terms, bounds
and ESS targeting; every stream form against a loop of plain solves; and the state rules of the four entries."""
import ctypes

import numpy as np
import pytest

from elite_cases import FAMILIES, KS, family, hand_rows, n_elites

pytestmark = pytest.mark.gpu

MLP_NX, MLP_NU = 10, 3
FRAC, LIMITS = 0.25, (1e-3, 1e3)


@pytest.fixture(scope="module")
def M(gpu_available):
    import mppi_hip
    return mppi_hip


def _setup(M, kind, K, H, B, **kw):
    """(engine, x0 [B,nx] f32, U0 [B,nu,H] f32): the analytic cartpole, or a seeded MLP (nu = 3, fp32, quad_est) -- the
    setups of tests/test_gpu_ess_target.py."""
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


def _same_set(got, want, msg=""):
    """(idx, count, tau[, ecost]) exactly: integer indices, bitwise tau / ecost."""
    assert np.array_equal(got[0], want[0]), (msg, "idx")
    assert np.array_equal(got[1], want[1]), (msg, "count", got[1], want[1])
    _same(got[2], want[2], (msg, "tau"))
    if len(got) > 3 and len(want) > 3:
        _same(got[3], want[3], (msg, "ecost"))


def _snap(torch, *ts):
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in ts)


def _softmin64(c, lam):
    """float64 softmin weights over the finite entries of c (0 elsewhere)."""
    c = np.asarray(c, np.float64)
    fin = np.isfinite(c)
    w = np.zeros_like(c)
    w[fin] = np.exp(-(c[fin] - c[fin].min()) / float(lam))
    return w / w.sum()


# ------------------------------------------------------------------------------------------ 1. the rule

@pytest.mark.parametrize("K", KS)
def test_elites_eval_equals_the_reference_exactly(M, K):
    """No rollout: elites_eval on seven cost families x the n_elite grid, B = 2 with rows that differ -- K below a
    wave, ragged, pad lanes (Kp > K), several ragged costs per thread, both sides of the switch between the kernel's two
    forms (4096 / 4097) and kMaxK.  idx and count as integers, tau and ecost bit for bit; two calls bitwise equal."""
    from mppi_hip.stats import elite_select_ref
    eng = M.Engine(M.Config(nx=4, nu=1, H=2, K=K, max_batch=2, lambda_=2.5))
    for name in FAMILIES:
        c = family(name, K)
        for n_elite in n_elites(c):
            eng.set_elites(n_elite)
            assert eng.elites() == n_elite
            got = eng.elites_eval(c)
            _same_set(got, elite_select_ref(c, n_elite), (name, K, n_elite))
            _same_set(eng.elites_eval(c), got, (name, K, n_elite, "two calls"))
    # a row without a finite cost: an empty set, and its neighbour is selected as usual
    c = family("gauss", K)
    c[0] = np.nan
    n_elite = max(1, K // 10)
    eng.set_elites(n_elite)
    idx, count, tau, ecost = eng.elites_eval(c)
    assert count[0] == 0 and np.isposinf(tau[0]) and np.all(np.isposinf(ecost[0])) and np.all(idx[0] == -1)
    _same_set((idx, count, tau, ecost), elite_select_ref(c, n_elite), "a row with no finite cost")
    assert count[1] == n_elite
    eng.close()


def test_elites_eval_on_the_hand_written_rows(M):
    """Ties straddling the threshold, -0.0 / +0.0, negatives, denormals (ordered by value, not flushed), NaN and both
    infinities, n_elite beyond the finite count, no finite cost, K = 1."""
    for name, row, n_elite, idx, count, tau, ecost in hand_rows():
        eng = M.Engine(M.Config(nx=4, nu=1, H=2, K=len(row), max_batch=2))
        eng.set_elites(n_elite)
        c = np.array([row, row[::-1]], np.float32)
        got = eng.elites_eval(c)
        want = (np.array(idx, np.int32), np.int32(count), np.float32(tau),
                np.array([np.inf if v is None else v for v in ecost], np.float32))
        _same_set(tuple(g[0] for g in got), want, name)
        eng.close()


# ------------------------------------------------------------------------------------------ 2. a solve uses it

@pytest.mark.parametrize("kind", ["cartpole", "mlp"])
@pytest.mark.parametrize("H", [7, 1])
def test_a_solve_weighs_the_elite_set_alone(M, kind, H):
    """Injected noise, n_elite = K // 10.  The weights are exactly 0 off the set and the float64 softmin over the
    elites on it, U the weighted noise sum over the elites (the tolerances of
    test_gpu_ess_target.test_a_solve_updates_with_the_lambda_it_chose for the same comparisons)."""
    from mppi_hip.stats import elite_select_ref, solve_stats_ref
    K, B = 130, 2
    n_elite = K // 10
    eng, x0, U0 = _setup(M, kind, K, H, B)
    nu, lam = U0.shape[1], eng.config.lambda_
    nz = (eng.config.sigma * np.random.RandomState(5).randn(B, nu, H, K)).astype(np.float32)
    ref = eng.solve(x0, U0, noise=nz, want_weights=True, stats=True)  # the same solve without elites
    eng.set_elites(n_elite)
    res = eng.solve(x0, U0, noise=nz, want_weights=True, stats=True)
    _same(res.costs, ref.costs, "elites change no cost")
    got = eng.elite_set(B)
    ev = eng.elites_eval(res.costs)
    _same_set(got, ev, "the solve's set is the kernel's on its costs")
    _same_set(eng.elite_set(B), got, "elites_eval leaves the solve's set readable")
    idx, count, tau, ecost = elite_select_ref(res.costs, n_elite)
    _same_set(ev, (idx, count, tau, ecost), "... and the reference's")
    assert np.all(count == n_elite)
    e64 = nz.astype(np.float64)
    for b in range(B):
        off = np.setdiff1d(np.arange(K), idx[b])
        assert np.all(res.weights[b, off] == 0.0), "a sample off the set has weight exactly 0"
        w = _softmin64(ecost[b], lam)
        assert np.count_nonzero(w) <= n_elite
        np.testing.assert_allclose(res.weights[b], w, rtol=0.0, atol=1e-5)
        Unew = U0[b] + np.einsum("k,uhk->uh", w[idx[b]], e64[b][:, :, idx[b]])  # the elites alone
        np.testing.assert_allclose(res.U[b], Unew, rtol=0.0, atol=1e-4)
        assert res.stats["n_finite"][b] == count[b]
        assert res.stats["k_best"][b] in idx[b] and res.stats["k_best"][b] == ref.stats["k_best"][b]
        want = solve_stats_ref(ecost[b], nz[b], lam=lam)
        np.testing.assert_allclose(res.stats["cost_weighted"][b], want["cost_weighted"], rtol=1e-4, atol=0.0)
    assert np.abs(res.weights - ref.weights).max() > 1e-3, "the truncation must move the weights"
    # disabling restores the handle: bitwise the first solve
    eng.set_elites(0)
    assert eng.elites() == 0
    off = eng.solve(x0, U0, noise=nz, want_weights=True, stats=True)
    for name in ("costs", "U", "u0", "weights"):
        _same(getattr(off, name), getattr(ref, name), name)
    for k, v in ref.stats.items():
        assert np.array_equal(off.stats[k], v), k
    eng.close()


# ------------------------------------------------------------------------------------------ 3. pass-through

@pytest.mark.parametrize("kind", ["cartpole", "mlp"])
def test_n_elite_k_is_the_solve_without_elites(M, kind):
    """n_elite = K with every cost finite: U, u0, weights and the statistics are bitwise the solve without elites.
    (The cartpole is compared in its unfused form on both sides -- ESS targeting pinned to cfg.lambda -- because its
    fused one-launch form combines the softmin block by block and differs in the last bits from reduce_kernel.)"""
    K, H, B = 130, 7, 2
    eng, x0, U0 = _setup(M, kind, K, H, B)
    nz = (eng.config.sigma * np.random.RandomState(5).randn(B, U0.shape[1], H, K)).astype(np.float32)
    if kind == "cartpole":
        eng.set_ess_target(FRAC, eng.config.lambda_, eng.config.lambda_)
    ref = eng.solve(x0, U0, noise=nz, want_weights=True, stats=True)
    assert np.all(np.isfinite(ref.costs))
    eng.set_elites(K)
    res = eng.solve(x0, U0, noise=nz, want_weights=True, stats=True)
    for name in ("costs", "U", "u0", "weights"):
        _same(getattr(res, name), getattr(ref, name), name)
    for k, v in ref.stats.items():
        assert np.array_equal(res.stats[k], v), k
    idx, count, _ = eng.elite_set(B)
    assert np.all(count == K) and np.array_equal(idx, np.tile(np.arange(K, dtype=np.int32), (B, 1)))
    eng.close()


# ------------------------------------------------------------------------------------------ 4. composition

@pytest.mark.parametrize("kind", ["cartpole", "mlp"])
def test_elites_behind_the_cost_terms_and_ahead_of_the_lambda_search(M, kind):
    """Control cost + rate cost + bounds + elites + ESS targeting: the set is the reference's on
    (costs + control term) + rate term, added in fp32 in that order, and the lambda is lambda_eval's on ecost."""
    from mppi_hip.stats import elite_select_ref
    K, H, B = 130, 7, 2
    n_elite = 20
    eng, x0, U0 = _setup(M, kind, K, H, B)
    nu, sigma = U0.shape[1], eng.config.sigma
    nz = (sigma * np.random.RandomState(5).randn(B, nu, H, K)).astype(np.float32)
    eng.set_control_cost(0.05)
    eng.set_rate_cost(np.linspace(0.4, 0.2, nu), anchor=True)
    eng.set_control_bounds(-0.6 * sigma, 0.5 * sigma)
    eng.set_ess_target(FRAC, *LIMITS)
    ref = eng.solve(x0, U0, noise=nz, want_weights=True)
    eng.set_elites(n_elite)
    res = eng.solve(x0, U0, noise=nz, want_weights=True, stats=True)
    _same(res.costs, ref.costs, "elites change no cost")
    wc = ((res.costs + eng.control_term(B)[0]).astype(np.float32) + eng.rate_term(B)).astype(np.float32)
    want = elite_select_ref(wc, n_elite)
    got = eng.elite_set(B)
    _same_set(got, want[:3], "the set of (costs + control term) + rate term")
    assert not np.array_equal(want[0], elite_select_ref(res.costs, n_elite)[0]), "the terms must move the set"
    lams = eng.lambdas(B)
    _same(lams, eng.lambda_eval(want[3]), "the search ran on ecost")
    assert not np.array_equal(_bits(lams), _bits(eng.lambda_eval(wc)))
    for b in range(B):
        np.testing.assert_allclose(res.weights[b], _softmin64(want[3][b], float(lams[b])), rtol=0.0, atol=1e-5)
        assert np.all(res.weights[b, np.setdiff1d(np.arange(K), want[0][b])] == 0.0)
        assert res.stats["n_finite"][b] == n_elite
    eng.close()


# ------------------------------------------------------------------------------------------ 5. streams

def _run_form(M, torch, kind, form, n, seed, adapt):
    """One stream form, n steps (device noise, shift + env step) with elites on.  Returns the state after the n steps,
    the last solve's set and the seed counter."""
    from mppi_hip.trajectory import run_stream
    K, H, B = 130, 8, 2
    dev = torch.device("cuda")
    eng, x0, U0 = _setup(M, kind, K, H, B)
    eng.set_elites(17)
    if adapt:
        eng.set_noise_model(*(([0.6], 0.7) if kind == "cartpole" else ([0.2, 0.5, 0.8], 0.7)))
        eng.set_noise_adapt(0.3)
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
            out["x_before"], out["u0_steps"], out["sets"] = [], [], []
            for i in range(n):
                if form == "plain":
                    out["x_before"].append(_snap(torch, tx)[0])
                eng.solve_device(B, tx.data_ptr(), tU.data_ptr(), None, seed=seed, u0_ptr=tu0.data_ptr(), shift=True,
                                 env_step=True, seed_counter=form == "plain", chain=form != "plain")
                if form == "plain":
                    out["u0_steps"].append(_snap(torch, tu0)[0])
                    out["sets"].append(eng.elite_set(B))
        out["x"], out["U"], out["u0"] = _snap(torch, tx, tU, tu0)
    out["set"] = eng.elite_set(B)
    out["law"] = eng.noise_model()[:2] if adapt else None
    out["ctr"] = eng.get_seed_counter()
    eng.close()
    return out


@pytest.mark.parametrize("kind", ["cartpole", "mlp"])
@pytest.mark.parametrize("adapt", [False, True], ids=["white", "adapting"])
def test_stream_forms_agree_bitwise(M, kind, adapt):
    """Plain counter solves, chained solves, a captured graph of 3 solves and graph_capture_traj via run_stream (shift +
    env step): bitwise equal x0, U, u0 and last elite set, seed counter 3 -- also with the noise adaptation on, whose
    moments then see the elites alone."""
    import torch
    n, seed = 3, 9
    outs = {f: _run_form(M, torch, kind, f, n, seed, adapt) for f in ("plain", "chain", "graph", "traj")}
    want = outs["plain"]
    for form, got in outs.items():
        assert got["ctr"] == n, form
        np.testing.assert_array_equal(got["U"], want["U"], err_msg=form)
        if form != "traj":
            np.testing.assert_array_equal(got["x"], want["x"], err_msg=form)
            np.testing.assert_array_equal(got["u0"], want["u0"], err_msg=form)
        _same_set(got["set"], want["set"], (form, "the last solve's set"))
        if adapt:
            _same(got["law"][0], want["law"][0], (form, "sigma_u"))
            _same(np.float32(got["law"][1]), np.float32(want["law"][1]), (form, "rho"))
    states, actions = outs["traj"]["traj"]
    np.testing.assert_array_equal(states, np.stack(want["x_before"]))
    np.testing.assert_array_equal(actions, np.stack(want["u0_steps"]))
    # the stream moved, and so did the set: each step's is its own
    assert len({s[0].tobytes() for s in want["sets"]}) == n
    assert all(np.all(s[1] == 17) for s in want["sets"])


def test_host_pointer_and_async_solves_agree_with_plain_device_solves(M):
    """The host-pointer solve and an ASYNC device solve of the same inputs and key: bitwise the same U, u0 and set."""
    import torch
    K, H, B, seed = 130, 8, 2, 4
    dev = torch.device("cuda")
    eng, x0, U0 = _setup(M, "mlp", K, H, B)
    eng.set_elites(17)
    host = eng.solve(x0, U0, seed=seed)
    host_set = eng.elite_set(B)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    for asynchronous in (False, True):
        tx, tU = torch.from_numpy(x0).to(dev), torch.from_numpy(U0).to(dev)
        tu0 = torch.zeros(B, MLP_NU, device=dev)
        eng.solve_device(B, tx.data_ptr(), tU.data_ptr(), None, seed=seed, u0_ptr=tu0.data_ptr(),
                         asynchronous=asynchronous)
        got_set = eng.elite_set(B)  # (waits for the stream)
        U, u0 = _snap(torch, tU, tu0)
        _same(U, host.U, ("U", asynchronous))
        _same(u0, host.u0, ("u0", asynchronous))
        _same_set(got_set, host_set, asynchronous)
    eng.close()


# ------------------------------------------------------------------------------------------ 6. state rules

def test_state_and_argument_errors(M):
    from mppi_hip import _lib as L
    K = 16
    eng = M.Engine(M.Config(nx=MLP_NX, nu=MLP_NU, H=4, K=K, max_batch=2))
    c = np.ones((2, K), np.float32)
    for call in (lambda: eng.elites_eval(c), lambda: eng.elite_set(1)):  # elites are off / no solve ran
        with pytest.raises(M.MPPIError) as ei:
            call()
        assert ei.value.code == L.MPPI_E_STATE
    for state in (0, 5):
        eng.set_elites(state)
        for bad in (-1, K + 1, 1 << 30):
            assert eng.lib.mppi_set_elites(eng._h, bad) == L.MPPI_E_ARG, bad
            assert b"mppi_set_elites" in eng.lib.mppi_last_error()
            assert eng.elites() == state, "a refused value changes nothing"
    eng.set_elites(K)  # the edges are allowed
    eng.set_elites(1)
    with pytest.raises(M.MPPIError) as ei:  # enabling alone is no solve
        eng.elite_set(1)
    assert ei.value.code == L.MPPI_E_STATE
    with pytest.raises(M.MPPIError) as ei:
        eng.elites_eval(np.ones((3, K), np.float32))  # beyond max_batch
    assert ei.value.code == L.MPPI_E_ARG
    # every output of the evaluation is optional
    eng.set_elites(3)
    cnt = np.zeros(2, np.int32)
    assert eng.lib.mppi_elites_eval(eng._h, 2, c.ctypes.data_as(ctypes.c_void_p), None, None, None, None) == L.MPPI_OK
    assert eng.lib.mppi_elites_eval(eng._h, 2, c.ctypes.data_as(ctypes.c_void_p), None,
                                    cnt.ctypes.data_as(ctypes.c_void_p), None, None) == L.MPPI_OK
    assert cnt.tolist() == [3, 3]
    assert eng.lib.mppi_elites_eval(eng._h, 2, None, None, None, None, None) == L.MPPI_E_ARG
    eng.close()


def test_set_elites_destroys_graphs_keeps_the_prefetched_noise_and_the_last_set(M):
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
    eng.graph_capture(B, n, tx.data_ptr(), tU.data_ptr(), tu0.data_ptr(), seed=seed)
    eng.graph_launch(sync=True)  # leaves a prefetched noise: the device counter is one ahead
    assert eng.get_seed_counter() == n
    eng.set_elites(17)
    assert eng.get_seed_counter() == n  # the key sequence is unchanged
    with pytest.raises(M.MPPIError) as ei:
        eng.graph_launch(sync=True)
    assert ei.value.code == L.MPPI_E_STATE and "mppi_graph_capture first" in str(ei.value)
    eng.graph_capture(B, n, tx.data_ptr(), tU.data_ptr(), tu0.data_ptr(), seed=seed)
    eng.graph_launch(sync=True)
    assert eng.get_seed_counter() == 2 * n
    idx, count, tau = eng.elite_set(B)
    assert idx.shape == (B, 17) and np.all(count == 17) and np.all(np.isfinite(tau))
    for bad in (B + 1, 0):  # beyond the batch of that launch
        with pytest.raises(M.MPPIError) as ei:
            eng.elite_set(bad)
        assert ei.value.code == L.MPPI_E_ARG, bad
    eng.set_elites(17)  # the same value: nothing changes, the graph stays
    eng.graph_launch(sync=True)
    eng.set_elites(18)  # a change destroys it
    with pytest.raises(M.MPPIError) as ei:
        eng.graph_launch(sync=True)
    assert ei.value.code == L.MPPI_E_STATE
    eng.set_elites(0)  # ... and so does disabling
    eng.graph_capture(B, n, tx.data_ptr(), tU.data_ptr(), tu0.data_ptr(), seed=seed)
    eng.set_elites(0)  # off -> off: nothing to destroy
    eng.graph_launch(sync=True)
    eng.close()

    # a prefetched noise survives set_elites: a chain with elites switched on after two steps goes on with the noise it
    # would have drawn -- what plain counter solves with the same switch draw
    a = start()
    chain(*a, 2)
    a[0].set_elites(17)
    got = chain(*a, 2)
    assert a[0].get_seed_counter() == 4
    eng_b, bx, bU, bu0 = start()
    for i in range(4):
        if i == 2:
            eng_b.set_elites(17)
        eng_b.solve_device(B, bx.data_ptr(), bU.data_ptr(), None, seed=seed, u0_ptr=bu0.data_ptr(), shift=True,
                           env_step=True, seed_counter=True)
    want = _snap(torch, bx, bU, bu0)
    for x, y in zip(got, want):
        np.testing.assert_array_equal(x, y)
    _same_set(a[0].elite_set(B), eng_b.elite_set(B))
    for e in (a[0], eng_b):
        e.close()


@pytest.mark.parametrize("kind", ["cartpole", "mlp"])
def test_launches_per_solve(M, kind):
    """A handle that never enables elites launches what it launched before (the cartpole: its one fused launch, no
    reduce); with elites the selection sits between the rollout and the reduce, and the cartpole takes three launches:
    rollout, elites and reduce all have a count in mppi_kernel_time."""
    K, H, B = 130, 7, 2
    eng, x0, U0 = _setup(M, kind, K, H, B)

    def counts():
        eng.profile(True)  # (resets the counters)
        eng.solve(x0, U0, seed=3)
        got = {k: eng.kernel_time(k)[0] for k in ("noise", "rollout", "elites", "lambda", "reduce", "stats")}
        eng.profile(False)
        return got

    fused = kind == "cartpole"
    base = dict(noise=1, rollout=1, stats=0, **{"lambda": 0})
    assert counts() == dict(base, elites=0, reduce=0 if fused else 1)
    eng.set_elites(13)
    assert counts() == dict(base, elites=1, reduce=1)
    eng.set_elites(0)
    assert counts() == dict(base, elites=0, reduce=0 if fused else 1)
    eng.close()
