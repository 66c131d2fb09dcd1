"""The sampling law adapted on the device (mppi_set_noise_adapt): the device-law generators against the by-value ones,
the update kernel against its numpy float32 restatement (mppi_hip.stats.adapt_noise_model_f32), every stream form
against a loop of plain solves, and the state rules of the three entries."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MLP_NX, MLP_NU = 10, 3
LIMITS = (1e-3, 10.0, 0.95)


@pytest.fixture(scope="module")
def M(gpu_available):
    import mppi_hip
    return mppi_hip


def _setup(M, kind, K, H, B, **kw):
    """(engine, x0 [B,nx] f32, U0 [B,nu,H] f32): the analytic cartpole, or a seeded MLP (nu = 3, fp32, quad_est)."""
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


@pytest.fixture(params=["direct", "lds"])
def path(request, monkeypatch):
    """Both generators (MPPI_NOISE_AR1, read per launch), in their by-value and their device-law forms."""
    monkeypatch.setenv("MPPI_NOISE_AR1", request.param)
    return request.param


def _model_for(kind):
    return ([0.6], 0.7) if kind == "cartpole" else ([0.2, 0.5, 0.8], 0.7)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def _same_law(a, b):
    """(sigma_u, rho) pairs, bit for bit."""
    assert np.array_equal(_bits(a[0]), _bits(b[0])), (a, b)
    assert _bits(np.float32(a[1])) == _bits(np.float32(b[1])), (a, b)


def _f32_step(law, st, rate, limits=LIMITS):
    from mppi_hip.stats import adapt_noise_model_f32
    return adapt_noise_model_f32(law[0], law[1], st["eps_m2"], st["eps_m11"], rate, *limits, n_finite=st["n_finite"])


def _snap(torch, *ts):
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in ts)


# ------------------------------------------------------------------------------------------ 1. one step

@pytest.mark.parametrize("kind", ["cartpole", "mlp"])
@pytest.mark.parametrize("H", [7, 1])
def test_one_step_draws_the_by_value_noise_and_moves_the_law_by_the_rule(M, kind, H, path):
    K, B, rate, seed = 130, 2, 0.3, 0x5151_0000_0007
    sig, rho = _model_for(kind)
    ref, x0, U0 = _setup(M, kind, K, H, B)
    ref.set_noise_model(sig, rho)
    r0 = ref.solve(x0, U0, seed=seed, stats=True)
    eng, _, _ = _setup(M, kind, K, H, B)
    eng.set_noise_model(sig, rho)
    eng.set_noise_adapt(rate)
    assert eng.noise_adapt() == tuple(float(np.float32(v)) for v in (rate,) + LIMITS)
    r1 = eng.solve(x0, U0, seed=seed)
    for name in ("costs", "U", "u0"):  # the device-law generators == the by-value ones; adapting changes no solve
        assert np.array_equal(getattr(r1, name), getattr(r0, name)), name
    st = eng.stats(B)  # the solve carried the statistics
    for k, v in r0.stats.items():
        assert np.array_equal(st[k], v), k
    init = (np.asarray(sig, np.float32), np.float32(rho))
    _same_law(eng.noise_law(0), init)
    s, r, active = eng.noise_model()
    assert active is True
    _same_law((s, r), _f32_step(init, st, rate))
    assert not np.array_equal(s, init[0])
    ref.close()
    eng.close()


# ------------------------------------------------------------------------------------------ 2, 3. streams

def _run_form(M, torch, kind, form, n, seed, rate, monkeypatch=None):
    """One stream form, two launches of n steps (shift + env step) with adaptation on.  Returns a dict: snaps (x0, U,
    u0 after each launch), hist (the law each of the 2n steps drew from; None where the form cannot be asked per
    step), law (the final law), stats (per step, graph only), ctr."""
    from mppi_hip.trajectory import run_stream
    K, H, B = 128, 8, 2
    dev = torch.device("cuda")
    eng, x0, U0 = _setup(M, kind, K, H, B)
    eng.set_noise_model(*_model_for(kind))
    eng.set_noise_adapt(rate)
    out = dict(snaps=[], hist=[], stats=[])
    if form == "traj":
        states, actions, U_end = run_stream(eng, x0, U0, n, seed=seed, launches=2)
        out["traj"] = (states, actions, U_end)
        out["hist"] = [None] * n + [eng.noise_law(i) for i in range(n)]
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
                out["hist"] += [eng.noise_law(i) for i in range(n)]
                out["stats"] += [eng.stats(B, step=i) for i in range(n)]
                out["after_launch"] = out.get("after_launch", []) + [eng.noise_model()[:2]]
        else:
            for i in range(2 * n):
                if form == "plain":
                    out["x_before"].append(_snap(torch, tx)[0])
                eng.solve_device(B, tx.data_ptr(), tU.data_ptr(), None, seed=seed, u0_ptr=tu0.data_ptr(), shift=True,
                                 env_step=True, seed_counter=form == "plain", chain=form != "plain")
                out["hist"].append(eng.noise_law(0))
                if form == "plain":
                    out["u0_steps"].append(_snap(torch, tu0)[0])
                if i + 1 in (n, 2 * n):
                    out["snaps"].append(_snap(torch, tx, tU, tu0))
    out["law"] = eng.noise_model()[:2]
    out["ctr"] = eng.get_seed_counter()
    out["init"] = tuple(np.asarray(v, np.float32) for v in _model_for(kind))
    eng.close()
    return out


@pytest.mark.parametrize("kind", ["cartpole", "mlp"])
def test_stream_forms_agree_bitwise_and_each_graph_step_follows_the_rule(M, kind, path, monkeypatch):
    """Plain counter solves, chained solves, one graph launched twice, graph_capture_traj via run_stream, and chained
    solves under MPPI_GEN_OVERLAP=1 (ignored while adapting): bitwise equal x0, U, u0, final law and per-step law
    history, seed counter 2n.  Then, along the graph stream, every step on its own inputs:
    noise_law(i + 1) == adapt_noise_model_f32(noise_law(i), stats(step=i)), the last against the law after the
    launch."""
    import torch
    n, seed, rate = 5, 9, 0.3
    outs = {f: _run_form(M, torch, kind, f, n, seed, rate) for f in ("plain", "chain", "graph", "traj")}
    monkeypatch.setenv("MPPI_GEN_OVERLAP", "1")
    outs["overlap"] = _run_form(M, torch, kind, "chain", n, seed, rate)
    monkeypatch.delenv("MPPI_GEN_OVERLAP")
    want = outs["plain"]
    for form, got in outs.items():
        assert got["ctr"] == 2 * n, form
        _same_law(got["law"], want["law"])
        for a, b in zip(got["hist"], want["hist"]):
            if a is not None:
                _same_law(a, b)
        for sa, sb in zip(got["snaps"], want["snaps"]):
            for a, b in zip(sa, sb):
                np.testing.assert_array_equal(a, b, err_msg=form)
    states, actions, U_end = outs["traj"]["traj"]
    np.testing.assert_array_equal(states, np.stack(want["x_before"]))
    np.testing.assert_array_equal(actions, np.stack(want["u0_steps"]))
    np.testing.assert_array_equal(U_end, want["snaps"][1][1])
    # adaptation took effect, and started from the law that was set
    _same_law(want["hist"][0], want["init"])
    assert not np.array_equal(want["law"][0], want["init"][0]) and want["law"][1] != want["init"][1]
    # per-step consistency along the graph (both launches)
    g = outs["graph"]
    for launch in range(2):
        for i in range(n):
            j = launch * n + i
            nxt = g["hist"][j + 1] if i + 1 < n else g["after_launch"][launch]
            _same_law(nxt, _f32_step(g["hist"][j], g["stats"][j], rate))


# ------------------------------------------------------------------------------------------ 4. host loop vs device

@pytest.mark.parametrize("kind", ["cartpole", "mlp"])
def test_first_step_agrees_with_the_host_adapting_loop_within_the_fp32_bound(M, kind, path):
    """get_stats -> float64 adapt_noise_model -> set_noise_model on one engine, the device adaptation on another, from
    the same state: after the first step sigma within rtol (nu + B + 8) 2^-24 and rho within that figure times
    max(1, sum|m11bar| / sum m2bar) (the count of fp32 roundings in the rule; tests/test_noise_adapt.py)."""
    from mppi_hip.stats import adapt_noise_model
    K, H, B, rate, seed = 130, 7, 2, 0.3, 77
    sig, rho = _model_for(kind)
    host, x0, U0 = _setup(M, kind, K, H, B)
    host.set_noise_model(sig, rho)
    st = host.solve(x0, U0, seed=seed, stats=True).stats
    s64, rho64 = adapt_noise_model(np.asarray(sig, np.float32), rho, st["eps_m2"], st["eps_m11"], rate, *LIMITS)
    host.set_noise_model(s64, rho64)
    dev, _, _ = _setup(M, kind, K, H, B)
    dev.set_noise_model(sig, rho)
    dev.set_noise_adapt(rate)
    dev.solve(x0, U0, seed=seed)
    s, r, _ = dev.noise_model()
    nu = len(sig)
    fig = (nu + B + 8) * 2.0 ** -24
    m2bar, m11bar = st["eps_m2"].astype(np.float64).mean(0), st["eps_m11"].astype(np.float64).mean(0)
    amp = max(1.0, np.abs(m11bar).sum() / m2bar.sum())
    print("sigma rel err", np.max(np.abs(s - s64) / s64), "bound", fig, "rho err", abs(r - rho64), "bound", fig * amp)
    np.testing.assert_allclose(s, s64, rtol=fig, atol=0.0)
    assert abs(r - rho64) <= fig * amp
    hs, hr, _ = host.noise_model()  # (the host loop's law is the float64 one rounded once)
    np.testing.assert_allclose(s, hs, rtol=fig + 2.0 ** -24, atol=0.0)
    host.close()
    dev.close()


# ------------------------------------------------------------------------------------------ 5. clips

def test_clips_land_exactly(M, path):
    K, H, B, seed = 130, 7, 2, 5
    for limits, rate, init, want_s, want_r in (
            ((1e-3, 0.3, 0.95), 0.3, ([0.5], 0.2), 0.3, None),   # sigma_max below the initial sigma
            ((2.0, 10.0, 0.95), 0.3, ([0.5], 0.2), 2.0, None),   # sigma_min above it
            ((1e-3, 10.0, 0.1), 1.0, ([0.5], 0.8), None, 0.1)):  # rho_hat ~ 0.8 > rho_max, rate 1
        eng, x0, U0 = _setup(M, "cartpole", K, H, B, lambda_=1e30)  # uniform weights
        eng.set_noise_model(*init)
        eng.set_noise_adapt(rate, *limits)
        eng.solve(x0, U0, seed=seed)
        s, r, _ = eng.noise_model()
        print(limits, "->", s, r)
        if want_s is not None:
            assert np.array_equal(s, np.full(1, want_s, np.float32))
        if want_r is not None:
            assert np.float32(r) == np.float32(want_r)
        eng.close()


# ------------------------------------------------------------------------------------------ 6. fixed point

def test_law_is_a_fixed_point_under_uniform_weights(M, path):
    """The shape and bars of test_device_law_is_recovered_from_the_moments (tests/test_gpu_stats.py): uniform weights
    over H * K = 64 * 4096 draws per solve, a standard error near 0.002, bars of ten.  rate = 1 replaces the law by
    the moments of the noise just drawn, twice in a row: the second step's noise follows the STORED law."""
    K, H, B = 4096, 64, 2
    eng, x0, U0 = _setup(M, "cartpole", K, H, B, lambda_=1e9)
    eng.set_noise_model([0.5], 0.8)
    eng.set_noise_adapt(1.0)
    drew = (np.asarray([0.5], np.float32), 0.8)
    for step in range(2):
        eng.solve(x0, U0, seed=0x1234 + step)
        s, r, _ = eng.noise_model()
        _same_law(eng.noise_law(0), drew)
        print("step", step, "drew", drew, "->", s, r)
        assert np.all(np.abs(s / drew[0] - 1.0) < 0.02)
        assert abs(r - drew[1]) < 0.02
        drew = (s, r)
    eng.close()


# ------------------------------------------------------------------------------------------ 7. non-finite batch

def test_a_batch_with_a_nonfinite_solve_leaves_the_law(M, path):
    from mppi_hip import _lib as L
    K, H, B = 130, 7, 2
    eng, x0, U0 = _setup(M, "cartpole", K, H, B)
    eng.set_noise_model([0.6], 0.7)
    eng.set_noise_adapt(0.3)
    bad = x0.copy()
    bad[1, :] = np.nan  # every cost of solve 1 is non-finite
    res = eng.solve(bad, U0, seed=3)
    assert res.status == L.MPPI_E_NONFINITE
    st = eng.stats(B)
    assert st["n_finite"].tolist() == [K, 0]
    init = (np.asarray([0.6], np.float32), np.float32(0.7))
    _same_law(eng.noise_model()[:2], init)
    _same_law(eng.noise_law(0), init)  # the history row is recorded all the same
    res = eng.solve(x0, U0, seed=3)  # ... and a finite batch moves it
    assert res.status == 0 and not np.array_equal(eng.noise_model()[0], init[0])
    eng.close()


# ------------------------------------------------------------------------------------------ 8. resume

@pytest.mark.parametrize("kind", ["cartpole", "mlp"])
def test_a_chained_stream_resumes_bit_for_bit_from_U_counter_law_and_x0(M, kind, path):
    """3 + 3 chained steps across a fresh engine == 6 uninterrupted: set_noise_model(saved) computes c on the host, the
    uninterrupted stream's c is the device's."""
    import torch
    K, H, B, seed, rate = 128, 8, 2, 9, 0.3
    dev = torch.device("cuda")

    def start(x0, U0, law, ctr):
        eng, _, _ = _setup(M, kind, K, H, B)
        eng.set_noise_model(*law)
        eng.set_noise_adapt(rate)
        eng.set_stream(torch.cuda.current_stream().cuda_stream)
        tx, tU = torch.from_numpy(x0).to(dev), torch.from_numpy(U0).to(dev)
        tu0 = torch.zeros(B, U0.shape[1], device=dev)
        eng.set_U(U0)
        eng.set_seed_counter(ctr)
        return eng, tx, tU, tu0

    def steps(eng, tx, tU, tu0, n):
        for _ in range(n):
            eng.solve_device(B, tx.data_ptr(), tU.data_ptr(), None, seed=seed, u0_ptr=tu0.data_ptr(), shift=True,
                             env_step=True, chain=True)
        return _snap(torch, tx, tU, tu0)

    _, x0, U0 = _setup(M, kind, K, H, B)
    whole = start(x0, U0, _model_for(kind), 0)
    want = steps(*whole, 6)
    want_law = whole[0].noise_model()[:2]
    first = start(x0, U0, _model_for(kind), 0)
    x3, U3, _ = steps(*first, 3)
    saved_law, saved_ctr = first[0].noise_model()[:2], first[0].get_seed_counter()
    assert saved_ctr == 3
    first[0].close()
    second = start(x3, U3, saved_law, saved_ctr)
    got = steps(*second, 3)
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b)
    _same_law(second[0].noise_model()[:2], want_law)
    assert second[0].get_seed_counter() == 6
    second[0].close()
    whole[0].close()


# ------------------------------------------------------------------------------------------ 9. state rules

def test_set_noise_adapt_destroys_graphs_keeps_the_key_and_rate_zero_keeps_the_law(M):
    import torch
    from mppi_hip import _lib as L
    K, H, B, n, seed = 128, 8, 2, 3, 21
    dev = torch.device("cuda")
    eng, x0, U0 = _setup(M, "cartpole", K, H, B)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    tx, tU = torch.from_numpy(x0).to(dev), torch.from_numpy(U0).to(dev)
    tu0 = torch.zeros(B, 1, device=dev)
    with pytest.raises(M.MPPIError) as ei:  # no adapting solve yet
        eng.noise_law(0)
    assert ei.value.code == L.MPPI_E_STATE
    eng.graph_capture(B, n, tx.data_ptr(), tU.data_ptr(), tu0.data_ptr(), seed=seed)
    eng.graph_launch(sync=True)  # leaves a prefetched noise: the device counter is one ahead
    assert eng.get_seed_counter() == n
    eng.set_noise_adapt(0.5)  # an inactive model becomes (cfg.sigma, 0), active
    assert eng.get_seed_counter() == n
    s, r, active = eng.noise_model()
    assert active is True and r == 0.0 and np.array_equal(s, np.full(1, eng.config.sigma, np.float32))
    with pytest.raises(M.MPPIError) as ei:
        eng.graph_launch(sync=True)
    assert ei.value.code == L.MPPI_E_STATE and "mppi_graph_capture first" in str(ei.value)
    with pytest.raises(M.MPPIError) as ei:  # enabling alone is no adapting solve
        eng.noise_law(0)
    assert ei.value.code == L.MPPI_E_STATE
    eng.graph_capture(B, n, tx.data_ptr(), tU.data_ptr(), tu0.data_ptr(), seed=seed)
    eng.graph_launch(sync=True)
    assert eng.get_seed_counter() == 2 * n
    eng.noise_law(n - 1)
    with pytest.raises(M.MPPIError) as ei:  # beyond the graph
        eng.noise_law(n)
    assert ei.value.code == L.MPPI_E_ARG
    with pytest.raises(M.MPPIError) as ei:
        eng.noise_law(-1)
    assert ei.value.code == L.MPPI_E_ARG
    adapted = eng.noise_model()
    assert not np.array_equal(adapted[0], s)
    # stats_eval leaves the law alone
    eng.stats_eval(np.ones((B, K), np.float32), np.ones((B, 1, H, K), np.float32))
    _same_law(eng.noise_model()[:2], adapted[:2])
    # rate = 0: back to the by-value path, the adapted law kept, graphs destroyed, key kept
    eng.set_noise_adapt(0.0)
    assert eng.noise_adapt()[0] == 0.0 and eng.get_seed_counter() == 2 * n
    _same_law(eng.noise_model()[:2], adapted[:2])
    assert eng.noise_model()[2] is True
    with pytest.raises(M.MPPIError) as ei:
        eng.graph_launch(sync=True)
    assert ei.value.code == L.MPPI_E_STATE
    eng.solve_device(B, tx.data_ptr(), tU.data_ptr(), None, seed=seed, u0_ptr=tu0.data_ptr(), seed_counter=True,
                     asynchronous=False)
    _same_law(eng.noise_model()[:2], adapted[:2])  # a solve no longer moves it
    # set_noise_model during adaptation resets the device law
    eng.set_noise_adapt(0.5)
    eng.solve_device(B, tx.data_ptr(), tU.data_ptr(), None, seed=seed, u0_ptr=tu0.data_ptr(), seed_counter=True,
                     asynchronous=False)
    assert not np.array_equal(eng.noise_model()[0], adapted[0])
    eng.set_noise_model([0.4], 0.3)
    _same_law(eng.noise_model()[:2], (np.asarray([0.4], np.float32), np.float32(0.3)))
    eng.set_noise_model(None, 0.0)  # the default law's values, still active under adaptation
    s, r, active = eng.noise_model()
    assert active is True and r == 0.0 and np.array_equal(s, np.full(1, eng.config.sigma, np.float32))
    eng.close()


def test_bad_arguments_are_refused_and_change_nothing(M):
    from mppi_hip import _lib as L
    eng = M.Engine(M.Config(nx=MLP_NX, nu=MLP_NU, H=4, K=16))
    lib = eng.lib
    nan, inf = float("nan"), float("inf")
    bad = [(-0.1, 1e-3, 10.0, 0.95), (1.5, 1e-3, 10.0, 0.95), (nan, 1e-3, 10.0, 0.95), (0.3, -1.0, 10.0, 0.95),
           (0.3, 2.0, 1.0, 0.95), (0.3, 1e-3, inf, 0.95), (0.3, nan, 10.0, 0.95), (0.3, 1e-3, nan, 0.95),
           (0.3, 1e-3, 10.0, 1.0), (0.3, 1e-3, 10.0, -0.1), (0.3, 1e-3, 10.0, nan), (0.0, 2.0, 1.0, 0.5)]
    for state in ("off", "on"):
        if state == "on":
            eng.set_noise_model([0.1, 0.5, 1.0], 0.5)
            eng.set_noise_adapt(0.25, 0.01, 5.0, 0.9)
        want, want_law = eng.noise_adapt(), eng.noise_model()
        for args in bad:
            assert lib.mppi_set_noise_adapt(eng._h, *(ctypes.c_float(v) for v in args)) == L.MPPI_E_ARG, args
            assert b"mppi_set_noise_adapt" in lib.mppi_last_error()
            assert eng.noise_adapt() == want, args
            got = eng.noise_model()
            assert np.array_equal(got[0], want_law[0]) and got[1:] == want_law[1:], args
    assert eng.noise_adapt() == tuple(float(np.float32(v)) for v in (0.25, 0.01, 5.0, 0.9))
    eng.set_noise_adapt(1.0, 0.0, 0.0, 0.0)  # the edges are allowed
    eng.close()
    wide = M.Engine(M.Config(nx=4, nu=33, H=2, K=16))  # the adapted law is an active model: nu <= 32
    assert lib.mppi_set_noise_adapt(wide._h, *(ctypes.c_float(v) for v in (0.3, 1e-3, 10.0, 0.95))) \
        == L.MPPI_E_UNSUPPORTED
    assert wide.noise_adapt()[0] == 0.0 and wide.noise_model()[2] is False
    assert lib.mppi_set_noise_adapt(wide._h, *(ctypes.c_float(v) for v in (0.0, 1e-3, 10.0, 0.95))) == L.MPPI_OK
    wide.close()
