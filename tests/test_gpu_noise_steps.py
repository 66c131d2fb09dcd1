"""The per-step sampling scale on the device (mppi_set_noise_steps, MPPI_FLAG_STEP_MOMENTS, mppi_set_noise_steps_adapt):
the table generators against noise.steps_filter and the AR(1) model, the moment pass against its numpy float32
restatement (stats.step_moments_f32) and the float64 definition, the refit kernel against stats.adapt_noise_steps_f32,
every stream form against a loop of plain solves, and the state rules of the entries."""
import ctypes
import os

import numpy as np
import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu

MLP_NX, MLP_NU = 10, 3
SIG, LIMITS = [0.2, 0.5, 0.8], (0.01, 3.0)


@pytest.fixture(scope="module")
def M(gpu_available):
    import mppi_hip
    return mppi_hip


def _setup(M, kind, K, H, B, **kw):
    """(engine, x0 [B,nx] f32, U0 [B,nu,H] f32): a seeded MLP (nx = 10, nu = 3, fp32, quad_est), or the golden
    CrossAttention humanoid (nu = 21, bf16)."""
    rs = np.random.RandomState(11)
    if kind == "ca":
        sd = M.load_npz(os.path.join(REPO, "tests", "golden", "ca_humanoid_weights.npz"))
        eng = M.Engine(M.Config.preset("humanoid_v3", K=K, H=H, precision=1, max_batch=B, **kw))
        eng.load_dynamics(*M.cross_attention_blob(sd)).set_cost("humanoid_v3")
        x0 = np.load(os.path.join(REPO, "tests", "golden", "g5_ca_humanoid_fwd.npz"))["x0_stride20"][:B]
        nu = 21
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
    return eng, np.ascontiguousarray(x0, np.float32), U0.astype(np.float32)


@pytest.fixture(params=["direct", "lds"])
def path(request, monkeypatch):
    """Both AR(1) generators (MPPI_NOISE_AR1, read per launch), in their table forms."""
    monkeypatch.setenv("MPPI_NOISE_AR1", request.param)
    return request.param


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def _same(a, b, msg=""):
    assert np.array_equal(_bits(a), _bits(b)), msg


def _table(B, nu, H, seed=3):
    return (0.1 + 0.9 * np.random.RandomState(seed).rand(B, nu, H)).astype(np.float32)


def _snap(torch, *ts):
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in ts)


def _device_weights(eng, costs):
    """The normalised weights the statistics' cost pass holds for these costs, bit for bit: the moment pass itself over
    one-hot noise rows -- row j is 1 at sample j -- gives m1[row j] = fmaf(w_j, 1, 0) + zeros = w_j exactly."""
    c = eng.config
    B, K, rows = costs.shape[0], c.K, c.nu * c.H
    w = np.zeros((B, K), np.float32)
    for k0 in range(0, K, rows):
        hot = np.zeros((rows, K), np.float32)
        n = min(rows, K - k0)
        hot[np.arange(n), k0 + np.arange(n)] = 1.0
        m1, _ = eng.step_moments_eval(costs, np.broadcast_to(hot.reshape(c.nu, c.H, K), (B, c.nu, c.H, K)))
        w[:, k0:k0 + n] = m1.reshape(B, rows)[:, :n]
    return w


# ------------------------------------------------------------------------------------------ 4. the law

@pytest.mark.parametrize("rho", [0.0, 0.9])
@pytest.mark.parametrize("H", [1, 7, 19])
def test_noise_under_a_table_is_the_table_times_the_unit_rows_bit_for_bit(M, H, rho, path):
    """K = 130 (Kp = 192: the pads are written like every lane), B = 2 with two different rows of the table."""
    from mppi_hip.noise import steps_filter
    K, B, seed = 130, 2, 0x5151_0000_0007
    eng, x0, U0 = _setup(M, "mlp", K, H, B)
    eng.set_noise_model(np.ones(MLP_NU), rho)
    unit = eng.noise_eval(B, seed)
    table = _table(B, MLP_NU, H)
    assert not np.array_equal(table[0], table[1])
    eng.set_noise_model(SIG, rho)  # the fill: not multiplied in while the table is on
    eng.set_noise_steps(table)
    _same(eng.noise_steps(B), table)
    _same(eng.noise_eval(B, seed), steps_filter(unit, table, 0.0))
    # a table of sigma_u broadcast reproduces the AR(1) model's noise and solve
    ref, _, _ = _setup(M, "mlp", K, H, B)
    ref.set_noise_model(SIG, rho)
    want_noise = ref.noise_eval(B, seed)
    r0 = ref.solve(x0, U0, seed=seed)
    eng.set_noise_steps(np.broadcast_to(np.asarray(SIG, np.float32)[:, None], (MLP_NU, H)))
    _same(eng.noise_eval(B, seed), want_noise)
    r1 = eng.solve(x0, U0, seed=seed)
    for name in ("costs", "U", "u0"):
        _same(getattr(r1, name), getattr(r0, name), name)
    # off: the AR(1) model again, sigma_u and rho as they stand
    eng.set_noise_steps(None)
    assert eng.noise_steps(B) is None
    s, r, active = eng.noise_model()
    assert active and np.array_equal(s, np.asarray(SIG, np.float32)) and np.float32(r) == np.float32(rho)
    _same(eng.noise_eval(B, seed), want_noise)
    ref.close()
    eng.close()


# ------------------------------------------------------------------------------------------ 5. the moments

SHAPES = [("mlp", 130, 1), ("mlp", 130, 7), ("mlp", 130, 19), ("mlp", 300, 1), ("mlp", 300, 7), ("mlp", 300, 19),
          ("ca", 130, 7)]


@pytest.mark.parametrize("kind,K,H", SHAPES)
def test_moments_change_no_solve_and_equal_the_cell_scheme_bit_for_bit(M, kind, K, H):
    """K = 130: one partial wave-chunk; K = 300 (Kp = 320): two, the second partial.  One kernel form."""
    from mppi_hip.stats import step_moments_f32, step_moments_ref
    B, seed = 2, 0x77_0000_0003
    ref, x0, U0 = _setup(M, kind, K, H, B)
    r0 = ref.solve(x0, U0, seed=seed, stats=True, want_weights=True)
    eng, _, _ = _setup(M, kind, K, H, B)
    r1 = eng.solve(x0, U0, seed=seed, step_moments=True, want_weights=True)
    for name in ("costs", "U", "u0", "weights"):
        _same(getattr(r1, name), getattr(r0, name), name)
    for k, v in r0.stats.items():
        assert np.array_equal(r1.stats[k], v), k
    assert eng.get_seed_counter() == ref.get_seed_counter()
    m1, m2 = eng.step_moments(B)
    _same(m1, r1.stats["step_m1"])
    _same(m2, r1.stats["step_m2"])
    noise = eng.noise_eval(B, seed)  # the solve's noise: the same key under the same law
    e1, e2 = eng.step_moments_eval(r1.costs, noise)
    _same(m1, e1, "eval m1")
    _same(m2, e2, "eval m2")
    w = _device_weights(eng, r1.costs)
    assert np.all(np.abs(w.sum(axis=1) - 1.0) < 1e-5)
    f1, f2 = step_moments_f32(w, noise)
    _same(m1, f1, "f32 m1")
    _same(m2, f2, "f32 m2")
    # ... and within the fp32 summation bound of the float64 sums over the same weights
    d1, d2 = step_moments_ref(None, noise, w=w)
    bound = K * 2.0 ** -24
    err2 = float(np.max(np.abs(m2 - d2) / d2))
    err1 = float(np.max(np.abs(m1 - d1) / np.sqrt(d2)))
    print(f"{kind} K={K} H={H}: m1 err {err1:.3e}, m2 rel err {err2:.3e}, bound {bound:.3e}")
    assert err1 <= bound and err2 <= bound
    m1b, m2b = eng.step_moments(B)  # the evaluations left the solve's moments readable
    _same(m1, m1b)
    _same(m2, m2b)
    ref.close()
    eng.close()


@pytest.mark.parametrize("kind,K,H", [("mlp", 130, 7), ("mlp", 300, 19), ("ca", 130, 7)])
def test_under_elites_the_moments_are_the_elite_mean_and_second_moment(M, kind, K, H):
    from mppi_hip.stats import elite_select_ref
    B, seed, n = 2, 0x77_0000_0005, K // 8
    eng, x0, U0 = _setup(M, kind, K, H, B, lambda_=1e6)
    eng.set_elites(n)
    r = eng.solve(x0, U0, seed=seed, step_moments=True)
    noise = eng.noise_eval(B, seed).astype(np.float64)
    idx, count, _, _ = elite_select_ref(r.costs, n)
    m1, m2 = eng.step_moments(B)
    bound = K * 2.0 ** -24
    for b in range(B):
        el = noise[b][:, :, idx[b, :count[b]]]
        mean, sq = el.mean(axis=-1), (el * el).mean(axis=-1)
        err2 = float(np.max(np.abs(m2[b] - sq) / sq))
        err1 = float(np.max(np.abs(m1[b] - mean) / np.sqrt(sq)))
        print(f"{kind} K={K} H={H} b={b}: elites {count[b]}, m1 err {err1:.3e}, m2 rel err {err2:.3e}, "
              f"bound {bound:.3e}")
        assert err1 <= bound and err2 <= bound
    eng.close()


# ------------------------------------------------------------------------------------------ 6. one refit step

@pytest.mark.parametrize("centred", [True, False])
@pytest.mark.parametrize("shift", [False, True])
@pytest.mark.parametrize("H", [1, 7])
def test_one_solve_refits_every_solves_rows_from_its_own_moments(M, H, shift, centred, path):
    from mppi_hip.stats import adapt_noise_steps_f32
    K, B, rate, seed = 130, 2, 0.3, 0x5151_0000_0009
    eng, x0, U0 = _setup(M, "mlp", K, H, 3)  # max_batch = 3 solved at B = 2: slot 2 stays
    table = _table(3, MLP_NU, H)
    eng.set_noise_model(SIG, 0.5)
    eng.set_noise_steps(table)
    eng.set_noise_steps_adapt(rate, *LIMITS, centred=centred)
    assert eng.noise_steps_adapt() == (float(np.float32(rate)), float(np.float32(LIMITS[0])),
                                       float(np.float32(LIMITS[1])), centred)
    ref, _, _ = _setup(M, "mlp", K, H, 3)
    ref.set_noise_model(SIG, 0.5)
    ref.set_noise_steps(table)
    r0 = ref.solve(x0[:B], U0[:B], seed=seed, shift=shift, stats=True)
    r1 = eng.solve(x0[:B], U0[:B], seed=seed, shift=shift)
    for name in ("costs", "U", "u0"):  # refitting changes no solve
        _same(getattr(r1, name), getattr(r0, name), name)
    st = eng.stats(B)
    m1, m2 = eng.step_moments(B)
    live = eng.noise_steps(3)
    want = adapt_noise_steps_f32(table[:B], m1, m2, rate, *LIMITS, centred=centred, shift=shift, fill=SIG,
                                 n_finite=st["n_finite"])
    _same(live[:B], want)
    _same(live[2], table[2], "slot 2")
    if H > 1:
        assert not np.array_equal(live[:B], table[:B])
        assert not np.array_equal(m1[0], m1[1]) and not np.array_equal(live[0], live[1])  # each its own moments
    # solve 1 with NaN states: its rows are only shifted, solve 0's are refit
    from mppi_hip import _lib as L
    eng.set_noise_steps(table)
    bad = x0[:B].copy()
    bad[1, :] = np.nan
    res = eng.solve(bad, U0[:B], seed=seed, shift=shift)
    assert res.status == L.MPPI_E_NONFINITE
    st = eng.stats(B)
    assert st["n_finite"].tolist() == [K, 0]
    m1, m2 = eng.step_moments(B)
    live = eng.noise_steps(B)
    _same(live, adapt_noise_steps_f32(table[:B], m1, m2, rate, *LIMITS, centred=centred, shift=shift, fill=SIG,
                                      n_finite=st["n_finite"]))
    only_shifted = np.concatenate([table[1][:, 1:], np.asarray(SIG, np.float32)[:, None]], axis=1) if shift else table[1]
    _same(live[1], only_shifted, "dead solve")
    ref.close()
    eng.close()


# ------------------------------------------------------------------------------------------ 7. stream forms

def _start(M, torch, extras, table, U0, ctr, K=128, H=8, B=2):
    eng, x0, _ = _setup(M, "mlp", K, H, B)
    eng.set_noise_model(SIG, 0.6)
    eng.set_noise_steps(table)
    if extras:
        eng.set_elites(K // 4)
        eng.set_elite_keep(4)
        eng.set_control_bounds(-0.4, 0.4)
        eng.set_rate_cost(0.05)
        eng.set_ess_target(0.5)
    eng.set_noise_steps_adapt(0.3, *LIMITS)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    eng.set_U(U0)
    eng.set_seed_counter(ctr)
    return eng


def _run_form(M, torch, form, n, seed, extras=False, resume=None):
    """One stream form, two launches of n steps (shift + env step) with the refit on.  resume = (x, U, table, ctr): one
    launch from that state instead.  Returns snaps (x0, U, u0 after each launch), the final table, the seed counter, the
    last step's moments and the state after launch 1."""
    K, H, B = 128, 8, 2
    dev = torch.device("cuda")
    _, x0, U0 = _setup(M, "mlp", K, H, B)
    table, ctr, launches = _table(B, MLP_NU, H), 0, 2
    if resume is not None:
        x0, U0, table, ctr = resume
        launches = 1
    eng = _start(M, torch, extras, table, U0, ctr)
    out = dict(snaps=[])
    if form == "traj":
        from mppi_hip.trajectory import run_stream
        assert resume is None
        states, actions, U_end = run_stream(eng, x0, U0, n, seed=seed, launches=2)
        out["traj"] = (states, actions, U_end)
    else:
        tx, tU = torch.from_numpy(x0.copy()).to(dev), torch.from_numpy(U0.copy()).to(dev)
        tu0 = torch.zeros(B, MLP_NU, device=dev)
        out["x_before"], out["u0_steps"] = [], []
        if form == "graph":
            eng.graph_capture(B, n, tx.data_ptr(), tU.data_ptr(), tu0.data_ptr(), seed=seed)
        for launch in range(launches):
            if form == "graph":
                eng.graph_launch(sync=True)
                out["moments"] = eng.step_moments(B, step=n - 1)
            else:
                for i in range(n):
                    if form == "plain":
                        out["x_before"].append(_snap(torch, tx)[0])
                    eng.solve_device(B, tx.data_ptr(), tU.data_ptr(), None, seed=seed, u0_ptr=tu0.data_ptr(),
                                     shift=True, env_step=True, seed_counter=form == "plain", chain=form != "plain")
                    if form == "plain":
                        out["u0_steps"].append(_snap(torch, tu0)[0])
                out["moments"] = eng.step_moments(B)
            out["snaps"].append(_snap(torch, tx, tU, tu0))
            if launch == 0:
                out["saved"] = (out["snaps"][0][0], out["snaps"][0][1], eng.noise_steps(B), eng.get_seed_counter())
    if form == "traj":
        out["moments"] = eng.step_moments(B, step=n - 1)
    out["table"] = eng.noise_steps(B)
    out["ctr"] = eng.get_seed_counter()
    eng.close()
    return out


def test_stream_forms_agree_bitwise_and_a_stream_resumes_from_table_U_and_counter(M, path, monkeypatch):
    import torch
    n, seed = 3, 9
    outs = {f: _run_form(M, torch, f, n, seed) for f in ("plain", "chain", "graph", "traj")}
    monkeypatch.setenv("MPPI_GEN_OVERLAP", "1")  # ignored while the refit is on
    outs["overlap"] = _run_form(M, torch, "chain", n, seed)
    monkeypatch.delenv("MPPI_GEN_OVERLAP")
    want = outs["plain"]
    for form, got in outs.items():
        assert got["ctr"] == 2 * n, form
        _same(got["table"], want["table"], form)
        for a, b in zip(got["moments"], want["moments"]):
            _same(a, b, form)
        for sa, sb in zip(got["snaps"], want["snaps"]):
            for a, b in zip(sa, sb):
                np.testing.assert_array_equal(a, b, err_msg=form)
    states, actions, U_end = outs["traj"]["traj"]
    np.testing.assert_array_equal(states, np.stack(want["x_before"]))
    np.testing.assert_array_equal(actions, np.stack(want["u0_steps"]))
    np.testing.assert_array_equal(U_end, want["snaps"][1][1])
    assert not np.array_equal(want["table"], _table(2, MLP_NU, 8))  # the refit took effect
    # a fresh handle restored from (table, U, seed counter) after launch 1 reproduces launch 2
    saved = want["saved"]
    assert saved[3] == n
    for form in ("plain", "chain", "graph"):
        got = _run_form(M, torch, form, n, seed, resume=saved)
        assert got["ctr"] == 2 * n
        _same(got["table"], want["table"], "resumed " + form)
        for a, b in zip(got["snaps"][0], want["snaps"][1]):
            np.testing.assert_array_equal(a, b, err_msg="resumed " + form)


def test_chain_graph_and_loop_agree_with_every_option_on(M):
    """Elites, kept elites, bounds, the rate term and the ESS target beside the refit."""
    import torch
    n, seed = 3, 9
    outs = {f: _run_form(M, torch, f, n, seed, extras=True) for f in ("plain", "chain", "graph")}
    want = outs["plain"]
    for form, got in outs.items():
        assert got["ctr"] == 2 * n, form
        _same(got["table"], want["table"], form)
        for a, b in zip(got["moments"], want["moments"]):
            _same(a, b, form)
        for sa, sb in zip(got["snaps"], want["snaps"]):
            for a, b in zip(sa, sb):
                np.testing.assert_array_equal(a, b, err_msg=form)
    plain = _run_form(M, torch, "plain", n, seed)
    assert not np.array_equal(plain["table"], want["table"])  # the options took effect


# ------------------------------------------------------------------------------------------ 8. state rules

def _state(eng):
    """Everything the refused setters could have touched."""
    s, r, active = eng.noise_model()
    steps = eng.noise_steps(1)
    cov = eng.noise_cov()
    return (s.tolist(), r, active, None if steps is None else steps.tolist(), eng.noise_knots()[:2],
            None if eng.noise_basis() is None else eng.noise_basis().tolist(), None if cov is None else cov[0].tolist(),
            eng.noise_adapt()[0], eng.control_cost(), eng.noise_steps_adapt())


def test_refused_pairs_in_both_orders_leave_the_state_intact_and_name_both_setters(M):
    from mppi_hip import _lib as L
    H = 6
    table = _table(1, MLP_NU, H)
    Sigma = np.diag(np.asarray([0.04, 0.25, 0.64], np.float32))
    others = {
        "mppi_set_noise_knots": lambda e: e.set_noise_knots(3, 1),
        "mppi_set_noise_basis": lambda e: e.set_noise_basis(np.eye(H, dtype=np.float32)),
        "mppi_set_noise_cov": lambda e: e.set_noise_cov(Sigma),
        "mppi_set_noise_adapt": lambda e: e.set_noise_adapt(0.3),
        "mppi_set_control_cost": lambda e: e.set_control_cost(0.5),
    }
    for name, enable in others.items():
        for first in ("table", "other"):
            eng = M.Engine(M.Config(nx=MLP_NX, nu=MLP_NU, H=H, K=16))
            (eng.set_noise_steps(table) if first == "table" else enable(eng))
            before = _state(eng)
            with pytest.raises(M.MPPIError) as ei:
                (enable(eng) if first == "table" else eng.set_noise_steps(table))
            assert ei.value.code == L.MPPI_E_UNSUPPORTED, (name, first)
            assert "mppi_set_noise_steps" in str(ei.value) and name in str(ei.value), str(ei.value)
            assert _state(eng) == before, (name, first)
            eng.close()
    # the covariance's adaptation goes with the covariance
    eng = M.Engine(M.Config(nx=MLP_NX, nu=MLP_NU, H=H, K=16))
    eng.set_noise_cov(Sigma)
    eng.set_noise_cov_adapt(0.3)
    with pytest.raises(M.MPPIError) as ei:
        eng.set_noise_steps(table)
    assert ei.value.code == L.MPPI_E_UNSUPPORTED and "mppi_set_noise_cov_adapt" in str(ei.value)
    eng.close()


def test_state_and_argument_errors_change_nothing(M):
    from mppi_hip import _lib as L
    H, B = 6, 2
    eng = M.Engine(M.Config(nx=MLP_NX, nu=MLP_NU, H=H, K=16, max_batch=B))
    lib = eng.lib
    table = _table(B, MLP_NU, H)
    nan, inf = float("nan"), float("inf")

    def set_steps(Bn, arr):
        a = None if arr is None else np.ascontiguousarray(arr, np.float32)
        return lib.mppi_set_noise_steps(eng._h, Bn, None if a is None else a.ctypes.data_as(ctypes.c_void_p))

    def set_adapt(*v):
        return lib.mppi_set_noise_steps_adapt(eng._h, ctypes.c_float(v[0]), ctypes.c_float(v[1]), ctypes.c_float(v[2]),
                                              int(v[3]))

    # the refit before the table
    assert set_adapt(0.3, 1e-3, 10.0, 1) == L.MPPI_E_STATE and b"mppi_set_noise_steps first" in lib.mppi_last_error()
    assert set_adapt(0.0, 1e-3, 10.0, 1) == L.MPPI_OK  # nothing to disable
    assert set_steps(0, None) == L.MPPI_OK  # nothing to disable
    bad_tables = []
    for v in (nan, inf, -inf, -0.5):
        t = table.copy()
        t[1, 2, 3] = v
        bad_tables.append((B, t))
    bad_tables += [(0, table), (B + 1, np.concatenate([table, table[:1]])), (-1, table)]
    bad_adapt = [(-0.1, 1e-3, 10.0, 1), (1.5, 1e-3, 10.0, 1), (nan, 1e-3, 10.0, 1), (0.3, 0.0, 10.0, 1),
                 (0.3, -1.0, 10.0, 1), (0.3, 2.0, 1.0, 1), (0.3, 1e-3, inf, 1), (0.3, nan, 10.0, 1), (0.3, 1e-3, nan, 1),
                 (0.3, 1e-3, 10.0, 2), (0.3, 1e-3, 10.0, -1)]
    for state in ("off", "on"):
        if state == "on":
            eng.set_noise_model(SIG, 0.5)
            eng.set_noise_steps(table)
            eng.set_noise_steps_adapt(0.25, 0.02, 5.0, centred=False)
        before = _state(eng)
        for Bn, t in bad_tables:
            assert set_steps(Bn, t) == L.MPPI_E_ARG, (state, Bn)
            assert b"mppi_set_noise_steps" in lib.mppi_last_error()
            assert _state(eng) == before
        for args in bad_adapt:
            assert set_adapt(*args) == L.MPPI_E_ARG, (state, args)
            assert b"mppi_set_noise_steps_adapt" in lib.mppi_last_error()
            assert _state(eng) == before
    assert eng.noise_steps_adapt() == (float(np.float32(0.25)), float(np.float32(0.02)), 5.0, False)
    # while on: the default path is refused, sigma_u and rho stay settable (the fill and rho), the table stays
    with pytest.raises(M.MPPIError) as ei:
        eng.set_noise_model(None, 0.0)
    assert ei.value.code == L.MPPI_E_STATE and "mppi_set_noise_steps" in str(ei.value)
    eng.set_noise_model([0.3, 0.3, 0.3], 0.2)
    _same(eng.noise_steps(B), table)
    with pytest.raises(M.MPPIError) as ei:  # the table goes only once the refit is off
        eng.set_noise_steps(None)
    assert ei.value.code == L.MPPI_E_STATE
    eng.set_noise_steps_adapt(0.0)
    assert eng.noise_steps_adapt()[0] == 0.0
    _same(eng.noise_steps(B), table)  # rate 0 keeps the table
    eng.set_noise_steps(table[0])  # [nu, H] broadcasts; B = 1 fills every slot
    _same(eng.noise_steps(B), np.stack([table[0], table[0]]))
    with pytest.raises(M.MPPIError) as ei:  # no flagged solve yet
        eng.step_moments(1)
    assert ei.value.code == L.MPPI_E_STATE
    eng.close()
    wide = M.Engine(M.Config(nx=4, nu=33, H=2, K=16))
    t = np.ones((1, 33, 2), np.float32)
    assert wide.lib.mppi_set_noise_steps(wide._h, 1, t.ctypes.data_as(ctypes.c_void_p)) == L.MPPI_E_UNSUPPORTED
    assert wide.noise_steps(1) is None and wide.noise_model()[2] is False
    wide.close()


def test_a_change_destroys_graphs_keeps_the_key_and_the_table_in_effect_keeps_them(M):
    import torch
    from mppi_hip import _lib as L
    K, H, B, n, seed = 128, 8, 2, 3, 21
    dev = torch.device("cuda")
    eng, x0, U0 = _setup(M, "mlp", K, H, B)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    tx, tU = torch.from_numpy(x0).to(dev), torch.from_numpy(U0).to(dev)
    tu0 = torch.zeros(B, MLP_NU, device=dev)
    table = _table(B, MLP_NU, H)

    def capture():
        eng.graph_capture(B, n, tx.data_ptr(), tU.data_ptr(), tu0.data_ptr(), seed=seed)

    def stale():
        with pytest.raises(M.MPPIError) as ei:
            eng.graph_launch(sync=True)
        assert ei.value.code == L.MPPI_E_STATE and "mppi_graph_capture first" in str(ei.value)

    capture()
    eng.graph_launch(sync=True)  # leaves a prefetched noise: the device counter is one ahead
    assert eng.get_seed_counter() == n
    eng.set_noise_steps(table)  # enabling
    assert eng.get_seed_counter() == n and eng.noise_model()[2] is True
    stale()
    capture()
    eng.graph_launch(sync=True)
    eng.set_noise_steps(table)  # the table in effect, bitwise: the graph and the prefetch stay
    eng.graph_launch(sync=True)
    assert eng.get_seed_counter() == 3 * n
    t2 = table.copy()
    t2[0, 0, 0] = np.nextafter(t2[0, 0, 0], np.float32(2.0))
    eng.set_noise_steps(t2)  # one bit
    assert eng.get_seed_counter() == 3 * n
    stale()
    capture()
    eng.set_noise_steps_adapt(0.3)  # enabling the refit
    stale()
    capture()
    eng.graph_launch(sync=True)
    eng.step_moments(B, step=n - 1)
    with pytest.raises(M.MPPIError) as ei:
        eng.step_moments(B, step=n)
    assert ei.value.code == L.MPPI_E_ARG
    moved = eng.noise_steps(B)
    assert not np.array_equal(moved, t2)
    eng.step_moments_eval(np.ones((B, K), np.float32), np.ones((B, MLP_NU, H, K), np.float32))  # never refits
    _same(eng.noise_steps(B), moved)
    eng.set_noise_steps_adapt(0.5)  # changing the settings
    stale()
    capture()
    eng.set_noise_steps_adapt(0.0)  # disabling: the table as it stands
    stale()
    _same(eng.noise_steps(B), moved)
    assert eng.get_seed_counter() == 4 * n
    eng.close()
