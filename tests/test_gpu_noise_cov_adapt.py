"""The sampling covariance adapted on the device (mppi_set_noise_cov_adapt): the update kernel against its numpy
restatement (mppi_hip.stats.adapt_noise_cov_f32: Sigma, L and Sinv bit for bit), every stream form against a loop of
plain solves, the control-cost term under the adapted law, and the state rules of the entries.  Modelled on
tests/test_gpu_noise_adapt.py."""
import ctypes
import os

import numpy as np
import pytest

from conftest import PKG, golden, golden_sd
from cov_cases import build_lin_host
from cross_cases import bits, sigma_of

pytestmark = pytest.mark.gpu

MLP_NX, MLP_NU = 10, 3
LIMITS = (1e-3, 10.0)
U32 = 2.0 ** -24


@pytest.fixture(scope="module")
def M(gpu_available):
    import mppi_hip
    return mppi_hip


@pytest.fixture(scope="module")
def lin_host(tmp_path_factory):
    return build_lin_host(tmp_path_factory.mktemp("cov_adapt_lin"), os.path.join(PKG, "csrc"))


def _setup(M, kind, K, H, B, **kw):
    """(engine, x0 [B,nx] f32, U0 [B,nu,H] f32): a seeded MLP (nu = 3, fp32, quad_est), or the CrossAttention humanoid
    net of tests/golden in bf16 (nu = 21: three row blocks of the cross moments' triangle, the last ragged)."""
    rs = np.random.RandomState(11)
    if kind == "ca":
        eng = M.Engine(M.Config.preset("humanoid_v3", K=K, H=H, max_batch=B, **kw))
        eng.load_dynamics(*M.cross_attention_blob(golden_sd("ca_humanoid_weights.npz"))).set_cost("humanoid_v3")
        x0 = golden("g5_ca_humanoid_fwd.npz")["x0_stride20"][:B]
        nu = 21
    else:
        from mppi_hip.nets import mlp_blob, synthetic_mlp
        cfg = dict(nx=MLP_NX, nu=MLP_NU, H=H, K=K, max_batch=B, lambda_=1.0, sigma=0.5, precision=0)
        cfg.update(kw)
        eng = M.Engine(M.Config(**cfg))
        eng.load_dynamics(*mlp_blob(synthetic_mlp(MLP_NX, MLP_NU, seed=0), MLP_NX, MLP_NU))
        eng.set_cost("quad_est")
        x0 = 0.3 * rs.randn(B, MLP_NX)
        nu = MLP_NU
    U0 = 0.1 * rs.randn(B, nu, H)
    return eng, np.ascontiguousarray(x0, np.float32), U0.astype(np.float32)


def _same_bits(a, b, what=""):
    assert np.array_equal(bits(a), bits(b)), what


def _same_law(got, want):
    """(Sigma, L, Sinv) triples, bit for bit"""
    for a, b, name in zip(got, want, ("Sigma", "L", "Sinv")):
        _same_bits(a, b, name)


def _f32_step(S, mx, n_finite, rate, limits=LIMITS):
    """adapt_noise_cov_f32 -> ((Sigma, L, Sinv), sigma_u, status)"""
    from mppi_hip.stats import adapt_noise_cov_f32
    S2, L, Sinv, sig, status = adapt_noise_cov_f32(S, mx, rate, *limits, n_finite=n_finite)
    return (S2, L, Sinv), sig, status


def _snap(torch, *ts):
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in ts)


# ------------------------------------------------------------------------------------------ 1. one step

@pytest.mark.parametrize("kind,H", [("mlp", 7), ("mlp", 1), ("ca", 7)])
def test_one_step_draws_the_by_value_noise_and_moves_the_law_by_the_rule(M, kind, H):
    K, B, rate, seed = 130, 2, 0.3, 0x5151_0000_0007
    ref, x0, U0 = _setup(M, kind, K, H, B)
    S = sigma_of(ref.config.nu)
    ref.set_noise_cov(S)
    r0 = ref.solve(x0, U0, seed=seed, cross=True)
    eng, _, _ = _setup(M, kind, K, H, B)
    eng.set_noise_cov(S)
    before = eng.noise_cov()
    eng.set_noise_cov_adapt(rate)
    assert eng.noise_cov_adapt() == tuple(float(np.float32(v)) for v in (rate,) + LIMITS) + (0,)
    r1 = eng.solve(x0, U0, seed=seed)
    for name in ("costs", "U", "u0"):  # adapting changes no solve: the noise is the setter's law's
        assert np.array_equal(getattr(r1, name), getattr(r0, name)), name
    st, mx = eng.stats(B), eng.cross_moments(B)  # the solve carried the statistics and the cross moments
    _same_bits(mx, r0.stats["eps_mx"])
    for k, v in r0.stats.items():
        if k != "eps_mx":
            assert np.array_equal(st[k], v), k
    _same_bits(eng.noise_cov_law(0), S)
    want, sig, status = _f32_step(S, mx, st["n_finite"], rate)
    assert status == 1
    _same_law(eng.noise_cov(), want)
    assert not np.array_equal(eng.noise_cov()[0], before[0])
    s, rho, active = eng.noise_model()
    assert active is True and rho == 0.0
    _same_bits(s, sig)
    assert eng.noise_cov_adapt()[3] == 0
    ref.close()
    eng.close()


# ------------------------------------------------------------------------------------------ 2, 3. streams

def _run_form(M, torch, kind, form, n, seed, rate):
    """One stream form, two launches of n steps (shift + env step) with adaptation on.  Returns a dict: snaps (x0, U,
    u0 after each launch), hist (the Sigma each of the 2n steps drew from; None where the form cannot be asked per
    step), law (the final Sigma, L, Sinv), per graph step the cross moments and n_finite, ctr, rejects."""
    from mppi_hip.trajectory import run_stream
    K, H, B = 128, 8, 2
    dev = torch.device("cuda")
    eng, x0, U0 = _setup(M, kind, K, H, B)
    nu = eng.config.nu
    eng.set_noise_cov(sigma_of(nu))
    eng.set_noise_cov_adapt(rate)
    out = dict(snaps=[], hist=[], mx=[], nf=[], after_launch=[])
    if form == "traj":
        states, actions, U_end = run_stream(eng, x0, U0, n, seed=seed, launches=2)
        out["traj"] = (states, actions, U_end)
        out["hist"] = [None] * n + [eng.noise_cov_law(i) for i in range(n)]
    else:
        eng.set_stream(torch.cuda.current_stream().cuda_stream)
        tx, tU = torch.from_numpy(x0).to(dev), torch.from_numpy(U0).to(dev)
        tu0 = torch.zeros(B, nu, device=dev)
        out["x_before"], out["u0_steps"] = [], []
        if form == "graph":
            eng.graph_capture(B, n, tx.data_ptr(), tU.data_ptr(), tu0.data_ptr(), seed=seed)
            for _ in range(2):
                eng.graph_launch(sync=True)
                out["snaps"].append(_snap(torch, tx, tU, tu0))
                out["hist"] += [eng.noise_cov_law(i) for i in range(n)]
                out["mx"] += [eng.cross_moments(B, step=i) for i in range(n)]
                out["nf"] += [eng.stats(B, step=i)["n_finite"] for i in range(n)]
                out["after_launch"].append(eng.noise_cov())
        else:
            for i in range(2 * n):
                if form == "plain":
                    out["x_before"].append(_snap(torch, tx)[0])
                eng.solve_device(B, tx.data_ptr(), tU.data_ptr(), None, seed=seed, u0_ptr=tu0.data_ptr(), shift=True,
                                 env_step=True, seed_counter=form == "plain", chain=form != "plain")
                out["hist"].append(eng.noise_cov_law(0))
                if form == "plain":
                    out["u0_steps"].append(_snap(torch, tu0)[0])
                if i + 1 in (n, 2 * n):
                    out["snaps"].append(_snap(torch, tx, tU, tu0))
    out["law"] = eng.noise_cov()
    out["ctr"] = eng.get_seed_counter()
    out["rejects"] = eng.noise_cov_adapt()[3]
    eng.close()
    return out


@pytest.mark.parametrize("kind", ["mlp", "ca"])
def test_stream_forms_agree_bitwise_and_each_graph_step_follows_the_rule(M, kind, monkeypatch):
    """Plain counter solves, chained solves, one graph launched twice, graph_capture_traj via run_stream, and chained
    solves under MPPI_GEN_OVERLAP=1 (ignored while adapting): bitwise equal x0, U, u0, final law (Sigma, L, Sinv) and
    per-step Sigma history, seed counter 2n, no rejected step.  Then, along the graph stream, every step on its own
    inputs: noise_cov_law(i + 1) == adapt_noise_cov_f32(noise_cov_law(i), cross_moments(step=i)) -- the restatement
    says "moved" for every step, which is what keeps the device's count of rejects at 0 -- the last of a launch
    against the law after it, with L and Sinv."""
    import torch
    n, seed, rate = 5, 9, 0.3
    outs = {f: _run_form(M, torch, kind, f, n, seed, rate) for f in ("plain", "chain", "graph", "traj")}
    monkeypatch.setenv("MPPI_GEN_OVERLAP", "1")
    outs["overlap"] = _run_form(M, torch, kind, "chain", n, seed, rate)
    monkeypatch.delenv("MPPI_GEN_OVERLAP")
    want = outs["plain"]
    nu = want["law"][0].shape[0]
    for form, got in outs.items():
        assert got["ctr"] == 2 * n, form
        assert got["rejects"] == 0, form
        _same_law(got["law"], want["law"])
        for a, b in zip(got["hist"], want["hist"]):
            if a is not None:
                _same_bits(a, b, form)
        for sa, sb in zip(got["snaps"], want["snaps"]):
            for a, b in zip(sa, sb):
                np.testing.assert_array_equal(a, b, err_msg=form)
    states, actions, U_end = outs["traj"]["traj"]
    np.testing.assert_array_equal(states, np.stack(want["x_before"]))
    np.testing.assert_array_equal(actions, np.stack(want["u0_steps"]))
    np.testing.assert_array_equal(U_end, want["snaps"][1][1])
    # adaptation took effect, off-diagonals included, and started from the law that was set
    _same_bits(want["hist"][0], sigma_of(nu))
    assert not np.array_equal(want["law"][0], sigma_of(nu))
    assert want["law"][0][1, 0] != sigma_of(nu)[1, 0]
    # per-step consistency along the graph (both launches)
    g = outs["graph"]
    for launch in range(2):
        for i in range(n):
            j = launch * n + i
            step, _, status = _f32_step(g["hist"][j], g["mx"][j], g["nf"][j], rate)
            assert status == 1, j
            if i + 1 < n:
                _same_bits(g["hist"][j + 1], step[0], f"step {j}")
            else:
                _same_law(g["after_launch"][launch], step)


# ------------------------------------------------------------------------------------------ 4. the control-cost term

def test_the_control_cost_term_reads_the_adapted_inverse_from_the_next_solve_on(M, lin_host):
    """With the term on: step i's coefficients are the host header's on the Sinv the law held BEFORE step i's update
    (step 0: the setter's; step 1: step 0's adapted one, which is adapt_noise_cov_f32's), bit for bit, and within
    control_term_ref's bound of the float64 statement with that Sinv."""
    from mppi_hip.stats import control_term_ref
    K, H, B, rate, gamma, seed = 130, 7, 2, 0.5, 0.5, 0xC0DE
    eng, x0, U0 = _setup(M, "mlp", K, H, B)
    nu = eng.config.nu
    eng.set_noise_cov(sigma_of(nu))
    eng.set_control_cost(gamma)
    eng.set_noise_cov_adapt(rate)
    U, law = U0, eng.noise_cov()
    for step in range(3):
        r = eng.solve(x0, U, seed=seed + step)
        term, lin = eng.control_term(B)
        _same_bits(lin, lin_host(law[2], U, gamma, 0.0), f"step {step}")
        _, lin64, A = control_term_ref(U, np.zeros((B, nu, H, 1)), None, 0.0, gamma, Sinv=law[2])
        assert np.all(np.abs(lin.astype(np.float64) - lin64) <= (nu + 8) * U32 * A), step
        want, _, status = _f32_step(law[0], eng.cross_moments(B), eng.stats(B)["n_finite"], rate)
        assert status == 1
        nxt = eng.noise_cov()
        _same_law(nxt, want)
        assert not np.array_equal(nxt[2], law[2])
        # mppi_control_term_eval uses the law in effect: the adapted one
        ev_lin = eng.control_term_eval(r.U, np.zeros((B, nu, H, K), np.float32))[1]
        _same_bits(ev_lin, lin_host(nxt[2], r.U, gamma, 0.0))
        U, law = r.U, nxt
    assert eng.noise_cov_adapt()[3] == 0
    eng.close()


# ------------------------------------------------------------------------------------------ 5. fixed point

def test_law_is_a_fixed_point_under_uniform_weights(M):
    """The shape and bars of test_law_is_a_fixed_point_under_uniform_weights (tests/test_gpu_noise_adapt.py): uniform
    weights over H * K = 64 * 4096 draws per solve, a standard error near 0.002 s_u s_v, bars of ten.  rate = 1
    replaces Sigma by the cross moments of the noise just drawn, twice in a row: the second step's noise follows the
    STORED law (its L, re-factored on the device)."""
    K, H, B = 4096, 64, 2
    eng, x0, U0 = _setup(M, "mlp", K, H, B, lambda_=1e9)
    drew = sigma_of(3)
    eng.set_noise_cov(drew)
    eng.set_noise_cov_adapt(1.0)
    for step in range(2):
        eng.solve(x0, U0, seed=0x1234 + step)
        S = eng.noise_cov()[0]
        _same_bits(eng.noise_cov_law(0), drew)
        s = np.sqrt(np.diag(drew).astype(np.float64))
        dev = np.abs(S.astype(np.float64) - drew) / np.outer(s, s)
        print("step", step, "max |S_new - S_drawn| / (s_u s_v) =", float(dev.max()))
        assert np.all(dev < 0.02)
        assert not np.array_equal(S, drew)
        drew = S
    assert eng.noise_cov_adapt()[3] == 0
    eng.close()


# ------------------------------------------------------------------------------------------ 6. non-finite batch

def test_a_batch_with_a_nonfinite_solve_leaves_the_law(M):
    from mppi_hip import _lib as L
    K, H, B = 130, 7, 2
    eng, x0, U0 = _setup(M, "mlp", K, H, B)
    S = sigma_of(3)
    eng.set_noise_cov(S)
    init = eng.noise_cov()
    eng.set_noise_cov_adapt(0.3)
    bad = x0.copy()
    bad[1, :] = np.nan  # every cost of solve 1 is non-finite
    res = eng.solve(bad, U0, seed=3)
    assert res.status == L.MPPI_E_NONFINITE
    assert eng.stats(B)["n_finite"].tolist() == [K, 0]
    _same_law(eng.noise_cov(), init)
    _same_bits(eng.noise_cov_law(0), S)  # the history row is recorded all the same
    assert eng.noise_cov_adapt()[3] == 0  # ... and nothing was rejected: the step did not run
    res = eng.solve(x0, U0, seed=3)  # a finite batch moves it
    assert res.status == 0 and not np.array_equal(eng.noise_cov()[0], S)
    eng.close()


def test_a_rejected_step_leaves_the_law_and_counts(M):
    """rate = 1 on a solve whose injected noise is all zero: every blended scale is 0, the step is rejected whole."""
    K, H, B = 130, 7, 2
    eng, x0, U0 = _setup(M, "mlp", K, H, B)
    eng.set_noise_cov(sigma_of(3))
    init = eng.noise_cov()
    eng.set_noise_cov_adapt(1.0)
    eng.solve(x0, U0, noise=np.zeros((B, 3, H, K), np.float32))
    _same_law(eng.noise_cov(), init)
    _same_bits(eng.noise_model()[0], np.sqrt(np.diag(init[0]).astype(np.float64)).astype(np.float32))
    assert eng.noise_cov_adapt()[3] == 1
    twin = (0.5 * np.random.RandomState(2).randn(B, 3, H, K)).astype(np.float32)
    eng.solve(x0, U0, noise=twin)  # ... and a solve with real noise moves it; the count stays
    assert not np.array_equal(eng.noise_cov()[0], init[0]) and eng.noise_cov_adapt()[3] == 1
    eng.close()


# ------------------------------------------------------------------------------------------ 7. resume

@pytest.mark.parametrize("kind", ["mlp", "ca"])
def test_a_chained_stream_resumes_bit_for_bit_from_U_counter_sigma_and_x0(M, kind):
    """3 + 3 chained steps across a fresh engine == 6 uninterrupted: set_noise_cov(saved Sigma) factors on the host
    what the uninterrupted stream's device factored -- the same arithmetic, so the same L and Sinv."""
    import torch
    K, H, B, seed, rate = 128, 8, 2, 9, 0.3
    dev = torch.device("cuda")

    def start(x0, U0, S, ctr):
        eng, _, _ = _setup(M, kind, K, H, B)
        eng.set_noise_cov(S)
        eng.set_noise_cov_adapt(rate)
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
    S0 = sigma_of(U0.shape[1])
    whole = start(x0, U0, S0, 0)
    want = steps(*whole, 6)
    want_law = whole[0].noise_cov()
    first = start(x0, U0, S0, 0)
    x3, U3, _ = steps(*first, 3)
    saved, saved_ctr = first[0].noise_cov(), first[0].get_seed_counter()
    assert saved_ctr == 3
    first[0].close()
    second = start(x3, U3, saved[0], saved_ctr)
    _same_law(second[0].noise_cov(), saved)  # the host's factor of the saved Sigma is the device's
    got = steps(*second, 3)
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b)
    _same_law(second[0].noise_cov(), want_law)
    assert second[0].get_seed_counter() == 6
    second[0].close()
    whole[0].close()


# ------------------------------------------------------------------------------------------ 8. state rules

def test_state_rules(M):
    import torch
    from mppi_hip import _lib as L
    K, H, B, n, seed = 128, 8, 2, 3, 21
    dev = torch.device("cuda")
    eng, x0, U0 = _setup(M, "mlp", K, H, B)
    S = sigma_of(3)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    tx, tU = torch.from_numpy(x0).to(dev), torch.from_numpy(U0).to(dev)
    tu0 = torch.zeros(B, 3, device=dev)
    with pytest.raises(M.MPPIError) as ei:  # enabling needs a covariance
        eng.set_noise_cov_adapt(0.5)
    assert ei.value.code == L.MPPI_E_STATE and "mppi_set_noise_cov" in str(ei.value)
    assert eng.noise_cov_adapt() == (0.0, float(np.float32(1e-3)), 10.0, 0)
    eng.set_noise_cov_adapt(0.0, 0.01, 5.0)  # disabling what is off keeps the limits
    assert eng.noise_cov_adapt() == (0.0, float(np.float32(0.01)), 5.0, 0)
    eng.set_noise_cov(S)
    with pytest.raises(M.MPPIError) as ei:  # no adapting solve yet
        eng.noise_cov_law(0)
    assert ei.value.code == L.MPPI_E_STATE
    eng.graph_capture(B, n, tx.data_ptr(), tU.data_ptr(), tu0.data_ptr(), seed=seed)
    eng.graph_launch(sync=True)  # leaves a prefetched noise: the device counter is one ahead
    assert eng.get_seed_counter() == n
    eng.set_noise_cov_adapt(0.5)
    assert eng.get_seed_counter() == n
    with pytest.raises(M.MPPIError) as ei:  # the graphs are gone
        eng.graph_launch(sync=True)
    assert ei.value.code == L.MPPI_E_STATE and "mppi_graph_capture first" in str(ei.value)
    with pytest.raises(M.MPPIError) as ei:  # enabling alone is no adapting solve
        eng.noise_cov_law(0)
    assert ei.value.code == L.MPPI_E_STATE
    eng.graph_capture(B, n, tx.data_ptr(), tU.data_ptr(), tu0.data_ptr(), seed=seed)
    eng.graph_launch(sync=True)
    assert eng.get_seed_counter() == 2 * n
    eng.noise_cov_law(n - 1)
    eng.cross_moments(B, step=n - 1)  # every adapting solve carries MPPI_FLAG_CROSS
    for bad in (n, -1):
        with pytest.raises(M.MPPIError) as ei:
            eng.noise_cov_law(bad)
        assert ei.value.code == L.MPPI_E_ARG
    adapted = eng.noise_cov()
    assert not np.array_equal(adapted[0], S)
    # the evaluations leave the law alone
    eng.cross_moments_eval(np.ones((B, K), np.float32), np.ones((B, 3, H, K), np.float32))
    eng.stats_eval(np.ones((B, K), np.float32), np.ones((B, 3, H, K), np.float32))
    _same_law(eng.noise_cov(), adapted)
    # NULL while on: refused; the knot law and the per-actuator adaptation stay refused as beside any covariance
    with pytest.raises(M.MPPIError) as ei:
        eng.set_noise_cov(None)
    assert ei.value.code == L.MPPI_E_STATE and "mppi_set_noise_cov_adapt" in str(ei.value)
    for call in (lambda: eng.set_noise_knots(4, 1), lambda: eng.set_noise_adapt(0.3)):
        with pytest.raises(M.MPPIError) as ei:
            call()
        assert ei.value.code == L.MPPI_E_UNSUPPORTED
    _same_law(eng.noise_cov(), adapted)
    # rate = 0: the adapted law kept (host copies refreshed), graphs destroyed, key kept
    eng.graph_capture(B, n, tx.data_ptr(), tU.data_ptr(), tu0.data_ptr(), seed=seed)
    eng.set_noise_cov_adapt(0.0)
    assert eng.noise_cov_adapt()[0] == 0.0 and eng.get_seed_counter() == 2 * n
    _same_law(eng.noise_cov(), adapted)
    _same_bits(eng.noise_model()[0], np.sqrt(np.diag(adapted[0]).astype(np.float64)).astype(np.float32))
    with pytest.raises(M.MPPIError) as ei:
        eng.graph_launch(sync=True)
    assert ei.value.code == L.MPPI_E_STATE
    eng.solve_device(B, tx.data_ptr(), tU.data_ptr(), None, seed=seed, u0_ptr=tu0.data_ptr(), seed_counter=True,
                     asynchronous=False)
    _same_law(eng.noise_cov(), adapted)  # a solve no longer moves it
    # set_noise_cov(Sigma) during adaptation resets the device law, even to the value last set
    eng.set_noise_cov(S)
    eng.set_noise_cov_adapt(0.5)
    eng.solve_device(B, tx.data_ptr(), tU.data_ptr(), None, seed=seed, u0_ptr=tu0.data_ptr(), seed_counter=True,
                     asynchronous=False)
    assert not np.array_equal(eng.noise_cov()[0], S)
    eng.set_noise_cov(S)
    from mppi_hip.noise import cov_factor
    _same_bits(eng.noise_cov()[0], S)
    _same_bits(eng.noise_cov()[1], cov_factor(S))
    with pytest.raises(M.MPPIError):  # ... and keeps its checks
        eng.set_noise_cov(np.float32([[1, 2, 0], [2, 1, 0], [0, 0, 1]]))
    _same_bits(eng.noise_cov()[0], S)
    eng.close()


def test_bad_arguments_are_refused_and_change_nothing(M):
    from mppi_hip import _lib as L
    eng = M.Engine(M.Config(nx=MLP_NX, nu=MLP_NU, H=4, K=16))
    lib = eng.lib
    nan, inf = float("nan"), float("inf")
    bad = [(-0.1, 1e-3, 10.0), (1.5, 1e-3, 10.0), (nan, 1e-3, 10.0), (0.3, -1.0, 10.0), (0.3, 0.0, 10.0),
           (0.3, 2.0, 1.0), (0.3, 1e-3, inf), (0.3, nan, 10.0), (0.3, 1e-3, nan), (0.0, 2.0, 1.0), (0.0, 0.0, 1.0)]
    for state in ("off", "on"):
        if state == "on":
            eng.set_noise_cov(sigma_of(MLP_NU))
            eng.set_noise_cov_adapt(0.25, 0.01, 5.0)
        want, want_law = eng.noise_cov_adapt(), eng.noise_cov()
        for args in bad:
            assert lib.mppi_set_noise_cov_adapt(eng._h, *(ctypes.c_float(v) for v in args)) == L.MPPI_E_ARG, args
            assert b"mppi_set_noise_cov_adapt" in lib.mppi_last_error()
            assert eng.noise_cov_adapt() == want, args
            got = eng.noise_cov()
            assert (got is None and want_law is None) or np.array_equal(got[0], want_law[0]), args
    assert eng.noise_cov_adapt() == tuple(float(np.float32(v)) for v in (0.25, 0.01, 5.0)) + (0,)
    eng.set_noise_cov_adapt(1.0, 0.5, 0.5)  # the edges are allowed
    buf = np.zeros((MLP_NU, MLP_NU), np.float32)
    assert lib.mppi_get_noise_cov_law(eng._h, 0, None) == L.MPPI_E_ARG
    assert lib.mppi_get_noise_cov_law(eng._h, 0, buf.ctypes.data_as(ctypes.c_void_p)) == L.MPPI_E_STATE
    assert lib.mppi_get_noise_cov_adapt(eng._h, None, None, None, None) == L.MPPI_OK  # every pointer may be NULL
    eng.close()
    wide = M.Engine(M.Config(nx=4, nu=33, H=2, K=16))  # the adapted covariance is an active model: nu <= 32
    assert lib.mppi_set_noise_cov_adapt(wide._h, *(ctypes.c_float(v) for v in (0.3, 1e-3, 10.0))) \
        == L.MPPI_E_UNSUPPORTED
    assert wide.noise_cov_adapt()[0] == 0.0 and wide.noise_cov() is None
    assert lib.mppi_set_noise_cov_adapt(wide._h, *(ctypes.c_float(v) for v in (0.0, 1e-3, 10.0))) == L.MPPI_OK
    wide.close()
