"""The control-cost term on the device (mppi_set_control_cost): the two kernels against float64 at bounds derived from
the number format, a solve whose softmin weighs costs + term, the term under ESS targeting, every stream form against
a loop of plain solves, and the state rules of the four entries.

Tolerances, with u = 2^-24 and n = nu H (derived, not tuned):
  |lin_gpu - lin_f64| <= 8 u A, A the absolute-value majorant of lin (mppi_hip.stats.control_term_ref returns it): the
      roundings csrc/control_cost.h counts.
  |term_gpu - sum(lin_gpu eps)_f64| <= n u / (1 - n u) * sum |lin_gpu| |eps|: the worst case of an fp32 sum of n
      fma'd products in any order (the kernel's chain of at most 16 + n / 16 roundings per k is one such order)."""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MLP_NX, MLP_NU = 10, 3
U32 = 2.0 ** -24
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


def _snap(torch, *ts):
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in ts)


def _env(**kv):
    """Context manager: environment knobs set for the calls inside (they are read per launch)."""
    class _E:
        def __enter__(self):
            self.old = {k: os.environ.get(k) for k in kv}
            os.environ.update(kv)

        def __exit__(self, *a):
            for k, v in self.old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
    return _E()


def _check_kernels(lin, term, U, nz, sigma_u, rho, gamma, msg):
    """Both derived bounds; returns the worst ratios (error / bound)."""
    from mppi_hip.stats import control_term_ref
    _, lin64, A = control_term_ref(U, nz, np.asarray(sigma_u, np.float32).astype(np.float64), float(np.float32(rho)),
                                   float(np.float32(gamma)))
    e_lin = np.abs(lin.astype(np.float64) - lin64)
    assert np.all(e_lin <= 8 * U32 * A), (msg, "lin", float((e_lin / np.maximum(A, 1e-300)).max() / U32))
    n = lin.shape[1] * lin.shape[2]
    l64, e64 = lin.astype(np.float64), nz.astype(np.float64)
    want = np.einsum("buh,buhk->bk", l64, e64)
    maj = np.einsum("buh,buhk->bk", np.abs(l64), np.abs(e64))
    e_term = np.abs(term.astype(np.float64) - want)
    bound = n * U32 / (1 - n * U32) * maj
    assert np.all(e_term <= bound), (msg, "term", float((e_term / np.maximum(bound, 1e-300)).max()))
    r_lin = float((e_lin[A > 0] / (8 * U32 * A[A > 0])).max()) if np.any(A > 0) else 0.0
    r_term = float((e_term[maj > 0] / bound[maj > 0]).max()) if np.any(maj > 0) else 0.0
    return r_lin, r_term


# ------------------------------------------------------------------------------------------ 1. the kernels

@pytest.mark.parametrize("K", [30, 75, 1100])
def test_control_term_eval_meets_the_derived_bounds(M, K):
    """No rollout: control_term_eval at B = 3 on K below a chunk / ragged / five 256-k chunks with a ragged last one,
    H in {1, 2, 17}, nu in {1, 3, 32}, rho in {0, 0.6}, per-actuator sigma with one entry 0 (nu = 1: once non-zero,
    once frozen).  Both bounds of the module docstring, a frozen actuator's lin exactly 0, two calls bitwise equal,
    MPPI_CTRL_COST_FORM=block and =split bitwise equal, the nontemporal knob bitwise equal to its default.
    Worst error / bound printed on an MI355X, K = 30 / 75 / 1100: lin 0.47 each (3.8 u A of the 8 allowed); term 0.91,
    0.91, 0.97 (the bound is tightest at nu = H = 1, where the sum is one product and the bound one rounding)."""
    B, gamma = 3, 0.7
    worst = [0.0, 0.0]
    for H in (1, 2, 17):
        for nu in (1, 3, 32):
            rs = np.random.RandomState(1000 * H + nu)
            eng = M.Engine(M.Config(nx=4, nu=nu, H=H, K=K, max_batch=B))
            eng.set_control_cost(gamma)
            U = rs.randn(B, nu, H).astype(np.float32)
            sigmas = [0.3 + rs.rand(nu).astype(np.float32)]
            if nu == 1:
                sigmas.append(np.zeros(1, np.float32))
            else:
                sigmas[0][1] = 0.0
            for sig in sigmas:
                nz = (np.maximum(sig, 0.5)[None, :, None, None] * rs.randn(B, nu, H, K)).astype(np.float32)
                for rho in (0.0, 0.6):
                    msg = (K, H, nu, rho, sig.tolist()[:3])
                    eng.set_noise_model(sig, rho)
                    term, lin = eng.control_term_eval(U, nz)
                    r = _check_kernels(lin, term, U, nz, sig, rho, gamma, msg)
                    worst = [max(worst[0], r[0]), max(worst[1], r[1])]
                    assert np.all(lin[:, sig == 0.0] == 0.0), msg
                    if nu == 1 and sig[0] == 0.0:
                        assert np.all(term == 0.0), msg
                    again = eng.control_term_eval(U, nz)
                    _same(again[0], term, (msg, "two calls"))
                    _same(again[1], lin, (msg, "two calls"))
                    for form in ("block", "split"):
                        with _env(MPPI_CTRL_COST_FORM=form):
                            _same(eng.control_term_eval(U, nz)[0], term, (msg, form))
                    for nt in ("0", "1"):
                        with _env(MPPI_CTRL_COST_NT=nt):
                            _same(eng.control_term_eval(U, nz)[0], term, (msg, "NT", nt))
            eng.close()
    print(f"K={K}: worst error / bound: lin {worst[0]:.3g}, term {worst[1]:.3g}")


def test_control_term_eval_state_and_argument_errors(M):
    from mppi_hip import _lib as L
    eng = M.Engine(M.Config(nx=4, nu=2, H=3, K=30, max_batch=2))
    U, nz = np.ones((2, 2, 3), np.float32), np.ones((2, 2, 3, 30), np.float32)
    assert eng.control_cost() == 0.0
    with pytest.raises(M.MPPIError) as ei:  # the term is off
        eng.control_term_eval(U, nz)
    assert ei.value.code == L.MPPI_E_STATE
    with pytest.raises(M.MPPIError) as ei:  # no solve with the term has run
        eng.control_term(1)
    assert ei.value.code == L.MPPI_E_STATE
    eng.set_control_cost(2.0)
    assert eng.control_cost() == 2.0
    term, lin = eng.control_term_eval(U, nz)  # the default law: cfg.sigma = 1, rho = 0 -> lin = gamma U, term = 12
    assert np.all(lin == 2.0) and np.all(term == 12.0)
    with pytest.raises(M.MPPIError) as ei:
        eng.control_term_eval(np.ones((3, 2, 3), np.float32), np.ones((3, 2, 3, 30), np.float32))  # beyond max_batch
    assert ei.value.code == L.MPPI_E_ARG
    with pytest.raises(M.MPPIError) as ei:  # an evaluation is no solve
        eng.control_term(1)
    assert ei.value.code == L.MPPI_E_STATE
    nan, inf = float("nan"), float("inf")
    for bad in (-1.0, nan, inf, -inf):  # refused, and nothing changes
        assert eng.lib.mppi_set_control_cost(eng._h, ctypes.c_float(bad)) == L.MPPI_E_ARG, bad
        assert b"mppi_set_control_cost" in eng.lib.mppi_last_error()
        assert eng.control_cost() == 2.0
    eng.set_control_cost(0.0)
    with pytest.raises(M.MPPIError) as ei:
        eng.control_term_eval(U, nz)
    assert ei.value.code == L.MPPI_E_STATE
    eng.close()


def test_a_nonfinite_injected_eps_makes_its_sample_nonfinite_and_no_other(M):
    """The header's rule: every row enters the sum, a frozen actuator's (lin = 0) and a zero nominal entry's included,
    so an injected inf or NaN makes that sample's term non-finite (0 * inf) -- and leaves every other sample's term
    bitwise what it is with clean noise, in both grid forms, as in the float64 restatement."""
    from mppi_hip.stats import control_term_ref
    B, nu, H, K = 2, 3, 17, 75
    rs = np.random.RandomState(8)
    eng = M.Engine(M.Config(nx=4, nu=nu, H=H, K=K, max_batch=B))
    eng.set_control_cost(0.7)
    sig = np.array([0.5, 0.0, 0.8], np.float32)
    eng.set_noise_model(sig, 0.0)  # rho = 0: lin[t] = gamma U[t] / sigma^2, so a zero U entry is a zero lin entry
    U = rs.randn(B, nu, H).astype(np.float32)
    U[:, 2, 4] = 0.0
    nz = rs.randn(B, nu, H, K).astype(np.float32)
    clean = eng.control_term_eval(U, nz)
    bad = nz.copy()
    bad[:, 1, :, 7] = np.inf   # the frozen actuator, every t
    bad[:, 1, 3, 9] = np.nan
    bad[:, 2, 4, 11] = -np.inf  # the zero nominal entry of a live actuator
    bad[0, 0, 2, 13] = np.inf   # a live row of solve 0
    hit = np.zeros((B, K), bool)
    hit[:, [7, 9, 11]], hit[0, 13] = True, True
    assert np.all(np.isfinite(clean[0])) and np.all(clean[1][:, 1] == 0.0) and np.all(clean[1][:, 2, 4] == 0.0)
    for form in (None, "block", "split"):
        with _env(**({"MPPI_CTRL_COST_FORM": form} if form else {})):
            got = eng.control_term_eval(U, bad)
        assert not np.isfinite(got[0][hit]).any(), form
        _same(got[0][~hit], clean[0][~hit], form)
        _same(got[1], clean[1], form)
    ref = control_term_ref(U, bad, sig.astype(np.float64), 0.0, float(np.float32(0.7)))[0]
    assert not np.isfinite(ref[hit]).any() and np.isfinite(ref[~hit]).all()
    eng.close()


# ------------------------------------------------------------------------------------------ 2. a solve uses it

def _softmin64(c, lam):
    """float64 softmin weights of one solve's costs (non-finite: weight 0)."""
    c = np.asarray(c, np.float64)
    fin = np.isfinite(c)
    w = np.zeros_like(c)
    w[fin] = np.exp(-(c[fin] - c[fin].min()) / lam)
    return w / w.sum()


@pytest.mark.parametrize("kind", ["cartpole", "mlp"])
@pytest.mark.parametrize("H", [7, 1])
def test_a_solve_weighs_costs_plus_term(M, kind, H):
    """Injected noise, gamma chosen (from the float64 reference) so that the term's spread equals the cost spread.
    The single non-finite cost comes from one sample whose noise is 3e38 on every row: the MLP's rollout overflows, and
    the cartpole's running cost squares the unclamped control (only the force is clamped to the control range)."""
    from mppi_hip import _lib as L
    from mppi_hip.stats import control_term_ref, solve_stats_ref
    K, B = 130, 2
    eng, x0, U0 = _setup(M, kind, K, H, B)
    nu, sigma, lam = U0.shape[1], eng.config.sigma, eng.config.lambda_
    nz = (sigma * np.random.RandomState(5).randn(B, nu, H, K)).astype(np.float32)
    ref = eng.solve(x0, U0, noise=nz, want_weights=True, stats=True)  # the same solve without the term
    t1 = control_term_ref(U0, nz, sigma, 0.0, 1.0)[0]
    gamma = float(np.float32(np.median(ref.costs.std(axis=1) / t1.std(axis=1))))
    eng.set_control_cost(gamma)
    assert eng.control_cost() == gamma
    res = eng.solve(x0, U0, noise=nz, want_weights=True, stats=True)
    term, lin = eng.control_term(B)
    _same(res.costs, ref.costs, "the term changes no cost")
    ev = eng.control_term_eval(U0, nz)
    _same(term, ev[0], "the solve's term is the kernels' on its U and noise")
    _same(lin, ev[1])
    _same(eng.control_term(B)[0], term, "control_term_eval leaves the solve's term readable")
    _check_kernels(lin, term, U0, nz, np.full(nu, sigma), 0.0, gamma, (kind, H))
    wc = (res.costs + term).astype(np.float32)  # formed in fp32, as the kernel forms it
    e64 = nz.astype(np.float64)
    moved = 0.0
    for b in range(B):
        w = _softmin64(wc[b], lam)
        moved = max(moved, np.abs(w - _softmin64(res.costs[b], lam)).max())
        np.testing.assert_allclose(res.weights[b], w, rtol=0.0, atol=1e-5)
        Unew = U0[b] + np.einsum("k,uhk->uh", w, e64[b])
        np.testing.assert_allclose(res.U[b], Unew, rtol=0.0, atol=1e-5)
        np.testing.assert_allclose(res.u0[b], Unew[:, 0], rtol=0.0, atol=1e-5)
        want = solve_stats_ref(wc[b], nz[b], lam=lam)
        for name in ("cost_min", "cost_weighted"):
            np.testing.assert_allclose(res.stats[name][b], want[name], rtol=1e-4, atol=0.0, err_msg=name)
    assert moved > 1e-3, "the term must move the weights, or the checks above pass vacuously"
    assert np.abs(res.weights - ref.weights).max() > 1e-3
    # every sample of solve 1 non-finite: MPPI_E_NONFINITE as before
    bad = x0.copy()
    bad[1, :] = np.nan
    assert eng.solve(bad, U0, noise=nz).status == L.MPPI_E_NONFINITE
    # one sample whose rollout overflows: its cost is non-finite, wcost too, its weight 0
    big = nz.copy()
    big[0, :, :, 5] = 3e38
    one = eng.solve(x0, U0, noise=big, want_weights=True)
    t_big = eng.control_term(B)[0]
    assert one.status == 0 and not np.isfinite(one.costs[0, 5])
    with np.errstate(invalid="ignore", over="ignore"):
        assert not np.isfinite(np.float32(one.costs[0, 5]) + np.float32(t_big[0, 5]))  # wcost, as the kernel forms it
    assert one.weights[0, 5] == 0.0 and np.all(np.isfinite(one.U)) and np.all(np.isfinite(one.u0))
    keep = np.arange(K) != 5
    assert np.all(np.isfinite(one.costs[0][keep])) and np.all(np.isfinite(t_big[0][keep]))
    w = np.zeros(K)
    w[keep] = _softmin64((one.costs[0][keep] + t_big[0][keep]).astype(np.float32), lam)
    np.testing.assert_allclose(one.weights[0], w, rtol=0.0, atol=1e-5)
    np.testing.assert_allclose(one.weights[1], _softmin64((one.costs[1] + t_big[1]).astype(np.float32), lam), rtol=0.0,
                               atol=1e-5)
    # disabling restores the handle: bitwise the first solve
    eng.set_control_cost(0.0)
    off = eng.solve(x0, U0, noise=nz, want_weights=True, stats=True)
    for name in ("costs", "U", "u0", "weights"):
        _same(getattr(off, name), getattr(ref, name), name)
    for k, v in ref.stats.items():
        assert np.array_equal(off.stats[k], v), k
    eng.close()


# ------------------------------------------------------------------------------------------ 3. with ESS targeting

@pytest.mark.parametrize("kind", ["cartpole", "mlp"])
def test_the_lambda_search_reads_costs_plus_term(M, kind):
    K, H, B = 130, 7, 2
    eng, x0, U0 = _setup(M, kind, K, H, B)
    nz = (eng.config.sigma * np.random.RandomState(5).randn(B, U0.shape[1], H, K)).astype(np.float32)
    eng.set_ess_target(FRAC, *LIMITS)
    plain = eng.solve(x0, U0, noise=nz)
    lam_plain = eng.lambdas(B)
    eng.set_control_cost(2.0)
    res = eng.solve(x0, U0, noise=nz, want_weights=True)
    lam = eng.lambdas(B)
    term = eng.control_term(B)[0]
    _same(res.costs, plain.costs)
    wc = (res.costs + term).astype(np.float32)  # formed in fp32, as the kernel forms it
    _same(lam, eng.lambda_eval(wc), "the search ran on costs + term")
    assert not np.array_equal(_bits(lam), _bits(lam_plain))
    for b in range(B):
        np.testing.assert_allclose(res.weights[b], _softmin64(wc[b], float(lam[b])), rtol=0.0, atol=1e-5)
    eng.close()


# ------------------------------------------------------------------------------------------ 4. streams

GAMMA_STREAM = 0.5


def _configure(eng, kind, full, gamma=GAMMA_STREAM):
    eng.set_control_cost(gamma)
    if full:
        eng.set_noise_model(*(([0.6], 0.7) if kind == "cartpole" else ([0.2, 0.5, 0.8], 0.7)))
        eng.set_noise_adapt(0.3)
        eng.set_ess_target(FRAC, *LIMITS)


def _run_form(M, torch, kind, form, n, seed, full):
    """One stream form, n steps (device noise, seed counter, shift + env step) with the term on (full: with
    set_noise_adapt and set_ess_target too).  Returns the state after the n steps, the per-step lambda and law where
    the form can be asked, the last solve's term and lin, and for the plain form what a resumed handle needs."""
    from mppi_hip.trajectory import run_stream
    K, H, B = 130, 8, 2
    dev = torch.device("cuda")
    eng, x0, U0 = _setup(M, kind, K, H, B)
    _configure(eng, kind, full)
    law = lambda i: tuple(np.asarray(v, np.float32) for v in eng.noise_law(i)) if full else None
    lams = lambda i: eng.lambdas(B, i) if full else None
    out = dict(lam=[], law=[])
    if form == "traj":
        states, actions, U_end = run_stream(eng, x0, U0, n, seed=seed)
        out["traj"] = (states, actions)
        out["U"] = U_end
        out["lam"] = [lams(i) for i in range(n)]
        out["law"] = [law(i) for i in range(n)]
    else:
        eng.set_stream(torch.cuda.current_stream().cuda_stream)
        tx, tU = torch.from_numpy(x0).to(dev), torch.from_numpy(U0).to(dev)
        tu0 = torch.zeros(B, U0.shape[1], device=dev)
        if form == "graph":
            eng.graph_capture(B, n, tx.data_ptr(), tU.data_ptr(), tu0.data_ptr(), seed=seed)
            eng.graph_launch(sync=True)
            out["lam"] = [lams(i) for i in range(n)]
            out["law"] = [law(i) for i in range(n)]
        else:
            out["x_before"], out["u0_steps"] = [], []
            for i in range(n):
                if form == "plain":
                    out["x_before"].append(_snap(torch, tx)[0])
                    out["U_before_last"] = _snap(torch, tU)[0]
                eng.solve_device(B, tx.data_ptr(), tU.data_ptr(), None, seed=seed, u0_ptr=tu0.data_ptr(), shift=True,
                                 env_step=True, seed_counter=form == "plain", chain=form != "plain")
                out["lam"].append(lams(0))
                out["law"].append(law(0))
                if form == "plain":
                    out["u0_steps"].append(_snap(torch, tu0)[0])
        out["x"], out["U"], out["u0"] = _snap(torch, tx, tU, tu0)
    out["term"], out["lin"] = eng.control_term(B)
    out["ctr"] = eng.get_seed_counter()
    if form == "plain":  # what a fresh handle needs to continue, and two more steps of this one
        out["saved"] = dict(x=out["x"].copy(), U=out["U"].copy(), ctr=out["ctr"], gamma=eng.control_cost(),
                            law=eng.noise_model() if full else None)
        for _ in range(2):
            eng.solve_device(B, tx.data_ptr(), tU.data_ptr(), None, seed=seed, u0_ptr=tu0.data_ptr(), shift=True,
                             env_step=True, seed_counter=True)
        out["after"] = _snap(torch, tx, tU, tu0) + eng.control_term(B)
    eng.close()
    return out


@pytest.mark.parametrize("kind", ["cartpole", "mlp"])
@pytest.mark.parametrize("full", [False, True], ids=["term", "term+adapt+ess"])
def test_stream_forms_agree_bitwise(M, kind, full):
    """Plain counter solves, chained solves, one captured graph and graph_capture_traj via run_stream, three steps:
    bitwise equal x0, U, u0, the last solve's term and lin, per-step lambda and law (full), seed counter 3.  With the
    law adapting, the last solve's lin is the float64 lin of the law that DREW its noise (the history row), not of the
    law the adapt kernel left behind it.  A fresh handle restored from (x, U, seed counter, law, gamma) continues
    bitwise."""
    import torch
    from mppi_hip.stats import control_term_ref
    n, seed, B = 3, 9, 2
    outs = {f: _run_form(M, torch, kind, f, n, seed, full) for f in ("plain", "chain", "graph", "traj")}
    want = outs["plain"]
    for form, got in outs.items():
        assert got["ctr"] == n, form
        np.testing.assert_array_equal(got["U"], want["U"], err_msg=form)
        if form != "traj":
            np.testing.assert_array_equal(got["x"], want["x"], err_msg=form)
            np.testing.assert_array_equal(got["u0"], want["u0"], err_msg=form)
        _same(got["term"], want["term"], (form, "term of the last solve"))
        _same(got["lin"], want["lin"], (form, "lin of the last solve"))
        for i, (a, b) in enumerate(zip(got["lam"], want["lam"])):
            if a is not None:
                _same(a, b, (form, "lambda of step", i))
        for i, (a, b) in enumerate(zip(got["law"], want["law"])):
            if a is not None:
                _same(a[0], b[0], (form, "sigma_u of step", i))
                _same(a[1], b[1], (form, "rho of step", i))
    states, actions = outs["traj"]["traj"]
    np.testing.assert_array_equal(states, np.stack(want["x_before"]))
    np.testing.assert_array_equal(actions, np.stack(want["u0_steps"]))
    # the term is live: lin is the float64 lin of the U the last solve started from, and not zero
    Ub = want["U_before_last"]
    nu = Ub.shape[1]
    if full:
        sig, rho = want["law"][-1]
        live_sig, live_rho, _ = want["saved"]["law"]
        assert not np.array_equal(sig, live_sig) and float(rho) != float(live_rho)  # the law moved behind the solve
    else:
        sig, rho = np.full(nu, {"cartpole": 1.0, "mlp": 0.5}[kind], np.float32), 0.0
    dummy = np.zeros(Ub.shape + (1,))
    _, lin64, A = control_term_ref(Ub, dummy, sig.astype(np.float64), float(rho), GAMMA_STREAM)
    assert np.all(np.abs(want["lin"] - lin64) <= 8 * U32 * A) and np.abs(lin64).max() > 0.0
    if full:
        _, lin_live, _ = control_term_ref(Ub, dummy, live_sig.astype(np.float64), float(live_rho), GAMMA_STREAM)
        assert np.any(np.abs(want["lin"] - lin_live) > 8 * U32 * A)
    # resume on a fresh handle
    dev = torch.device("cuda")
    s = want["saved"]
    eng, _, _ = _setup(M, kind, 130, 8, B)
    _configure(eng, kind, full, gamma=s["gamma"])
    if full:
        eng.set_noise_model(s["law"][0], s["law"][1])
    eng.set_seed_counter(s["ctr"])
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    tx, tU = torch.from_numpy(s["x"]).to(dev), torch.from_numpy(s["U"]).to(dev)
    tu0 = torch.zeros(B, nu, device=dev)
    for _ in range(2):
        eng.solve_device(B, tx.data_ptr(), tU.data_ptr(), None, seed=seed, u0_ptr=tu0.data_ptr(), shift=True,
                         env_step=True, chain=True)
    got = _snap(torch, tx, tU, tu0) + eng.control_term(B)
    for a, b in zip(got, want["after"]):
        _same(a, b, "resumed")
    eng.close()


# ------------------------------------------------------------------------------------------ 5. state rules

@pytest.mark.parametrize("kind", ["cartpole", "mlp"])
def test_launches_per_solve(M, kind):
    """A handle with the term off launches what it launched before (the cartpole: its one fused launch, no reduce);
    with the term on, "ctrl_cost" counts once per solve between the rollout and the reduce and the cartpole leaves its
    fused form; off again: as at first."""
    K, H, B = 130, 7, 2
    eng, x0, U0 = _setup(M, kind, K, H, B)

    def counts():
        eng.profile(True)  # (resets the counters)
        eng.solve(x0, U0, seed=3)
        got = {k: eng.kernel_time(k)[0] for k in ("noise", "rollout", "ctrl_cost", "lambda", "reduce", "stats")}
        eng.profile(False)
        return got

    fused = kind == "cartpole"
    off = dict(noise=1, rollout=1, ctrl_cost=0, reduce=0 if fused else 1, stats=0, **{"lambda": 0})
    assert counts() == off
    eng.set_control_cost(0.5)
    assert counts() == dict(noise=1, rollout=1, ctrl_cost=1, reduce=1, stats=0, **{"lambda": 0})
    eng.set_ess_target(FRAC, *LIMITS)
    assert counts() == dict(noise=1, rollout=1, ctrl_cost=1, reduce=1, stats=0, **{"lambda": 1})
    eng.set_ess_target(0.0)
    eng.set_control_cost(0.0)
    assert counts() == off
    eng.close()


def test_set_control_cost_destroys_graphs_and_keeps_the_prefetched_noise(M):
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

    def refused(eng):
        with pytest.raises(M.MPPIError) as ei:
            eng.graph_launch(sync=True)
        assert ei.value.code == L.MPPI_E_STATE and "mppi_graph_capture first" in str(ei.value)

    eng, tx, tU, tu0 = start()
    capture = lambda: eng.graph_capture(B, n, tx.data_ptr(), tU.data_ptr(), tu0.data_ptr(), seed=seed)
    capture()
    eng.graph_launch(sync=True)  # leaves a prefetched noise: the device counter is one ahead
    assert eng.get_seed_counter() == n
    eng.set_control_cost(0.0)  # off -> off: nothing to destroy
    eng.graph_launch(sync=True)
    eng.set_control_cost(0.5)  # enabling destroys the graph, keeps the key sequence
    assert eng.get_seed_counter() == 2 * n
    refused(eng)
    with pytest.raises(M.MPPIError) as ei:  # enabling alone is no solve with the term
        eng.control_term(B)
    assert ei.value.code == L.MPPI_E_STATE
    capture()
    eng.graph_launch(sync=True)
    assert eng.get_seed_counter() == 3 * n
    eng.control_term(B)
    for bad in (B + 1, 0):
        with pytest.raises(M.MPPIError) as ei:
            eng.control_term(bad)
        assert ei.value.code == L.MPPI_E_ARG
    eng.set_control_cost(0.5)  # the gamma in effect: a no-op, the graph stays
    eng.graph_launch(sync=True)
    eng.set_control_cost(0.75)  # a change destroys it
    refused(eng)
    capture()
    eng.set_control_cost(0.0)  # ... and so does disabling
    refused(eng)
    eng.close()

    # a prefetched noise survives set_control_cost: a chain with gamma set after two steps goes on with the noise it
    # would have drawn -- what plain counter solves with the same switch draw
    a = start()
    chain(*a, 2)
    a[0].set_control_cost(0.5)
    got = chain(*a, 2)
    assert a[0].get_seed_counter() == 4
    eng_b, bx, bU, bu0 = start()
    for i in range(4):
        if i == 2:
            eng_b.set_control_cost(0.5)
        eng_b.solve_device(B, bx.data_ptr(), bU.data_ptr(), None, seed=seed, u0_ptr=bu0.data_ptr(), shift=True,
                           env_step=True, seed_counter=True)
    want = _snap(torch, bx, bU, bu0)
    for x, y in zip(got, want):
        np.testing.assert_array_equal(x, y)
    _same(a[0].control_term(B)[0], eng_b.control_term(B)[0])
    # ... and control_term_eval drops it with the key sequence unchanged
    U1, nz1 = np.ones((B, MLP_NU, H), np.float32), np.ones((B, MLP_NU, H, K), np.float32)
    a[0].control_term_eval(U1, nz1)
    assert a[0].get_seed_counter() == 4
    got = chain(*a, 1)
    eng_b.solve_device(B, bx.data_ptr(), bU.data_ptr(), None, seed=seed, u0_ptr=bu0.data_ptr(), shift=True,
                       env_step=True, seed_counter=True)
    for x, y in zip(got, _snap(torch, bx, bU, bu0)):
        np.testing.assert_array_equal(x, y)
    for e in (a[0], eng_b):
        e.close()
