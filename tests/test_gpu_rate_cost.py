"""The control-rate cost term on the device (mppi_set_rate_cost): the kernel against float64 at a bound derived from
the number format, a solve whose softmin weighs costs (+ control term) + rate term, every stream form against a loop of
plain solves with the previously applied control carried on the device, and the state rules of the six entries.

Tolerance, with u = 2^-24 and n = nu (H - t0) summands (t0 = 0 with the anchor, 1 without), all non-negative (derived,
not tuned):
  |term_gpu - term_f64| <= (n + 4) u / (1 - (n + 4) u) * term_f64: one rounding for d, one for q = r d, one per fma,
      in any summation order (the kernel's cells are one such order); v = clamp(U + eps) is formed in fp32 on both
      sides (mppi_hip.stats.rate_term_ref), so it carries no error."""
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
    setups of tests/test_gpu_control_cost.py."""
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


def _check_term(term, U, nz, r, up, clamp, msg):
    """The derived bound; returns the worst error / bound."""
    from mppi_hip.stats import rate_term_ref
    want = rate_term_ref(U, nz, np.asarray(r, np.float32).astype(np.float64), up, clamp)
    n = U.shape[1] * (U.shape[2] - (0 if up is not None else 1))
    g = (n + 4) * U32
    bound = g / (1.0 - g) * want
    err = np.abs(term.astype(np.float64) - want)
    assert np.all(err <= bound), (msg, float((err / np.maximum(bound, 1e-300)).max()))
    if n == 0:
        assert np.all(term == 0.0), msg
    return float((err[want > 0] / bound[want > 0]).max()) if np.any(want > 0) else 0.0


# ------------------------------------------------------------------------------------------ 1. the kernel

@pytest.mark.parametrize("K", [30, 75, 1100])
def test_rate_term_eval_meets_the_derived_bound(M, K):
    """No rollout: rate_term_eval at B = 3 on K below a chunk / ragged / five 256-k chunks with a ragged last one,
    H in {1, 2, 17}, nu in {1, 3, 32}, the anchor on and off, ctrl_clamp 0 and a value that binds on a third of the
    elements, r with one zero entry.  At 16 rows per cell at the least, nu = 3, H = 17 puts cell boundaries inside an
    actuator's row (rows 16, 32, 48 of 51) and nu = 32, H = 17 exactly on row starts (34 rows per cell).  The bound of
    the module docstring, two calls bitwise equal, MPPI_RATE_COST_FORM=block and =split bitwise equal, the nontemporal
    knob bitwise equal to its default.
    Worst error / bound printed on an MI355X, K = 30 / 75 / 1100: 0.617, 0.634, 0.704 (the bound is tightest where n is
    smallest: nu = 1, H = 1 with the anchor is one summand, 5 u allowed, and d's rounding enters its square twice)."""
    B = 3
    worst = 0.0
    for H in (1, 2, 17):
        for nu in (1, 3, 32):
            rs = np.random.RandomState(1000 * H + nu)
            U = rs.randn(B, nu, H).astype(np.float32)
            nz = ((0.3 + rs.rand(nu))[None, :, None, None] * rs.randn(B, nu, H, K)).astype(np.float32)
            up = rs.randn(B, nu).astype(np.float32)
            r = (0.2 + rs.rand(nu)).astype(np.float32)
            if nu > 1:
                r[1] = 0.0
            binding = float(np.float32(np.quantile(np.abs(U[..., None] + nz), 2.0 / 3.0)))
            for clamp in (0.0, binding):
                eng = M.Engine(M.Config(nx=4, nu=nu, H=H, K=K, max_batch=B, ctrl_clamp=clamp))
                eng.set_prev_control(np.full((B, nu), 7.0, np.float32))  # (the handle's: an explicit u_prev wins)
                for anchor in (False, True):
                    msg = (K, H, nu, clamp, anchor)
                    eng.set_rate_cost(r, anchor=anchor)
                    got_r, got_a, active = eng.rate_cost()
                    assert np.array_equal(got_r, r) and got_a == anchor and active
                    term = eng.rate_term_eval(U, nz, up)
                    worst = max(worst, _check_term(term, U, nz, r, up if anchor else None, clamp, msg))
                    _same(eng.rate_term_eval(U, nz, up), term, (msg, "two calls"))
                    for form in ("block", "split"):
                        with _env(MPPI_RATE_COST_FORM=form):
                            _same(eng.rate_term_eval(U, nz, up), term, (msg, form))
                    for nt in ("0", "1"):
                        with _env(MPPI_RATE_COST_NT=nt):
                            _same(eng.rate_term_eval(U, nz, up), term, (msg, "NT", nt))
                _same(eng.prev_control(B), np.full((B, nu), 7.0), "an evaluation leaves the handle's u_prev")
                eng.set_prev_control(up)  # u_prev = None: the handle's
                _same(eng.rate_term_eval(U, nz), term, (K, H, nu, clamp, "the handle's u_prev"))
                eng.close()
    print(f"K={K}: worst error / bound: term {worst:.3g}")


def test_exact_cases_on_the_device(M):
    eng = M.Engine(M.Config(nx=4, nu=1, H=2, K=30, max_batch=1))
    U, nz = np.zeros((1, 1, 2), np.float32), np.zeros((1, 1, 2, 30), np.float32)
    nz[0, 0, 1] = 3.0
    eng.set_rate_cost(2.0, anchor=False)
    assert np.all(eng.rate_term_eval(U, nz) == 18.0)
    eng.set_rate_cost(2.0, anchor=True)
    assert np.all(eng.rate_term_eval(U, nz) == 18.0)  # u_prev reads as zeros until it is set
    assert np.all(eng.rate_term_eval(U, nz, [[1.0]]) == 20.0)
    assert np.all(eng.prev_control(1) == 0.0)
    eng.close()
    eng = M.Engine(M.Config(nx=4, nu=1, H=2, K=30, max_batch=1, ctrl_clamp=1.0))
    eng.set_rate_cost(2.0, anchor=False)
    assert np.all(eng.rate_term_eval(U, nz) == 2.0)  # v = [0, 1]
    eng.close()
    eng = M.Engine(M.Config(nx=4, nu=3, H=1, K=30, max_batch=2))  # H = 1 without the anchor: exactly 0
    eng.set_rate_cost([1.0, 0.0, 2.0], anchor=False)
    t = eng.rate_term_eval(np.ones((2, 3, 1), np.float32), np.random.RandomState(0).randn(2, 3, 1, 30))
    assert np.all(t == 0.0) and not np.any(np.signbit(t))
    U5 = np.full((2, 3, 1), 0.5, np.float32)  # constant U, zero noise
    assert np.all(eng.rate_term_eval(U5, np.zeros((2, 3, 1, 30), np.float32)) == 0.0)
    eng.close()


@pytest.mark.parametrize("clamp", [0.0, 0.9])
def test_a_nonfinite_injected_eps_makes_its_sample_nonfinite_and_no_other(M, clamp):
    """The header's rule: every row enters the sum -- an r[u] == 0 row, an unanchored t = 0 and, with ctrl_clamp on, an
    infinite control the clamp would have made finite included -- so an injected inf or NaN makes that sample's term
    non-finite and leaves every other sample's term bitwise what it is with clean noise, in both grid forms, anchored
    or not, as in the float64 restatement."""
    from mppi_hip.stats import rate_term_ref
    B, nu, H, K = 2, 3, 17, 75
    rs = np.random.RandomState(8)
    eng = M.Engine(M.Config(nx=4, nu=nu, H=H, K=K, max_batch=B, ctrl_clamp=clamp))
    r = np.array([0.5, 0.0, 0.8], np.float32)
    U = rs.randn(B, nu, H).astype(np.float32)
    nz = rs.randn(B, nu, H, K).astype(np.float32)
    up = rs.randn(B, nu).astype(np.float32)
    bad = nz.copy()
    bad[:, 1, :, 7] = np.inf    # the r == 0 actuator, every t
    bad[:, 1, 3, 9] = np.nan
    bad[:, 2, 0, 11] = -np.inf  # t = 0 of a live actuator
    bad[0, 0, 16, 13] = np.inf  # a live row of solve 0: row 16 of 51, the first row of cell 1
    bad[1, 2, 13, 15] = np.nan  # row 47: the row cell 3, which begins inside actuator 2's row, reads once more
    bad[1, 0, 15, 17] = np.inf  # row 15: likewise for cell 1
    hit = np.zeros((B, K), bool)
    hit[:, [7, 9, 11]], hit[0, 13], hit[1, [15, 17]] = True, True, True
    for anchor in (False, True):
        eng.set_rate_cost(r, anchor=anchor)
        clean = eng.rate_term_eval(U, nz, up)
        assert np.all(np.isfinite(clean))
        for form in (None, "block", "split"):
            with _env(**({"MPPI_RATE_COST_FORM": form} if form else {})):
                got = eng.rate_term_eval(U, bad, up)
            assert not np.isfinite(got[hit]).any(), (anchor, form)
            _same(got[~hit], clean[~hit], (anchor, form))
        ref = rate_term_ref(U, bad, r.astype(np.float64), up if anchor else None, clamp)
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
    """Injected noise, the anchor on with a u_prev of its own, r chosen (from the float64 reference) so that the term's
    spread equals the cost spread.  Then with the control-cost term and ESS targeting also on, with bounds on and
    binding, and off again."""
    from mppi_hip.stats import project_noise_ref, rate_term_ref, solve_stats_ref
    K, B = 130, 2
    eng, x0, U0 = _setup(M, kind, K, H, B)
    nu, sigma, lam, clamp = U0.shape[1], eng.config.sigma, eng.config.lambda_, eng.config.ctrl_clamp
    rs = np.random.RandomState(5)
    nz = (sigma * rs.randn(B, nu, H, K)).astype(np.float32)
    up = (0.3 * rs.randn(B, nu)).astype(np.float32)
    ref = eng.solve(x0, U0, noise=nz, want_weights=True, stats=True)  # the same solve without the term
    t1 = rate_term_ref(U0, nz, 1.0, up, clamp)
    r = np.full(nu, np.float32(np.median(ref.costs.std(axis=1) / t1.std(axis=1))), np.float32)
    if nu > 1:
        r[1] *= 0.5
    eng.set_prev_control(up)
    eng.set_rate_cost(r, anchor=True)
    res = eng.solve(x0, U0, noise=nz, want_weights=True, stats=True)
    term = eng.rate_term(B)
    _same(res.costs, ref.costs, "the term changes no cost")
    _same(eng.prev_control(B), up, "a solve without shift leaves u_prev as it is")
    _same(term, eng.rate_term_eval(U0, nz, up), "the solve's term is the kernel's on its U, noise and u_prev")
    _same(term, eng.rate_term_eval(U0, nz), "... which is the handle's")
    _same(eng.rate_term(B), term, "rate_term_eval leaves the solve's term readable")
    _check_term(term, U0, nz, r, up, clamp, (kind, H))
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
    # with the control-cost term and ESS targeting: wcost = (costs + ctrl) + rate, and the search reads it
    eng.set_control_cost(0.05)
    eng.set_ess_target(FRAC, *LIMITS)
    both = eng.solve(x0, U0, noise=nz, want_weights=True)
    _same(both.costs, ref.costs)
    _same(eng.rate_term(B), term, "the rate term does not depend on what it is added to")
    wc2 = ((both.costs + eng.control_term(B)[0]).astype(np.float32) + term).astype(np.float32)
    lams = eng.lambdas(B)
    _same(lams, eng.lambda_eval(wc2), "the search ran on (costs + control term) + rate term")
    for b in range(B):
        np.testing.assert_allclose(both.weights[b], _softmin64(wc2[b], float(lams[b])), rtol=0.0, atol=1e-5)
    eng.set_ess_target(0.0)
    eng.set_control_cost(0.0)
    # with bounds on and binding: the term is the kernel's on the projected noise
    lo, hi = -0.6 * sigma, 0.5 * sigma
    eng.set_control_bounds(lo, hi)
    eng.solve(x0, U0, noise=nz)
    proj, counts = project_noise_ref(U0, nz, lo, hi)
    assert counts.min() > 0
    t_b = eng.rate_term(B)
    _same(t_b, eng.rate_term_eval(U0, proj, up), "the solve's term is the kernel's on the projected noise")
    assert not np.array_equal(_bits(t_b), _bits(term))
    eng.set_control_bounds(None, None)
    # disabling restores the handle: bitwise the first solve
    eng.set_rate_cost(None)
    assert eng.rate_cost()[1:] == (False, False) and np.all(eng.rate_cost()[0] == 0.0)
    off = eng.solve(x0, U0, noise=nz, want_weights=True, stats=True)
    for name in ("costs", "U", "u0", "weights"):
        _same(getattr(off, name), getattr(ref, name), name)
    for k, v in ref.stats.items():
        assert np.array_equal(off.stats[k], v), k
    eng.close()


# ------------------------------------------------------------------------------------------ 3. streams

def _configure(eng, kind, full):
    nu = eng.config.nu
    eng.set_rate_cost(np.linspace(0.4, 0.2, nu), anchor=True)
    if full:
        eng.set_noise_model(*(([0.6], 0.7) if kind == "cartpole" else ([0.2, 0.5, 0.8], 0.7)))
        eng.set_noise_adapt(0.3)
        eng.set_ess_target(FRAC, *LIMITS)
        eng.set_control_cost(0.5)
        eng.set_control_bounds(-0.5, 0.4)


UP0 = 0.35  # the previous control every stream starts from (not the zeros a fresh handle reads)


def _run_form(M, torch, kind, form, n, seed, full):
    """One stream form, n steps (device noise, seed counter, shift + env step) with the anchored term on (full: with
    set_noise_model / set_noise_adapt, set_ess_target, set_control_cost and set_control_bounds too).  Returns the state
    after the n steps, the last solve's term, u_prev, and for the plain form what a resumed handle needs."""
    from mppi_hip.trajectory import run_stream
    K, H, B = 130, 8, 2
    dev = torch.device("cuda")
    eng, x0, U0 = _setup(M, kind, K, H, B)
    nu = U0.shape[1]
    _configure(eng, kind, full)
    eng.set_prev_control(np.full((B, nu), UP0, np.float32))
    out = {}
    if form == "traj":
        states, actions, U_end = run_stream(eng, x0, U0, n, seed=seed)
        out["traj"] = (states, actions)
        out["U"] = U_end
    else:
        eng.set_stream(torch.cuda.current_stream().cuda_stream)
        tx, tU = torch.from_numpy(x0).to(dev), torch.from_numpy(U0).to(dev)
        tu0 = torch.zeros(B, nu, device=dev)
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
                    _same(eng.prev_control(B), out["u0_steps"][-1], ("u_prev after step", i, "is its u0"))
        out["x"], out["U"], out["u0"] = _snap(torch, tx, tU, tu0)
    out["term"] = eng.rate_term(B)
    out["up"] = eng.prev_control(B)
    out["ctr"] = eng.get_seed_counter()
    if form == "plain":  # what a fresh handle needs to continue, and two more steps of this one
        out["saved"] = dict(x=out["x"].copy(), U=out["U"].copy(), ctr=out["ctr"], up=out["up"].copy(),
                            law=eng.noise_model() if full else None)
        for _ in range(2):
            eng.solve_device(B, tx.data_ptr(), tU.data_ptr(), None, seed=seed, u0_ptr=tu0.data_ptr(), shift=True,
                             env_step=True, seed_counter=True)
        out["after"] = _snap(torch, tx, tU, tu0) + (eng.rate_term(B), eng.prev_control(B))
    eng.close()
    return out


@pytest.mark.parametrize("kind", ["cartpole", "mlp"])
@pytest.mark.parametrize("full", [False, True], ids=["term", "term+adapt+ess+ctrl+bounds"])
def test_stream_forms_agree_bitwise(M, kind, full):
    """Plain counter solves, chained solves, one captured graph and graph_capture_traj via run_stream, three steps:
    bitwise equal x0, U, u0, the last solve's term, u_prev, seed counter 3; u_prev after step i is the u0 of step i.
    A fresh handle restored from (x, U, seed counter, law, the settings, u_prev) continues bitwise; the same restore
    without u_prev does not, so the anchor is live."""
    import torch
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
        _same(got["up"], want["up"], (form, "u_prev"))
        _same(got["up"], want["u0"], (form, "u_prev is the last u0"))
    states, actions = outs["traj"]["traj"]
    np.testing.assert_array_equal(states, np.stack(want["x_before"]))
    np.testing.assert_array_equal(actions, np.stack(want["u0_steps"]))
    assert np.abs(want["term"]).max() > 0.0
    # resume on a fresh handle: with u_prev bitwise, without it not
    dev = torch.device("cuda")
    s = want["saved"]
    nu = s["U"].shape[1]
    resumed = {}
    for with_up in (True, False):
        eng, _, _ = _setup(M, kind, 130, 8, B)
        _configure(eng, kind, full)
        if full:
            eng.set_noise_model(s["law"][0], s["law"][1])
        eng.set_seed_counter(s["ctr"])
        if with_up:
            eng.set_prev_control(s["up"])
        eng.set_stream(torch.cuda.current_stream().cuda_stream)
        tx, tU = torch.from_numpy(s["x"]).to(dev), torch.from_numpy(s["U"]).to(dev)
        tu0 = torch.zeros(B, nu, device=dev)
        for _ in range(2):
            eng.solve_device(B, tx.data_ptr(), tU.data_ptr(), None, seed=seed, u0_ptr=tu0.data_ptr(), shift=True,
                             env_step=True, chain=True)
        resumed[with_up] = _snap(torch, tx, tU, tu0) + (eng.rate_term(B), eng.prev_control(B))
        eng.close()
    for a, b in zip(resumed[True], want["after"]):
        _same(a, b, "resumed")
    assert not np.array_equal(_bits(resumed[False][1]), _bits(want["after"][1])), "U must depend on u_prev"
    assert not np.array_equal(_bits(resumed[False][3]), _bits(want["after"][3])), "the term must depend on u_prev"


# ------------------------------------------------------------------------------------------ 4. state rules

@pytest.mark.parametrize("kind", ["cartpole", "mlp"])
def test_launches_per_solve(M, kind):
    """A handle with the term off launches what it launched before (the cartpole: its one fused launch, no reduce);
    with the term on, "rate_cost" counts once per solve -- the term launches and, in a shift solve with the anchor, the
    store of u_prev together -- and the cartpole leaves its fused form; off again: as at first."""
    K, H, B = 130, 7, 2
    eng, x0, U0 = _setup(M, kind, K, H, B)
    names = ("noise", "rollout", "ctrl_cost", "bounds", "rate_cost", "lambda", "reduce", "stats")

    def counts(**kw):
        eng.profile(True)  # (resets the counters)
        eng.solve(x0, U0, seed=3, **kw)
        got = {k: eng.kernel_time(k)[0] for k in names}
        eng.profile(False)
        return got

    fused = kind == "cartpole"
    off = dict.fromkeys(names, 0)
    off.update(noise=1, rollout=1, reduce=0 if fused else 1)
    on = dict(off, rate_cost=1, reduce=1)
    assert counts() == off and counts(shift=True) == off
    eng.set_rate_cost(0.5, anchor=True)
    assert counts() == on and counts(shift=True) == on
    eng.set_rate_cost(0.5, anchor=False)
    assert counts() == on and counts(shift=True) == on
    eng.set_control_cost(0.5)
    assert counts(shift=True) == dict(on, ctrl_cost=1)
    eng.set_control_cost(0.0)
    eng.set_rate_cost(None)
    assert counts() == off and counts(shift=True) == off
    eng.close()


def test_state_and_argument_errors(M):
    from mppi_hip import _lib as L
    eng = M.Engine(M.Config(nx=4, nu=2, H=3, K=30, max_batch=2))
    U, nz = np.ones((2, 2, 3), np.float32), np.ones((2, 2, 3, 30), np.float32)
    assert eng.rate_cost()[1:] == (False, False)
    assert np.all(eng.prev_control(2) == 0.0)  # zeros before anything was set
    for call in (lambda: eng.rate_term_eval(U, nz), lambda: eng.rate_term(1)):  # the term is off / no solve ran
        with pytest.raises(M.MPPIError) as ei:
            call()
        assert ei.value.code == L.MPPI_E_STATE
    eng.set_prev_control([[1.0, 2.0], [3.0, 4.0]])  # allowed with the term off
    assert eng.prev_control(2).tolist() == [[1.0, 2.0], [3.0, 4.0]]
    for bad_B in (0, 3):
        buf = np.zeros((3, 2), np.float32)
        p = buf.ctypes.data_as(ctypes.c_void_p)
        assert eng.lib.mppi_set_prev_control(eng._h, bad_B, p) == L.MPPI_E_ARG
        assert eng.lib.mppi_get_prev_control(eng._h, bad_B, p) == L.MPPI_E_ARG
    eng.set_rate_cost([2.0, 0.0], anchor=True)
    assert np.all(eng.rate_term_eval(U, nz) == 2.0)  # u = 0: v = 2 against u_prev = 1 and 3, r = 2; u = 1: r = 0
    with pytest.raises(M.MPPIError) as ei:
        eng.rate_term_eval(np.ones((3, 2, 3), np.float32), np.ones((3, 2, 3, 30), np.float32))  # beyond max_batch
    assert ei.value.code == L.MPPI_E_ARG
    with pytest.raises(M.MPPIError) as ei:  # an evaluation is no solve
        eng.rate_term(1)
    assert ei.value.code == L.MPPI_E_STATE
    nan, inf = float("nan"), float("inf")
    for bad in ([-1.0, 1.0], [nan, 1.0], [inf, 1.0], [1.0, -inf], [0.0, 0.0]):  # refused, and nothing changes
        a = np.asarray(bad, np.float32)
        assert eng.lib.mppi_set_rate_cost(eng._h, a.ctypes.data_as(L._fp), 0) == L.MPPI_E_ARG, bad
        assert b"mppi_set_rate_cost" in eng.lib.mppi_last_error()
        got = eng.rate_cost()
        assert got[0].tolist() == [2.0, 0.0] and got[1:] == (True, True)
    with pytest.raises(ValueError):
        eng.set_rate_cost([1.0, 2.0, 3.0])
    eng.set_rate_cost(None)
    with pytest.raises(M.MPPIError) as ei:
        eng.rate_term_eval(U, nz)
    assert ei.value.code == L.MPPI_E_STATE
    assert eng.prev_control(2).tolist() == [[1.0, 2.0], [3.0, 4.0]]  # disabling leaves u_prev
    eng.close()
    big = M.Engine(M.Config(nx=4, nu=33, H=2, K=30))  # the weights travel as a kernel argument
    with pytest.raises(M.MPPIError) as ei:
        big.set_rate_cost(1.0)
    assert ei.value.code == L.MPPI_E_UNSUPPORTED
    big.set_rate_cost(None)  # nothing to disable: fine at any nu
    assert not big.rate_cost()[2]
    big.close()


def test_set_rate_cost_destroys_graphs_and_keeps_the_prefetched_noise(M):
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
    eng.set_rate_cost(None)  # off -> off: nothing to destroy
    eng.set_prev_control(np.ones((B, MLP_NU), np.float32))  # data: destroys nothing
    eng.graph_launch(sync=True)
    eng.set_rate_cost(0.5)  # enabling destroys the graph, keeps the key sequence
    assert eng.get_seed_counter() == 2 * n
    refused(eng)
    with pytest.raises(M.MPPIError) as ei:  # enabling alone is no solve with the term
        eng.rate_term(B)
    assert ei.value.code == L.MPPI_E_STATE
    capture()
    eng.graph_launch(sync=True)
    assert eng.get_seed_counter() == 3 * n
    eng.rate_term(B)
    for bad in (B + 1, 0):
        with pytest.raises(M.MPPIError) as ei:
            eng.rate_term(bad)
        assert ei.value.code == L.MPPI_E_ARG
    eng.set_rate_cost(0.5)  # the values in effect: a no-op, the graph stays
    eng.set_prev_control(np.zeros((B, MLP_NU), np.float32))  # ... and u_prev may change between launches
    eng.graph_launch(sync=True)
    _same(eng.prev_control(B), _snap(torch, tu0)[0], "the graph stored its last u0")
    eng.set_rate_cost(0.75)  # a change of r destroys it
    refused(eng)
    capture()
    eng.set_rate_cost(0.75, anchor=False)  # ... a change of the anchor
    refused(eng)
    capture()
    eng.set_rate_cost(None)  # ... and disabling
    refused(eng)
    eng.close()

    # a prefetched noise survives set_rate_cost: a chain with the term set after two steps goes on with the noise it
    # would have drawn -- what plain counter solves with the same switch draw
    a = start()
    chain(*a, 2)
    a[0].set_rate_cost(0.5)
    got = chain(*a, 2)
    assert a[0].get_seed_counter() == 4
    eng_b, bx, bU, bu0 = start()
    for i in range(4):
        if i == 2:
            eng_b.set_rate_cost(0.5)
        eng_b.solve_device(B, bx.data_ptr(), bU.data_ptr(), None, seed=seed, u0_ptr=bu0.data_ptr(), shift=True,
                           env_step=True, seed_counter=True)
    want = _snap(torch, bx, bU, bu0)
    for x, y in zip(got, want):
        np.testing.assert_array_equal(x, y)
    _same(a[0].rate_term(B), eng_b.rate_term(B))
    # ... and rate_term_eval drops it with the key sequence unchanged
    U1, nz1 = np.ones((B, MLP_NU, H), np.float32), np.ones((B, MLP_NU, H, K), np.float32)
    a[0].rate_term_eval(U1, nz1)
    assert a[0].get_seed_counter() == 4
    got = chain(*a, 1)
    eng_b.solve_device(B, bx.data_ptr(), bU.data_ptr(), None, seed=seed, u0_ptr=bu0.data_ptr(), shift=True,
                       env_step=True, seed_counter=True)
    for x, y in zip(got, _snap(torch, bx, bU, bu0)):
        np.testing.assert_array_equal(x, y)
    for e in (a[0], eng_b):
        e.close()
