"""Dynamics-model ensembles on the device (mppi_load_member, mppi_set_ensemble): a handle with the ensemble off is the
handle that never loaded a member; member e's costs are, bit for bit, the costs of a handle that loaded blob e alone,
the combined costs and the spread the rule of csrc/ensemble.h over them; identical members are the single model, bare
and under the CEM stack, for every family of dynamics; the cartpole parameter ensemble; the combining kernel against its
numpy restatement; every stream form against the loop of plain solves; env_member; and the state rules of the entries.
Every comparison but the weights' (atol 1e-5, the bar of tests/test_gpu_parity.py) is bitwise."""
import os

import numpy as np
import pytest

from conftest import REPO
from ensemble_cases import MODES, assert_hand, bits, grid, hand_cases, same_bits

pytestmark = pytest.mark.gpu

K0, B0, H0, SEED = 130, 2, 8, 7  # Kp = 192: the pads are live
NX, NU = 10, 3
KERNELS = ("noise", "rollout", "reduce", "update", "stats", "lambda", "ctrl_cost", "bounds", "rate_cost", "elites",
           "keep", "cross", "cov_adapt", "step_mom", "step_adapt", "iter", "ensemble")
BOX = 0.3


@pytest.fixture(scope="module")
def M(gpu_available):
    import mppi_hip
    return mppi_hip


def _blob(M, kind, e):
    """Member e of a family: (dynamics kind, blob)."""
    from mppi_hip.nets import feature_attention_blob, mlp_blob, synthetic_feature_attention, synthetic_mlp
    if kind == "mlp":
        return mlp_blob(synthetic_mlp(NX, NU, seed=e), NX, NU)
    if kind == "fa":
        return feature_attention_blob(synthetic_feature_attention(4, 1, 64, seed=e), 4, 1, 64)
    if kind == "ca":
        return M.cross_attention_blob(M.load_npz(os.path.join(REPO, "tests", "golden", "ca_humanoid_weights.npz")))
    # the cartpole: the default parameters with the pole mass (entry 1 of the 10) scaled 0.8 / 1.0 / 1.2
    p = _cart_default(M).copy()
    p[1] *= np.float32((0.8, 1.0, 1.2)[e])
    return 1, p.tobytes()


_CART = []


def _cart_default(M):
    """The analytic cartpole's 10 parameters as the library derives them from models/cartpole.xml (m_cart, m_pole, l,
    inertia, damping, gear, ctrl_lo, ctrl_hi, g, dt; oracle/mppi_ref.py::_cartpole_params states the derivation), in
    double and rounded once; the cartpole test holds them to the library's own defaults."""
    if not _CART:
        rho, r, L, pi = 1000.0, 0.045, 0.6, 3.14159265358979323846
        m_cyl, m_sph = rho * pi * r * r * L, rho * 4.0 / 3.0 * pi * r * r * r
        inertia = m_cyl * (L * L / 12.0 + r * r / 4.0) + m_sph * (2.0 * r * r / 5.0 + L * L / 4.0 + 3.0 * L * r / 8.0)
        _CART.append(np.array([rho * 0.4 * 0.2 * 0.1, m_cyl + m_sph, L / 2.0, inertia, 0.05, 50.0, -1.0, 1.0, 9.81, 0.01],
                              np.float32))
    return _CART[0]


def _setup(M, kind, members=(0,), H=H0, K=K0, B=B0, precision=0, **kw):
    """(engine, x0, U0): member 0 = members[0] through load_dynamics, the others through load_member; nothing enabled.
    mlp: the synthetic MLP (nx 10, nu 3, quad_est); ca: the golden CrossAttention humanoid; fa: the synthetic
    FeatureAttention (4, 1, 64) under the cartpole cost; cartpole: the analytic model pinned to its unfused form."""
    rs = np.random.RandomState(11)
    if kind == "mlp":
        cfg = dict(nx=NX, nu=NU, H=H, K=K, max_batch=B, lambda_=1.0, sigma=0.5, precision=precision)
        cfg.update(kw)
        eng = M.Engine(M.Config(**cfg))
        cost, x0 = "quad_est", 0.3 * rs.randn(B, NX)
    elif kind == "ca":
        eng = M.Engine(M.Config.preset("humanoid_v3", K=K, H=H, precision=precision, max_batch=B, **kw))
        cost = "humanoid_v3"
        x0 = np.load(os.path.join(REPO, "tests", "golden", "g5_ca_humanoid_fwd.npz"))["x0_stride20"][:B]
    elif kind == "fa":
        eng = M.Engine(M.Config(nx=4, nu=1, H=H, K=K, max_batch=B, lambda_=1.0, sigma=0.5, precision=precision, **kw))
        cost, x0 = "cartpole", np.stack([[0.0, 0.2 + 0.3 * b, 0.0, 0.0] for b in range(B)])
    else:
        eng = M.Engine(M.Config.preset("cartpole_py", K=K, H=H, max_batch=B, **kw))
        cost, x0 = "cartpole", np.stack([[0.0, 0.2 + 0.3 * b, 0.0, 0.0] for b in range(B)])
    eng.load_dynamics(*_blob(M, kind, members[0])).set_cost(cost)
    for e, m in enumerate(members[1:], 1):
        eng.load_member(e, *_blob(M, kind, m))
    if kind == "cartpole":  # the unfused form on every handle, as tests/test_gpu_elites.py pins it
        eng.set_ess_target(0.25, eng.config.lambda_, eng.config.lambda_)
    U0 = 0.1 * rs.randn(B, eng.config.nu, H)
    return eng, np.ascontiguousarray(x0, np.float32), U0.astype(np.float32)


def _cem(eng, B=B0):
    """The "cem" stack of tests/test_gpu_iterations.py."""
    c = eng.config
    sig = (0.2 + 0.6 * np.arange(c.nu) / max(c.nu - 1, 1)).astype(np.float32)
    eng.set_elites(13)
    eng.set_elite_keep(5)
    eng.set_noise_model(sig, 0.5)
    eng.set_noise_steps((0.1 + 0.9 * np.random.RandomState(3).rand(B, c.nu, c.H)).astype(np.float32))
    eng.set_noise_steps_adapt(0.5, 0.01, 3.0, centred=True)
    eng.set_control_bounds(-BOX, BOX)
    eng.set_rate_cost(0.05, anchor=True)
    eng.set_ess_target(0.2)
    return eng


def _eq(a, b, msg):
    """Bitwise: floats by their bits, everything else by value; tuples and dicts member by member."""
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


def _snap(torch, *ts):
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in ts)


def _tensors(torch, eng, x0, U0):
    dev = torch.device("cuda")
    c = eng.config
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    return (torch.from_numpy(x0).to(dev), torch.from_numpy(U0).to(dev), torch.zeros(x0.shape[0], c.nu, device=dev),
            torch.zeros(x0.shape[0], c.K, device=dev))


def _code(M, fn):
    with pytest.raises(M.MPPIError) as ei:
        fn()
    return ei.value


# ------------------------------------------------------------------------------------------ 1. off is off

def test_off_is_the_handle_that_never_loaded_a_member(M):
    """Fresh; members loaded but never enabled; enabled and set back to 1: every output of a host solve and two chained
    solves, the seed counter and every kernel's launch count are equal, and "ensemble" never ran."""
    import torch
    outs = []
    for touch in ("fresh", "loaded", "set back"):
        eng, x0, U0 = _setup(M, "mlp", (0,) if touch == "fresh" else (0, 1, 2))
        if touch == "set back":
            eng.set_ensemble(3, "worst", 0.5, 2).set_ensemble(1, "mean_std", 2.0)
            assert eng.ensemble()["n"] == 1 and eng.ensemble()["n_loaded"] == 3
        eng.profile(True)
        res = eng.solve(x0, U0, seed=SEED, shift=True, want_weights=True)
        tx, tU, tu0, tc = _tensors(torch, eng, x0, res.U)
        for _ in range(2):
            eng.solve_device(B0, tx.data_ptr(), tU.data_ptr(), None, seed=SEED, u0_ptr=tu0.data_ptr(),
                             costs_ptr=tc.data_ptr(), shift=True, env_step=True, chain=True)
        dev = _snap(torch, tx, tU, tu0, tc)
        eng.profile(False)
        counts = {k: eng.kernel_time(k)[0] for k in KERNELS}
        outs.append(((res.U, res.u0, res.costs, res.weights), dev, eng.get_seed_counter(), eng.rollout_kernel(), counts))
        eng.close()
    for o in outs[1:]:
        _eq(o[:4], outs[0][:4], "off against the fresh handle")
        assert o[4] == outs[0][4], (o[4], outs[0][4])
    assert outs[0][4]["ensemble"] == 0 and outs[0][4]["rollout"] == 3, outs[0][4]


# ------------------------------------------------------------------------------------------ 2. the defining loop

_SINGLE = {}


def _single_costs(M, kind, e, noise_kind, **kw):
    """io.costs of a handle that loaded member e alone, on the shared inputs and key (cached: the modes share it)."""
    key = (kind, e, noise_kind, tuple(sorted(kw.items())))
    if key not in _SINGLE:
        eng, x0, U0 = _setup(M, kind, (e,), **kw)
        nz = _noise(eng) if noise_kind == "injected" else None
        _SINGLE[key] = eng.solve(x0, U0, noise=nz, seed=SEED).costs
        eng.close()
    return _SINGLE[key]


def _noise(eng):
    c = eng.config
    nz = (c.sigma * np.random.RandomState(5).randn(B0, c.nu, c.H, c.K)).astype(np.float32)
    nz[0, 0, 0, 3] = np.nan  # one sample no member can roll: +inf in every mode
    return nz


def _defining_loop(M, kind, members, mode, noise_kind, kappa=0.5, **kw):
    from mppi_hip.stats import ensemble_combine_f32, softmin_weights_ref
    n = len(members)
    eng, x0, U0 = _setup(M, kind, members, **kw)
    eng.set_ensemble(n, mode, kappa)
    eng.profile(True)
    nz = _noise(eng) if noise_kind == "injected" else None
    res = eng.solve(x0, U0, noise=nz, seed=SEED, want_weights=True)
    eng.profile(False)
    assert eng.kernel_time("ensemble")[0] == 1 and eng.kernel_time("rollout")[0] == n
    mc = np.stack([eng.member_costs(e, B0) for e in range(n)])
    for e, m in enumerate(members):
        _eq(mc[e], _single_costs(M, kind, m, noise_kind, **kw), (kind, mode, noise_kind, "member", e))
    assert not same_bits(mc[0], mc[1])  # the members do differ
    want_cost, want_sd = ensemble_combine_f32(mc, mode, kappa)
    _eq(res.costs, want_cost, (kind, mode, noise_kind, "io.costs is the rule over the members' costs"))
    _eq(eng.ensemble_spread(B0), want_sd, (kind, mode, noise_kind, "the spread"))
    if noise_kind == "injected":
        assert res.costs[0, 3] == np.inf and want_sd[0, 3] == np.inf
    assert np.isfinite(want_sd).sum() >= B0 * K0 - 1 and (want_sd > 0).mean() > 0.9  # the members do disagree
    w = softmin_weights_ref(res.costs, eng.config.lambda_, eng.config.norm_eps)
    np.testing.assert_allclose(res.weights, w, rtol=0, atol=1e-5)
    eng.close()


@pytest.mark.parametrize("noise_kind", ["keyed", "injected"])
@pytest.mark.parametrize("mode", MODES)
def test_member_costs_are_the_single_handles_and_the_costs_the_rule_over_them(M, mode, noise_kind):
    _defining_loop(M, "mlp", (0, 1, 2), mode, noise_kind)


# ------------------------------------------------------------------------------------------ 3. identical members

def _identical(M, kind, n, mode, H=H0, precision=0):
    """(outputs of the ensemble handle, outputs of the single handle, the spread): a host solve that shifts, with its
    statistics, then two chained device solves with the env step."""
    import torch
    outs = []
    for ens in (True, False):
        eng, x0, U0 = _setup(M, kind, (0,) * n if ens else (0,), H=H, precision=precision)
        _cem(eng)
        if ens:
            eng.set_ensemble(n, mode, 0.0)
        res = eng.solve(x0, U0, seed=SEED, shift=True, stats=True, want_weights=True)
        host = (res.U, res.u0, res.costs, res.weights, res.stats)
        tx, tU, tu0, tc = _tensors(torch, eng, x0, res.U)
        for _ in range(2):
            eng.solve_device(B0, tx.data_ptr(), tU.data_ptr(), None, seed=SEED, u0_ptr=tu0.data_ptr(),
                             costs_ptr=tc.data_ptr(), shift=True, env_step=True, chain=True, stats=True)
        out = {"host": host, "dev": _snap(torch, tx, tU, tu0, tc), "stats": eng.stats(B0, 0),
               "ctr": eng.get_seed_counter(), "kept": eng.kept(B0)}
        if ens:
            sd = eng.ensemble_spread(B0)
        outs.append(out)
        eng.close()
    return outs[0], outs[1], sd


@pytest.mark.parametrize("n,mode", [(2, "mean"), (4, "mean"), (3, "worst"), (8, "mean")])
def test_identical_members_are_the_single_net_under_the_cem_stack(M, n, mode):
    got, want, sd = _identical(M, "mlp", n, mode)
    _eq(got, want, ("identical members", n, mode))
    assert not bits(sd).any(), (n, mode, sd)  # +0 everywhere


def test_identical_members_at_worst_n3_have_zero_spread(M):
    """n = 3 identical members at WORST: the spread is +0 on every sample.  The sequential sum alone would not give it
    (3 c is not always a float: the spread about fl(fl(3 c) r) is an ulp of c on about a third of these costs); the
    rule's line for equal members does (csrc/ensemble.h)."""
    got, want, sd = _identical(M, "mlp", 3, "worst")
    print(f"n = 3 worst: {int((bits(sd) != 0).sum())} of {sd.size} samples with sd != +0, max sd {float(sd.max()):.3e}")
    assert not bits(sd).any(), (int((bits(sd) != 0).sum()), float(sd.max()))


@pytest.mark.parametrize("kind,H,precision", [("ca", H0, 1), ("fa", 4, 1), ("mlp", H0, 2)],
                         ids=["ca bf16", "fa (4, 1, 64)", "mlp split"])
def test_identical_members_are_the_single_net_in_every_family(M, kind, H, precision):
    got, want, sd = _identical(M, kind, 2, "mean", H=H, precision=precision)
    _eq(got, want, ("identical members", kind))
    assert not bits(sd).any(), (kind, sd)


# ------------------------------------------------------------------------------------------ 4. the cartpole

def test_cartpole_parameter_ensemble_is_the_defining_loop(M):
    """Pole mass x 0.8 / 1.0 / 1.2 at WORST against three single handles pinned to the unfused form."""
    assert _blob(M, "cartpole", 1)[1] == _cart_default(M).tobytes()
    eng, x0, U0 = _setup(M, "cartpole", (1,))
    ref = M.Engine(eng.config)
    ref.load_dynamics(1).set_cost("cartpole").set_ess_target(0.25, eng.config.lambda_, eng.config.lambda_)
    _eq(eng.solve(x0, U0, seed=SEED).costs, ref.solve(x0, U0, seed=SEED).costs, "member 1 is the default cartpole")
    eng.close()
    ref.close()
    _defining_loop(M, "cartpole", (0, 1, 2), "worst", "keyed")


# ------------------------------------------------------------------------------------------ 5. the kernel

@pytest.mark.parametrize("K", [130, 4])
def test_ensemble_eval_equals_the_restatement_on_the_shared_cases(M, K):
    from mppi_hip.stats import ensemble_combine_f32
    eng = M.Engine(M.Config(nx=4, nu=1, H=2, K=K, max_batch=2))
    ns = set()
    for name, n, mode, kappa, m in grid(K):
        cost, sd = eng.ensemble_eval(m, mode, kappa)
        want = ensemble_combine_f32(m, mode, kappa)
        _eq(cost, want[0], (name, K, "cost"))
        _eq(sd, want[1], (name, K, "sd"))
        _eq(eng.ensemble_eval(m, mode, kappa), (cost, sd), (name, "two calls"))
        ns.add(n)
    assert ns == set(range(2, 9))
    if K == 4:
        for name, members, mode, kappa, want_cost, want_sd in hand_cases():
            m = np.array(members, np.float32)
            row = np.zeros((m.shape[0], 1, K), np.float32)
            row[:, 0, :m.shape[1]] = m
            cost, sd = eng.ensemble_eval(row, mode, kappa)
            assert_hand(name, cost[0], sd[0], want_cost, want_sd)
    # the evaluation leaves the handle alone: no ensemble is on, no solve has run
    assert eng.ensemble()["n"] == 1
    assert _code(M, lambda: eng.member_costs(0, 1)).code == M._lib.MPPI_E_STATE
    eng.close()


# ------------------------------------------------------------------------------------------ 6. stream forms

_LOOPS = {}


def _ens2(M, n_iter=1, pop=None):
    eng, x0, U0 = _setup(M, "mlp", (0, 1))
    eng.set_ensemble(2, "mean_std", 0.5)
    if n_iter > 1:
        eng.set_iterations(n_iter)
    if pop:
        eng.set_population(pop)
    return eng, x0, U0


def _loop(M, torch, steps, n_iter=1, pop=None):
    """`steps` plain device solves on the seed counter with SHIFT | ENV_STEP, synchronised one by one."""
    key = (steps, n_iter, pop)
    if key in _LOOPS:
        return _LOOPS[key]
    eng, x0, U0 = _ens2(M, n_iter, pop)
    tx, tU, tu0, tc = _tensors(torch, eng, x0, U0)
    out = {"x_before": [], "state": [], "member": [], "sd": []}
    for s in range(steps):
        out["x_before"].append(_snap(torch, tx)[0])
        eng.solve_device(B0, tx.data_ptr(), tU.data_ptr(), None, seed=SEED, u0_ptr=tu0.data_ptr(),
                         costs_ptr=tc.data_ptr(), shift=True, env_step=True, seed_counter=True, asynchronous=False)
        out["state"].append(_snap(torch, tx, tU, tu0, tc))
        out["member"].append(np.stack([eng.member_costs(e, B0) for e in range(2)]))
        out["sd"].append(eng.ensemble_spread(B0))
    out["ctr"] = eng.get_seed_counter()
    eng.close()
    _LOOPS[key] = out
    return out


@pytest.mark.parametrize("n_iter,pop", [(1, None), (2, (130, 70))], ids=["n_iter 1", "n_iter 2, population (130, 70)"])
@pytest.mark.parametrize("form", ["chain", "async", "graph", "traj"])
def test_stream_forms_equal_the_loop_of_plain_solves(M, form, n_iter, pop):
    import torch
    steps = 3
    want = _loop(M, torch, steps, n_iter, pop)
    eng, x0, U0 = _ens2(M, n_iter, pop)
    tx, tU, tu0, tc = _tensors(torch, eng, x0, U0)
    msg = (form, n_iter, pop)
    if form in ("chain", "async"):
        for s in range(steps):
            if form == "chain":
                eng.solve_device(B0, tx.data_ptr(), tU.data_ptr(), None, seed=SEED, u0_ptr=tu0.data_ptr(),
                                 costs_ptr=tc.data_ptr(), shift=True, env_step=True, chain=True)
            else:
                eng.solve_device(B0, tx.data_ptr(), tU.data_ptr(), None, seed=SEED, u0_ptr=tu0.data_ptr(),
                                 costs_ptr=tc.data_ptr(), shift=True, env_step=True, seed_counter=True,
                                 asynchronous=True)
            if form == "chain":
                _eq(_snap(torch, tx, tU, tu0, tc), want["state"][s], (msg, "state behind step", s))
    else:
        dev = torch.device("cuda")
        trx = torch.zeros(steps, B0, NX, device=dev)
        tru = torch.zeros(steps, B0, NU, device=dev)
        traj = dict(traj_x_ptr=trx.data_ptr(), traj_u_ptr=tru.data_ptr()) if form == "traj" else {}
        eng.graph_capture_traj(B0, steps, tx.data_ptr(), tU.data_ptr(), tu0.data_ptr(), costs_ptr=tc.data_ptr(),
                               seed=SEED, **traj)
        eng.graph_launch(sync=True)
        if form == "traj":
            sx, su = _snap(torch, trx, tru)
            _eq(sx, np.stack(want["x_before"]), (msg, "traj_x"))
            _eq(su, np.stack([s[2] for s in want["state"]]), (msg, "traj_u"))
    _eq(_snap(torch, tx, tU, tu0, tc), want["state"][-1], (msg, "final state"))
    _eq(np.stack([eng.member_costs(e, B0) for e in range(2)]), want["member"][-1], (msg, "member costs"))
    _eq(eng.ensemble_spread(B0), want["sd"][-1], (msg, "spread"))
    assert eng.get_seed_counter() == want["ctr"] == steps * n_iter
    eng.close()


# ------------------------------------------------------------------------------------------ 7. env_member

def test_the_env_step_runs_env_member(M):
    import torch
    eng, x0, U0 = _setup(M, "mlp", (0, 1))
    eng.set_ensemble(2, "mean", 0.0, env_member=1)
    assert eng.ensemble() == {"n": 2, "mode": "mean", "kappa": 0.0, "env_member": 1, "n_loaded": 2}
    tx, tU, tu0, tc = _tensors(torch, eng, x0, U0)
    eng.solve_device(B0, tx.data_ptr(), tU.data_ptr(), None, seed=SEED, u0_ptr=tu0.data_ptr(), env_step=True,
                     asynchronous=False)
    x1, u0 = _snap(torch, tx, tu0)
    eng.close()
    xs = []
    for e in (0, 1):  # a one-step handle of net e fed zero noise keeps U: it applies the ensemble's u0
        one, _, _ = _setup(M, "mlp", (e,), H=1, K=64)
        dev = torch.device("cuda")
        t1x = torch.from_numpy(x0).to(dev)
        t1U = torch.from_numpy(np.ascontiguousarray(u0[:, :, None])).to(dev)
        t1u0, zero = torch.zeros(B0, NU, device=dev), torch.zeros(B0, NU, 1, 64, device=dev)
        one.set_stream(torch.cuda.current_stream().cuda_stream)
        one.solve_device(B0, t1x.data_ptr(), t1U.data_ptr(), zero.data_ptr(), u0_ptr=t1u0.data_ptr(), env_step=True,
                         asynchronous=False)
        x, u = _snap(torch, t1x, t1u0)
        _eq(u, u0, "the one-step handle applied the same control")
        xs.append(x)
        one.close()
    _eq(x1, xs[1], "x0 after the env step is net 1's")
    assert not same_bits(xs[0], xs[1])


# ------------------------------------------------------------------------------------------ 8. state rules

def test_state_and_argument_errors(M):
    import torch
    L = M._lib
    from mppi_hip.nets import mlp_blob, synthetic_mlp
    kind, blob1 = _blob(M, "mlp", 1)
    fresh = M.Engine(M.Config(nx=NX, nu=NU, H=H0, K=K0, max_batch=B0, precision=0))
    assert fresh.ensemble() == {"n": 1, "mode": "mean", "kappa": 0.0, "env_member": 0, "n_loaded": 0}
    assert _code(M, lambda: fresh.load_member(1, kind, blob1)).code == L.MPPI_E_STATE  # member 0 first
    assert _code(M, lambda: fresh.set_ensemble(2)).code == L.MPPI_E_ARG
    fresh.set_ensemble(1)  # off stays off
    fresh.close()

    eng, x0, U0 = _setup(M, "mlp", (0,))
    for e in (0, -1, 8):
        assert _code(M, lambda: eng.load_member(e, kind, blob1)).code == L.MPPI_E_ARG
    assert _code(M, lambda: eng.load_member(2, kind, blob1)).code == L.MPPI_E_ARG  # densely
    assert _code(M, lambda: eng.load_member(1, 1, None)).code == L.MPPI_E_ARG  # member 0's kind
    assert _code(M, lambda: eng.load_member(1, kind, blob1[:100])).code == L.MPPI_E_UNSUPPORTED  # what the loader refuses
    assert eng.ensemble()["n_loaded"] == 1
    eng.load_member(1, kind, blob1)
    # a member of another hidden size is routed on its own
    wide = mlp_blob(synthetic_mlp(NX, NU, hidden_dim=64, seed=2), NX, NU, hidden_dim=64)
    eng.load_member(2, *wide)
    assert eng.ensemble()["n_loaded"] == 3
    for bad in ((0, 0, 0.0, 0), (4, 0, 0.0, 0), (9, 0, 0.0, 0), (2, 3, 0.0, 0), (2, -1, 0.0, 0),
                (2, 1, float("nan"), 0), (2, 1, float("inf"), 0), (2, 0, 0.0, 2), (2, 0, 0.0, -1), (1, 0, 0.0, 1)):
        assert eng.lib.mppi_set_ensemble(eng._h, *bad) == L.MPPI_E_ARG, bad
        assert eng.ensemble()["n"] == 1
    assert _code(M, lambda: eng.member_costs(0, B0)).code == L.MPPI_E_STATE
    eng.set_ensemble(3, "mean_std", -0.5, 1)
    assert eng.ensemble() == {"n": 3, "mode": "mean_std", "kappa": -0.5, "env_member": 1, "n_loaded": 3}
    assert eng.lib.mppi_set_ensemble(eng._h, 3, 7, 0.0, 0) == L.MPPI_E_ARG
    assert eng.ensemble() == {"n": 3, "mode": "mean_std", "kappa": -0.5, "env_member": 1, "n_loaded": 3}
    assert _code(M, lambda: eng.ensemble_spread(B0)).code == L.MPPI_E_STATE  # no solve under the setting yet
    e = _code(M, lambda: eng.load_dynamics(kind, blob1))
    assert e.code == L.MPPI_E_STATE and "mppi_set_ensemble" in str(e)
    res = eng.solve(x0, U0, seed=SEED)
    assert np.isfinite(res.costs).all() and np.isfinite(eng.member_costs(2, B0)).all()
    assert _code(M, lambda: eng.member_costs(3, B0)).code == L.MPPI_E_ARG
    assert _code(M, lambda: eng.member_costs(0, B0 + 1)).code == L.MPPI_E_ARG
    # reloading a loaded member replaces it: member 2 becomes net 1, the members 1 and 2 then agree
    eng.load_member(2, kind, blob1)
    eng.solve(x0, U0, seed=SEED)
    _eq(eng.member_costs(2, B0), eng.member_costs(1, B0), "the reloaded member")
    # off: load_dynamics is allowed again and frees the members behind member 0
    eng.set_ensemble(1)
    eng.load_dynamics(kind, blob1)
    assert eng.ensemble()["n_loaded"] == 1
    eng.close()

    # the CrossAttention net in split mode: refused, both setters named, nothing changed
    ca, _, _ = _setup(M, "ca", (0,), precision=2)
    e = _code(M, lambda: ca.load_member(1, *_blob(M, "ca", 0)))
    assert e.code == L.MPPI_E_UNSUPPORTED and "mppi_load_member" in str(e) and "mppi_set_ensemble" in str(e)
    assert ca.ensemble()["n_loaded"] == 1 and _code(M, lambda: ca.set_ensemble(2)).code == L.MPPI_E_ARG
    ca.close()

    # a change destroys captured graphs and drops the prefetched noise; the value in effect keeps both
    eng, x0, U0 = _setup(M, "mlp", (0, 1))
    tx, tU, tu0, tc = _tensors(torch, eng, x0, U0)
    eng.set_ensemble(2, "mean", 0.0)
    eng.graph_capture(B0, 2, tx.data_ptr(), tU.data_ptr(), tu0.data_ptr(), seed=SEED)
    eng.graph_launch(sync=True)
    assert eng.get_seed_counter() == 2
    eng.set_ensemble(2, "mean", 0.0, 0)
    eng.graph_launch(sync=True)
    assert eng.get_seed_counter() == 4
    eng.set_ensemble(2, "worst", 0.0)
    assert _code(M, lambda: eng.graph_launch(sync=True)).code == L.MPPI_E_STATE
    assert eng.get_seed_counter() == 4  # the prefetch was dropped, the counter stepped back: no key skipped
    eng.close()


def test_a_chained_stream_whose_setting_changes_draws_the_loops_keys(M):
    """Chained solves under n = 1, 2 (MEAN_STD), 2 (WORST), 1 on one stream against the loop of plain counter solves
    with the same settings: the state, U, u0, costs and the counter."""
    import torch
    plan = ((1, "mean", 0.0), (2, "mean_std", 0.5), (2, "worst", 0.0), (1, "mean", 0.0))
    outs = []
    for chain in (True, False):
        eng, x0, U0 = _setup(M, "mlp", (0, 1))
        tx, tU, tu0, tc = _tensors(torch, eng, x0, U0)
        for n, mode, kappa in plan:
            eng.set_ensemble(n, mode, kappa)
            for _ in range(2):
                eng.solve_device(B0, tx.data_ptr(), tU.data_ptr(), None, seed=SEED, u0_ptr=tu0.data_ptr(),
                                 costs_ptr=tc.data_ptr(), shift=True, env_step=True, chain=chain,
                                 seed_counter=not chain, asynchronous=chain)
        outs.append((_snap(torch, tx, tU, tu0, tc), eng.get_seed_counter()))
        eng.close()
    assert outs[0][1] == 2 * len(plan)
    _eq(outs[0], outs[1], "chained, the setting changing mid-stream")
