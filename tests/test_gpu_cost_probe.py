"""The running costs of csrc/costs.h on designed states, through every fc rollout kernel that inlines them.
Needs an MI355X.

tests/cost_probe_cases.py builds probe nets whose next state is an exact, designed function of the sample's control
(MLP: x' = base + S u; folded cross-attention: x' = x + step), designed states that reach every branch of atan2_fast,
atan_cephes and asin_fast and move every gathered entry alone, and the float64 reference (oracle.mppi_ref.COSTS).  Every
designed value has at most 8 significant bits and the nets' weights are 0 and +-1, so precision 0, 1 and 2 hand the cost
the same fp32 state and are held to one bar: |cost - reference| <= 1e-5 x the sum of the reference's absolute terms
(the project's fp32 cost bar).  tests/test_cost_probe.py checks the premises on the CPU.

Each test prints "PROBE <what> <max error in units of the bar>"; DESIGN.md (section 0) records the figures.
"""
import numpy as np
import pytest

import cost_probe_cases as C
from oracle import mppi_ref as R

pytestmark = pytest.mark.gpu

KNOBS = ("MPPI_FC_GENERIC", "MPPI_FC_WAVE", "MPPI_X3M", "MPPI_X3M32", "MPPI_X3_TILES", "MPPI_X3_WAVE", "MPPI_X3_PAIR",
         "MPPI_X3D", "MPPI_X3H", "MPPI_X3H_NS", "MPPI_X3_F16", "MPPI_X3_F16_L2", "MPPI_X3_L1_TERMS")

# route -> (precision, routing knobs, the kernel family mppi_rollout_kernel must name) for MLPStatePredictor(., ., 128, 2)
# at the sweep's shape (4 solves of K = 1024: 256 sample tiles, below every batch threshold of fc_route.h, so the unforced
# routes are the M-split kernels).  MPPI_F32_STREAM is read once per process (fc_route.h) and cannot be flipped between
# tests of one process: the streamed fp32 kernel is left out.
MLP_ROUTES = {
    "f32": (0, {}, "fc_rollout_kernel_f32"),
    "bf16": (1, {}, "fc_rollout_kernel"),
    "bf16-wave0": (1, {"MPPI_FC_WAVE": "0"}, "fc_rollout_kernel"),
    "bf16-wave1": (1, {"MPPI_FC_WAVE": "1"}, "fc_wave_mlp_kernel<ns=1>"),
    "bf16-wave2": (1, {"MPPI_FC_WAVE": "2"}, "fc_wave_mlp_kernel<ns=2>"),
    "x3": (2, {}, "fc_rollout_kernel_x3w<l1=3>"),
    "x3-tiles1": (2, {"MPPI_X3_TILES": "1"}, "fc_rollout_kernel_x3<l1=3>"),
    "x3-tiles2": (2, {"MPPI_X3_TILES": "2"}, "fc_rollout_kernel_x3w<l1=3>"),
    "x3m": (2, {"MPPI_X3M": "1"}, "fc_wave_mlp_x3_kernel"),
    "x3m32": (2, {"MPPI_X3M32": "1"}, "fc_wave32_mlp_x3_kernel"),
    "generic-f32": (0, {"MPPI_FC_GENERIC": "1"}, "fc_generic_kernel"),
    "generic-bf16": (1, {"MPPI_FC_GENERIC": "1"}, "fc_generic_kernel"),
}
# the folded humanoid CA at K = 64, B = 1 (MPPI_FC_GENERIC is read when the net is loaded, the others per launch)
_F16, _B16 = {"MPPI_X3_F16": "1"}, {"MPPI_X3_F16": "0", "MPPI_X3_L1_TERMS": "3"}
_WAVE, _PAIR = {"MPPI_X3_WAVE": "2", "MPPI_X3_PAIR": "0"}, {"MPPI_X3_WAVE": "2", "MPPI_X3_PAIR": "1"}
CA_ROUTES = {
    "f32": (0, [({}, "fc_rollout_kernel_f32")]),
    "bf16": (1, [({}, "fc_rollout_kernel"), ({"MPPI_FC_WAVE": "1"}, "fc_wave_kernel<ns=1>"),
                 ({"MPPI_FC_WAVE": "2"}, "fc_wave_kernel<ns=2>"), ({"MPPI_FC_WAVE": "3"}, "fc_wave32_kernel")]),
    "x3": (2, [(_F16, "fc_rollout_kernel_x3h<f16>"), ({**_F16, "MPPI_X3H": "0"}, "fc_rollout_kernel_x3d<f16>"),
               ({"MPPI_X3_F16": "0", "MPPI_X3_L1_TERMS": "2"}, "fc_rollout_kernel_x3d<l1=2>"),
               (_B16, "fc_rollout_kernel_x3w<l1=3>"), ({**_B16, "MPPI_X3_TILES": "1"}, "fc_rollout_kernel_x3<l1=3>"),
               ({**_PAIR, **_F16}, "fc_wave32_x3p_kernel<f16>"), ({**_PAIR, **_B16}, "fc_wave32_x3p_kernel<l1=3>"),
               ({**_WAVE, **_F16}, "fc_wave32_x3_kernel<f16>"), ({**_WAVE, **_B16}, "fc_wave32_x3_kernel<l1=3>")]),
    "generic-f32": (0, [({"MPPI_FC_GENERIC": "1"}, "fc_generic_kernel")]),
    "generic-bf16": (1, [({"MPPI_FC_GENERIC": "1"}, "fc_generic_kernel")]),
}


@pytest.fixture(scope="module")
def M(gpu_available):
    import mppi_hip
    return mppi_hip


def _set_knobs(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _mlp_engine(M, monkeypatch, cost, route, K, H, B, **cfg):
    """An engine with the cost's probe MLP loaded under the route's knobs (left set: most are read per launch)."""
    from mppi_hip.nets import mlp_blob
    precision, env, kernel = MLP_ROUTES[route]
    c = C.sweep_case(cost)
    _set_knobs(monkeypatch, env)
    kw = dict(terminal_weight=0.0, ctrl_clamp=0.0)
    kw.update(cfg)
    eng = M.Engine(M.Config(nx=c["nx"], nu=c["nu"], H=H, K=K, max_batch=B, lambda_=1.0, sigma=1.0, precision=precision,
                            **kw))
    eng.load_dynamics(*mlp_blob(c["sd"], c["nx"], c["nu"])).set_cost(cost)
    return eng, kernel


def _in_bars(got, ref, scale):
    """|got - ref| in units of the bar (1e-5 x the reference's absolute terms); a non-finite cost counts as inf."""
    got = np.asarray(got, np.float64)
    return np.where(np.isfinite(got), np.abs(got - ref) / (C.BAR * scale), np.inf)


def _assert_bar(what, got, ref, scale):
    e = _in_bars(got, ref, scale)
    i = np.unravel_index(int(np.argmax(e)), e.shape)
    print(f"PROBE {what} {e.max():.3f}")
    assert e.max() <= 1.0, (f"{what}: {e.max():.3f} bars at {i}: got {np.asarray(got)[i]!r}, reference {ref[i]!r}, "
                            f"scale {scale[i]!r}; {int((e > 1).sum())} of {e.size} rows over the bar")
    return e


# ------------------------------------------------------------------------------------------------ the premise

@pytest.mark.parametrize("precision", [0, 1, 2])
@pytest.mark.parametrize("cost", ["humanoid_v3", "quad_jl"])
def test_env_step_lands_on_the_designed_state(M, monkeypatch, cost, precision):
    """The probe MLP on the device: an env step (shift, K = 16, H = 1, zero injected noise, so u0 = U[:, 0]) moves x0 to
    base + S u0 bit for bit at every precision, from designed states x0 that the net must cancel."""
    import torch
    from mppi_hip.nets import mlp_blob
    _set_knobs(monkeypatch, {})
    c = C.sweep_case(cost)
    nx, nu, B = c["nx"], c["nu"], 4
    rows = [3, 300, 700, 1000]
    x0 = np.ascontiguousarray(c["states"][2, rows])
    u0 = np.ascontiguousarray(c["u"][1, rows])
    want = np.ascontiguousarray(c["states"][1, rows])
    assert not np.array_equal(x0, want)
    dev = torch.device("cuda")
    eng = M.Engine(M.Config(nx=nx, nu=nu, H=1, K=16, max_batch=B, lambda_=1.0, sigma=1.0, terminal_weight=0.0,
                            precision=precision))
    try:
        eng.load_dynamics(*mlp_blob(c["sd"], nx, nu)).set_cost(cost)
        eng.set_stream(torch.cuda.current_stream().cuda_stream)
        tx = torch.from_numpy(x0.copy()).to(dev)
        tU = torch.from_numpy(u0.reshape(B, nu, 1).copy()).to(dev)
        tn = torch.zeros(B, nu, 1, 16, device=dev)
        tu0 = torch.zeros(B, nu, device=dev)
        eng.solve_device(B, tx.data_ptr(), tU.data_ptr(), tn.data_ptr(), seed=1, u0_ptr=tu0.data_ptr(), shift=True,
                         env_step=True, asynchronous=False)
        torch.cuda.synchronize()
        got, got_u0 = tx.cpu().numpy(), tu0.cpu().numpy()
    finally:
        eng.close()
    np.testing.assert_array_equal(got_u0, u0)
    np.testing.assert_array_equal(got, want)


# ------------------------------------------------------------------------------------------------ the sweep

@pytest.mark.parametrize("route", list(MLP_ROUTES))
@pytest.mark.parametrize("cost", list(C.DIMS))
def test_sweep(M, monkeypatch, cost, route):
    """4 x 1024 designed states at H = 1 (U = 0, injected noise, no terminal term, no clamp): every sample's cost
    within the bar of the float64 reference, on the kernel the route names.  The single-angle rows (one of roll, pitch,
    yaw alone, every other term at or near zero) are reported apart: there the bar holds the angle itself."""
    c = C.sweep_case(cost)
    B, K = C.SWEEP_B, C.SWEEP_K
    x0 = np.ascontiguousarray(c["states"][[1, 2, 3, 0], 7])  # designed states the net must cancel
    eng, kernel = _mlp_engine(M, monkeypatch, cost, route, K, 1, B)
    try:
        res = eng.solve(x0, np.zeros((B, c["nu"], 1), np.float32), noise=c["noise"], ctx=c["ctx"], want_weights=True)
        kern = eng.rollout_kernel()
    finally:
        eng.close()
    assert kern == kernel, kern
    assert res.status == 0
    e = _assert_bar(f"sweep {cost} {route}", res.costs, c["ref"], c["scale"])
    if cost.startswith("humanoid"):
        q = c["states"][0][:, 3:7]
        alone = ((q != 0).sum(axis=1) == 2) & (q[:, 0] != 0)
        assert alone.sum() >= 3 * C.MIN_ROWS
        print(f"PROBE sweep-single-angle {cost} {route} {e[0][alone].max():.3f}")
    for b in range(B):
        np.testing.assert_allclose(res.weights[b], R.softmin_weights(res.costs[b].astype(np.float64), 1.0), atol=1e-5)


@pytest.mark.parametrize("route", ["generic-f32", "generic-bf16"])
@pytest.mark.parametrize("cost", ["humanoid_v3", "quad_jl"])
def test_sweep_generic_with_pad_lanes(M, monkeypatch, cost, route):
    """The generic kernel at K = 75 (Kp = 80: five pad lanes in the last 16-sample group), 75 rows spread over each
    solve of the sweep."""
    c = C.sweep_case(cost)
    B, K = C.SWEEP_B, 75
    pick = (np.arange(K) * 13 + 5) % C.SWEEP_K
    x0 = np.ascontiguousarray(c["states"][[1, 2, 3, 0], 7])
    eng, kernel = _mlp_engine(M, monkeypatch, cost, route, K, 1, B)
    try:
        res = eng.solve(x0, np.zeros((B, c["nu"], 1), np.float32), noise=np.ascontiguousarray(c["noise"][..., pick]),
                        ctx=c["ctx"])
        kern = eng.rollout_kernel()
    finally:
        eng.close()
    assert kern == kernel, kern
    assert res.costs.shape == (B, K) and res.status == 0
    _assert_bar(f"sweep-K75 {cost} {route}", res.costs, c["ref"][:, pick], c["scale"][:, pick])


# ------------------------------------------------------------------------------------- steps and the terminal term

@pytest.mark.parametrize("route", ["f32", "generic-f32", "bf16", "bf16-wave1", "x3", "x3m"])
@pytest.mark.parametrize("H", [101, 50])
def test_steps_and_terminal_term(M, monkeypatch, H, route):
    """humanoid_v1 over H steps with terminal_weight 2 and another designed state at every (step, sample): the summed
    reference takes the left foot while t mod 100 < 50 and passes t = H, zero control, to the terminal term.  The
    context's feet differ and every sample stands far from one foot around the switches, so a step index off by one at
    50 or 100 moves the cost by thousands of bars (tests/test_cost_probe.py checks that); H = 50 adds the case where H
    and H - 1 fall on different feet in the terminal term.  Default route and one per-wave route per precision (fp32
    has no per-wave kernel: the generic kernel stands in)."""
    s = C.steps_case(H)
    K = s["K"]
    eng, kernel = _mlp_engine(M, monkeypatch, "humanoid_v1", route, K, H, 1, terminal_weight=s["terminal_weight"])
    try:
        res = eng.solve(s["x0"], np.zeros((21, H), np.float32), noise=s["noise"], ctx=s["ctx"][None])
        kern = eng.rollout_kernel()
    finally:
        eng.close()
    assert kern == kernel, kern
    assert res.status == 0
    _assert_bar(f"steps H={H} {route}", res.costs, s["ref"], s["scale"])


# ------------------------------------------------------------------------------------------------ ctrl_clamp

@pytest.mark.parametrize("route", ["f32", "bf16", "bf16-wave1", "x3", "x3m", "generic-bf16"])
def test_ctrl_clamp_saturates_state_and_control_term(M, monkeypatch, route):
    """ctrl_clamp = 0.75 with designed controls beyond it (most are): the state the cost sees is base + S clip(u) and
    the control term uses clip(u), as oracle.mppi_ref.rollout clips."""
    cost, clamp, b = "humanoid_v3", 0.75, 1
    c = C.sweep_case(cost)
    K = C.SWEEP_K
    noise = c["noise"][b]
    assert (np.abs(noise) > clamp).mean() > 0.5
    x0 = c["states"][2, 11]
    ref, scale = C.rollout_reference(cost, C.probe_dynamics(c["base"], c["S"]), x0, np.zeros((c["nu"], 1)), noise,
                                     c["ctx"][b], ctrl_clamp=clamp)
    unclamped = c["ref"][b]
    assert (np.abs(unclamped - ref) > 100 * C.BAR * scale).mean() > 0.9  # ignoring the clamp would show
    eng, kernel = _mlp_engine(M, monkeypatch, cost, route, K, 1, 1, ctrl_clamp=clamp)
    try:
        res = eng.solve(x0, np.zeros((c["nu"], 1), np.float32), noise=noise, ctx=c["ctx"][b][None])
        kern = eng.rollout_kernel()
    finally:
        eng.close()
    assert kern.split("<")[0] == kernel.split("<")[0], kern
    _assert_bar(f"clamp {route}", res.costs, ref, scale)


# ------------------------------------------------------------------------------------------------ CA-only kernels

@pytest.mark.parametrize("i", range(len(C.CA_STATES)))
@pytest.mark.parametrize("group", list(CA_ROUTES))
def test_ca_kernels(M, monkeypatch, group, i):
    """The kernels only the folded cross-attention net reaches, on the CA probe (x' = x + step: designed states i and
    i + 1 at t = 1, 2, and state i + 1 again in the terminal term, for every sample): K = 64, H = 2, B = 1,
    terminal_weight 2, both humanoid costs, every kernel of the precision forced by its knobs and named.  The 64
    samples differ by their control terms only."""
    from mppi_hip.nets import cross_attention_blob
    precision, arms = CA_ROUTES[group]
    K, H, tw = 64, 2, 2.0
    case = C.ca_case(i)
    step64 = case["step"].astype(np.float64)
    rs = np.random.RandomState(40 + i)
    noise = (rs.randint(-C.QMAX, C.QMAX + 1, (21, H, K)) / C.GRID).astype(np.float32)
    dyn = lambda x, u: x + step64[None, :]
    _set_knobs(monkeypatch, arms[0][0] if group.startswith("generic") else {})
    eng = M.Engine(M.Config(nx=55, nu=21, H=H, K=K, max_batch=1, lambda_=1.0, sigma=1.0, terminal_weight=tw,
                            precision=precision))
    worst = 0.0
    try:
        eng.load_dynamics(*cross_attention_blob(C.probe_ca(case["step"])))
        for cost in ("humanoid_v3", "humanoid_v1"):
            ctx = C.CONTEXTS[cost][1 + i % 3].astype(np.float32)
            ref, scale = C.rollout_reference(cost, dyn, case["x0"], np.zeros((21, H)), noise, ctx, terminal_weight=tw)
            assert len(np.unique(ref)) == K
            eng.set_cost(cost)
            for env, kernel in arms:
                _set_knobs(monkeypatch, env)
                res = eng.solve(case["x0"], np.zeros((21, H), np.float32), noise=noise, ctx=ctx[None])
                kern = eng.rollout_kernel()
                assert kern == kernel, (kern, kernel)
                e = _in_bars(res.costs, ref, scale)
                worst = max(worst, float(e.max()))
                assert e.max() <= 1.0, f"{kernel} {cost} state {i}: {e.max():.3f} bars; got {res.costs[:4]}, ref {ref[:4]}"
    finally:
        eng.close()
    print(f"PROBE ca {group} state {i} {worst:.3f}")


# --------------------------------------------------------------------------------------- a non-finite sample

@pytest.mark.parametrize("bad", [np.nan, np.inf], ids=["nan", "inf"])
@pytest.mark.parametrize("route", list(MLP_ROUTES))
def test_nonfinite_sample_poisons_only_itself(M, monkeypatch, route, bad):
    """One designed control of one sample is NaN (or +inf) at the middle step of H = 3: that sample's cost is non-finite
    and its weight 0, every other sample's cost is bitwise the cost of the same solve without it, and the solve's
    status stays clear (it still has finite costs)."""
    cost, K, H, k_bad, t_bad, u_bad = "humanoid_v3", 64, 3, 37, 1, 4
    c = C.sweep_case(cost)
    rs = np.random.RandomState(5)
    pool = c["u"][1:].reshape(-1, c["nu"])
    clean = np.ascontiguousarray(pool[rs.randint(0, len(pool), (H, K))].transpose(2, 0, 1))
    dirty = clean.copy()
    dirty[u_bad, t_bad, k_bad] = bad
    ctx = c["ctx"][2][None]
    x0 = c["states"][3, 9]
    eng, kernel = _mlp_engine(M, monkeypatch, cost, route, K, H, 1, terminal_weight=1.0)
    try:
        U = np.zeros((c["nu"], H), np.float32)
        a = eng.solve(x0, U, noise=clean, ctx=ctx, want_weights=True)
        b = eng.solve(x0, U, noise=dirty, ctx=ctx, want_weights=True)
        kern = eng.rollout_kernel()
    finally:
        eng.close()
    assert kern.split("<")[0] == kernel.split("<")[0], kern
    assert np.isfinite(a.costs).all() and a.status == 0
    assert not np.isfinite(b.costs[k_bad]) and b.weights[k_bad] == 0.0
    others = np.arange(K) != k_bad
    np.testing.assert_array_equal(b.costs[others], a.costs[others])
    assert b.status == 0
    np.testing.assert_allclose(b.weights.sum(), 1.0, atol=1e-5)
    w = R.softmin_weights(np.where(others, a.costs.astype(np.float64), np.inf), 1.0)
    np.testing.assert_allclose(b.weights, w, atol=1e-5)


@pytest.mark.parametrize("bad", [np.nan, np.inf], ids=["nan", "inf"])
@pytest.mark.parametrize("group", list(CA_ROUTES))
def test_nonfinite_sample_poisons_only_itself_ca(M, monkeypatch, group, bad):
    """The same on the folded humanoid cross-attention net (the shipped checkpoint, K = 64, B = 1 as the CA sweep), on
    every kernel of CA_ROUTES: one control of one sample is NaN (or +inf) at the middle step of H = 3."""
    from conftest import golden, golden_sd
    from mppi_hip.nets import cross_attention_blob
    precision, arms = CA_ROUTES[group]
    K, H, k_bad, t_bad, u_bad = 64, 3, 37, 1, 4
    rs = np.random.RandomState(6)
    clean = (0.75 * rs.randn(21, H, K)).astype(np.float32)
    dirty = clean.copy()
    dirty[u_bad, t_bad, k_bad] = bad
    x0 = golden("g5_ca_humanoid_fwd.npz")["x0_stride20"][3].astype(np.float32)
    U = (0.1 * rs.randn(21, H)).astype(np.float32)
    others = np.arange(K) != k_bad
    _set_knobs(monkeypatch, arms[0][0] if group.startswith("generic") else {})
    eng = M.Engine(M.Config(nx=55, nu=21, H=H, K=K, max_batch=1, lambda_=1.0, sigma=1.0, terminal_weight=1.0,
                            precision=precision))
    try:
        eng.load_dynamics(*cross_attention_blob(golden_sd("ca_humanoid_weights.npz"))).set_cost("humanoid_v3")
        for env, kernel in arms:
            _set_knobs(monkeypatch, env)
            a = eng.solve(x0, U, noise=clean, want_weights=True)
            b = eng.solve(x0, U, noise=dirty, want_weights=True)
            kern = eng.rollout_kernel()
            assert kern == kernel, (kern, kernel)
            assert np.isfinite(a.costs).all() and a.status == 0
            assert not np.isfinite(b.costs[k_bad]) and b.weights[k_bad] == 0.0, kernel
            np.testing.assert_array_equal(b.costs[others], a.costs[others], err_msg=kernel)
            assert b.status == 0
            np.testing.assert_allclose(b.weights.sum(), 1.0, atol=1e-5)
            w = R.softmin_weights(np.where(others, a.costs.astype(np.float64), np.inf), 1.0)
            np.testing.assert_allclose(b.weights, w, atol=1e-5)
    finally:
        eng.close()
