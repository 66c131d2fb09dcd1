"""Every state and control slot of the fc rollouts, exactly, on every route.  Needs an MI355X.

tests/slot_probe_cases.py builds the rotation probe (an MLPStatePredictor with weights 0 / +-1 whose residual dynamics
are x' = P x + S u: the state rotates through the entries the cost reads and every control lands in a state entry), its
designed inputs at the shapes where the 64 + 32 slot layout changes (nx below, at and above the 32-slot split, next to
and beyond the bias pair of the per-wave MLP kernels, nu from 1 to 32) and the float64 reference.  Every value formed on
the way has 8 significant bits, so precision 0, 1 and 2 are held to one bar of the cost probe (|cost - reference| <=
1e-5 x the reference's absolute terms), while a dropped, exchanged or shifted slot moves some sample by 100 bars or
more (tests/test_slot_probe.py holds both premises on the CPU).  The folded cross-attention net ignores the action;
its control slots are held through the control term of humanoid_v3 at nu = 1 .. 32.

Each test prints "PROBE <what> <max error in units of the bar>"; DESIGN.md (section 0) records the figures.
"""
import numpy as np
import pytest

import slot_probe_cases as S
from oracle import mppi_ref as R
from test_gpu_cost_probe import CA_ROUTES, KNOBS, MLP_ROUTES, _assert_bar, _in_bars, _set_knobs  # noqa: F401

pytestmark = pytest.mark.gpu

SHAPE_IDS = [S.shape_id(s) for s in S.SHAPES]
K_PITCH = 64  # csrc/mppi_internal.h kKpAlign: the device pitch of the sample axis
# the knobs that pick a kernel family (the others pick the split CA's numeric form, which every fallback keeps)
ROUTING = ("MPPI_FC_WAVE", "MPPI_X3_WAVE", "MPPI_X3_PAIR", "MPPI_X3M", "MPPI_X3M32")
# csrc/fc_route.h fc_route_can_run, for the per-wave MLP kernels: the bias pair sits in state slots 62 and 63; the
# 32-sample forms (and the bf16 kernel, whose waves pair two tiles of one solve) need whole 32-sample wave-tiles
MLP_GATES = {"fc_wave_mlp_kernel": lambda nx, Kp: nx <= 62 and Kp % 32 == 0,
             "fc_wave_mlp_x3_kernel": lambda nx, Kp: nx <= 62,
             "fc_wave32_mlp_x3_kernel": lambda nx, Kp: nx <= 62 and Kp % 32 == 0}
# ... and for the per-wave CA kernels: the control slots their operands hold
CA_GATES = {"fc_wave_kernel": lambda nu: nu <= 24, "fc_wave32_kernel": lambda nu: 20 <= nu <= 22,
            "fc_wave32_x3_kernel": lambda nu: 20 <= nu <= 22, "fc_wave32_x3p_kernel": lambda nu: 20 <= nu <= 22}
# MPPI_FC_WAVE=3 asks for two tiles per wave, on 32x32x16 MFMAs where that variant applies: where it does not, the
# knob still holds two tiles per wave on fc_wave_kernel if that kernel can run the shape
CA_NEXT = {"fc_wave32_kernel": "fc_wave_kernel<ns=2>"}


@pytest.fixture(scope="module")
def M(gpu_available):
    import mppi_hip
    return mppi_hip


def _family(kernel: str) -> str:
    return kernel.split("<")[0]


def _mlp_solve(M, monkeypatch, c, precision, env):
    """Both solves of a rotation case on a fresh engine under `env`; (result, kernel name)."""
    from mppi_hip.nets import mlp_blob
    _set_knobs(monkeypatch, env)
    eng = M.Engine(M.Config(nx=c["nx"], nu=c["nu"], H=c["H"], K=S.K, max_batch=S.B, lambda_=1.0, sigma=1.0,
                            terminal_weight=0.0, ctrl_clamp=0.0, precision=precision))
    try:
        eng.load_dynamics(*mlp_blob(c["sd"], c["nx"], c["nu"])).set_cost(S.COST)
        res = eng.solve(c["x0"], c["U0"], noise=c["noise"], ctx=c["ctx"], want_weights=True)
        return res, eng.rollout_kernel()
    finally:
        eng.close()


@pytest.mark.parametrize("route", list(MLP_ROUTES))
@pytest.mark.parametrize("shape", S.SHAPES, ids=SHAPE_IDS)
def test_mlp_slots(M, monkeypatch, shape, route):
    """The rotation probe (B = 2, K = 90, H = nx + 2, quad_est with goal 0 and no terminal term): every sample's cost
    within one bar of the float64 reference, the weights the softmin of the engine's own costs, on the kernel the route
    names where that kernel can hold the shape, and on the engine's unforced choice for the precision where it cannot
    (nx = 63, 64 under the per-wave knobs: state slots 62 and 63 are those kernels' bias pair)."""
    nx, nu = shape
    c = S.mlp_case(nx, nu)
    precision, env, kernel = MLP_ROUTES[route]
    gate = MLP_GATES.get(_family(kernel))
    Kp = -(-S.K // K_PITCH) * K_PITCH
    if gate is not None and not gate(nx, Kp):
        _, kernel = _mlp_solve(M, monkeypatch, c, precision, {k: v for k, v in env.items() if k not in ROUTING})
        assert _family(kernel) not in MLP_GATES, kernel
    res, kern = _mlp_solve(M, monkeypatch, c, precision, env)
    assert kern == kernel, (kern, kernel)
    assert res.status == 0
    assert res.costs.shape == (S.B, S.K)
    _assert_bar(f"slots {S.shape_id(shape)} {route}", res.costs, c["ref"], c["scale"])
    for b in range(S.B):
        np.testing.assert_allclose(res.weights[b], R.softmin_weights(res.costs[b].astype(np.float64), 1.0), atol=1e-5)


@pytest.mark.parametrize("precision", [0, 1, 2])
@pytest.mark.parametrize("shape", S.SHAPES, ids=SHAPE_IDS)
def test_mlp_env_step_moves_every_slot(M, monkeypatch, shape, precision):
    """The rotation probe on the device: an env step (shift, K = 16, H = 1, zero injected noise, so u0 = U[:, 0]) moves
    x0 to P x0 + S u0 bit for bit at every precision, with every control slot nonzero, and returns u0 unchanged."""
    import torch
    from mppi_hip.nets import mlp_blob
    _set_knobs(monkeypatch, {})
    nx, nu = shape
    c = S.mlp_case(nx, nu)
    i = np.arange(nu)
    u0 = np.stack([np.where((i + b) % 2 == 0, 1, -1) * (3 + (5 * i + 4 * b) % 13) for b in range(S.B)]) / S.GRID
    want = c["x0"].astype(np.float64) @ c["P"].T + u0 @ c["S"].T
    u0, want = u0.astype(np.float32), want.astype(np.float32)
    assert (want != c["x0"]).any(axis=1).all() and (u0 != 0).all()
    dev = torch.device("cuda")
    eng = M.Engine(M.Config(nx=nx, nu=nu, H=1, K=16, max_batch=S.B, lambda_=1.0, sigma=1.0, terminal_weight=0.0,
                            precision=precision))
    try:
        eng.load_dynamics(*mlp_blob(c["sd"], nx, nu)).set_cost(S.COST)
        eng.set_stream(torch.cuda.current_stream().cuda_stream)
        tx = torch.from_numpy(c["x0"].copy()).to(dev)
        tU = torch.from_numpy(u0.reshape(S.B, nu, 1).copy()).to(dev)
        tn = torch.zeros(S.B, nu, 1, 16, device=dev)
        tu0 = torch.zeros(S.B, nu, device=dev)
        eng.solve_device(S.B, tx.data_ptr(), tU.data_ptr(), tn.data_ptr(), seed=1, u0_ptr=tu0.data_ptr(), shift=True,
                         env_step=True, asynchronous=False)
        torch.cuda.synchronize()
        got, got_u0 = tx.cpu().numpy(), tu0.cpu().numpy()
    finally:
        eng.close()
    np.testing.assert_array_equal(got_u0, u0)
    np.testing.assert_array_equal(got, want)


CA_ARMS = [(group, i) for group, (_, arms) in CA_ROUTES.items() for i in range(len(arms))]


def _ca_solve(M, monkeypatch, c, precision, env):
    from mppi_hip.nets import cross_attention_blob
    _set_knobs(monkeypatch, env)  # (MPPI_FC_GENERIC is read when the net is loaded, the others per launch)
    eng = M.Engine(M.Config(nx=55, nu=c["nu"], H=S.CA_H, K=S.CA_K, max_batch=1, lambda_=1.0, sigma=1.0,
                            terminal_weight=0.0, precision=precision))
    try:
        eng.load_dynamics(*cross_attention_blob(c["sd"])).set_cost(S.CA_COST)
        res = eng.solve(c["x0"], c["U"], noise=c["noise"], ctx=c["ctx"][None])
        return res, eng.rollout_kernel()
    finally:
        eng.close()


@pytest.mark.parametrize("nu", [19, 25])
def test_ca_split_solves_unforced_outside_the_humanoid_nu(M, monkeypatch, nu):
    """Precision 2 with no knob at all, at a control count fc_wave32_x3p_kernel cannot hold: the engine's probe of
    the loaded net leaves that kernel out and measures the fp16 form on fc_rollout_kernel_x3h alone (it used to launch
    it regardless, and the first solve failed with "x3 layer-1 probe: invalid argument"), and the solve holds the bar."""
    from mppi_hip.nets import cross_attention_blob
    c = S.ca_case(nu)
    _set_knobs(monkeypatch, {})
    eng = M.Engine(M.Config(nx=55, nu=nu, H=S.CA_H, K=S.CA_K, max_batch=1, lambda_=1.0, sigma=1.0,
                            terminal_weight=0.0, precision=2))
    try:
        eng.load_dynamics(*cross_attention_blob(c["sd"])).set_cost(S.CA_COST)
        res = eng.solve(c["x0"], c["U"], noise=c["noise"], ctx=c["ctx"][None])
        kern, (terms, l1_err), (form, f16_err) = eng.rollout_kernel(), eng.x3_layer1(), eng.x3_f16()
    finally:
        eng.close()
    assert res.status == 0
    assert terms in (2, 3) and l1_err >= 0 and f16_err >= 0, (terms, l1_err, form, f16_err)  # both probes ran
    assert _family(kern) in ("fc_rollout_kernel_x3h", "fc_rollout_kernel_x3d", "fc_rollout_kernel_x3w"), kern
    assert (_family(kern) == "fc_rollout_kernel_x3h") == (form >= 1), (kern, form)
    _assert_bar(f"ca-slots-unforced nu={nu} {kern}", res.costs, c["ref"], c["scale"])


@pytest.mark.parametrize("group,i", CA_ARMS, ids=[f"{g}-{i}" for g, i in CA_ARMS])
@pytest.mark.parametrize("nu", S.CA_NUS)
def test_ca_control_slots(M, monkeypatch, nu, group, i):
    """The folded humanoid CA with nu controls (x' = x + step from a designed state, K = 64, B = 1, H = 3, one-hot
    noise over (control slot, step) on a nominal U, humanoid_v3 without a terminal term): every cost within one bar of
    the float64 reference on every arm of CA_ROUTES; the arm's kernel is named where its operands hold nu controls
    (fc_wave_kernel: nu <= 24; the 32-sample kernels: 20 <= nu <= 22), and elsewhere the engine's choice with the
    routing knobs unset (the forced numeric form kept)."""
    c = S.ca_case(nu)
    precision, arms = CA_ROUTES[group]
    env, kernel = arms[i]
    gate = CA_GATES.get(_family(kernel))
    if gate is not None and not gate(nu):
        nxt = CA_NEXT.get(_family(kernel))
        if nxt is not None and CA_GATES[_family(nxt)](nu):
            kernel = nxt
        else:
            _, kernel = _ca_solve(M, monkeypatch, c, precision, {k: v for k, v in env.items() if k not in ROUTING})
            assert _family(kernel) not in CA_GATES, kernel
    res, kern = _ca_solve(M, monkeypatch, c, precision, env)
    assert kern == kernel, (kern, kernel)
    assert res.status == 0
    _assert_bar(f"ca-slots nu={nu} {group}-{i} {kern}", res.costs, c["ref"], c["scale"])
