"""The split mode's fp16 form (MPPI_PREC_BF16X3, fc_route.h x3_f16_on) on states its probe never saw. Needs an MI355X.

The form is accepted per loaded net by the engine's probe (mppi_api.hip x3_probe) on up to 64 states of the FIRST
solve; an MPPI handle then solves other states for the rest of its life.  Here one engine probes on logged states and
then solves a different batch, and every solve of that batch is held to the mode's documented bar: costs within rtol
1e-4 of the fp32 oracle.  The CA surrogate ignores the action, so the form's error is one number per state: many states
(16 per set), few samples (K = 64), config #4's horizon (H = 64, where the error peaks: it grows with the steps).

State sets (16 states each, built from tests/golden/g5_ca_humanoid_fwd.npz x0_stride20 and the fp32 oracle dynamics):
  late    logged 48..63
  jitter  logged 8..23 + 0.5 randn (RandomState(7)): joint and velocity excursions
  drift   logged 0..15 after 256 zero-action steps of the fp32 oracle surrogate (the net's own trajectory)
Arms: every kernel that can run the fp16 form, reached as tests/test_gpu_fullsize.py reaches them.

A CPU emulation of the form (tools/x3_error_budget.py, schemes f16x2w,f16x1,f16x2w) puts these sets at 2.6e-5 ..
7.8e-5 of the fp32 path; DESIGN.md §4 holds the GPU figures each case prints.
"""
import os

import numpy as np
import pytest

from conftest import golden, golden_sd
from oracle import mppi_ref as R
from oracle import nets_ref as N

pytestmark = pytest.mark.gpu

K, H, B, NU, NX = 64, 64, 16, 21, 55
BAR = 1e-4         # MPPI_PREC_BF16X3: costs against the fp32 oracle (include/mppi.h)
PROBE_TOL = 7.5e-5  # fc_route.h kX3ProbeTol

ARMS = {  # arm -> (routing knobs, the kernel's name in its fp16 form)
    "x3h": ({}, "fc_rollout_kernel_x3h<f16>"),
    "x3d": ({"MPPI_X3H": "0"}, "fc_rollout_kernel_x3d<f16>"),
    "x3p": ({"MPPI_X3_WAVE": "2", "MPPI_X3_PAIR": "1"}, "fc_wave32_x3p_kernel<f16>"),
    "x3_wave32": ({"MPPI_X3_WAVE": "2", "MPPI_X3_PAIR": "0"}, "fc_wave32_x3_kernel<f16>"),
}
SETS = ("late", "jitter", "drift")


@pytest.fixture(scope="module")
def M(gpu_available):
    import mppi_hip
    return mppi_hip


def _ctx(b):
    """tests/test_gpu_fullsize.py's per-solve real-env context."""
    return R.humanoid_context(swing_foot_x=-0.2 + 0.1 * b, swing_knee_x=0.05 * b, swing_vx=0.3 - 0.05 * b,
                              foot_clearance=0.01 * b, leg_clearance=-0.02 if b % 2 else 0.1)


def _v1_ctx(b):
    return R.humanoid_v1_context([0.05 * b, 0.1, 0.0], [-0.05, -0.1, 0.0], [1.0 + 0.1 * b, 0.2, 1.28])


@pytest.fixture(scope="module")
def case(M):
    """Inputs shared by every test, and the fp32 oracle's costs, computed once per state set and left unchanged."""
    sd = golden_sd("ca_humanoid_weights.npz")
    dyn = N.learned_dynamics(N.ca_fold(sd, 28, 27, 21), NX, "fp32")
    logged = golden("g5_ca_humanoid_fwd.npz")["x0_stride20"].astype(np.float32)
    drift = logged[:B].copy()
    zero_u = np.zeros((B, NU), np.float32)
    for _ in range(256):
        drift = dyn(drift, zero_u).astype(np.float32)
    states = {
        "probe": logged[:B],
        "late": logged[48:64],
        "jitter": (logged[8:24] + 0.5 * np.random.RandomState(7).randn(B, NX)).astype(np.float32),
        "drift": drift,
    }
    rs = np.random.RandomState(61)
    U0 = (0.1 * rs.randn(B, NU, H)).astype(np.float32)
    noise = (0.75 * rs.randn(B, NU, H, K)).astype(np.float32)
    ctx = np.stack([_ctx(b % 8) for b in range(B)]).astype(np.float32)
    ctx_v1 = np.stack([_v1_ctx(b) for b in range(B)]).astype(np.float32)
    cfg = M.Config.preset("humanoid_v3", K=K, H=H)
    pre = R.Preset("offprobe", K=K, H=H, lam=cfg.lambda_, sigma=0.75, terminal_weight=cfg.terminal_weight)

    def oracle(x0, cfun, cx):
        return np.stack([R.rollout(pre, dyn, cfun, x0[b], U0[b], noise[b], ctx=cx[b], dtype=np.float32)
                         for b in range(B)])

    ref = {name: oracle(x, R.humanoid_v3_cost, ctx) for name, x in states.items()}
    ref["probe_v1"] = oracle(states["probe"], R.humanoid_v1_cost, ctx_v1)
    for r in ref.values():
        assert np.isfinite(r).all()
        r.setflags(write=False)
    return dict(sd=sd, states=states, U0=U0, noise=noise, ctx=ctx, ctx_v1=ctx_v1, pre=pre, ref=ref)


def _engine(M, sd, cost="humanoid_v3"):
    from mppi_hip.nets import cross_attention_blob
    eng = M.Engine(M.Config.preset("humanoid_v3", K=K, H=H, precision=2, max_batch=B))
    eng.load_dynamics(*cross_attention_blob(sd)).set_cost(cost)
    return eng


def _worst(costs, ref):
    """(max relative error over solves and samples, its solve index); a non-finite cost counts as inf."""
    rel = np.where(np.isfinite(costs), np.abs(costs.astype(np.float64) - ref) / np.abs(ref), np.inf)
    b = int(np.argmax(rel.max(axis=1)))
    return float(rel[b].max()), b


def _assert_bar(res, ref, pre, what):
    worst, b = _worst(res.costs, ref)
    print(f"{what}: worst rel err {worst:.3e} at state {b}")
    assert np.isfinite(res.costs).all(), f"{what}: non-finite costs (first at state {b})"
    assert worst <= BAR, f"{what}: worst rel err {worst:.3e} at state {b} (bar {BAR:g})"
    for s in range(len(ref)):
        w_own = R.softmin_weights(res.costs[s].astype(np.float64), pre.lam)
        np.testing.assert_allclose(res.weights[s], w_own, atol=1e-5, err_msg=f"{what}: weights of solve {s}")
    return worst


@pytest.mark.parametrize("probe_B", [16, 1])
@pytest.mark.parametrize("name", SETS)
@pytest.mark.parametrize("arm", list(ARMS))
def test_fp16_form_holds_off_probe(M, case, monkeypatch, arm, name, probe_B):
    """One handle: the first solve (logged states [:probe_B]) is the probe's batch and runs the arm's kernel in its
    fp16 form; the second solve, all 16 states of the set, must still meet the fp32 bar on every solve.  Which kernel
    form the second solve runs is the engine's business (it may keep the fp16 form or take a bf16 one)."""
    env, kernel = ARMS[arm]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    c = case
    eng = _engine(M, c["sd"])
    try:
        p = probe_B
        first = eng.solve(c["states"]["probe"][:p], c["U0"][:p], noise=c["noise"][:p], ctx=c["ctx"][:p],
                          want_weights=True)
        kern, (f16, err) = eng.rollout_kernel(), eng.x3_f16()
        assert kern == kernel, kern
        assert f16 == 1 and 0.0 <= err <= PROBE_TOL, (f16, err)
        second = eng.solve(c["states"][name], c["U0"], noise=c["noise"], ctx=c["ctx"], want_weights=True)
        kern2 = eng.rollout_kernel()
    finally:
        eng.close()
    _assert_bar(first, c["ref"]["probe"][:p], c["pre"], f"{arm} probe batch [:{p}] (probe {err:.2e})")
    _assert_bar(second, c["ref"][name], c["pre"], f"{arm} {name} probe_B={p} ({kern2})")


def test_set_cost_reprobes(M, case):
    """The probe measures a relative COST error, under the cost set at that moment: mppi_set_cost returns the handle to
    "not probed" (mppi_x3_layer1 products 0, as after mppi_load_dynamics) and the next solve probes again under the new
    cost; its costs meet the bar against the oracle with that cost on every solve."""
    c = case
    x0 = c["states"]["probe"]
    eng = _engine(M, c["sd"])
    try:
        assert eng.x3_layer1()[0] == 0
        res3 = eng.solve(x0, c["U0"], noise=c["noise"], ctx=c["ctx"], want_weights=True)
        l1, f16 = eng.x3_layer1(), eng.x3_f16()
        assert l1[0] in (2, 3) and l1[1] >= 0.0 and f16[1] >= 0.0, (l1, f16)
        eng.set_cost("humanoid_v1")
        assert eng.x3_layer1()[0] == 0, eng.x3_layer1()
        res1 = eng.solve(x0, c["U0"], noise=c["noise"], ctx=c["ctx_v1"], want_weights=True)
        l1_v1, f16_v1 = eng.x3_layer1(), eng.x3_f16()
    finally:
        eng.close()
    assert l1_v1[0] in (2, 3) and l1_v1[1] >= 0.0 and f16_v1[1] >= 0.0, (l1_v1, f16_v1)
    _assert_bar(res3, c["ref"]["probe"], c["pre"], "humanoid_v3 before set_cost")
    _assert_bar(res1, c["ref"]["probe_v1"], c["pre"], "humanoid_v1 after set_cost")


def test_set_cost_makes_captured_graphs_stale(M, case):
    """A graph captured on a probed split-mode handle holds the probe's decision (and the cost) in its kernels:
    mppi_set_cost destroys it, as mppi_set_noise_model does; the next capture probes again and launches."""
    import torch
    from mppi_hip import _lib as L
    c = case
    n, Bg = 2, 2
    dev = torch.device("cuda")
    eng = _engine(M, c["sd"])
    try:
        eng.set_stream(torch.cuda.current_stream().cuda_stream)
        tx = torch.from_numpy(c["states"]["probe"][:Bg].copy()).to(dev)
        tU = torch.from_numpy(c["U0"][:Bg].copy()).to(dev)
        tu0 = torch.zeros(Bg, NU, device=dev)
        eng.graph_capture(Bg, n, tx.data_ptr(), tU.data_ptr(), tu0.data_ptr(), seed=3)
        assert eng.x3_layer1()[0] in (2, 3)  # probed before the capture
        eng.graph_launch(sync=True)
        eng.set_cost("humanoid_v1")
        assert eng.x3_layer1()[0] == 0
        with pytest.raises(M.MPPIError) as ei:
            eng.graph_launch(sync=True)
        assert ei.value.code == L.MPPI_E_STATE and "mppi_graph_capture first" in str(ei.value)
        eng.graph_capture(Bg, n, tx.data_ptr(), tU.data_ptr(), tu0.data_ptr(), seed=3)
        assert eng.x3_layer1()[0] in (2, 3)
        eng.graph_launch(sync=True)
        assert np.isfinite(tx.cpu().numpy()).all()
    finally:
        eng.close()


def test_wave32_fp16_form_at_full_horizon(M, case):
    """fc_wave32_x3_kernel's fp16 form at H = 64 (it runs where config #4's 32-solve shard lands, fc_route.h BOUNDARY;
    the probe checks fc_wave32_x3p_kernel and fc_rollout_kernel_x3h, never this kernel): within 1e-4 of the fp32 oracle
    on every one of 16 logged states, and within 8e-5 of fc_wave32_x3p_kernel on the same inputs (the bound the fp16
    kernels hold among themselves, test_split_x3d_kernel_matches_x3w_and_oracle)."""
    c = case
    x0 = c["states"]["probe"]
    out = {}
    for arm in ("x3_wave32", "x3p"):
        env, kernel = ARMS[arm]
        os.environ.update(env)
        try:
            eng = _engine(M, c["sd"])
            out[arm] = eng.solve(x0, c["U0"], noise=c["noise"], ctx=c["ctx"], want_weights=True)
            kern, f16 = eng.rollout_kernel(), eng.x3_f16()
            eng.close()
        finally:
            for v in env:
                os.environ.pop(v, None)
        assert kern == kernel and f16[0] == 1, (kern, f16)
    _assert_bar(out["x3_wave32"], c["ref"]["probe"], c["pre"], "x3_wave32 logged [:16]")
    _assert_bar(out["x3p"], c["ref"]["probe"], c["pre"], "x3p logged [:16]")
    between, b = _worst(out["x3_wave32"].costs, out["x3p"].costs.astype(np.float64))
    print(f"x3_wave32 vs x3p: worst rel diff {between:.3e} at state {b}")
    assert between <= 8e-5, f"x3_wave32 vs x3p: worst rel diff {between:.3e} at state {b}"
