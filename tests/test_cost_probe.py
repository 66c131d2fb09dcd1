"""The cost probe's premises, on the CPU (tests/cost_probe_cases.py; the kernels run it in tests/test_gpu_cost_probe.py).

The probe nets realise x' = base + S u (MLP) and x' = x + step (cross-attention) bit for bit in every restatement of
the nets the oracle has, the designed states cover every branch of the cost's trigonometry with at least MIN_ROWS rows,
and every trig argument is exact in float32, so the float64 reference and an fp32 kernel evaluate the functions at the
same point.
"""
import numpy as np
import pytest

import cost_probe_cases as C
from oracle import mppi_ref as R
from oracle import nets_ref as N

COSTS = list(C.DIMS)


@pytest.mark.parametrize("cost", COSTS)
def test_probe_mlp_is_base_plus_S_u_bit_for_bit(cost):
    """x + net([x, u]) == base + S u exactly, from a designed x (another row's state), in the float64 module
    restatement and in the engine's fc stack at fp32 and at bf16 rounding points."""
    c = C.sweep_case(cost)
    nx, nu = c["nx"], c["nu"]
    u = c["u"].reshape(-1, nu)
    want = c["states"].reshape(-1, nx)
    x = np.roll(want, 17, axis=0)  # whatever x was
    xin = np.concatenate([x, u], axis=1)
    assert np.array_equal(want.astype(np.float64), c["base"].astype(np.float64) + u.astype(np.float64) @ c["S"].T)
    got = x.astype(np.float64) + N.mlp_forward(c["sd"], xin)
    assert np.array_equal(got, want.astype(np.float64))
    stack = N.mlp_stack(c["sd"])
    for prec in ("fp32", "bf16"):
        d = N.fcstack_forward(stack, xin, prec)
        assert d.dtype == np.float32
        assert np.array_equal(x + d[:, :nx], want), prec
        assert np.array_equal(N.learned_dynamics(stack, nx, prec)(x, u), want), prec
    # what the layers are fed survives bf16: states, controls (hence the relu units, which are their parts)
    assert np.array_equal(R.bf16_round(xin), xin)


def test_probe_mlp_fills_the_hidden_layer():
    """55 states and 9 gathered entries take exactly the 128 hidden units of the specialised MLP route."""
    sd = C.sweep_case("humanoid_v3")["sd"]
    assert sd["network.0.weight"].shape == (128, 76) and (np.abs(sd["network.0.weight"]).sum(axis=1) == 1).all()
    assert set(np.unique(sd["network.6.weight"])) == {-1.0, 0.0, 1.0}


@pytest.mark.parametrize("i", range(len(C.CA_STATES)))
def test_probe_ca_steps_by_its_bias(i):
    """The CA probe net returns `step` for every input, bit for bit: the module restatement (float64), its fold, the
    LayerNorm fold (the folded rstd path), at fp32 and bf16 rounding points.  Nothing ahead of the zeroed last layer is
    non-finite (gamma, beta, the folded beta', every activation), so 0 x h is 0."""
    case = C.ca_case(i)
    sd = C.probe_ca(case["step"])
    rs = np.random.RandomState(i)
    x = np.concatenate([case["x0"][None], case["states"], rs.randn(5, 55).astype(np.float32)])
    u = rs.randn(len(x), 21).astype(np.float32)
    step64 = case["step"].astype(np.float64)
    assert np.array_equal(N.ca_forward(sd, x.astype(np.float64), 28, 27), np.tile(step64, (len(x), 1)))
    fold = N.ca_fold(sd, 28, 27, 21)
    lnf = N.ln_fold(fold)
    g, be = fold[0]["ln"]
    assert np.isfinite(g).all() and np.isfinite(be).all() and np.isfinite(lnf[0]["lnfold"]).all()
    xin = np.concatenate([x, u], axis=1)
    for stack in (fold, lnf):
        for prec in ("fp64", "fp32", "bf16"):
            h = N.fcstack_forward(stack[:2], xin, prec)
            assert np.isfinite(h).all()
            d = N.fcstack_forward(stack, xin, prec)
            assert np.array_equal(d.astype(np.float64), np.tile(step64, (len(x), 1))), prec
    # the rollout visits the designed states: x0 + step, x0 + 2 step, exactly in fp32
    x1 = case["x0"] + case["step"]
    assert np.array_equal(x1, case["states"][0]) and np.array_equal(x1 + case["step"], case["states"][1])


def test_ca_states_cover_the_roll_branches():
    """The 8 CA states: roll in each quadrant, each atan range at least twice, x == 0, and the pitch clamp binding."""
    a = C.trig_args(C.CA_STATES[:, 3:7] / C.GRID)
    y, x = a["roll_y"], a["roll_x"]
    for sx in (1, -1):
        for sy in (1, -1):
            assert ((np.sign(x) == sx) & (np.sign(y) == sy)).any(), (sx, sy)
    k = C.humanoid_classes(C.CA_STATES[:, 3:7] / C.GRID)
    assert min(k["roll: |y/x| low"], k["roll: |y/x| mid"], k["roll: |y/x| big"]) >= 2, k
    assert k["roll: x == 0"] >= 1 and k["pitch: a > +1"] + k["pitch: a < -1"] >= 1


HUMANOID = ["humanoid_v3", "humanoid_v1"]


def _all_quats(cost):
    return C.sweep_case(cost)["states"].reshape(-1, 55)[:, 3:7]


@pytest.mark.parametrize("cost", HUMANOID)
def test_every_branch_class_holds_enough_rows(cost):
    """Hard condition: every branch class of atan2_fast, atan_cephes and asin_fast, for roll and for yaw, the rows next
    to both atan thresholds on each side, the pitch edges and the single-angle rows hold at least MIN_ROWS rows."""
    k = C.humanoid_classes(_all_quats(cost))
    assert len(k) == 2 * 19 + 7 + 3
    short = {name: n for name, n in k.items() if n < C.MIN_ROWS}
    assert not short, short
    # ... and the hand-built rows alone already do for the classes seeded rows cannot be trusted to reach
    ks = C.humanoid_classes(C.special_quats() / 128.0)
    for name, n in ks.items():
        if "just" in name or "== 0" in name or "alone" in name or "pitch: a" in name or "== 0.5" in name:
            assert n >= C.MIN_ROWS, (name, n)


@pytest.mark.parametrize("cost", HUMANOID)
def test_threshold_rows_are_distinct_arguments(cost):
    """The rows next to a threshold are not one argument repeated: per threshold and side, every float32 step within
    ULPS of it is hit, by at least 16 different (|y|, x) pairs in all."""
    a = C.trig_args(_all_quats(cost), np.float32)
    for ang in ("roll", "yaw"):
        y, x = np.abs(a[ang + "_y"]), a[ang + "_x"]
        ok = (x != 0) & (y > 0)
        y, x = y[ok], x[ok]
        d = C._ulps_from((y / np.abs(x)).astype(np.float32), C.ATAN_T1), C._ulps_from((y / np.abs(x)).astype(np.float32),
                                                                                      C.ATAN_T2)
        for dd in d:
            for side in ((dd <= 0) & (dd >= -C.ULPS), (dd > 0) & (dd <= C.ULPS)):
                assert len(np.unique(np.stack([y[side], x[side]]), axis=1).T) >= 16, ang
                assert len(np.unique(dd[side])) >= C.ULPS, (ang, np.unique(dd[side]))


def test_trig_arguments_are_exact_in_float32():
    """float32 and float64 evaluation of every trig argument of every designed row agree bitwise (the humanoid sweeps,
    the stepped case's states and the CA states)."""
    s = C.steps_case()
    c = C.sweep_case("humanoid_v1")
    stepped = c["base"][None, None, :].astype(np.float64) + np.einsum("xu,uhk->hkx", c["S"], s["noise"].astype(np.float64))
    for q in (_all_quats("humanoid_v3"), _all_quats("humanoid_v1"), stepped[..., 3:7].astype(np.float32), (C.CA_STATES[:, 3:7] / C.GRID).astype(np.float32)):
        assert q.dtype == np.float32
        a32, a64 = C.trig_args(q, np.float32), C.trig_args(q, np.float64)
        for name in a32:
            assert a32[name].dtype == np.float32
            assert np.array_equal(a32[name].astype(np.float64), a64[name]), name


@pytest.mark.parametrize("cost", COSTS)
def test_designed_values_are_exact_in_every_form(cost):
    """Every designed state entry and control has at most 8 significant bits (bf16 keeps it, so do fp16 and a hi / lo
    split), and the magnitudes stay where the issue puts them: states below 2, controls below 4."""
    c = C.sweep_case(cost)
    for a in (c["states"], c["u"], c["base"], c["noise"]):
        assert np.array_equal(R.bf16_round(a), a)
        assert np.array_equal(a.astype(np.float16).astype(np.float32), a)
    assert np.abs(c["states"]).max() < 2 and np.abs(c["u"]).max() < 4
    s = C.steps_case()
    assert np.array_equal(R.bf16_round(s["noise"]), s["noise"]) and np.array_equal(R.bf16_round(s["x0"]), s["x0"])


@pytest.mark.parametrize("cost", COSTS)
def test_reference_terms_sum_to_the_oracle_cost(cost):
    """cost_terms (whose absolute sum is the tolerance scale) is the oracle's cost split into its terms, for t on both
    sides of humanoid_v1's swing switch; the scale is never zero, so the bar is never vacuous or impossible."""
    c = C.sweep_case(cost)
    f = R.COSTS[cost]
    for b in range(C.SWEEP_B):
        x, u, ctx = c["states"][b].astype(np.float64), c["u"][b].astype(np.float64), c["ctx"][b].astype(np.float64)
        for t in (1, 49, 50, 99, 100, 101):
            want = f(x, u, ctx, t) if getattr(f, "takes_t", False) else f(x, u, ctx)
            terms = C.cost_terms(cost, x, u, ctx, t)
            np.testing.assert_allclose(terms.sum(axis=-1), want, rtol=1e-13, atol=1e-13)
        np.testing.assert_array_equal(C.reference(cost, c["states"][b], c["u"][b], c["ctx"][b], 1)[0], c["ref"][b])
    assert c["scale"].min() > 1e-3 and (c["scale"] >= np.abs(c["ref"]) * (1 - 1e-12)).all()


def test_one_entry_at_a_time_rows_move_the_cost():
    """In solves 1..3 each gathered entry has rows where it alone moves, and every such family changes the reference
    cost (a swapped or dropped cost_idx slot cannot hide): at least 8 distinct costs per entry."""
    for cost in COSTS:
        c = C.sweep_case(cost)
        idx = C.COST_IDX[cost]
        for b in range(1, C.SWEEP_B):
            v = c["states"][b][:, idx]
            for i in range(len(idx)):
                rows = slice(i * C.MIN_ROWS, (i + 1) * C.MIN_ROWS)
                others = np.delete(v[rows], i, axis=1)
                assert (others == others[0]).all() and len(np.unique(v[rows, i])) >= 8, (cost, b, i)
                assert len(np.unique(c["ref"][b][rows])) >= 8, (cost, b, i)
            # the anchor the families move away from: every term of the cost non-zero, no two equal
            anchor = c["states"][b][C.MIN_ROWS].copy()       # family 1, row 0: entry 1 moved ...
            anchor[idx[1]] = c["states"][b][0, idx[1]]        # ... put back from family 0
            terms = C.cost_terms(cost, anchor, c["u"][b][0] * 0 + 1, c["ctx"][b], 1)
            assert (terms != 0).all() and len(np.unique(np.round(terms, 9))) == len(terms), (cost, b, terms)


@pytest.mark.parametrize("H", [101, 50])
def test_stepped_case_separates_the_swing_sides(H):
    """The stepped humanoid_v1 cases: a step index off by one at the 50 or 100 switch moves the summed cost by far more
    than the bar; at H = 50 so does H - 1 in the terminal term (at H = 101 both H and H - 1 are left-foot steps)."""
    s = C.steps_case(H)
    c = C.sweep_case("humanoid_v1")
    ctx = s["ctx"].astype(np.float64)
    assert ctx[3] != ctx[4] and ctx[5] != 0
    dyn = C.probe_dynamics(c["base"], c["S"])
    K = s["K"]
    x = np.repeat(s["x0"].astype(np.float64)[None], K, axis=0)
    shifted = np.zeros(K)
    for t in range(H):
        u = s["noise"][:, t, :].T.astype(np.float64)
        x = dyn(x, u)
        shifted += R.humanoid_v1_cost(x, u, ctx, t)      # t instead of t + 1
    shifted += s["terminal_weight"] * R.humanoid_v1_cost(x, np.zeros((K, 21)), ctx, H)
    assert (np.abs(shifted - s["ref"]) > 100 * C.BAR * s["scale"]).all()
    if H == 50:
        z = np.zeros((K, 21))
        off = s["terminal_weight"] * (R.humanoid_v1_cost(x, z, ctx, H - 1) - R.humanoid_v1_cost(x, z, ctx, H))
        assert (np.abs(off) > 100 * C.BAR * s["scale"]).all()
