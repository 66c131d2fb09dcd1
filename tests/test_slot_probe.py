"""The slot probe's premises, on the CPU (tests/slot_probe_cases.py; the kernels run it in tests/test_gpu_slot_probe.py).

Per shape: every value a kernel forms on the way (layer-0 pre-activations, states) has 8 significant bits, so the
oracle's fp32, bf16-emulating and float64 evaluations agree to a hundredth of the bar, and every fault of the list (a
dropped, exchanged or shifted slot) moves some sample's reference cost by at least 100 bars.  The last point is what
gives the one-bar check on the device its meaning: it fails if someone weakens the designed inputs.

test_dense_net_hides_a_one_slot_fault measures why a probe is needed at all: on a seeded dense net the same faults stay
below the bars the parity tests hold.
"""
import numpy as np
import pytest

import cost_probe_cases as C
import slot_probe_cases as S
from oracle import mppi_ref as R
from oracle import nets_ref as N

SHAPE_IDS = [S.shape_id(s) for s in S.SHAPES]


def _bars(got, ref, scale):
    return np.abs(np.asarray(got, np.float64) - ref) / (C.BAR * scale)


@pytest.mark.parametrize("shape", S.SHAPES, ids=SHAPE_IDS)
def test_rotation_net_is_P_x_plus_S_u_bit_for_bit(shape):
    """x + net([x, u]) == P x + S u exactly on designed inputs, in the module restatement and in the engine's fc stack
    at fp32 and at bf16 rounding points; the weights are 0 and +-1 and the biases 0."""
    nx, nu = shape
    c = S.mlp_case(nx, nu)
    sd = c["sd"]
    assert sd["network.0.weight"].shape == (128, nx + nu)
    assert set(np.unique(sd["network.0.weight"])) <= {-2.0, -1.0, 0.0, 1.0, 2.0}
    assert set(np.unique(sd["network.6.weight"])) == {-1.0, 0.0, 1.0}
    assert not any(np.any(sd[f"network.{i}.bias"]) for i in (0, 2, 4, 6))
    assert (c["S"].sum(axis=0) == 1).all() and (c["P"].sum(axis=0) == 1).all() and (c["P"].sum(axis=1) == 1).all()
    x = np.concatenate([c["x0"], np.roll(c["x0"], 5, axis=1)])
    u = np.concatenate([c["noise"][0, :, 0, :2].T, c["U0"][1, :, 1:2].T - c["noise"][1, :, 1, :2].T])
    want = x.astype(np.float64) @ c["P"].T + u.astype(np.float64) @ c["S"].T
    xin = np.concatenate([x, u], axis=1)
    assert np.array_equal(x.astype(np.float64) + N.mlp_forward(sd, xin), want)
    stack = N.mlp_stack(sd)
    for prec in ("fp64", "fp32", "bf16"):
        assert np.array_equal(N.learned_dynamics(stack, nx, prec)(x, u).astype(np.float64), want), prec
    assert np.array_equal(x.astype(np.float64) + xin.astype(np.float64) @ S.linear_map(sd).T, want)


@pytest.mark.parametrize("shape", S.SHAPES, ids=SHAPE_IDS)
def test_designed_inputs(shape):
    """B = 2 different x0 (integers / 64, 1 <= |int| <= 20, no zero entry), K = 90, H = nx + 2, U0 nonzero at a few
    places, each sample's noise nonzero in control slot k mod nu alone at one step, samples of neighbouring slots with
    different values, every control slot moved by some sample; all of it exact in bf16 and fp16."""
    nx, nu = shape
    c = S.mlp_case(nx, nu)
    assert c["x0"].shape == (2, nx) and c["noise"].shape == (2, nu, nx + 2, 90) and c["H"] == nx + 2
    xi = c["x0"] * S.GRID
    assert np.array_equal(xi, np.rint(xi)) and np.abs(xi).min() >= 1 and np.abs(xi).max() <= 20
    assert not np.array_equal(c["x0"][0], c["x0"][1])
    for b in range(S.B):
        assert (np.abs(np.diff(xi[b])) > 0).all() and xi[b, 0] != xi[b, -1]    # a swap of neighbours shows
        assert 1 <= np.count_nonzero(c["U0"][b]) <= 3
        nz = c["noise"][b] != 0
        assert (nz.sum(axis=(0, 1)) == 1).all()                                  # one (slot, step) per sample
        slot = nz.any(axis=1).argmax(axis=0)
        assert np.array_equal(slot, np.arange(S.K) % nu)
        v = c["noise"][b].sum(axis=(0, 1))
        assert (v[:-1] != v[1:]).all()
    for a in (c["x0"], c["U0"], c["noise"]):
        assert np.array_equal(R.bf16_round(a), a) and np.array_equal(a.astype(np.float16).astype(np.float32), a)


@pytest.mark.parametrize("shape", S.SHAPES, ids=SHAPE_IDS)
def test_every_value_has_eight_significant_bits(shape):
    """The bit-width condition: in float64, every layer-0 pre-activation and every state of every step of both solves
    is an integer / 64 of magnitude at most 255 / 64."""
    nx, nu = shape
    c = S.mlp_case(nx, nu)
    for b in range(S.B):
        top, whole = S.widths(c["sd"], c["x0"][b], c["U0"][b], c["noise"][b])
        print(f"SLOTS widths {S.shape_id(shape)} solve {b}: largest |integer| {top}")
        assert whole and top <= S.MAX_INT, (b, top, whole)


@pytest.mark.parametrize("shape", S.SHAPES, ids=SHAPE_IDS)
def test_oracle_precisions_agree_to_a_hundredth_of_the_bar(shape):
    """The fp32 oracle, the bf16-emulating oracle and the float64 reference within 0.01 bar of each other (the two
    float32 evaluations see the same states, so they are bitwise equal), the scale is the reference's own absolute
    terms, and the reference's weights are the softmin of its costs."""
    nx, nu = shape
    c = S.mlp_case(nx, nu)
    stack = N.mlp_stack(c["sd"])
    worst = 0.0
    for b in range(S.B):
        c32 = S.mlp_costs(c, N.learned_dynamics(stack, nx, "fp32"), b, np.float32)
        cbf = S.mlp_costs(c, N.learned_dynamics(stack, nx, "bf16"), b, np.float32)
        assert c32.dtype == np.float32 and np.array_equal(c32, cbf)
        e = _bars(c32, c["ref"][b], c["scale"][b])
        worst = max(worst, float(e.max()))
        assert e.max() <= 0.01, (b, e.max())
        # quad_est's terms are all non-negative: the scale is the cost itself
        np.testing.assert_allclose(c["scale"][b], c["ref"][b], rtol=1e-12)
        np.testing.assert_allclose(c["weights"][b], R.softmin_weights(c["ref"][b], 1.0), rtol=1e-12)
        assert len(np.unique(c["ref"][b])) >= 40 and c["scale"][b].min() > 0.5
    print(f"SLOTS precisions {S.shape_id(shape)}: fp32 / bf16 oracle within {worst:.4f} bars of float64")


@pytest.mark.parametrize("shape", S.SHAPES, ids=SHAPE_IDS)
def test_every_fault_moves_a_cost_by_100_bars(shape):
    """Every fault of mlp_faults moves at least one sample's float64 reference cost by FAULT_BARS bars or more.  The
    faulted nets are rolled out through their linear map (slot_probe_cases.linear_map), which is checked here against
    the fc stack on the first fault of each kind."""
    nx, nu = shape
    c = S.mlp_case(nx, nu)
    assert S.FAULT_BARS == 100.0
    seen, weakest, n = set(), (np.inf, ""), 0
    for name, sd in S.mlp_faults(c["sd"], nx, nu):
        dyn = S.linear_dynamics(S.linear_map(sd))
        kind = " ".join(w for w in name.split() if not w.isdigit())
        moved = 0.0
        for b in range(S.B):
            got = S.mlp_costs(c, dyn, b)
            if kind not in seen:
                want = S.mlp_costs(c, N.learned_dynamics(N.mlp_stack(sd), nx), b)
                np.testing.assert_allclose(got, want, rtol=1e-12, err_msg=name)
            moved = max(moved, float(_bars(got, c["ref"][b], c["scale"][b]).max()))
            if moved >= S.FAULT_BARS and kind in seen:
                break                               # one sample suffices
        seen.add(kind)
        n += 1
        assert moved >= S.FAULT_BARS, f"{name}: moves no sample by more than {moved:.1f} bars"
        weakest = min(weakest, (moved, name))
    want_n = (nx + nu) + nx + (nx - 1) + (nu - 1) + (nx > 32) + (nu > 1)
    assert n == want_n, (n, want_n)
    print(f"SLOTS faults {S.shape_id(shape)}: {n} faults, weakest {weakest[0]:.0f} bars ({weakest[1]})")


# ------------------------------------------------------------------------------------------------- the CA control probe

@pytest.mark.parametrize("nu", S.CA_NUS)
def test_ca_control_probe(nu):
    """The CA probe with nu controls: the net returns `step` bit for bit whatever the action (module restatement, fold
    and LayerNorm fold at fp64 / fp32 / bf16), the states x0 + t step and their trig arguments are exact in float32, the
    controls are integers / 4 with 8 significant bits, the noise is one-hot per sample and reaches every control slot,
    and the float32 evaluation of the reference lies within a quarter of a bar of it (about 30 float32 additions of
    terms bounded by the scale: 30 x 2^-24 = 1.8e-6 of the scale)."""
    c = S.ca_case(nu)
    sd, step64 = c["sd"], c["step"].astype(np.float64)
    assert sd["action_encoder.weight"].shape == (128, nu) and np.any(sd["action_encoder.weight"])
    u = (c["U"][:, :, None] + c["noise"])                            # [nu, H, K]
    ui = u * S.CA_GRID
    assert np.array_equal(ui, np.rint(ui)) and np.abs(ui).max() <= S.MAX_INT
    assert np.array_equal(R.bf16_round(u), u) and np.array_equal(R.bf16_round(c["U"]), c["U"])
    nz = c["noise"] != 0
    assert (nz.sum(axis=(0, 1)) == 1).all() and nz.any(axis=(1, 2)).all()
    assert np.array_equal(nz.any(axis=1).argmax(axis=0), np.arange(S.CA_K) % nu)
    assert nz.any(axis=(0, 2)).all()                                 # every step carries some sample's noise
    if nu > 1:
        assert (np.sign(c["U"][:-1]) != np.sign(c["U"][1:])).all()   # an exchange of neighbouring rows shows
    xs = np.stack([c["x0"] + np.float32(t) * c["step"] for t in range(S.CA_H + 1)])
    assert np.array_equal(xs.astype(np.float64), c["x0"].astype(np.float64) + np.arange(S.CA_H + 1)[:, None] * step64)
    a32, a64 = C.trig_args(xs[:, 3:7], np.float32), C.trig_args(xs[:, 3:7], np.float64)
    assert all(np.array_equal(a32[k].astype(np.float64), a64[k]) for k in a32)
    uu = np.ascontiguousarray(u[:, 0, :len(xs)].T)
    xin = np.concatenate([xs, uu], axis=1)
    assert np.array_equal(N.ca_forward(sd, xs.astype(np.float64), 28, 27), np.tile(step64, (len(xs), 1)))
    fold = N.ca_fold(sd, 28, 27, nu)
    for stack in (fold, N.ln_fold(fold)):
        for prec in ("fp64", "fp32", "bf16"):
            d = N.fcstack_forward(stack, xin, prec)
            assert np.array_equal(d.astype(np.float64), np.tile(step64, (len(xs), 1))), prec
    pre = R.Preset("slots", K=S.CA_K, H=S.CA_H, lam=1.0, sigma=1.0, terminal_weight=0.0)
    c32 = R.rollout(pre, lambda x, u_: x + c["step"][None, :], R.COSTS[S.CA_COST], c["x0"], c["U"], c["noise"],
                    ctx=c["ctx"], dtype=np.float32)
    e = _bars(c32, c["ref"], c["scale"])
    print(f"SLOTS ca nu={nu}: float32 oracle within {e.max():.4f} bars of float64")
    assert e.max() <= 0.25
    assert len(np.unique(c["ref"])) >= S.CA_K // 2


@pytest.mark.parametrize("nu", S.CA_NUS)
def test_every_ca_fault_moves_a_cost_by_100_bars(nu):
    """A zeroed control row of the noise, or one exchanged with its neighbour, moves some sample's reference cost by
    FAULT_BARS bars or more."""
    c = S.ca_case(nu)
    dyn = S.ca_dynamics(c["step"])
    weakest, n = (np.inf, ""), 0
    for name, noise in S.ca_faults(c["noise"]):
        got, _ = C.rollout_reference(S.CA_COST, dyn, c["x0"], c["U"], noise, c["ctx"])
        moved = float(_bars(got, c["ref"], c["scale"]).max())
        assert moved >= S.FAULT_BARS, f"{name}: moves no sample by more than {moved:.1f} bars"
        weakest = min(weakest, (moved, name))
        n += 1
    assert n == 2 * nu - 1
    print(f"SLOTS ca faults nu={nu}: {n} faults, weakest {weakest[0]:.0f} bars ({weakest[1]})")


# ------------------------------------------------------------------------------------------------- why a probe

@pytest.mark.parametrize("shape", [(31, 16), (33, 1), (62, 32), (64, 32)], ids=S.shape_id)
def test_dense_net_hides_a_one_slot_fault(shape):
    """The motivation, measured: on a seeded dense MLP (PyTorch's default init, quad_est with its own goal, H = 6,
    K = 64, x0 ~ 0.1 N(0, 1), noise ~ 0.4 N(0, 1)) a dropped input column of layer 0 or an un-updated state slot moves
    the median sample's cost by less, relative to the cost, than the 5e-3 the bf16 parity tests allow; the worst such
    fault stays invisible to them.  (Figures in DESIGN.md, section 0.)"""
    from mppi_hip.nets import synthetic_mlp
    nx, nu = shape
    H, K = 6, 64
    sd = synthetic_mlp(nx, nu, seed=9)
    rs = np.random.RandomState(4)
    x0, U0, noise = 0.1 * rs.randn(nx), 0.1 * rs.randn(nu, H), 0.4 * rs.randn(nu, H, K)
    pre = R.Preset("dense", K=K, H=H, lam=10.0, sigma=0.4)

    def costs(d):
        return R.rollout(pre, N.learned_dynamics(N.mlp_stack(d), nx), R.COSTS["quad_est"], x0, U0, noise)

    ref = costs(sd)
    col, row = [], []
    for j in range(3, nx):                           # (entries 0..2 are the ones the cost reads)
        W = sd["network.0.weight"].copy()
        W[:, j] = 0
        col.append(np.median(np.abs(costs({**sd, "network.0.weight": W}) - ref) / ref))
        W = sd["network.6.weight"].copy()
        W[j, :] = 0
        row.append(np.median(np.abs(costs({**sd, "network.6.weight": W}) - ref) / ref))
    print(f"SLOTS dense {S.shape_id(shape)}: dropped input column moves the median cost by {min(col):.1e} .. "
          f"{max(col):.1e} relative, un-updated state slot by {min(row):.1e} .. {max(row):.1e}")
    assert min(col) < 5e-3 and min(row) < 5e-3
