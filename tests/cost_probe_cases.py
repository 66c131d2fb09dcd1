"""Designed states for the running costs, and the probe nets that put them in front of the rollout kernels.

Pure numpy (tests/test_cost_probe.py checks everything here on the CPU; tests/test_gpu_cost_probe.py runs it through
the kernels).  The engine's learned dynamics are residual, x' = x + net([x, u]) (oracle/nets_ref.py::learned_dynamics),
so the MLP probe net cancels the state it is given:

  layer 0   unit 2j = relu(+x_j), unit 2j+1 = relu(-x_j) for every state entry j; behind them, for the i-th entry the
            cost gathers, unit 2 nx + 2i = relu(+u_i) and 2 nx + 2i + 1 = relu(-u_i).  Weights +-1, bias 0.
  hidden    the identity.
  output    row j = -(unit 2j - unit 2j+1) + base_j, and row cost_idx[i] also + (unit 2nx+2i - unit 2nx+2i+1).

Hence x' = x + (base + S u - x) = base + S u with S[cost_idx[i], i] = 1, whatever x was: every step of a horizon is
designed on its own through U[:, t] + eps[:, t, k].  Every designed value has at most 8 significant bits (a multiple of
1/64 below 4 in magnitude; the quaternions next to an atan threshold multiples of 1/128 below 2, moved from a zero
base): exact in bf16, fp16 and a hi / lo split; the +-1 weights are exact in every form and every partial
sum is again such a value, so precision 0, 1 and 2 must hand the cost the same fp32 state.  55 states and 9 gathered
entries fill the 128 hidden units exactly.

The folded cross-attention net ignores the action; its probe is the shipped checkpoint with the last layer's weight
zeroed and its bias set to a step d, so the state after t steps is x0 + t d for every sample.
"""
from __future__ import annotations

import functools
import os

import numpy as np

from oracle import mppi_ref as R

GRID = 64          # designed values are integers / GRID
QMAX = 127         # |integer| of a designed state entry: |value| < 2
HIDDEN = 128
BAR = 1e-5         # the project's fp32 cost bar (tests/test_gpu_parity.py, tests/test_native_math.py), here relative
                   # to the sum of the absolute values of the reference's terms
MIN_ROWS = 32      # designed rows every branch class must hold
ULPS = 4           # "next to a threshold": within this many fp32 steps of it
ATAN_T1 = np.float32(0.4142135623730950)  # csrc/costs.h atan_cephes: mid above this, big above T2
ATAN_T2 = np.float32(2.414213562373095)

HUMANOID_IDX = [0, 1, 2, 3, 4, 5, 6, 28, 29]  # csrc/costs.h cost_idx
COST_IDX = {"humanoid_v3": HUMANOID_IDX, "humanoid_v1": HUMANOID_IDX,
            "quad_jl": [1, 2, 6, 7, 19, 20, 25, 26, 27], "quad_est": [0, 1, 2]}
DIMS = {"humanoid_v3": (55, 21), "humanoid_v1": (55, 21), "quad_jl": (37, 12), "quad_est": (37, 12)}
SWEEP_B, SWEEP_K = 4, 1024
_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ------------------------------------------------------------------------------------------------------ probe nets

def selector(nx: int, nu: int, cost: str) -> np.ndarray:
    """S [nx, nu]: control i moves the i-th entry the cost gathers."""
    S = np.zeros((nx, nu))
    for i, j in enumerate(COST_IDX[cost]):
        S[j, i] = 1.0
    return S


def probe_mlp(nx: int, nu: int, cost: str, base) -> dict:
    """MLPStatePredictor(nx, nu, 128, 2) state dict with x + net([x, u]) = base + S u (module docstring)."""
    idx = COST_IDX[cost]
    assert 2 * nx + 2 * len(idx) <= HIDDEN and len(idx) <= nu
    W0 = np.zeros((HIDDEN, nx + nu), np.float32)
    W3 = np.zeros((nx, HIDDEN), np.float32)
    for j in range(nx):
        W0[2 * j, j], W0[2 * j + 1, j] = 1.0, -1.0
        W3[j, 2 * j], W3[j, 2 * j + 1] = -1.0, 1.0
    for i, j in enumerate(idx):
        a = 2 * nx + 2 * i
        W0[a, nx + i], W0[a + 1, nx + i] = 1.0, -1.0
        W3[j, a], W3[j, a + 1] = 1.0, -1.0
    eye, zero = np.eye(HIDDEN, dtype=np.float32), np.zeros(HIDDEN, np.float32)
    return {"network.0.weight": W0, "network.0.bias": zero.copy(), "network.2.weight": eye.copy(),
            "network.2.bias": zero.copy(), "network.4.weight": eye.copy(), "network.4.bias": zero.copy(),
            "network.6.weight": W3, "network.6.bias": np.asarray(base, np.float32).copy()}


def probe_ca(step) -> dict:
    """The humanoid cross-attention checkpoint (28, 27, 21, hidden 128) with fusion_layer.4.weight = 0 and
    fusion_layer.4.bias = step: x + net([x, u]) = x + step for every x and u.  Everything ahead of the last layer (the
    encoders, the attention values, LayerNorm's gamma and beta) stays the trained net's."""
    with np.load(os.path.join(_GOLDEN, "ca_humanoid_weights.npz")) as z:
        sd = {k: z[k].copy() for k in z.files}
    sd["fusion_layer.4.weight"] = np.zeros_like(sd["fusion_layer.4.weight"])
    sd["fusion_layer.4.bias"] = np.asarray(step, np.float32).copy()
    assert sd["fusion_layer.4.bias"].shape == (55,)
    return sd


# ------------------------------------------------------------------------- the trig arguments, and their branch classes

def trig_args(q, dtype=np.float64) -> dict:
    """(y, x) of roll and yaw and the unclamped argument of pitch as csrc/costs.h forms them, in `dtype`."""
    q = np.asarray(q, dtype)
    q0, q1, q2, q3 = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    one, two = dtype(1.0), dtype(2.0)
    return dict(roll_y=two * (q0 * q1 + q2 * q3), roll_x=one - two * (q1 * q1 + q2 * q2),
                pitch=two * (q0 * q2 - q3 * q1),
                yaw_y=two * (q0 * q3 + q1 * q2), yaw_x=one - two * (q2 * q2 + q3 * q3))


def _ulps_from(r32: np.ndarray, thr: np.float32) -> np.ndarray:
    """Signed distance of positive float32 r32 from thr in float32 steps."""
    return r32.view(np.int32).astype(np.int64) - int(np.float32(thr).view(np.int32))


def humanoid_classes(q) -> dict:
    """Rows per branch class of atan2_fast / atan_cephes (roll, yaw) and asin_fast (pitch) among quaternions q [n, 4]."""
    q = np.asarray(q, np.float32)
    a = trig_args(q, np.float32)
    out = {}
    for ang in ("roll", "yaw"):
        y, x = a[ang + "_y"], a[ang + "_x"]
        nz = x != 0
        r = np.abs(y[nz] / x[nz]).astype(np.float32)
        out.update({f"{ang}: x > 0": (x > 0).sum(), f"{ang}: x < 0": (x < 0).sum(), f"{ang}: x == 0": (x == 0).sum(),
                    f"{ang}: y > 0": (y > 0).sum(), f"{ang}: y < 0": (y < 0).sum(), f"{ang}: y == 0": (y == 0).sum(),
                    f"{ang}: x < 0, y > 0": ((x < 0) & (y > 0)).sum(), f"{ang}: x < 0, y < 0": ((x < 0) & (y < 0)).sum(),
                    f"{ang}: x < 0, y == 0": ((x < 0) & (y == 0)).sum(),
                    f"{ang}: x == 0, y > 0": ((x == 0) & (y > 0)).sum(),
                    f"{ang}: x == 0, y < 0": ((x == 0) & (y < 0)).sum(),
                    f"{ang}: x == 0, y == 0": ((x == 0) & (y == 0)).sum(),
                    f"{ang}: |y/x| low": (r <= ATAN_T1).sum(), f"{ang}: |y/x| mid": ((r > ATAN_T1) & (r <= ATAN_T2)).sum(),
                    f"{ang}: |y/x| big": (r > ATAN_T2).sum()})
        pos = r[r > 0]
        for name, thr in (("T1", ATAN_T1), ("T2", ATAN_T2)):
            d = _ulps_from(pos, thr)
            out[f"{ang}: |y/x| just under {name}"] = ((d <= 0) & (d >= -ULPS)).sum()
            out[f"{ang}: |y/x| just over {name}"] = ((d > 0) & (d <= ULPS)).sum()
    p = a["pitch"]
    ap = np.abs(p)
    out.update({"pitch: |a| < 0.5": (ap < 0.5).sum(), "pitch: |a| == 0.5": (ap == 0.5).sum(),
                "pitch: 0.5 < |a| < 1": ((ap > 0.5) & (ap < 1)).sum(), "pitch: a == +1": (p == 1).sum(),
                "pitch: a == -1": (p == -1).sum(), "pitch: a > +1": (p > 1).sum(), "pitch: a < -1": (p < -1).sum()})
    q0, q1, q2, q3 = q.T
    out["roll alone"] = ((q2 == 0) & (q3 == 0) & (q0 != 0) & (q1 != 0)).sum()
    out["pitch alone"] = ((q1 == 0) & (q3 == 0) & (q0 != 0) & (q2 != 0) & (a["roll_x"] > 0)).sum()
    out["yaw alone"] = ((q1 == 0) & (q2 == 0) & (q0 != 0) & (q3 != 0)).sum()
    return {k: int(v) for k, v in out.items()}


# ------------------------------------------------------------------------------------- designed quaternions (integers)

def _threshold_quats(thr: np.float32, over: bool, rng, n: int = MIN_ROWS + 4) -> np.ndarray:
    """n quaternions, as integers in units of 1/128 (|a| <= 255: still 8 significant bits), whose roll ratio |y/x| lies
    within ULPS float32 steps of thr on one side.  In units of 1/16384, x = 16384 - 2 (a1^2 + a2^2) and y = 2 (a0 a1 +
    a2 a3): for every (a1, a2) take the two reachable y next to thr |x| and keep those that are close enough and have a
    solution |a0|, |a3| <= 255; one row per (a1, a2, y), so the rows' ratios differ."""
    a = np.arange(1, 2 * QMAX + 2)
    A1, A2 = np.meshgrid(a, a, indexing="ij")
    aX = np.abs(16384 - 2 * (A1 * A1 + A2 * A2))
    g2 = 2 * np.gcd(A1, A2)
    lo = np.floor(np.float64(thr) * aX / g2).astype(np.int64) * g2
    a3 = np.arange(-2 * QMAX - 1, 2 * QMAX + 2)
    rows = []
    for Y in (lo, lo + g2):
        r32 = Y.astype(np.float32) / np.maximum(aX, 1).astype(np.float32)  # both exact: the correctly rounded ratio
        d = _ulps_from(r32, thr)
        ok = (aX > 0) & (Y > 0) & (((d > 0) & (d <= ULPS)) if over else ((d <= 0) & (d >= -ULPS)))
        for i1, i2 in zip(*np.nonzero(ok)):
            a1, a2, m = int(a[i1]), int(a[i2]), int(Y[i1, i2]) // 2
            rem = m - a3 * a2
            sel = np.nonzero((rem % a1 == 0) & (np.abs(rem // a1) <= 2 * QMAX + 1))[0]
            if len(sel):
                j = sel[rng.randint(len(sel))]
                rows.append((rem[j] // a1, a1, a2, a3[j]))
    rows = np.array(rows, np.int64).reshape(-1, 4)
    assert len(rows) >= n, len(rows)
    rows = rows[rng.permutation(len(rows))][:n]
    # the other sign patterns with the same |y| and x: (a0, a3) -> -(a0, a3) flips y, so does (a1, a2) -> -(a1, a2)
    s03 = rng.choice([-1, 1], len(rows))
    s12 = rng.choice([-1, 1], len(rows))
    return rows * np.stack([s03, s12, s12, s03], axis=1)


def _roll_to_yaw(rows: np.ndarray) -> np.ndarray:
    """yaw(q0, q1, q2, q3) = roll(q0, q3, q2, q1): swap q1 and q3."""
    return rows[:, [0, 3, 2, 1]]


def _pitch_quats(target_lo: int, target_hi: int, n: int, rng) -> np.ndarray:
    """n integer quaternions with a0 a2 - a3 a1 (= 2048 x the pitch argument) in [target_lo, target_hi]."""
    rows = []
    while len(rows) < n:
        a1, a3 = rng.randint(-QMAX, QMAX + 1, 2)
        a2 = int(rng.choice([-1, 1])) * int(rng.randint(1, QMAX + 1))
        t = int(rng.randint(target_lo, target_hi + 1))
        num = t + a3 * a1
        if num % a2 == 0 and abs(num // a2) <= QMAX:
            rows.append((num // a2, a1, a2, a3))
    return np.array(rows, np.int64)


def _ri(rng, n, lo=-QMAX, hi=QMAX):
    return rng.randint(lo, hi + 1, n)


def _nonzero(rng, n, hi=QMAX):
    return rng.choice([-1, 1], n) * rng.randint(1, hi + 1, n)


@functools.lru_cache(maxsize=None)
def special_quats() -> np.ndarray:
    """The hand-built quaternion rows, integers in units of 1/128: thresholds (odd multiples occur), and on the 1/64
    grid x == 0, single angles and pitch edges."""
    rng = np.random.RandomState(20250)
    n = MIN_ROWS
    z = np.zeros(n, np.int64)
    out, fine = [], []
    for thr in (ATAN_T1, ATAN_T2):
        for over in (False, True):
            r = _threshold_quats(thr, over, rng)
            fine += [r, _roll_to_yaw(r)]
    # x == 0 exactly: q1 = q2 = +-1/2 (roll; y = +-q0 +- q3), q2 = q3 = +-1/2 (yaw): y > 0, y < 0, y == 0
    for k in range(3):
        a0 = _nonzero(rng, n, 100)
        s1, s2 = rng.choice([-1, 1], n), rng.choice([-1, 1], n)
        d = rng.randint(1, 27, n)
        y = (d, -d, z)[k]                  # y = s1 a0 + s2 a3 (units of 1/64)
        a3 = s2 * (y - s1 * a0)
        r = np.stack([a0, 32 * s1, 32 * s2, a3], axis=1)
        out += [r, _roll_to_yaw(r)]
    # one angle alone: roll (q2 = q3 = 0), yaw (q1 = q2 = 0), both signs of x and y; pitch (q1 = q3 = 0, x > 0)
    r = np.stack([_nonzero(rng, 2 * n), _nonzero(rng, 2 * n, 45), np.zeros(2 * n, np.int64), np.zeros(2 * n, np.int64)],
                 axis=1)                                                       # x > 0
    r[n:, 1] = rng.choice([-1, 1], n) * rng.randint(46, QMAX + 1, n)          # x < 0
    out += [r, _roll_to_yaw(r)]
    a2 = _nonzero(rng, 2 * n, 45)
    r = np.stack([_nonzero(rng, 2 * n), np.zeros(2 * n, np.int64), a2, np.zeros(2 * n, np.int64)], axis=1)
    out.append(r)
    # y == 0 with x < 0 (atan2 = +-pi): q0 = q3 = 0 and q1 large (roll), q0 = q1 = 0 and q3 large (yaw)
    r = np.stack([z, rng.choice([-1, 1], n) * rng.randint(46, QMAX + 1, n), _ri(rng, n), z], axis=1)
    out += [r, _roll_to_yaw(r)]
    for a0, a2 in ((32, 32), (64, 16), (-64, -16), (64, 32), (-64, 32), (64, -32), (127, 45), (-127, 45), (100, 40)):
        out.append(np.array([[a0, 0, a2, 0]], np.int64))           # pitch alone at 0.5, +-1 and beyond
    # pitch argument a = (a0 a2 - a3 a1) / 2048: exactly +-0.5, exactly +-1, beyond +-1 (the seeded rows fill (0.5, 1))
    for lo, hi in ((1024, 1024), (-1024, -1024), (2048, 2048), (-2048, -2048), (2049, 6000), (-6000, -2049)):
        out.append(_pitch_quats(lo, hi, n, rng))
    # the identity, its negative, zero, the corners
    out.append(np.array([[64, 0, 0, 0], [-64, 0, 0, 0], [0, 0, 0, 0], [QMAX] * 4, [-QMAX] * 4, [0, 64, 0, 0],
                         [0, 0, 64, 0], [0, 0, 0, 64], [45, 45, 0, 0], [45, 0, 45, 0], [45, 0, 0, 45]], np.int64))
    q = np.concatenate(fine + [2 * r for r in out])
    assert np.abs(q).max() <= 2 * QMAX + 1
    q.setflags(write=False)
    return q


def _random_quats(rng, n) -> np.ndarray:
    """Unit quaternions from every quadrant, some scaled off the unit sphere, rounded to the grid; a third uniform."""
    g = rng.randn(n, 4)
    g = g / np.linalg.norm(g, axis=1, keepdims=True) * rng.choice([1.0, 1.0, 0.75, 1.25, 1.5], (n, 1))
    q = np.clip(np.rint(g * GRID), -QMAX, QMAX).astype(np.int64)
    uni = rng.rand(n) < 1.0 / 3
    q[uni] = _ri(rng, (int(uni.sum()), 4))
    return q


# ------------------------------------------------------------------------------------------ the reference's terms

def cost_terms(cost: str, x, u, ctx, t: int = 1) -> np.ndarray:
    """The terms of oracle.mppi_ref.COSTS[cost] in float64, [..., n]; their sum is the cost (checked on the CPU) and
    the sum of their absolute values is the tolerance scale."""
    x, u = np.asarray(x, np.float64), np.asarray(u, np.float64)
    usq = np.sum(u ** 2, axis=-1)
    if cost in ("humanoid_v3", "humanoid_v1"):
        c = np.asarray(ctx, np.float64)
        px, py, pz, vx, vy = x[..., 0], x[..., 1], x[..., 2], x[..., 28], x[..., 29]
        a = trig_args(x[..., 3:7])
        roll, yaw = np.arctan2(a["roll_y"], a["roll_x"]), np.arctan2(a["yaw_y"], a["yaw_x"])
        pitch = np.arcsin(np.clip(a["pitch"], -1.0, 1.0))
        if cost == "humanoid_v3":
            ftx = px + 0.5
            terms = [5 * roll ** 2, 5 * pitch ** 2, 0.075 * yaw ** 2, 12.5 * np.hypot(px - c[0], py - c[1]),
                     5 * np.abs(c[2] - pz), np.hypot(vx - 0.3, vy), 8 * np.abs(c[3] - ftx), 3 * (c[4] - ftx) ** 2,
                     c[5] + 0 * px, 0.01 * usq]
        else:
            left = (t % 100) < 50
            terms = [5 * roll ** 2, 5 * pitch ** 2, 12 * np.hypot(px - c[0], py - c[1]), 2.25 * (c[2] - pz),
                     np.hypot(vx - 0.5, vy), 10 * ((c[3] if left else c[4]) - (px + 0.5)) ** 2,
                     (c[5] if left else -c[5]) + 0 * px, c[6] + 0 * px, 0.01 * usq]
    elif cost == "quad_jl":
        nq = R.QUAD_NQ
        terms = [500 * (x[..., 2] - 0.45) ** 2, 1000 * (x[..., nq] - 0.6) ** 2, 500 * x[..., 6] ** 2,
                 500 * x[..., 7] ** 2, 20 * x[..., nq + 6] ** 2, 20 * x[..., nq + 7] ** 2, 20 * x[..., nq + 8] ** 2,
                 1000 * x[..., 1] ** 2, 1000 * x[..., nq + 1] ** 2, 0.1 * usq]
    elif cost == "quad_est":
        g = np.asarray(ctx, np.float64)[:3]
        terms = [(x[..., i] - g[i]) ** 2 for i in range(3)] + [0.1 * usq]
    else:
        raise KeyError(cost)
    return np.stack(terms, axis=-1)


def reference(cost: str, x, u, ctx, t: int = 1):
    """(cost, scale): oracle.mppi_ref.COSTS[cost] in float64 on the designed fp32 state x with control u, and the sum
    of the absolute values of its terms."""
    f = R.COSTS[cost]
    x64, u64 = np.asarray(x, np.float64), np.asarray(u, np.float64)
    c64 = None if ctx is None else np.asarray(ctx, np.float64)
    ref = f(x64, u64, c64, t) if getattr(f, "takes_t", False) else f(x64, u64, c64)
    return ref, np.abs(cost_terms(cost, x64, u64, c64, t)).sum(axis=-1)


def rollout_reference(cost: str, dyn, x0, U, noise, ctx, terminal_weight: float = 0.0, ctrl_clamp: float = 0.0):
    """(costs [K], scale [K]) of a whole rollout in float64: oracle.mppi_ref.rollout, and beside it the same loop over
    the absolute terms (the running terms, then terminal_weight x the terms at t = H with zero control)."""
    nu, H, K = noise.shape
    pre = R.Preset("probe", K=K, H=H, lam=1.0, sigma=1.0, ctrl_clamp=ctrl_clamp, terminal_weight=terminal_weight)
    c64 = None if ctx is None else np.asarray(ctx, np.float64)
    ref = R.rollout(pre, dyn, R.COSTS[cost], np.asarray(x0, np.float64), U, noise, ctx=c64, dtype=np.float64)
    x = np.repeat(np.asarray(x0, np.float64)[None, :], K, axis=0)
    scale = np.zeros(K)
    for t in range(H):
        u = np.asarray(U[:, t], np.float64)[None, :] + np.asarray(noise[:, t, :], np.float64).T
        if ctrl_clamp > 0:
            u = np.clip(u, -ctrl_clamp, ctrl_clamp)
        x = dyn(x, u)
        scale += np.abs(cost_terms(cost, x, u, c64, t + 1)).sum(axis=-1)
    if terminal_weight:
        scale += abs(terminal_weight) * np.abs(cost_terms(cost, x, np.zeros((K, nu)), c64, H)).sum(axis=-1)
    return ref, scale


def probe_dynamics(base, S):
    """The map the MLP probe net realises, in float64: x' = base + S u."""
    base, S = np.asarray(base, np.float64), np.asarray(S, np.float64)
    return lambda x, u: base[None, :] + np.asarray(u, np.float64) @ S.T


# ---------------------------------------------------------------------------------------------------- the contexts

# humanoid_v3: [tx, ty, tz, swing_foot_x, swing_knee_x, const, 0, 0].  Row 0 is "neutral": with the base state below
# every term but the angles, the (tiny) velocity term and the control term vanishes, so the trig rows of solve 0 are
# held almost alone.  Rows 1..3 make every term non-zero and distinct.
_CTX_V3 = np.array([[0.5, -0.25, 1.25, 1.0, 1.0, 0.0, 0, 0],
                    [1.5, -0.5, 1.0, 0.75, -0.25, 0.125, 0, 0],
                    [-0.75, 1.25, 0.5, -1.5, 1.75, -0.0625, 0, 0],
                    [1.75, 0.75, -0.25, 0.25, -1.0, 0.3125, 0, 0]])
# humanoid_v1: [tx, ty, tz, left_foot_x, right_foot_x, 0.01 (zr - zl), 0.1 |yl - yr|, 0]; left != right in rows 1..3
_CTX_V1 = np.array([[0.5, -0.25, 1.25, 1.0, 1.0, 0.0, 0.0, 0],
                    [1.5, -0.5, 1.0, 0.75, -0.5, 0.046875, 0.03125, 0],
                    [-0.75, 1.25, 0.5, -1.5, 1.25, -0.015625, 0.109375, 0],
                    [1.75, 0.75, -0.25, 0.25, -1.0, 0.078125, 0.0625, 0]])
_CTX_QE = np.array([[1.5, 0.25, 0.375, 0, 0, 0, 0, 0], [-0.5, 1.0, 0.25, 0, 0, 0, 0, 0],
                    [0.75, -1.25, 1.5, 0, 0, 0, 0, 0], [2.0, 0.0, 0.34375, 0, 0, 0, 0, 0]])
CONTEXTS = {"humanoid_v3": _CTX_V3, "humanoid_v1": _CTX_V1, "quad_jl": np.zeros((4, 8)), "quad_est": _CTX_QE}


def _base(cost: str) -> np.ndarray:
    """The probe net's output bias: a seeded grid state; the humanoid's gathered entries are the neutral ones."""
    nx, _ = DIMS[cost]
    rng = np.random.RandomState(77 + nx)
    base = _ri(rng, nx, -63, 63) / GRID
    if cost.startswith("humanoid"):
        base[HUMANOID_IDX] = [0.5, -0.25, 1.25, 0.0, 0.0, 0.0, 0.0, 0.296875 if cost == "humanoid_v3" else 0.515625, 0.0]
    return base


def _one_at_a_time(rng, anchor: np.ndarray, n_each: int) -> np.ndarray:
    """For every gathered entry i, n_each rows equal to `anchor` but for entry i, which takes other grid values."""
    rows = []
    for i in range(len(anchor)):
        r = np.repeat(anchor[None, :], n_each, axis=0)
        r[:, i] = _ri(rng, n_each)
        rows.append(r)
    return np.concatenate(rows)


def _humanoid_rows(cost: str, rng) -> tuple[np.ndarray, np.ndarray]:
    """(v [B, K, 9], extra [B, K, 12]), in units of 1/64: the gathered entries and the controls that move nothing."""
    B, K = SWEEP_B, SWEEP_K
    base_i = _base(cost)[HUMANOID_IDX] * GRID
    sq = special_quats() / 2.0
    assert len(sq) <= K
    v = np.zeros((B, K, 9))
    extra = np.zeros((B, K, 12))
    # solve 0: the neutral context and base position / velocity; only the quaternion moves
    v[0] = base_i
    v[0, :len(sq), 3:7] = sq
    v[0, len(sq):, 3:7] = _random_quats(rng, K - len(sq))
    # solves 1..3: everything moves.  One-entry-at-a-time rows around an anchor whose terms are all non-zero and
    # distinct, the special quaternions again under other positions, then seeded rows
    anchors = np.array([[40, -24, 56, 52, 20, -28, 12, 36, -44], [-72, 100, 8, -36, 60, 24, 44, -20, 68],
                        [96, 16, -48, 28, -56, 40, -16, 84, 32]], np.int64)
    for b in range(1, B):
        v[b] = _ri(rng, (K, 9))
        one = _one_at_a_time(rng, anchors[b - 1], MIN_ROWS)
        v[b, :len(one)] = one
        pick = rng.permutation(len(sq))[:K - len(one) - 256]
        v[b, len(one):len(one) + len(pick), 3:7] = sq[pick]
        v[b, len(one) + len(pick):, 3:7] = _random_quats(rng, K - len(one) - len(pick))
        extra[b] = _ri(rng, (K, 12))
    return v, extra


def _quad_rows(cost: str, rng) -> tuple[np.ndarray, np.ndarray]:
    n, nu = len(COST_IDX[cost]), DIMS[cost][1]
    B, K = SWEEP_B, SWEEP_K
    v = _ri(rng, (B, K, n))
    extra = _ri(rng, (B, K, nu - n))
    # zero, the corners, and the grid neighbours of the cost's constants (0.45 -> 29/64, 0.6 -> 38/64)
    hand = np.array([[0] * 9, [QMAX] * 9, [-QMAX] * 9, [29, 38] * 4 + [29], [38, 29] * 4 + [38]], np.int64)[:, :n]
    for b in range(B):
        # (quad_jl's weights repeat, so the anchor's magnitudes must not)
        anchor = (np.roll(np.array([20, -36, 52, -12, 44, 28, -60, 8, 68], np.int64), b) * (-1) ** b
                  if cost == "quad_jl" else np.array([[20, -36, 52], [-44, 12, 36], [60, 8, -24], [100, -4, 16]],
                                                     np.int64)[b])
        one = _one_at_a_time(rng, anchor, MIN_ROWS)
        v[b, :len(one)] = one
        v[b, len(one):len(one) + len(hand)] = hand
    extra[0] = 0
    return v, extra


@functools.lru_cache(maxsize=None)
def sweep_case(cost: str) -> dict:
    """The H = 1 sweep of one cost: B x K designed states, the injected noise that produces them from U = 0, the
    per-solve contexts and the float64 reference with its scale.  Arrays are read-only."""
    nx, nu = DIMS[cost]
    idx = COST_IDX[cost]
    rng = np.random.RandomState({"humanoid_v3": 3, "humanoid_v1": 1, "quad_jl": 7, "quad_est": 9}[cost])
    v, extra = (_humanoid_rows if cost.startswith("humanoid") else _quad_rows)(cost, rng)
    base = _base(cost)
    S = selector(nx, nu, cost)
    u = np.concatenate([v / GRID - base[idx], extra / GRID], axis=-1)          # [B, K, nu]
    states = base[None, None, :] + u @ S.T                                       # [B, K, nx], exact
    ctx = CONTEXTS[cost]
    ref, scale = zip(*(reference(cost, states[b].astype(np.float32), u[b].astype(np.float32), ctx[b], 1)
                       for b in range(SWEEP_B)))
    out = dict(cost=cost, nx=nx, nu=nu, base=base.astype(np.float32), S=S, sd=probe_mlp(nx, nu, cost, base),
               states=states.astype(np.float32), u=u.astype(np.float32),
               noise=np.ascontiguousarray(u.transpose(0, 2, 1)[:, :, None, :]).astype(np.float32),  # [B, nu, 1, K]
               ctx=ctx.astype(np.float32), ref=np.stack(ref), scale=np.stack(scale))
    assert np.array_equal(out["states"].astype(np.float64), states) and np.array_equal(out["u"].astype(np.float64), u)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def steps_case(H: int = 101, K: int = 64, terminal_weight: float = 2.0) -> dict:
    """humanoid_v1 over H steps with another designed state at every (step, sample): rows of the humanoid sweep drawn
    by a seeded permutation, a context whose left and right feet differ, and the summed float64 reference (t mod 100 <
    50 per step, t = H and zero control in the terminal term)."""
    c = sweep_case("humanoid_v1")
    rng = np.random.RandomState(101)
    pool = c["u"][1:].reshape(-1, c["nu"])                       # solves 1..3: everything moves
    pick = rng.randint(0, len(pool), (H, K))
    noise = np.ascontiguousarray(pool[pick].transpose(2, 0, 1))  # [nu, H, K]
    # around the swing switches every sample stands where the two feet cost very differently, on opposite sides at the
    # two switches, so that a step index off by one (either way) cannot cancel between them
    for t1, px in ((49, 1.0), (50, 1.0), (99, -1.5), (100, -1.5)):
        if t1 <= H:
            noise[0, t1 - 1, :] = px - c["base"][0]
    ctx = np.array([1.5, -0.5, 1.0, 1.25, -0.75, 0.046875, 0.03125, 0.0], np.float32)
    x0 = c["states"][2, 5]
    ref, scale = rollout_reference("humanoid_v1", probe_dynamics(c["base"], c["S"]), x0, np.zeros((c["nu"], H)), noise,
                                   ctx, terminal_weight=terminal_weight)
    out = dict(H=H, K=K, terminal_weight=terminal_weight, noise=noise, ctx=ctx, x0=x0, ref=ref, scale=scale)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


# ----------------------------------------------------------------------------------------------- the CA probe's states

# 8 designed humanoid states (the 9 gathered entries, integers / 64): roll in each quadrant and atan range, x == 0, and
# the pitch clamp binding.  (q0, q1, q2, q3) with q2 = q3 = 0 has roll = atan2(2 q0 q1, 1 - 2 q1^2).
CA_STATES = np.array([
    [40, -24, 56, 60, 8, 0, 0, 36, -44],      # x > 0, y > 0, |y/x| low  (0.24)
    [-72, 100, 8, 60, -24, 0, 0, -20, 68],    # x > 0, y < 0, mid        (0.98)
    [96, 16, -48, 64, 44, 4, 0, 84, 32],      # x > 0 small: big         (25.)
    [12, -60, 72, 20, 64, 0, 0, 44, 12],      # x < 0, y > 0, mid        (0.625)
    [-28, 36, 64, -90, 50, 0, 6, -52, 24],    # x < 0, y < 0, big        (10.)
    [56, 8, -16, 20, -100, 0, 0, 28, -36],    # x < 0, y < 0, low        (0.25)
    [24, -44, 40, 48, 32, 32, -20, 16, 60],   # x == 0 exactly, y > 0
    [-8, 52, 20, 120, 0, 90, 0, -12, 8],      # pitch argument 2 q0 q2 = 5.3: the clamp binds (and roll = pi)
], np.int64)


def ca_case(i: int, H: int = 2) -> dict:
    """Net i of the CA probe: with x0 = 2 s_i - s_j and step = s_j - s_i (j = i + 1 mod 8) the rollout visits the
    designed states s_i at t = 1 and s_j at t = 2, for every sample."""
    assert H == 2
    j = (i + 1) % len(CA_STATES)
    s = np.zeros((2, 55))
    s[0, HUMANOID_IDX], s[1, HUMANOID_IDX] = CA_STATES[i] / GRID, CA_STATES[j] / GRID
    step = s[1] - s[0]
    return dict(x0=(s[0] - step).astype(np.float32), step=step.astype(np.float32), states=s.astype(np.float32))
