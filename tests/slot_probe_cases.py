"""Designed inputs that move every state and control slot of the fc rollouts, and the probe nets that carry them.

Pure numpy (tests/test_slot_probe.py checks everything here on the CPU; tests/test_gpu_slot_probe.py runs it through
the kernels).  The specialised fc kernels put the state into 64 slots (index i below qp = min(nx, 32) in slot i, above it
in slot 32 + (i - qp); csrc/mppi_nets.cpp slot_of / src_of) and the controls into 32 more.  tests/cost_probe_cases.py
moves only the entries the cost gathers; here every slot reaches them.

The rotation probe is an MLPStatePredictor(nx, nu, 128, 2) whose residual dynamics are x + net([x, u]) = P x + S u with
(P x)_j = x_{(j+1) mod nx} and control i added to state i mod nx:

  layer 0   unit 2j = relu(+a_j), unit 2j+1 = relu(-a_j), a_j = x_{(j+1) mod nx} - x_j + (S u)_j.  Weights 0, +-1.
  hidden    the identity.
  output    row j = unit 2j - unit 2j+1 = a_j.  Every bias is 0.

Every state entry passes through entries 0, 1, 2 (the ones quad_est reads) within nx steps, and every control lands in
a state entry, so over H = nx + 2 steps the cost sees every input column of layer 0, every output row and the carry of
every slot.  All designed values are integers / 64 and tests/test_slot_probe.py checks that every layer-0
pre-activation and every state of every step is one of magnitude at most 255 / 64: 8 significant bits, exact in bf16,
fp16 and a hi / lo split, so precision 0, 1 and 2 must produce the same fp32 states and are held to the cost probe's
bar (cost_probe_cases.BAR x the sum of the reference's absolute terms).

The folded cross-attention net ignores the action, so its control slots show in the cost's control term alone: the CA
control probe is cost_probe_cases.probe_ca (x' = x + step) with an action encoder of nu columns, one-hot noise per
sample over (control slot, step) on a nominal U that differs between neighbouring slots, under humanoid_v3.
"""
from __future__ import annotations

import functools

import numpy as np

import cost_probe_cases as C
from oracle import mppi_ref as R
from oracle import nets_ref as N

GRID = C.GRID
HIDDEN = C.HIDDEN
MAX_INT = 255                      # |integer| of every designed value, pre-activation and state: 8 significant bits
SHAPES = [(3, 1), (16, 16), (31, 16), (32, 17), (33, 1), (62, 32), (63, 32), (64, 32)]
B, K = 2, 90                       # Kp = 96: six live pad samples
COST = "quad_est"
FAULT_BARS = 100.0                 # every listed fault moves some sample's reference cost by at least this many bars

CA_NUS = [1, 19, 20, 22, 23, 24, 25, 32]
CA_K, CA_H = 64, 3
CA_COST = "humanoid_v3"
CA_GRID = 4                        # the CA probe's controls are integers / 4 (|integer| <= MAX_INT)


def shape_id(shape) -> str:
    return f"{shape[0]}x{shape[1]}"


# ------------------------------------------------------------------------------------------------- the rotation probe

def rotation(nx: int, nu: int) -> tuple[np.ndarray, np.ndarray]:
    """(P [nx, nx], S [nx, nu]): (P x)_j = x_{(j+1) mod nx}; control i feeds state i mod nx."""
    P = np.zeros((nx, nx))
    S = np.zeros((nx, nu))
    for j in range(nx):
        P[j, (j + 1) % nx] = 1.0
    for i in range(nu):
        S[i % nx, i] = 1.0
    return P, S


def probe_rotation(nx: int, nu: int) -> dict:
    """MLPStatePredictor(nx, nu, 128, 2) state dict with x + net([x, u]) = P x + S u (module docstring)."""
    assert 2 <= nx and 2 * nx <= HIDDEN
    P, S = rotation(nx, nu)
    A = np.concatenate([P - np.eye(nx), S], axis=1)                 # a = A [x; u]
    W0 = np.zeros((HIDDEN, nx + nu), np.float32)
    W3 = np.zeros((nx, HIDDEN), np.float32)
    W0[0:2 * nx:2], W0[1:2 * nx:2] = A, -A
    for j in range(nx):
        W3[j, 2 * j], W3[j, 2 * j + 1] = 1.0, -1.0
    assert set(np.unique(W0)) <= {-2.0, -1.0, 0.0, 1.0, 2.0}
    eye, zero = np.eye(HIDDEN, dtype=np.float32), np.zeros(HIDDEN, np.float32)
    return {"network.0.weight": W0, "network.0.bias": zero.copy(), "network.2.weight": eye.copy(),
            "network.2.bias": zero.copy(), "network.4.weight": eye.copy(), "network.4.bias": zero.copy(),
            "network.6.weight": W3, "network.6.bias": np.zeros(nx, np.float32)}


def linear_map(sd: dict) -> np.ndarray:
    """A [nx, nx + nu] with net(xin) = A xin, for a state dict of the probe's form: identity hidden layers, zero
    biases, layer-0 rows and last-layer columns in +- pairs, so that relu(a) - relu(-a) = a whatever the rows hold.
    Every fault of mlp_faults keeps that form (it moves whole columns of layer 0 and whole rows of the last layer), so
    the faulted references are rolled out through A; tests/test_slot_probe.py checks A against the fc stack."""
    W0, W3 = np.asarray(sd["network.0.weight"], np.float64), np.asarray(sd["network.6.weight"], np.float64)
    eye = np.eye(HIDDEN)
    assert np.array_equal(sd["network.2.weight"], eye) and np.array_equal(sd["network.4.weight"], eye)
    assert all(not np.any(sd[f"network.{i}.bias"]) for i in (0, 2, 4, 6))
    assert np.array_equal(W0[1::2], -W0[0::2]) and np.array_equal(W3[:, 1::2], -W3[:, 0::2])
    return W3[:, 0::2] @ W0[0::2]


def linear_dynamics(A):
    """x' = x + A [x; u] in float64."""
    A = np.asarray(A, np.float64)
    return lambda x, u: x + np.concatenate([x, u], axis=-1) @ A.T


def _x0(nx: int, b: int) -> np.ndarray:
    """Integers, 1 <= |v| <= 20, neighbours (and entries 31 / 32) of different magnitude, the two solves different."""
    j = np.arange(nx)
    mag = 1 + (7 * j + 11 * b + 3) % 20
    sign = np.where((j + b) % 3 == 1, -1, 1)
    return sign * mag


def _U0(nu: int, H: int, b: int) -> np.ndarray:
    """The nominal controls, integers: zero but at three designed (slot, step) places per solve."""
    U = np.zeros((nu, H), np.int64)
    places = ([(0, 1, 9), (nu // 2, 0, -11), (nu - 1, 2, 13)], [(0, 2, -10), (nu // 3, 1, 12), (nu - 1, 0, -7)])[b]
    for slot, step, v in places:
        U[slot, step] += v
    return U


def _noise(nu: int, H: int, b: int) -> np.ndarray:
    """The injected noise, integers [nu, H, K]: sample k moves control slot k mod nu alone, at one of the first three
    steps, by 16..32 (sign by sample); samples of neighbouring slots carry different values."""
    n = np.zeros((nu, H, K), np.int64)
    for k in range(K):
        mag = 16 + (5 * k + 3 * b) % 17
        sign = -1 if (k // nu + k) % 2 else 1
        n[k % nu, (k // nu + b) % 3, k] = sign * mag
    return n


def widths(sd: dict, x0, U, noise) -> tuple[int, bool]:
    """(the largest |value| x 64 among the layer-0 pre-activations and the states of every step of the float64 rollout,
    whether all of them are integers / 64)."""
    W0 = np.asarray(sd["network.0.weight"], np.float64)
    dyn = N.learned_dynamics(N.mlp_stack(sd), len(x0))
    x = np.repeat(np.asarray(x0, np.float64)[None], noise.shape[2], axis=0)
    top, whole = float(np.abs(x).max() * GRID), True
    for t in range(noise.shape[1]):
        u = np.asarray(U[:, t], np.float64)[None, :] + np.asarray(noise[:, t, :], np.float64).T
        pre = np.concatenate([x, u], axis=1) @ W0.T
        x = dyn(x, u)
        for a in (pre, x):
            top = max(top, float(np.abs(a).max() * GRID))
            whole = whole and bool(np.array_equal(np.rint(a * GRID), a * GRID))
    return int(round(top)), whole


def _preset(H: int) -> R.Preset:
    return R.Preset("slots", K=K, H=H, lam=1.0, sigma=1.0, terminal_weight=0.0)


@functools.lru_cache(maxsize=None)
def mlp_case(nx: int, nu: int) -> dict:
    """One shape of the rotation probe: the net, B = 2 solves' designed x0 / U0 / noise (float32, exact), the goal
    context, and the float64 reference (oracle.mppi_ref.mppi_solve through the fc stack) with its scale.  Read-only."""
    H = nx + 2
    sd = probe_rotation(nx, nu)
    x0 = np.stack([_x0(nx, b) for b in range(B)]) / GRID
    U0 = np.stack([_U0(nu, H, b) for b in range(B)]) / GRID
    noise = np.stack([_noise(nu, H, b) for b in range(B)]) / GRID
    ctx = np.zeros((B, 8))                                          # quad_est's goal (0, 0, 0)
    dyn = N.learned_dynamics(N.mlp_stack(sd), nx)
    ref, weights, scale = [], [], []
    for b in range(B):
        s = R.mppi_solve(_preset(H), dyn, R.COSTS[COST], x0[b], U0[b], noise[b], ctx=ctx[b], dtype=np.float64)
        c, sc = C.rollout_reference(COST, dyn, x0[b], U0[b], noise[b], ctx[b])
        assert np.array_equal(c, s["costs"])
        ref.append(s["costs"]), weights.append(s["weights"]), scale.append(sc)
    P, S = rotation(nx, nu)
    out = dict(nx=nx, nu=nu, H=H, sd=sd, P=P, S=S, x0=x0.astype(np.float32), U0=U0.astype(np.float32),
               noise=noise.astype(np.float32), ctx=ctx.astype(np.float32), ref=np.stack(ref),
               weights=np.stack(weights), scale=np.stack(scale))
    for name in ("x0", "U0", "noise"):
        assert np.array_equal(out[name].astype(np.float64), locals()[name])
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def mlp_costs(case: dict, dyn, b: int, dtype=np.float64) -> np.ndarray:
    """The rollout costs of solve b of a case under another dynamics (a faulted net, another precision)."""
    return R.rollout(_preset(case["H"]), dyn, R.COSTS[COST], case["x0"][b].astype(dtype), case["U0"][b],
                     case["noise"][b], ctx=case["ctx"][b].astype(dtype), dtype=dtype)


# ------------------------------------------------------------------------------------------------- the fault list

def _with(sd: dict, **parts) -> dict:
    out = {k: v.copy() for k, v in sd.items()}
    out.update(parts)
    return out


def mlp_faults(sd: dict, nx: int, nu: int):
    """(name, faulted state dict) for every one-slot error a packer or an operand build can make: a dropped input
    column, an un-updated output row, two neighbouring columns exchanged (state with state, control with control),
    the columns on the two sides of the 32-slot split exchanged, and the control columns shifted by one."""
    W0, W3 = sd["network.0.weight"], sd["network.6.weight"]
    for j in range(nx + nu):
        W = W0.copy()
        W[:, j] = 0
        yield f"zero input column {j}", _with(sd, **{"network.0.weight": W})
    for j in range(nx):
        W = W3.copy()
        W[j, :] = 0
        yield f"zero output row {j}", _with(sd, **{"network.6.weight": W})
    pairs = [(j, j + 1) for j in range(nx - 1)] + [(nx + i, nx + i + 1) for i in range(nu - 1)]
    for a, b in pairs:
        W = W0.copy()
        W[:, [a, b]] = W[:, [b, a]]
        yield f"swap input columns {a} and {b}", _with(sd, **{"network.0.weight": W})
    if nx > 32:
        W = W0.copy()
        W[:, [31, 32]] = W[:, [32, 31]]
        yield "swap the columns of state 31 and 32", _with(sd, **{"network.0.weight": W})
    if nu > 1:
        W = W0.copy()
        W[:, nx:] = np.roll(W0[:, nx:], 1, axis=1)
        yield "shift the control columns by one", _with(sd, **{"network.0.weight": W})


def ca_faults(noise: np.ndarray):
    """(name, faulted noise [nu, H, K]): one control row zeroed, or exchanged with its neighbour."""
    nu = noise.shape[0]
    for c in range(nu):
        n = noise.copy()
        n[c] = 0
        yield f"zero control row {c}", n
    for c in range(nu - 1):
        n = noise.copy()
        n[[c, c + 1]] = n[[c + 1, c]]
        yield f"swap control rows {c} and {c + 1}", n


# ------------------------------------------------------------------------------------------------- the CA control probe

_CA_STEP = np.array([3, -2, 1, 0, 0, 0, 0, 2, -1], np.int64)        # per step, on the gathered entries; the quaternion
                                                                      # stays the designed one


@functools.lru_cache(maxsize=None)
def ca_case(nu: int) -> dict:
    """The folded humanoid CA with nu controls: x0 a designed state of cost_probe_cases.CA_STATES (another one per nu),
    x' = x + step, K = 64 samples whose noise is one-hot over (control slot k mod nu, step) with designed values on a
    nominal U whose neighbouring slots differ, and the float64 reference under humanoid_v3 with its scale."""
    i = CA_NUS.index(nu)
    x0, step = np.zeros(55), np.zeros(55)
    x0[C.HUMANOID_IDX], step[C.HUMANOID_IDX] = C.CA_STATES[i] / GRID, _CA_STEP / GRID
    sd = C.probe_ca(step)
    r, c = np.meshgrid(np.arange(HIDDEN), np.arange(nu), indexing="ij")
    sd["action_encoder.weight"] = (((r + 3 * c) % 7 - 3) / 8.0).astype(np.float32)
    slot, t = np.meshgrid(np.arange(nu), np.arange(CA_H), indexing="ij")
    U = np.where(slot % 2 == 0, 1, -1) * (8 + (3 * slot + t) % 5)   # integers / 4: +-2 .. 3, neighbours of other sign
    noise = np.zeros((nu, CA_H, CA_K), np.int64)
    for k in range(CA_K):
        noise[k % nu, (k + k // nu) % CA_H, k] = (-1 if k % 3 == 1 else 1) * (64 + (5 * k) % 61)
    assert np.abs(U[:, :, None] + noise).max() <= MAX_INT
    U, noise = U / CA_GRID, noise / CA_GRID
    ctx = C.CONTEXTS[CA_COST][1 + i % 3]
    ref, scale = C.rollout_reference(CA_COST, ca_dynamics(step), x0, U, noise, ctx)
    out = dict(nu=nu, i=i, sd=sd, x0=x0.astype(np.float32), step=step.astype(np.float32), U=U.astype(np.float32),
               noise=noise.astype(np.float32), ctx=ctx.astype(np.float32), ref=ref, scale=scale)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def ca_dynamics(step):
    step = np.asarray(step, np.float64)
    return lambda x, u: x + step[None, :]
