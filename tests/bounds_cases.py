"""Inputs shared by tests/test_control_bounds.py (host) and tests/test_gpu_control_bounds.py (device): the main cases,
whose boxes bind on a fixed share of every actuator's elements, and the edge boxes of csrc/ctrl_bounds.h."""
import numpy as np

# K: below one 256-wide chunk with pad lanes (30 -> Kp 64; 75 -> Kp 128) and five chunks, the last one partial (1100 ->
# Kp 1152); H: one row, two, and more than the eight rows a wave may take; nu: one, odd, and the most the box carries
MAIN_SHAPES = [(1, 1, 1, 30), (3, 3, 2, 75), (1, 32, 17, 30), (3, 1, 17, 1100), (1, 3, 1, 1100), (3, 32, 2, 30),
               (1, 3, 17, 75)]  # (B, nu, H, K)


def main_case(B, nu, H, K, seed=0, sigma=0.5):
    """U [B, nu, H], eps [B, nu, H, K], lo, hi [nu] (float32): per actuator the box is cut from the sampled controls
    U + eps themselves, at their 15 % and 80 % points, so about a third of every actuator's elements project -- some on
    each side -- whatever the shape.  The tests assert the share from project_noise_ref's counts (5 % .. 60 %)."""
    rs = np.random.RandomState(1000 + seed)
    U = (0.2 * rs.randn(B, nu, H)).astype(np.float32)
    eps = (sigma * rs.randn(B, nu, H, K)).astype(np.float32)
    s = (U[..., None] + eps).astype(np.float32)
    lo = np.array([np.percentile(s[:, u], 15.0) for u in range(nu)], np.float32)
    hi = np.array([np.percentile(s[:, u], 80.0) for u in range(nu)], np.float32)
    return U, eps, lo, hi


def share_ok(counts, H, K):
    """every (b, u) projected between 5 % and 60 % of its H K elements"""
    f = np.asarray(counts, np.float64) / (H * K)
    return bool(np.all(f >= 0.05) and np.all(f <= 0.60))


EDGE_KINDS = ("wide", "no_zero", "pinned", "upper_only", "lower_only", "infinite", "U_outside")


def edge_case(B, nu, H, K, first=0, seed=0):
    """Actuator u gets edge box EDGE_KINDS[(first + u) % 7]:
      wide        [-100, 100] around |s| < ~5: untouched, count 0
      no_zero     [-2.8, -0.9] (a Go1 calf joint): a box that excludes zero
      pinned      lo == hi = 0.25
      upper_only  (-inf, 0.1]     lower_only  [0, +inf)     infinite  (-inf, +inf): count 0, the array unchanged
      U_outside   [-1, 1] with U = 50 on the whole row: every finite element projects (count H K less the NaNs)
    Every row also carries a NaN (stays a NaN, uncounted), a +inf (-> hi - U unless hi = +inf) and a -inf where the
    shape has room (K >= 3).  Returns U, eps, lo, hi and the kinds per actuator."""
    rs = np.random.RandomState(2000 + seed)
    U = (0.5 * rs.randn(B, nu, H)).astype(np.float32)
    eps = rs.randn(B, nu, H, K).astype(np.float32)
    inf = np.float32(np.inf)
    box = {"wide": (-100.0, 100.0), "no_zero": (-2.8, -0.9), "pinned": (0.25, 0.25), "upper_only": (-inf, 0.1),
           "lower_only": (0.0, inf), "infinite": (-inf, inf), "U_outside": (-1.0, 1.0)}
    kinds = [EDGE_KINDS[(first + u) % len(EDGE_KINDS)] for u in range(nu)]
    lo = np.array([box[k][0] for k in kinds], np.float32)
    hi = np.array([box[k][1] for k in kinds], np.float32)
    for u, k in enumerate(kinds):
        if k == "U_outside":
            U[:, u, :] = 50.0
    if K >= 3:
        eps[:, :, :, 0] = np.nan
        eps[:, :, H - 1, 1] = inf
        eps[:, :, 0, 2] = -inf
    return U, eps, lo, hi, kinds


def bits(a):
    """float32 array -> its bit patterns (NaNs compare equal when their bits do)"""
    return np.ascontiguousarray(a, np.float32).view(np.uint32)
