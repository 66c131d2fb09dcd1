"""Cost families and the case grid of elite truncation, shared by tests/test_elites.py (the numpy reference and the host
form of the rule) and tests/test_gpu_elites.py (the kernel).  Not a test module."""
import numpy as np

from ess_cases import FAMILIES as ESS_FAMILIES
from ess_cases import family as ess_family

FAMILIES = ESS_FAMILIES + ("quantised", "signed")
KS = (1, 30, 75, 1100, 2500, 4096, 4097, 32768)


def family(name, K, B=2, seed=0):
    """costs [B, K] float32, rows differing per b: the five families of ess_cases, and
    quantised  round(gauss * 4) / 4: many duplicates at every rank
    signed     gauss - 50: both signs, zeros possible only by accident"""
    if name in ESS_FAMILIES:
        return ess_family(name, K, B, seed)
    rs = np.random.RandomState(7000 + 1000 * FAMILIES.index(name) + K + seed)
    g = 50.0 + 10.0 * rs.randn(B, K)
    c = np.round(g * 4.0) / 4.0 if name == "quantised" else g - 50.0
    return c.astype(np.float32)


def n_elites(c):
    """The n_elite values of one [B, K] case: {1, 2, K // 10, n - 1, n, n + 1, K} with n the finite count of row 0,
    kept where they lie in 1..K."""
    K = c.shape[1]
    n = int(np.isfinite(c[0]).sum())
    return sorted({v for v in (1, 2, K // 10, n - 1, n, n + 1, K) if 1 <= v <= K})


def hand_rows():
    """(name, row, n_elite, idx, count, tau, ecost-as-a-list-with-None-for-inf): rows written out by hand."""
    nan, inf = float("nan"), float("inf")
    den = float(np.float32(1e-45))  # the smallest denormal
    return [
        ("five equal minima, three admitted: the lowest indices",
         [3.0, 1.0, 2.0, 1.0, 1.0, 5.0, 1.0, 1.0], 3, [1, 3, 4], 3, 1.0, [None, 1.0, None, 1.0, 1.0, None, None, None]),
        ("ties straddle the threshold behind a strict minimum",
         [2.0, 0.5, 2.0, 2.0], 3, [0, 1, 2], 3, 2.0, [2.0, 0.5, 2.0, None]),
        ("-0.0 and +0.0 are one cost: index order decides",
         [0.0, -0.0, 1.0, -0.0, -1.0], 3, [0, 1, 4], 3, 0.0, [0.0, -0.0, None, None, -1.0]),
        ("negative costs", [-1.0, -3.0, -2.0, 4.0], 2, [1, 2], 2, -2.0, [None, -3.0, -2.0, None]),
        ("denormals order by value",
         [den, 0.0, -den, 2 * den], 2, [1, 2], 2, 0.0, [None, 0.0, -den, None]),
        ("... and are not flushed onto zero",
         [den, 0.0, 2 * den, 3 * den], 2, [0, 1], 2, den, [den, 0.0, None, None]),
        ("NaN, +inf and -inf are never elite",
         [nan, 4.0, -inf, inf, 3.0, nan, 5.0], 2, [1, 4], 2, 4.0, [None, 4.0, None, None, 3.0, None, None]),
        ("n_elite beyond the finite count: every finite sample",
         [nan, 4.0, -inf, inf, 3.0], 4, [1, 4, -1, -1], 2, 4.0, [None, 4.0, None, None, 3.0]),
        ("no finite cost", [nan, inf, -inf], 2, [-1, -1], 0, inf, [None, None, None]),
        ("K = 1", [7.0], 1, [0], 1, 7.0, [7.0]),
        ("K = 1, not finite", [nan], 1, [-1], 0, inf, [None]),
    ]
