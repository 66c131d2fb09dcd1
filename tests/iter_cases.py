"""Cases of the best-sample tracking of mppi_set_iterations, shared by tests/test_iterations.py (the numpy reference and
the host form of the rule) and tests/test_gpu_iterations.py (the kernel).  Not a test module."""
import numpy as np

from elite_cases import family
from keep_cases import bits, inputs, same_bits  # noqa: F401  (re-exported for the two test modules)

NAN, INF = float("nan"), float("inf")


def hand_cases():
    """(name, U [nu][H], noise [nu][H][K], costs [K], clamp, stored or None, it, (v [nu][H], cost, k, iter)): rows
    written out by hand (every sum is exact in float32)."""
    U = [[1.0, 2.0, 4.0]]
    eps = [[[0.5, -1.0, 0.25, 8.0], [0.5, 0.5, -2.0, 8.0], [1.0, -4.0, 0.0, 8.0]]]  # [1][3][4]
    old = ([[7.0, 7.0, 7.0]], 2.0, 9, 0)
    zero = [[0.0, 0.0, 0.0]]
    return [
        ("a tie at the minimum: the lowest k wins", U, eps, [3.0, 1.0, 1.0, 9.0], 0.0, None, 0,
         ([[0.0, 2.5, 0.0]], 1.0, 1, 0)),
        ("-0.0 against +0.0: one cost, the lower k; the stored cost keeps its sign bit", U, eps, [0.0, 1.0, -0.0, 5.0],
         0.0, None, 2, ([[1.5, 2.5, 5.0]], 0.0, 0, 2)),
        ("... whichever comes first", U, eps, [1.0, -0.0, 0.0, 5.0], 0.0, None, 1, ([[0.0, 2.5, 0.0]], -0.0, 1, 1)),
        ("NaN and +-inf mixed in are never candidates", U, eps, [NAN, -INF, 4.0, INF], 0.0, None, 3,
         ([[1.25, 0.0, 4.0]], 4.0, 2, 3)),
        ("all non-finite with reset: the reset state", U, eps, [NAN, INF, -INF, NAN], 0.0, None, 0,
         (zero, INF, -1, -1)),
        ("all non-finite without reset: the stored best stays", U, eps, [NAN, INF, -INF, NAN], 0.0, old, 1, old),
        ("strictness: an equal cost does not replace", U, eps, [5.0, 2.0, 3.0, 4.0], 0.0, old, 1, old),
        ("a lower cost replaces", U, eps, [5.0, 1.5, 3.0, 4.0], 0.0, old, 1, ([[0.0, 2.5, 0.0]], 1.5, 1, 1)),
        ("a stored +0.0 is not replaced by -0.0", U, eps, [-0.0, 1.0, 2.0, 3.0], 0.0, (zero, 0.0, 4, 0), 1,
         (zero, 0.0, 4, 0)),
        ("anything finite replaces a stored +inf", U, eps, [9.0, 8.0, 3e38, 7.0], 0.0, (zero, INF, -1, -1), 2,
         ([[9.0, 10.0, 12.0]], 7.0, 3, 2)),
        ("ctrl_clamp on with a sample beyond it, both sides", U, eps, [9.0, 8.0, 7.0, 1.0], 3.0, None, 0,
         ([[3.0, 3.0, 3.0]], 1.0, 3, 0)),
        ("... and the other side", U, eps, [9.0, 1.0, 7.0, 8.0], 2.0, None, 0, ([[0.0, 2.0, 0.0]], 1.0, 1, 0)),
        ("K = 1", [[1.0], [-2.0]], [[[0.5]], [[0.25]]], [3.0], 0.0, None, 0, ([[1.5], [-1.75]], 3.0, 0, 0)),
        ("K = 1, not finite", [[1.0], [-2.0]], [[[0.5]], [[0.25]]], [NAN], 0.0, None, 0, ([[0.0], [0.0]], INF, -1, -1)),
    ]


def stored_for(U, eps, costs):
    """A stored best (v, cost, k, iter) for a reset = 0 run on costs [B, K]: solve 0 holds a cost between its row's
    best and worst finite cost (the candidate replaces it unless the row has one finite value), solve 1 exactly its
    row's minimum (strictness: it stays), further solves +inf; a row without a finite cost holds 1.0."""
    B, nu, H = U.shape
    v = (np.arange(B * nu * H, dtype=np.float32).reshape(B, nu, H) * np.float32(0.25) - np.float32(1.0))
    cost = np.full(B, np.inf, np.float32)
    for b in range(B):
        fin = costs[b][np.isfinite(costs[b])]
        if fin.size == 0:
            cost[b] = np.float32(1.0)
        elif b == 0:
            cost[b] = np.sort(fin)[fin.size // 2]
        elif b == 1:
            cost[b] = fin.min()
    k = (np.arange(B, dtype=np.int32) * 3 + 1).astype(np.int32)
    it = np.zeros(B, np.int32)
    return v, cost, k, it


def grid():
    """(name, B, nu, H, K, ctrl_clamp, costs [B, K], reset): the grid the host form and the kernel are held to."""
    out = []
    for K, H in ((1, 1), (5, 1), (30, 3), (130, 7)):
        for fam in ("gauss", "ties", "nan", "quantised", "signed", "none"):
            if fam == "none":  # an all-non-finite row beside a normal one
                c = family("gauss", K)
                c[0, :] = np.array([np.nan, np.inf, -np.inf], np.float32)[np.arange(K) % 3]
            else:
                c = family(fam, K)
                if fam == "nan" and K >= 5:  # (the other non-finite costs too)
                    c[:, 1], c[:, K - 2] = np.inf, -np.inf
            for clamp in (0.0, 1.25):
                for reset in (1, 0):
                    out.append((f"{fam}-K{K}-H{H}-c{clamp}-r{reset}", 2, 3, H, K, clamp, c, reset))
    return out
