"""Cases of keep / shift elites (mppi_set_elite_keep), shared by tests/test_elite_keep.py (the numpy references and the
host form of the rule) and tests/test_gpu_elite_keep.py (the kernels).  Not a test module."""
import numpy as np

from elite_cases import family

NAN, INF = float("nan"), float("inf")


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def same_bits(a, b):
    """Bitwise equality of two float32 arrays; a NaN equals a NaN whatever its payload (the host compiler, numpy and the
    device may each form another quiet NaN from the same operation)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def inputs(B, nu, H, K, seed=0, scale=1.0):
    """(U [B, nu, H], noise [B, nu, H, K]) float32, seeded; some exact zeros and a -0.0 in both."""
    rs = np.random.RandomState(9100 + 97 * B + 31 * nu + 7 * H + K + seed)
    U = (0.5 * rs.randn(B, nu, H)).astype(np.float32)
    eps = (scale * rs.randn(B, nu, H, K)).astype(np.float32)
    eps[:, :, :, ::7] *= np.float32(3.0)
    U.flat[0] = np.float32(-0.0)
    eps.flat[:: max(eps.size // 13, 1)] = np.float32(0.0)
    eps.flat[1] = np.float32(-0.0)
    return U, eps


def grid():
    """(name, B, nu, H, K, n_keep, shift, ctrl_clamp, costs [B, K]): the grid the host form and the kernels are held to."""
    out = []
    for K, H in ((1, 1), (5, 1), (30, 3), (130, 8)):
        for fam in ("gauss", "ties", "nan", "quantised", "signed"):
            c = family(fam, K)
            if fam == "nan" and K >= 5:  # (the other non-finite costs too)
                c[:, 1], c[:, K - 2] = np.inf, -np.inf
            n = int(np.isfinite(c[0]).sum())
            for n_keep in sorted({v for v in (1, 2, 17, n, n + 1, K) if 1 <= v <= K}):
                for shift in (0, 1):
                    for clamp in (0.0, 1.25):
                        out.append((f"{fam}-K{K}-H{H}-n{n_keep}-s{shift}-c{clamp}", 2, 3, H, K, n_keep, shift, clamp, c))
    return out


def hand_cases():
    """(name, U [nu][H], noise [nu][H][K], costs [K], n_keep, shift, clamp, v [nu][H][n_keep], kcost, idx, count,
    steps): rows written out by hand (every sum is exact in float32)."""
    U = [[1.0, 2.0, 4.0]]
    eps = [[[0.5, -1.0, 0.25, 8.0], [0.5, 0.5, -2.0, 8.0], [1.0, -4.0, 0.0, 8.0]]]  # [1][3][4]
    cases = [
        ("shift 0: the two best in ascending k", U, eps, [3.0, 1.0, 2.0, 9.0], 2, 0, 0.0,
         [[[0.0, 1.25], [2.5, 0.0], [0.0, 4.0]]], [1.0, 2.0], [1, 2], 2, 3),
        ("shift 1: step t holds step t + 1, the last row is +0.0", U, eps, [3.0, 1.0, 2.0, 9.0], 2, 1, 0.0,
         [[[2.5, 0.0], [0.0, 4.0], [0.0, 0.0]]], [1.0, 2.0], [1, 2], 2, 2),
        ("count < n_keep from NaN and +-inf costs", U, eps, [NAN, 5.0, -INF, INF], 3, 0, 0.0,
         [[[0.0, 0.0, 0.0], [2.5, 0.0, 0.0], [0.0, 0.0, 0.0]]], [5.0, INF, INF], [1, -1, -1], 1, 3),
        ("ties at the threshold go to the lower k", U, eps, [2.0, 2.0, 2.0, 1.0], 2, 0, 0.0,
         [[[1.5, 9.0], [2.5, 10.0], [5.0, 12.0]]], [2.0, 1.0], [0, 3], 2, 3),
        ("ctrl_clamp on with a sample beyond it", U, eps, [9.0, 8.0, 7.0, 1.0], 1, 0, 3.0,
         [[[3.0], [3.0], [3.0]]], [1.0], [3], 1, 3),
        ("ctrl_clamp on, both sides", U, eps, [9.0, 1.0, 7.0, 8.0], 1, 0, 2.0,
         [[[0.0], [2.0], [0.0]]], [1.0], [1], 1, 3),
        ("no finite cost: count 0, v all +0.0", U, eps, [NAN, INF, NAN, -INF], 2, 0, 0.0,
         [[[0.0, 0.0], [0.0, 0.0], [0.0, 0.0]]], [INF, INF], [-1, -1], 0, 3),
        ("H = 1 with shift: steps 0, nothing stored", [[1.0]], [[[0.5, -1.0]]], [2.0, 1.0], 1, 1, 0.0,
         [[[0.0]]], [1.0], [1], 1, 0),
        ("-0.0 + -0.0 stays -0.0 without a clamp", [[-0.0]], [[[-0.0, 1.0]]], [1.0, 2.0], 1, 0, 0.0,
         [[[-0.0]]], [1.0], [0], 1, 1),
        ("... and reads +0.0 through the clamp's c + (s - s)", [[-0.0]], [[[-0.0, 1.0]]], [1.0, 2.0], 1, 0, 5.0,
         [[[0.0]]], [1.0], [0], 1, 1),
    ]
    return cases


def hand_inject_cases():
    """(name, U [nu][H], noise [nu][H][K], v [nu][H][n_keep], count, steps, out [nu][H][K])."""
    U = [[1.0, 2.0, 4.0]]
    eps = [[[9.0, 9.5, -0.0], [8.0, 8.5, NAN], [7.0, 7.5, INF]]]
    v = [[[1.5, 0.0], [2.0, 2.5], [-4.0, 5.0]]]
    return [
        ("both columns, every step", U, eps, v, 2, 3, [[[0.5, -1.0, -0.0], [0.0, 0.5, NAN], [-8.0, 1.0, INF]]]),
        ("count 1: column 1 untouched", U, eps, v, 1, 3, [[[0.5, 9.5, -0.0], [0.0, 8.5, NAN], [-8.0, 7.5, INF]]]),
        ("steps 2: the last row keeps its fresh noise", U, eps, v, 2, 2,
         [[[0.5, -1.0, -0.0], [0.0, 0.5, NAN], [7.0, 7.5, INF]]]),
        ("count 0: nothing", U, eps, v, 0, 3, eps),
        ("steps 0: nothing", U, eps, v, 2, 0, eps),
    ]
