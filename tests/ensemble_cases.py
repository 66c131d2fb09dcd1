"""Shared cases of the ensemble's combining rule (csrc/ensemble.h): rows written out by hand with the answer beside them,
and a seeded grid.  tests/test_ensemble.py runs them through the numpy restatement and the sanitised host program,
tests/test_gpu_ensemble.py through the kernel (mppi_ensemble_eval).  Every comparison is bitwise."""
import numpy as np

MODES = ("mean", "mean_std", "worst")
INF = float("inf")
NAN = float("nan")
BIG = 3.0e38  # two of them overflow fp32
BIG2 = 2.9e38  # ... and so do BIG and this one, which are not the same number


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def same_bits(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def hand_cases():
    """(name, members [n][K], mode, kappa, cost [K], sd [K]): every answer follows from the rule with exact arithmetic
    (small integers and powers of two: no rounding anywhere), or from its non-finite branches."""
    c = []
    # two members a step apart: mean 2, deviations -1 and +1, q = 2, q r = 1
    c.append(("n2 mean", [[1.0, 8.0], [3.0, 8.0]], "mean", 0.0, [2.0, 8.0], [1.0, 0.0]))
    c.append(("n2 mean_std", [[1.0, 8.0], [3.0, 8.0]], "mean_std", 0.5, [2.5, 8.0], [1.0, 0.0]))
    c.append(("n2 optimism", [[1.0, 8.0], [3.0, 8.0]], "mean_std", -0.5, [1.5, 8.0], [1.0, 0.0]))
    c.append(("n2 worst", [[1.0, 8.0], [3.0, 8.0]], "worst", 0.0, [3.0, 8.0], [1.0, 0.0]))
    c.append(("n2 worst, the larger first", [[3.0, -2.0], [1.0, -4.0]], "worst", 7.0, [3.0, -2.0], [1.0, 1.0]))
    # ties and zeros: -0 + -0 = -0, -0 r = -0; the deviations are +0; of two zeros the maximum is +0
    c.append(("zeros, mean", [[-0.0, -0.0, 0.0], [-0.0, 0.0, -0.0]], "mean", 0.0, [-0.0, 0.0, 0.0], [0.0, 0.0, 0.0]))
    c.append(("zeros, worst", [[-0.0, -0.0, 0.0], [-0.0, 0.0, -0.0]], "worst", 0.0, [-0.0, 0.0, 0.0], [0.0, 0.0, 0.0]))
    c.append(("zeros, mean_std", [[-0.0, -0.0], [-0.0, 0.0]], "mean_std", 1.0, [0.0, 0.0], [0.0, 0.0]))  # fmaf(1, +0, -0) = +0
    # a member that is not finite takes the sample out, whatever the mode
    for mode in MODES:
        c.append((f"+inf member, {mode}", [[1.0, 1.0], [INF, 2.0], [2.0, 3.0]], mode, 0.5,
                  [INF, {"mean": 2.0, "mean_std": None, "worst": 3.0}[mode]], [INF, None]))
        c.append((f"nan member, {mode}", [[NAN, 4.0], [1.0, 4.0]], mode, 0.5, [INF, 4.0], [INF, 0.0]))
        c.append((f"-inf member, {mode}", [[5.0, 4.0], [-INF, 4.0]], mode, -1.0, [INF, 4.0], [INF, 0.0]))
    # a sum that overflows: the mean and the spread are +inf, the maximum is still the members'
    c.append(("overflow, mean", [[BIG], [BIG2]], "mean", 0.0, [INF], [INF]))
    c.append(("overflow, worst", [[BIG2], [BIG]], "worst", 0.0, [BIG], [INF]))
    c.append(("overflow, mean_std", [[BIG], [BIG2]], "mean_std", 0.5, [INF], [INF]))
    c.append(("overflow, optimism", [[BIG], [BIG2]], "mean_std", -0.5, [INF], [INF]))  # -inf + inf = NaN -> +inf
    c.append(("overflow, kappa 0", [[BIG], [BIG2]], "mean_std", 0.0, [INF], [INF]))  # 0 inf = NaN -> +inf
    c.append(("overflow downwards, mean", [[-BIG], [-BIG2]], "mean", 0.0, [INF], [INF]))  # -inf -> +inf
    c.append(("overflow downwards, worst", [[-BIG], [-BIG2]], "worst", 0.0, [-BIG2], [INF]))
    # identical members are the single model, whatever n and the mode: the mean of n equal numbers is that number (0.1
    # is not a dyadic number: 3 x 0.1f rounds), also where their sum would overflow
    for n in (2, 3, 4, 8):
        for mode in MODES:
            zero = 0.0 if mode == "mean_std" else -0.0  # fmaf(kappa, +0, -0) = +0: the one cost that is not c itself
            c.append((f"identical n{n} {mode}", [[0.1, -7.3, BIG, -0.0]] * n, mode, 2.0, [0.1, -7.3, BIG, zero],
                      [0.0, 0.0, 0.0, 0.0]))
    # ... and one member a bit apart is not identical: the sums as written (3 x 0.5 and 3 x 0.25 are exact)
    c.append(("n3 two equal", [[0.5, 0.25], [0.5, 0.25], [0.5, 1.0]], "worst", 0.0, [0.5, 1.0], [0.0, None]))
    # eight members 1..8: mean 4.5, q = 42, q r = 5.25
    c.append(("n8 mean", [[float(e + 1)] for e in range(8)], "mean", 0.0, [4.5], [float(np.sqrt(np.float32(5.25)))]))
    c.append(("n8 worst", [[float(e + 1)] for e in range(8)], "worst", 0.0, [8.0], [float(np.sqrt(np.float32(5.25)))]))
    return c


def assert_hand(name, got_cost, got_sd, want_cost, want_sd):
    """A None in the answer: that entry is not written out by hand (it rounds)."""
    for k, (wc, ws) in enumerate(zip(want_cost, want_sd)):
        if wc is not None:
            assert bits(got_cost)[k] == bits(np.float32(wc))[()], (name, "cost", k, got_cost, want_cost)
        if ws is not None:
            assert bits(got_sd)[k] == bits(np.float32(ws))[()], (name, "sd", k, got_sd, want_sd)


def grid(K=130, B=2):
    """(name, n, mode, kappa, members [n, B, K] float32): every n in 2..8 and mode; costs of the rollouts' magnitude with,
    per row, a NaN, a +inf and a -inf member somewhere, a tie between all members, an all-zero sample with mixed signs,
    identical members, a sum that overflows and a spread that does."""
    out = []
    for n in range(2, 9):
        for mi, mode in enumerate(MODES):
            rs = np.random.RandomState(100 * n + mi)
            m = (50.0 + 10.0 * rs.randn(n, B, K)).astype(np.float32)
            m *= (1.0 + 0.05 * rs.randn(n, 1, 1)).astype(np.float32)  # members that disagree systematically
            if K >= 16:
                m[rs.randint(n), 0, 3] = np.nan
                m[rs.randint(n), 0, 5] = np.inf
                m[rs.randint(n), B - 1, 7] = -np.inf
                m[:, 0, 9] = m[0, 0, 9]
                m[:, B - 1, 11] = np.where(np.arange(n) % 2, -0.0, 0.0)
                m[:, 0, 13] = BIG
                m[:, B - 1, 15] = np.where(np.arange(n) % 2, -BIG, BIG)
                m[:, :, K - 1] = m[0, :, K - 1]  # the last sample before the pads: identical members
            else:
                m[rs.randint(n), 0, 1] = np.nan
                m[:, B - 1, 2] = m[0, B - 1, 2]
            kappa = (0.0, 0.5, -0.75, 2.0)[(n + mi) % 4]
            out.append((f"n{n} {mode} kappa {kappa}", n, mode, kappa, m))
    return out
