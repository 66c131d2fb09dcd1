"""Cost families and the float64 acceptance check of ESS targeting, shared by tests/test_ess_target.py (the host form
of the rule) and tests/test_gpu_ess_target.py (the kernel).  Not a test module."""
import numpy as np

FAMILIES = ("gauss", "gaps", "lognormal", "ties", "nan")
FRACS = (0.02, 0.1, 0.5)
BOUNDS = (1e-4, 1e4)
N_TIES = 5


def family(name, K, B=2, seed=0):
    """costs [B, K] float32 of one family:
    gauss      50 +- 10
    gaps       cumulative exponential gaps of mean 200 (one-hot weights at any moderate lambda)
    lognormal  exp(3 N(0, 1))
    ties       gauss with N_TIES (or K, if fewer) exact ties one below its minimum
    nan        gauss with 20 % NaN (at least one entry kept finite)"""
    rs = np.random.RandomState(1000 * FAMILIES.index(name) + K + seed)
    if name == "gaps":
        c = np.cumsum(rs.exponential(200.0, (B, K)), axis=1)
        c = np.take_along_axis(c, np.argsort(rs.rand(B, K), axis=1), axis=1)  # (not sorted along k)
    elif name == "lognormal":
        c = np.exp(3.0 * rs.randn(B, K))
    else:
        c = 50.0 + 10.0 * rs.randn(B, K)
    c = c.astype(np.float32)
    if name == "ties":
        for b in range(B):
            idx = rs.permutation(K)[:min(N_TIES, K)]
            c[b, idx] = np.float32(np.floor(c[b].min()) - 1.0)
    if name == "nan":
        mask = rs.rand(B, K) < 0.2
        mask[:, 0] = False
        c[mask] = np.nan
    return c


def check_row(costs, lam, ess_frac, lambda_min, lambda_max):
    """The two float64 conditions on one row's lambda; returns |ESS64(lam) - T| / T at an interior lambda (else None).
        ess_ref(c, lam (1 + 1e-5)) >= T (1 - 1e-4)   unless lam is lambda_max
        ess_ref(c, lam (1 - 1e-5)) <= T (1 + 1e-4)   unless lam is lambda_min
    1e-5 follows from the search's 2e-6 bracket, 1e-4 is the bar the statistics' ess holds against float64."""
    from mppi_hip.stats import ess_ref, ess_target_ref
    lam = float(lam)
    lo, hi = float(np.float32(lambda_min)), float(np.float32(lambda_max))
    assert lo <= lam <= hi, (lam, lo, hi)
    T = ess_target_ref(costs, ess_frac)
    up, down = ess_ref(costs, lam * (1.0 + 1e-5)), ess_ref(costs, lam * (1.0 - 1e-5))
    if lam != hi:
        assert up >= T * (1.0 - 1e-4), ("ESS above lambda falls short of the target", lam, up, T)
    if lam != lo:
        assert down <= T * (1.0 + 1e-4), ("ESS below lambda already exceeds the target", lam, down, T)
    return abs(ess_ref(costs, lam) - T) / T if lo < lam < hi else None
