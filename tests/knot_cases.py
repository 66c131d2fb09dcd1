"""Cases shared by tests/test_noise_knots.py (host) and tests/test_gpu_noise_knots.py (device): the smallest shapes at
which the knot law (csrc/noise_knots.h, noise_knot_kernel) can go wrong."""
import numpy as np

K, B = 130, 2            # K: no multiple of 4 (pad lanes K..Kp = 192 exist); B: more than one (b, u) row per launch
HS = (1, 7, 9)           # one step; odd; a multiple of P = 3
ORDERS = (0, 1, 3)
RHOS = (0.0, 0.9)


def knot_counts(H):
    """P in {1, 2, 3, H} as far as P <= H: one knot, the fewest that interpolate, a window that slides for order 3 and
    the identity."""
    return sorted({P for P in (1, 2, 3, H) if P <= H})


GRID = [(H, P) for H in HS for P in knot_counts(H)]   # (H, P)
TABLE_GRID = GRID + [(64, 8)]                         # ... and config #4's horizon with 8 knots


def sigma_u(nu):
    """non-uniform per-actuator scales (float32)"""
    return np.array([0.7, 0.2, 1.3][:nu], np.float32)


def bits(a):
    """float32 array -> its bit patterns"""
    return np.ascontiguousarray(a, np.float32).view(np.uint32)
