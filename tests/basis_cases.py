"""Cases shared by tests/test_noise_basis.py (host) and tests/test_gpu_noise_basis.py (device): the smallest shapes at
which the basis law (csrc/noise_basis.h; noise_basis_mfma_kernel, noise_basis_kernel) can go wrong."""
import numpy as np

K, B = 130, 2            # K: no multiple of 4 (pad lanes K..Kp = 192 exist); B: more than one (b, u) row per launch
HS = (1, 7, 9)           # one step; odd; none a multiple of the kernels' tile of 16 steps
# (H, R): the MFMA form's 64 and 128 accumulators; the VALU form's LDS worst case of each block width (R <= 64: 256 k)
BIG = ((64, 64), (128, 128))
TAIL = (20, 5)           # (H, R): two tiles of steps, the second partly stored
TALL = (130, 3)          # (H, R): past the 128 steps of the MFMA form
WIDE = (9, 3, 1100)      # (H, R, K): Kp = 1152, more than one block along k, the last one partly idle


def basis_counts(H):
    """R in {1, 2, 3, H} as far as R <= H: one column, a chain of one fmaf, of two, and a square table."""
    return sorted({R for R in (1, 2, 3, H) if R <= H})


GRID = [(H, R) for H in HS for R in basis_counts(H)]   # (H, R)


def table(H, R, seed=0):
    """a random table M [H, R] (float32) from a fixed RandomState"""
    return np.random.RandomState(1000 * H + 10 * R + seed).randn(H, R).astype(np.float32)


def sparse_table(H, R):
    """a random table with its first column and one row zero and one more entry per row -0: chains that begin with,
    pass through and consist of signed zeros (the MFMA form starts its accumulators at -0 and pads R with -0)"""
    M = table(H, R, seed=3)
    M[:, 0] = 0.0
    M[H // 2, :] = 0.0
    M[np.arange(H), np.arange(H) % R] = -0.0
    return M


def sigma_u(nu):
    """non-uniform per-actuator scales (float32)"""
    return np.array([0.7, 0.2, 1.3][:nu], np.float32)


def bits(a):
    """float32 array -> its bit patterns"""
    return np.ascontiguousarray(a, np.float32).view(np.uint32)
