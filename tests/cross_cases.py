"""Cases shared by the host and device tests of the weighted cross moments (csrc/cross_moments.h, cross_moment_kernel)
and of the covariance adapted from them (csrc/noise_cov_adapt.h, noise_cov_adapt_kernel): the smallest shapes at which
they can go wrong, the reference computed once per shape."""
import functools
import os
import subprocess

import numpy as np

from cov_cases import B, HS, K, NUS, bits, sigma_of  # noqa: F401  (re-exported)

# (nu, H, K).  K = 130 pads to Kp = 192: one wave-chunk with inactive lanes; H = 1 and 7: one step, segments of one
# step.  H = 33 with K = 1030 (Kp = 1088): five wave-chunks, the last with 16 of 64 lanes, and 11 segments of L = 3
# steps, so more than 64 cells per pair (the finish pass wraps) -- at nu = 21 and 32, where the triangle has more than
# one 8 x 8 tile, a ragged last row block (21 = 8 + 8 + 5) and, at 32, more tiles than one block's waves
SHAPES = [(nu, H, K) for nu in NUS for H in HS] + [(21, 33, 1030), (32, 33, 1030)]
FORMS = ("direct", "seg", None)  # MPPI_CROSS_FORM; None: the launcher's own choice
_TESTS = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(_TESTS, "native", "cross_adapt_host.cpp")
CSRC = os.path.join(os.path.dirname(_TESTS), "humanoid_mppi-rl_amd", "csrc")


def shape_id(s):
    return "nu%d-H%d-K%d" % s


@functools.lru_cache(maxsize=None)
def case(nu, H, K_):
    """(costs [B, K], noise [B, nu, H, K]) float32, random: costs around 100 with a few non-finite entries (their
    weights are 0), noise with correlated rows so that the off-diagonal moments are far from 0."""
    rs = np.random.RandomState(7000 + 100 * nu + H + K_)
    costs = (100.0 + 5.0 * rs.randn(B, K_)).astype(np.float32)
    costs[0, 0], costs[B - 1, K_ - 1], costs[0, K_ // 2] = np.nan, np.inf, -np.inf
    z = rs.randn(B, nu, H, K_)
    noise = (z + 0.5 * np.roll(z, 1, axis=1)).astype(np.float32)
    for a in (costs, noise):
        a.setflags(write=False)
    return costs, noise


@functools.lru_cache(maxsize=None)
def exact_case(nu, H, K_):
    """(costs, w, noise): costs that are one finite value or +inf, so the device's weights are known to the bit --
    every finite cost equals the minimum, its unnormalised weight is __expf(-0) = 1 exactly, and w = 1 / n_finite by
    one correctly rounded fp32 division (norm_eps = 0): the inputs of the bitwise comparison with cross_moments_f32."""
    rs = np.random.RandomState(9000 + 100 * nu + H + K_)
    costs = np.full((B, K_), 3.5, np.float32)
    costs[rs.rand(B, K_) < 0.4] = np.inf
    costs[:, 1] = 3.5
    n = np.isfinite(costs).sum(axis=1).astype(np.float32)
    w = np.where(np.isfinite(costs), (np.float32(1.0) / n)[:, None], np.float32(0.0)).astype(np.float32)
    noise = case(nu, H, K_)[1]
    for a in (costs, w):
        a.setflags(write=False)
    return costs, w, noise


@functools.lru_cache(maxsize=None)
def exact_want(nu, H, K_):
    """cross_moments_f32 of exact_case, once per shape"""
    from mppi_hip.stats import cross_moments_f32
    _, w, noise = exact_case(nu, H, K_)
    out = cross_moments_f32(w, noise)
    out.setflags(write=False)
    return out


def moments_like(nu, seed, scale=0.3, Bn=B):
    """eps_mx-like input of the update rule: Bn symmetric positive definite float32 matrices [Bn, nu, nu], symmetric
    bit for bit"""
    rs = np.random.RandomState(seed)
    A = rs.randn(Bn, nu, nu + 5)
    M = np.einsum("bij,bkj->bik", A, A) / (nu + 5) * scale
    lo = np.tril(M).astype(np.float32)
    return lo + np.tril(lo, -1).transpose(0, 2, 1)


# ---- tests/native/cross_adapt_host.cpp: the two headers through g++

def rows(lines, n):
    return np.array([[float.fromhex(x) for x in ln.split()] for ln in lines[:n]], np.float64).astype(np.float32)


def build_host(d):
    """tests/native/cross_adapt_host.cpp through g++ in directory d -> the program's path"""
    exe = str(d / "cross_adapt_host")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-I", CSRC, SRC, "-o", exe],
                       capture_output=True, text=True)
    if r.returncode != 0:
        raise AssertionError(r.stderr)
    return exe


def host_cross(exe, d, w, noise, env=None):
    """the program's cross mode: w [B, K], noise [B, nu, H, K] -> mx [B, nu, nu] float32"""
    Bn, nu, H, K = noise.shape
    Kp = (K + 63) // 64 * 64
    wp = np.zeros((Bn, Kp), np.float32)
    wp[:, :K] = w
    ep = np.zeros((Bn, nu, H, Kp), np.float32)
    ep[..., :K] = noise
    wp.tofile(d / "w.f32")
    ep.tofile(d / "noise.f32")
    r = subprocess.run([exe, "cross", str(Bn), str(nu), str(H), str(Kp), str(d / "w.f32"), str(d / "noise.f32")],
                       capture_output=True, text=True, timeout=240, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    return rows(r.stdout.strip().splitlines(), Bn * nu).reshape(Bn, nu, nu)
