"""The engine's sampling law on the host (include/mppi.h mppi_set_noise_model; csrc/noise_model.h).

    e[0] = z[0];   e[t] = rho * e[t-1] + sqrt(1 - rho^2) * z[t];   eps = sigma_u[u] * e[t]

Every step has unit variance before scaling and corr(e[t], e[s]) = rho^|t-s|.  The device runs the recursion in fp32;
this restatement is float64 (the reference for tests, and the filter of MPPIModel's noise="numpy" mode).

The knot law (mppi_set_noise_knots; csrc/noise_knots.h) draws the row at P knots and interpolates it to the H steps:
knot_table and knot_filter restate it in float32, operation by operation, bitwise what the device draws.

The horizon basis (mppi_set_noise_basis; csrc/noise_basis.h) applies a dense M [H, R] along the horizon to R white
normals: basis_filter restates it bitwise, colored_basis builds the table of iCEM's power-law noise.

The cross-actuator covariance (mppi_set_noise_cov; csrc/noise_cov.h) mixes the unit-variance rows of the actuators with
the Cholesky factor of a full Sigma: cov_factor, cov_mix and cov_filter restate it the same way, bitwise.

The per-step scale (mppi_set_noise_steps) replaces sigma_u[u] by a table S[b][u][t]: steps_filter restates it, bitwise
the device's on float32 normals and ar1_filter's own arithmetic otherwise.
"""
from __future__ import annotations

import numpy as np


def ar1_filter(z, rho: float = 0.0, sigma_u=None) -> np.ndarray:
    """Apply the law to standard normals z [..., nu, H, K] (float64 result of the same shape).

    sigma_u: scalar or [nu] per-actuator standard deviations (None = 1); it broadcasts along the actuator axis only.
    rho = 0 returns sigma_u * z exactly."""
    z = np.asarray(z, np.float64)
    if z.ndim < 3:
        raise ValueError("ar1_filter: z must be [..., nu, H, K]")
    rho = float(rho)
    if not 0.0 <= rho < 1.0:
        raise ValueError("ar1_filter: rho must be in [0, 1)")
    nu, H = z.shape[-3], z.shape[-2]
    s = np.ones(nu) if sigma_u is None else np.asarray(sigma_u, np.float64).ravel()
    if s.size == 1:
        s = np.full(nu, s[0])
    if s.shape != (nu,):
        raise ValueError(f"ar1_filter: sigma_u must have {nu} entries, got {s.size}")
    if not (np.all(np.isfinite(s)) and np.all(s >= 0.0)):
        raise ValueError("ar1_filter: sigma_u entries must be finite and >= 0")
    e = z.copy()
    if rho != 0.0:
        c = np.sqrt(1.0 - rho * rho)
        for t in range(1, H):
            e[..., t, :] = rho * e[..., t - 1, :] + c * z[..., t, :]
    return s[:, None, None] * e


# ---- the knot law (include/mppi.h mppi_set_noise_knots; csrc/noise_knots.h), restated bit for bit

def knot_table(H: int, P: int, order: int) -> tuple[np.ndarray, np.ndarray]:
    """The table of a knot law: (idx [H, 4] int32, w [H, 4] float32), four taps per horizon step.  The numpy
    restatement of csrc/noise_knots.h knot_table, operation by operation in float64 and rounded to float32 once:
    bitwise what mppi_get_noise_knots returns.

    order 0 holds knot (t * P) // H; orders 1 (linear) and 3 (uniform Catmull-Rom, clamped ends) interpolate at
    s = t (P - 1) / (H - 1) between knots j = min(floor(s), P - 2) and j + 1."""
    H, P, order = int(H), int(P), int(order)
    if not (1 <= P <= H and order in (0, 1, 3)):
        raise ValueError("knot_table: need 1 <= P <= H and order in {0, 1, 3}")
    idx = np.zeros((H, 4), np.int32)
    w = np.zeros((H, 4), np.float64)
    t = np.arange(H, dtype=np.int64)
    if order == 0 or H == 1 or P == 1:
        idx[:] = ((t * P) // H if order == 0 else 0 * t)[:, None]
        w[:, 0] = 1.0
        return idx, w.astype(np.float32)
    s = (t * (P - 1)).astype(np.float64) / np.float64(H - 1)
    j = np.minimum(np.floor(s).astype(np.int64), P - 2)
    a = s - j.astype(np.float64)
    if order == 1:
        idx[:] = np.stack([j, j + 1, j, j], axis=1)
        w[:, 0] = 1.0 - a
        w[:, 1] = a
        return idx, w.astype(np.float32)
    idx[:] = np.clip(np.stack([j - 1, j, j + 1, j + 2], axis=1), 0, P - 1)
    a2 = a * a
    a3 = a2 * a
    w[:, 0] = ((-a3 + 2.0 * a2) - a) * 0.5
    w[:, 1] = ((3.0 * a3 - 5.0 * a2) + 2.0) * 0.5
    w[:, 2] = ((-(3.0 * a3) + 4.0 * a2) + a) * 0.5
    w[:, 3] = (a3 - a2) * 0.5
    return idx, w.astype(np.float32)


def _fma32(a, b, c) -> np.ndarray:
    """fmaf(a, b, c) of float32 arrays, correctly rounded.  a * b is exact in float64 (48 bits); the sum with c is
    formed there with its rounding error (TwoSum), and the float64 sum is moved off an exact float32 tie towards the
    true value before the final rounding: the one case in which rounding twice differs from rounding once."""
    a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    f = s.astype(np.float32)
    d = s - f.astype(np.float64)  # exact
    g = np.nextafter(f, np.where(d > 0, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32))
    tie = (d != 0) & (d == g.astype(np.float64) - s) & (err != 0)
    s = np.where(tie, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def ar1_filter_f32(z, rho: float = 0.0) -> np.ndarray:
    """The unit-variance AR(1) row of csrc/noise_model.h in float32, operation by operation, along axis -2 of
    z [..., H, K]: e[0] = z[0], e[t] = fmaf(rho, e[t-1], c * z[t]), c = sqrtf(1 - rho * rho)."""
    z = np.asarray(z, np.float32)
    rho = np.float32(rho)
    c = np.sqrt(np.float32(1.0) - rho * rho, dtype=np.float32)
    e = z.copy()
    for t in range(1, z.shape[-2]):
        e[..., t, :] = _fma32(rho, e[..., t - 1, :], c * z[..., t, :])
    return e


def knot_filter(z, P: int, order: int, rho: float = 0.0, sigma_u=None) -> np.ndarray:
    """The knot law over given standard normals z [..., nu, H, K] (float32 result of the same shape): only
    z[..., :P, :] is read, as the normals of the P knots.  float32 with every fmaf of csrc/noise_knots.h emulated
    (correctly rounded): bitwise what the device draws (Engine.noise_eval) from the same normals.

        kn = AR(1)(rho) over z[..., :P, :];   e[t] = sum_i w[t][i] kn[idx[t][i]] (in tap order);   eps = sigma_u[u] e[t]

    sigma_u: scalar or [nu] (None = 1)."""
    z = np.asarray(z, np.float32)
    if z.ndim < 3:
        raise ValueError("knot_filter: z must be [..., nu, H, K]")
    rho = float(rho)
    if not 0.0 <= rho < 1.0:
        raise ValueError("knot_filter: rho must be in [0, 1)")
    nu, H = z.shape[-3], z.shape[-2]
    idx, w = knot_table(H, P, order)
    s = np.ones(nu, np.float32) if sigma_u is None else np.asarray(sigma_u, np.float32).ravel()
    if s.size == 1:
        s = np.full(nu, s[0], np.float32)
    if s.shape != (nu,):
        raise ValueError(f"knot_filter: sigma_u must have {nu} entries, got {s.size}")
    kn = ar1_filter_f32(z[..., :P, :], rho)
    e = w[:, 0][:, None] * kn[..., idx[:, 0], :]
    for i in (1, 2, 3):
        e = _fma32(w[:, i][:, None], kn[..., idx[:, i], :], e)
    return (s[:, None, None] * e).astype(np.float32)


# ---- the horizon basis (include/mppi.h mppi_set_noise_basis; csrc/noise_basis.h), restated bit for bit

def basis_filter(z, M, sigma_u=None) -> np.ndarray:
    """The basis law over given standard normals z [..., nu, H, K] (float32 result of the same shape): only
    z[..., :R, :] is read, as the R white normals of M [H, R].  float32 with every fmaf of csrc/noise_basis.h emulated
    (correctly rounded): bitwise what the device draws (Engine.noise_eval) from the same normals.

        e[t] = M[t][0] z[0];   e[t] = fmaf(M[t][r], z[r], e[t]), r = 1 .. R-1 ascending;   eps = sigma_u[u] e[t]

    sigma_u: scalar or [nu] (None = 1)."""
    z = np.asarray(z, np.float32)
    M = np.asarray(M, np.float32)
    if z.ndim < 3:
        raise ValueError("basis_filter: z must be [..., nu, H, K]")
    nu, H = z.shape[-3], z.shape[-2]
    if M.ndim != 2 or M.shape[0] != H or not 1 <= M.shape[1] <= H:
        raise ValueError(f"basis_filter: M must be [H = {H}, R] with 1 <= R <= H, got {list(M.shape)}")
    s = np.ones(nu, np.float32) if sigma_u is None else np.asarray(sigma_u, np.float32).ravel()
    if s.size == 1:
        s = np.full(nu, s[0], np.float32)
    if s.shape != (nu,):
        raise ValueError(f"basis_filter: sigma_u must have {nu} entries, got {s.size}")
    e = M[:, 0][:, None] * z[..., 0:1, :]
    for r in range(1, M.shape[1]):
        e = _fma32(M[:, r][:, None], z[..., r:r + 1, :], e)
    return (s[:, None, None] * e).astype(np.float32)


def colored_basis(H: int, beta: float, n_basis: int | None = None, dtype=np.float32) -> np.ndarray:
    """The table M [H, R] of coloured (power-law) noise along the horizon, S(f) ~ f^-beta (iCEM): a real Fourier basis
    whose column pair of frequency j carries the amplitude s_j = j^(-beta / 2).  Computed in float64 and rounded to
    float32 once (dtype=np.float64 returns it unrounded).

    Columns in the order DC, cos 1, sin 1, cos 2, sin 2, ..., and for even H a last Nyquist column:
        M[t][0] = g sqrt(2) s_1        M[t][2j-1] = 2 g s_j cos(2 pi j t / H)        M[t][2j] = 2 g s_j sin(2 pi j t / H)
        Nyquist: g sqrt(2) s_{H/2} (-1)^t
    with g such that every row of the kept columns has unit 2-norm: sigma_u is the scale at every step.  M M^T is
    circulant with eigenvalues lambda_j / lambda_1 = j^-beta (lambda_0 = lambda_1); beta = 0 gives M M^T = I.
    n_basis keeps the first columns (a low-pass law); it must be odd or H, so that the pairs stay whole and the variance
    stays constant in t."""
    H = int(H)
    beta = float(beta)
    if H < 1 or not np.isfinite(beta):
        raise ValueError("colored_basis: need H >= 1 and a finite beta")
    R = H if n_basis is None else int(n_basis)
    if not 1 <= R <= H or (R != H and R % 2 == 0):
        raise ValueError("colored_basis: n_basis must be in 1..H and odd or equal to H")
    dtype = np.dtype(dtype)
    if dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise ValueError("colored_basis: dtype must be float32 or float64")
    if H == 1:
        return np.ones((1, 1), dtype)
    t = np.arange(H, dtype=np.int64)
    M = np.zeros((H, H), np.float64)
    s = lambda j: float(j) ** (-0.5 * beta)
    M[:, 0] = np.sqrt(2.0) * s(1)
    for j in range(1, (H - 1) // 2 + 1):
        a = 2.0 * np.pi * ((j * t) % H).astype(np.float64) / H  # (the angle reduced in integers)
        M[:, 2 * j - 1] = 2.0 * s(j) * np.cos(a)
        M[:, 2 * j] = 2.0 * s(j) * np.sin(a)
    if H % 2 == 0:
        M[:, H - 1] = np.sqrt(2.0) * s(H // 2) * np.where(t % 2 == 0, 1.0, -1.0)
    M = M[:, :R]
    g = 1.0 / np.sqrt(np.sum(M[0] * M[0]))  # (constant in t: whole pairs)
    return (g * M).astype(dtype)


# ---- the per-step scale (include/mppi.h mppi_set_noise_steps), restated bit for bit

def steps_filter(z, table, rho: float = 0.0) -> np.ndarray:
    """The per-step law over standard normals z [..., nu, H, K]: eps[..., u, t, k] = table[..., u, t] * e[..., u, t, k]
    with e the unit-variance AR(1) row of z.  table: [nu, H] (every leading index of z takes it) or [..., nu, H]
    matching z's leading axes -- one table per solve.

    The arithmetic follows z's dtype.  float32 z: the device's own operations -- ar1_filter_f32's recursion, then one
    float32 product per element -- bitwise what the device draws (Engine.noise_eval) from the same normals; unit rows
    taken from the device (noise_eval under sigma_u = 1) go through with rho = 0, which leaves them as they are.
    Any other dtype: float64 in ar1_filter's own operations, so a table that is sigma_u broadcast along the horizon
    gives ar1_filter(z, rho, sigma_u) bit for bit."""
    z = np.asarray(z)
    if z.ndim < 3:
        raise ValueError("steps_filter: z must be [..., nu, H, K]")
    rho = float(rho)
    if not 0.0 <= rho < 1.0:
        raise ValueError("steps_filter: rho must be in [0, 1)")
    f32 = z.dtype == np.float32
    S = np.asarray(table, np.float32 if f32 else np.float64)
    nu, H = z.shape[-3], z.shape[-2]
    if S.ndim < 2 or S.shape[-2:] != (nu, H) or (S.ndim > 2 and S.shape[:-2] != z.shape[:-3]):
        raise ValueError(f"steps_filter: table must be [{nu}, {H}] or {list(z.shape[:-3])} + [{nu}, {H}], "
                         f"got {list(S.shape)}")
    if not (np.all(np.isfinite(S)) and np.all(S >= 0.0)):
        raise ValueError("steps_filter: table entries must be finite and >= 0")
    if f32:
        e = ar1_filter_f32(z, rho) if rho != 0.0 else z
        return (S[..., None] * e).astype(np.float32)
    z = np.asarray(z, np.float64)
    e = z.copy()
    if rho != 0.0:
        c = np.sqrt(1.0 - rho * rho)
        for t in range(1, H):
            e[..., t, :] = rho * e[..., t - 1, :] + c * z[..., t, :]
    return S[..., None] * e


# ---- the cross-actuator covariance (include/mppi.h mppi_set_noise_cov; csrc/noise_cov.h), restated bit for bit

def cov_factor(Sigma) -> np.ndarray:
    """The Cholesky factor L [nu, nu] (float32, lower, the strict upper triangle 0) of Sigma [nu, nu] (float32): the
    restatement of csrc/noise_cov.h cov_factor in Python doubles, operation by operation (Cholesky-Banachiewicz, row by
    row, one product and one difference at a time), rounded to float32 once: bitwise what mppi_get_noise_cov returns.
    ValueError when Sigma is not finite, not symmetric bit for bit or a pivot is not > 0 and finite."""
    S = np.asarray(Sigma, np.float32)
    if S.ndim != 2 or S.shape[0] != S.shape[1] or S.shape[0] < 1:
        raise ValueError("cov_factor: Sigma must be [nu, nu]")
    nu = S.shape[0]
    if not np.all(np.isfinite(S)) or not np.array_equal(S, S.T):
        raise ValueError("cov_factor: Sigma must be finite and symmetric bit for bit")
    Sd = [[float(S[u, v]) for v in range(nu)] for u in range(nu)]
    Ld = [[0.0] * nu for _ in range(nu)]
    for u in range(nu):
        for v in range(u + 1):
            a = Sd[u][v]
            for j in range(v):
                p = Ld[u][j] * Ld[v][j]
                a = a - p
            if u == v:
                if not (a > 0.0 and np.isfinite(a)):
                    raise ValueError(f"cov_factor: Sigma is not positive definite (pivot {u} is {a})")
                Ld[u][u] = float(np.sqrt(a))
            else:
                Ld[u][v] = a / Ld[v][v]
    return np.array(Ld, np.float64).astype(np.float32)


def cov_mix(e, L) -> np.ndarray:
    """eps[..., u, t, k] = sum_{v <= u} L[u][v] e[..., v, t, k] in float32 in the order of csrc/noise_cov.h (the first
    product, then one fmaf per v, correctly rounded): bitwise what the device writes.  e [..., nu, H, K], L [nu, nu]
    (only the lower triangle is read)."""
    e = np.asarray(e, np.float32)
    L = np.asarray(L, np.float32)
    if e.ndim < 3 or L.shape != (e.shape[-3], e.shape[-3]):
        raise ValueError("cov_mix: e must be [..., nu, H, K] and L [nu, nu]")
    out = np.empty_like(e)
    for u in range(L.shape[0]):
        acc = L[u, 0] * e[..., 0, :, :]
        for v in range(1, u + 1):
            acc = _fma32(L[u, v], e[..., v, :, :], acc)
        out[..., u, :, :] = acc
    return out


def cov_filter(z, Sigma_or_L, rho: float = 0.0, is_factor: bool | None = None) -> np.ndarray:
    """The covariance law over given standard normals z [..., nu, H, K] (float32 result of the same shape):
    cov_mix(ar1_filter_f32(z, rho), L).  Sigma_or_L: a lower-triangular matrix (its strict upper triangle exactly 0) is
    taken as the factor L itself -- what Engine.noise_cov reports --, anything else as Sigma and factored by
    cov_factor.  A diagonal matrix (nu = 1 included) is therefore read as L: say is_factor=False for a diagonal Sigma
    (is_factor=True / False settles the reading whatever the matrix looks like)."""
    M = np.asarray(Sigma_or_L, np.float32)
    rho = float(rho)
    if not 0.0 <= rho < 1.0:
        raise ValueError("cov_filter: rho must be in [0, 1)")
    if M.ndim != 2 or M.shape[0] != M.shape[1]:
        raise ValueError("cov_filter: Sigma_or_L must be [nu, nu]")
    if is_factor is None:
        is_factor = not np.any(np.triu(M, 1))
    L = M if is_factor else cov_factor(M)
    return cov_mix(ar1_filter_f32(z, rho), L)
