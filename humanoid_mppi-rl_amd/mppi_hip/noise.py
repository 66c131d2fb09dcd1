"""The engine's sampling law on the host (include/mppi.h mppi_set_noise_model; csrc/noise_model.h).

    e[0] = z[0];   e[t] = rho * e[t-1] + sqrt(1 - rho^2) * z[t];   eps = sigma_u[u] * e[t]

Every step has unit variance before scaling and corr(e[t], e[s]) = rho^|t-s|.  The device runs the recursion in fp32;
this restatement is float64 (the reference for tests, and the filter of MPPIModel's noise="numpy" mode).
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
