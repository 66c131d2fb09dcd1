"""Solve diagnostics on the host (include/mppi.h mppi_solve_stats, MPPI_FLAG_STATS; csrc/kernels_stats.hip).

Per solve, with F = {k : isfinite(c_k)}, beta = min_F c, wt_k = exp(-(c_k - beta) / lambda) on F and 0 elsewhere,
S = sum wt and w_k = wt_k / (S + norm_eps) -- the weights of the update itself:

    cost_min / cost_max / cost_mean / cost_std   over F (population std)
    cost_weighted = sum_k w_k c_k
    ess           = S^2 / sum wt_k^2                        in [1, |F|]
    entropy       = -sum p ln p, p = wt / S (0 ln 0 = 0)    in [0, ln |F|]
    free_energy   = beta - lambda ln(S / |F|)
    n_finite = |F|,  k_best = the lowest k attaining beta
    eps_m2 [u]  = 1/H     sum_t      sum_k w_k eps[u,t,k]^2
    eps_m11[u]  = 1/(H-1) sum_{t>=1} sum_k w_k eps[u,t,k] eps[u,t-1,k]     (0 when H == 1)

The device computes these in fp32 (fp64 for the cost sums); solve_stats_ref is the float64 restatement: the reference
of the tests, and for users.  adapt_noise_model turns the moments into the next sampling law; adapt_noise_model_f32 is
the same step as the device takes it (mppi_set_noise_adapt), float32 operation by operation.

ESS targeting (mppi_set_ess_target; csrc/ess_target.h is the fp32 rule): per solve the device chooses lambda_b in
[lambda_min, lambda_max] so that the solve's own costs give a requested effective sample size.  With F, beta and wt as
above, n = |F|, ESS(lambda) = (sum wt)^2 / sum wt^2 and the target T = max(1, ess_frac * n):

    n == 0:                 lambda_b = the configured lambda (the solve reports MPPI_E_NONFINITE)
    ESS(lambda_min) >= T:   lambda_b = lambda_min    (ties at the minimum, n == 1, all costs equal)
    ESS(lambda_max) <  T:   lambda_b = lambda_max
    otherwise               the root of ESS(lambda) = T; the device returns the upper end hi of an fp32 bracket
                            ESS(lo) < T <= ESS(hi) with hi / lo <= 1 + 2e-6

ess_ref and ess_lambda_ref are the float64 restatement (the true root by bisection to convergence).

The control-cost term (mppi_set_control_cost; csrc/control_cost.h is the fp32 rule for lin): the softmin weighs
costs + term with

    lin[b, u, t] = gamma / sigma_u[u]^2 * (P U[b, u, :])[t]       (sigma_u[u] == 0: 0)
    term[b, k]   = sum_{u,t} lin[b, u, t] * eps[b, u, t, k]

P the precision matrix of the unit-variance AR(1) row (ar1_precision).  control_term_ref is the float64 restatement.

Per-actuator control bounds (mppi_set_control_bounds; csrc/ctrl_bounds.h is the rule): ahead of the rollout the
solve's noise becomes eps' = clip(U + eps, lo, hi) - U, element by element in float32 and only where the box binds.
project_noise_ref is the numpy restatement: a select and one subtract, so it equals the device bit for bit.

The control-rate cost term (mppi_set_rate_cost; csrc/rate_cost.h is the fp32 rule): the softmin weighs costs
(+ control term) + rate term with

    v[b, u, t, k] = clamp(U[b, u, t] + eps'[b, u, t, k])          the control the rollout applied, float32
    rate[b, k]    = sum_u r[u] sum_t (v[u, t] - v[u, t-1])^2      v[u, -1] = u_prev[b, u] with the anchor, else t >= 1

rate_term_ref is the float64 restatement.

Elite truncation (mppi_set_elites; csrc/elite_select.h is the rule): of the finite costs the softmin would weigh, only
the n_elite lowest keep their cost, ordered by (cost, k) -- ties at the threshold go to the lower k, -0.0 equals +0.0 --
and every other sample's becomes +inf.  elite_select_ref is the numpy restatement, a stable argsort: it equals the
device exactly.

Keep / shift elites (mppi_set_elite_keep; csrc/elite_keep.h is the rule): the n_keep best sampled control sequences of
a solve, v = clamp(U + eps') taken at step t + shift, are stored and become the first columns of the next solve's noise
as eps = v - U.  keep_store_ref and keep_inject_ref are the float32 restatements -- one add, the clamp form of
rate_cost_v, one subtract -- and equal the device bit for bit.

Weighted cross moments (MPPI_FLAG_CROSS; csrc/cross_moments.h is the fp32 definition):

    eps_mx[u, v] = 1/H sum_t sum_k w_k eps[u,t,k] eps[v,t,k]

cross_moments_ref is the float64 restatement (from the costs, with the weights above); cross_moments_f32 is the device's
own summation -- the cell scheme of csrc/cross_moments.h, float32 operation by operation -- from float32 weights, and
equals the device bit for bit.

The adapted covariance (mppi_set_noise_cov_adapt; csrc/noise_cov_adapt.h is the fp32 rule): Sigma moves towards the
batch mean of eps_mx, its standard deviations are clipped with the correlations kept, and L and Sigma^-1 are factored
again.  adapt_noise_cov is the float64 restatement, adapt_noise_cov_f32 the step as the device takes it, bit for bit.

Weighted per-step moments (MPPI_FLAG_STEP_MOMENTS; csrc/step_moments.h is the fp32 definition):

    m1[u, t] = sum_k w_k eps[u,t,k]          m2[u, t] = sum_k w_k eps[u,t,k]^2

step_moments_ref is the float64 restatement, step_moments_f32 the device's own summation, bit for bit.  The refit of
the per-step sampling scales (mppi_set_noise_steps_adapt; csrc/step_law.h is the fp32 rule) moves every solve's table
towards its own moments, about the weighted mean or about zero, and shifts it with the nominal: adapt_noise_steps is
the float64 restatement, adapt_noise_steps_f32 the step as the device takes it, bit for bit.

Dynamics-model ensembles (mppi_set_ensemble; csrc/ensemble.h is the fp32 rule): every sample is rolled under each of n
members and the members' costs become one cost per sample -- their mean, mean + kappa * population std, or maximum --
beside their spread.  ensemble_combine_f32 is the rule as the device takes it, bit for bit.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

FIELDS = ("cost_min", "cost_max", "cost_mean", "cost_std", "cost_weighted", "ess", "entropy", "free_energy",
          "n_finite", "k_best")


def solve_stats_ref(costs, noise=None, lam: float = 1.0, norm_eps: float = 0.0) -> dict:
    """costs [B, K] (or [K]), noise None or [B, nu, H, K] (or [nu, H, K]) -> the dictionary Engine.stats returns:
    every field of mppi_solve_stats as an array [B] (float64; n_finite and k_best int64) and, with noise, eps_m2 and
    eps_m11 [B, nu].  No finite cost: n_finite 0, k_best -1, ess = entropy = cost_std = cost_weighted = 0,
    cost_min = cost_max = cost_mean = free_energy = +inf, both moments 0."""
    c = np.asarray(costs, np.float64)
    single = c.ndim == 1
    c = c.reshape(-1, c.shape[-1])
    B, K = c.shape
    out = {n: np.zeros(B, np.int64 if n in ("n_finite", "k_best") else np.float64) for n in FIELDS}
    w = np.zeros((B, K))
    for b in range(B):
        fin = np.isfinite(c[b])
        n = int(fin.sum())
        out["n_finite"][b] = n
        if n == 0:
            for name in ("cost_min", "cost_max", "cost_mean", "free_energy"):
                out[name][b] = np.inf
            out["k_best"][b] = -1
            continue
        cf = c[b][fin]
        beta = cf.min()
        wt = np.zeros(K)
        wt[fin] = np.exp(-(cf - beta) / lam)
        S = wt.sum()
        w[b] = wt / (S + norm_eps)
        p = wt[wt > 0.0] / S
        out["cost_min"][b], out["cost_max"][b], out["cost_mean"][b] = beta, cf.max(), cf.mean()
        out["cost_std"][b] = np.sqrt(np.mean((cf - cf.mean()) ** 2))
        out["cost_weighted"][b] = np.sum(w[b][fin] * cf)
        out["ess"][b] = S * S / np.sum(wt * wt)
        out["entropy"][b] = -np.sum(p * np.log(p))
        out["free_energy"][b] = beta - lam * np.log(S / n)
        out["k_best"][b] = int(np.flatnonzero(fin & (c[b] == beta))[0])
    if noise is not None:
        e = np.asarray(noise, np.float64)
        e = e.reshape(B, -1, e.shape[-2], K)
        H = e.shape[2]
        out["eps_m2"] = np.einsum("bk,buhk->bu", w, e * e) / H
        out["eps_m11"] = (np.einsum("bk,buhk->bu", w, e[:, :, 1:] * e[:, :, :-1]) / (H - 1) if H > 1
                          else np.zeros((B, e.shape[1])))
    return {k: v[0] for k, v in out.items()} if single else out


def adapt_noise_model(sigma_u, rho: float, eps_m2, eps_m11, rate: float, sigma_min: float = 1e-3,
                      sigma_max: float = 10.0, rho_max: float = 0.95):
    """One step of the sampling law towards the noise that won the last solve(s): (sigma_u [nu], rho) for
    Engine.set_noise_model.  Pure.

    eps_m2, eps_m11: the weighted noise moments [B, nu] (or [nu]) of Engine.stats.  They are moments about the NOMINAL
    U (about zero noise), as the update itself is -- not about the weighted mean of the noise -- so a solve whose
    winners share an offset widens sigma_u rather than only moving U.

        var     <- (1 - rate) sigma_u^2 + rate * mean_b eps_m2;   sigma_u = sqrt(var) clipped to [sigma_min, sigma_max]
        rho_hat  = sum_u mean_b eps_m11 / sum_u mean_b eps_m2,    clipped to [0, rho_max]   (0 if the denominator is 0)
        rho     <- (1 - rate) rho + rate * rho_hat

    rate = 0 returns the law unchanged (sigma_u still clipped).  ValueError on rate outside [0, 1], rho outside [0, 1),
    rho_max outside [0, 1), sigma_min > sigma_max or negative, non-finite or negative sigma_u / eps_m2, non-finite
    eps_m11, or moments whose last axis is not nu."""
    s = np.atleast_1d(np.asarray(sigma_u, np.float64)).ravel()
    m2 = np.asarray(eps_m2, np.float64)
    m11 = np.asarray(eps_m11, np.float64)
    rate, rho = float(rate), float(rho)
    if not 0.0 <= rate <= 1.0:
        raise ValueError("adapt_noise_model: rate must be in [0, 1]")
    if not 0.0 <= rho < 1.0:
        raise ValueError("adapt_noise_model: rho must be in [0, 1)")
    if not 0.0 <= rho_max < 1.0:
        raise ValueError("adapt_noise_model: rho_max must be in [0, 1)")
    if not 0.0 <= sigma_min <= sigma_max or not np.isfinite(sigma_max):
        raise ValueError("adapt_noise_model: need 0 <= sigma_min <= sigma_max < inf")
    if not (np.all(np.isfinite(s)) and np.all(s >= 0.0)):
        raise ValueError("adapt_noise_model: sigma_u entries must be finite and >= 0")
    if m2.shape != m11.shape or m2.ndim not in (1, 2) or m2.shape[-1] != s.size:
        raise ValueError(f"adapt_noise_model: eps_m2 and eps_m11 must both be [B, {s.size}] or [{s.size}]")
    if not (np.all(np.isfinite(m2)) and np.all(m2 >= 0.0) and np.all(np.isfinite(m11))):
        raise ValueError("adapt_noise_model: moments must be finite (eps_m2 >= 0)")
    m2 = m2.reshape(-1, s.size).mean(axis=0)
    m11 = m11.reshape(-1, s.size).mean(axis=0)
    var = (1.0 - rate) * s * s + rate * m2
    sigma_new = np.clip(np.sqrt(var), sigma_min, sigma_max)
    den = m2.sum()
    rho_hat = float(np.clip(m11.sum() / den, 0.0, rho_max)) if den > 0.0 else 0.0
    return sigma_new, (1.0 - rate) * rho + rate * rho_hat


def _round_f32(v) -> np.float32:
    """The exact rational v rounded once to fp32 (nearest, ties to even)."""
    f = np.float32(float(v))  # (rounded twice: the neighbours decide)
    best = None
    for c in (f, np.nextafter(f, np.float32(np.inf)), np.nextafter(f, np.float32(-np.inf))):
        if not np.isfinite(c):
            continue
        d = abs(Fraction(float(c)) - v)
        even = (int(np.float32(c).view(np.uint32)) & 1) == 0
        if best is None or d < best[0] or (d == best[0] and even and not best[2]):
            best = (d, np.float32(c), even)
    return f if best is None else best[1]


def _fma32(a, b, c) -> np.float32:
    """fmaf(a, b, c): the exact a * b + c rounded once to fp32 (non-finite operands as numpy propagates them)."""
    a, b, c = np.float32(a), np.float32(b), np.float32(c)
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        with np.errstate(all="ignore"):
            return np.float32(np.float64(a) * np.float64(b) + np.float64(c))
    v = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    if abs(v) >= Fraction(2) ** 128:
        return np.float32(np.inf if v > 0 else -np.inf)
    return _round_f32(v)


def adapt_noise_model_f32(sigma_u, rho, eps_m2, eps_m11, rate, sigma_min=1e-3, sigma_max=10.0, rho_max=0.95,
                          n_finite=None):
    """The device's adaptation step (csrc/noise_adapt.h, mppi_set_noise_adapt) restated in numpy float32, operation by
    operation: (sigma_u [nu] float32, rho float32) after one step from the law (sigma_u, rho) and the moments
    eps_m2, eps_m11 [B, nu] (or [nu]) of one batch.  Bitwise what noise_adapt_kernel writes.

        if any n_finite[b] == 0: the law is returned unchanged
        m2bar[u]  = (m2[0][u] + m2[1][u] + ...) / float32(B)        sequential float32 sums, b ascending; m11bar alike
        var       = fmaf(rate, m2bar[u], (1 - rate) * (s * s));     sigma_u[u] = min(max(sqrt(var), sigma_min), sigma_max)
        den, num  = sum_u m2bar[u], sum_u m11bar[u]                 u ascending
        rho_hat   = clamp(num / den, 0, rho_max) if den > 0 else 0
        rho       = fmaf(rate, rho_hat, (1 - rate) * rho)
        a non-finite var or rho leaves that entry as it was

    adapt_noise_model is the same rule in float64 (it raises on invalid input, this one follows the kernel)."""
    f = np.float32
    s = np.atleast_1d(np.asarray(sigma_u, f)).ravel().copy()
    nu = s.size
    m2 = np.asarray(eps_m2, f).reshape(-1, nu)
    m11 = np.asarray(eps_m11, f).reshape(-1, nu)
    B = m2.shape[0]
    rho, rate, lo, hi, rho_max = f(rho), f(rate), f(sigma_min), f(sigma_max), f(rho_max)
    if n_finite is not None and np.any(np.asarray(n_finite).ravel()[:B] == 0):
        return s, rho

    def mean(col):
        acc = f(0.0)
        for b in range(B):
            acc = f(acc + col[b])
        return f(acc / f(B))

    with np.errstate(all="ignore"):
        keep = f(f(1.0) - rate)
        m2bar = [mean(m2[:, u]) for u in range(nu)]
        m11bar = [mean(m11[:, u]) for u in range(nu)]
        for u in range(nu):
            var = _fma32(rate, m2bar[u], f(keep * f(s[u] * s[u])))
            r = np.sqrt(var, dtype=f)
            if not (np.isfinite(var) and np.isfinite(r)):
                continue
            r = lo if r < lo else r
            r = hi if r > hi else r
            s[u] = r
        den, num = f(0.0), f(0.0)
        for u in range(nu):
            den = f(den + m2bar[u])
            num = f(num + m11bar[u])
        rho_hat = f(0.0)
        if den > 0.0:
            rho_hat = f(num / den)
            rho_hat = f(0.0) if rho_hat < 0.0 else rho_hat
            rho_hat = rho_max if rho_hat > rho_max else rho_hat
        r = _fma32(rate, rho_hat, f(keep * rho))
    return s, (r if np.isfinite(r) else rho)


def ess_ref(costs, lam) -> float:
    """ESS(lam) of one solve's costs [K] in float64: non-finite costs carry weight 0; 0.0 when no cost is finite."""
    c = np.asarray(costs, np.float64).ravel()
    cf = c[np.isfinite(c)]
    if cf.size == 0:
        return 0.0
    with np.errstate(under="ignore"):
        wt = np.exp(-(cf - cf.min()) / float(lam))
    S = wt.sum()
    return float(S * S / np.sum(wt * wt))


def ess_target_ref(costs, ess_frac: float) -> float:
    """The target T = max(1, ess_frac * n_finite) of one solve's costs [K]."""
    n = int(np.isfinite(np.asarray(costs, np.float64)).sum())
    return max(1.0, float(ess_frac) * n)


def ess_lambda_ref(costs, ess_frac: float, lambda_min: float, lambda_max: float, lam_default: float = 1.0):
    """The lambda of ESS targeting in float64 (the rule of csrc/ess_target.h with the true root): costs [B, K] -> [B]
    (or [K] -> a float).  ESS(lambda_min) >= T gives lambda_min, ESS(lambda_max) < T gives lambda_max, otherwise the
    root of ESS(lambda) = T by bisection in log lambda until the bracket stops shrinking; a row without a finite cost
    gives lam_default (the handle's configured lambda).  ValueError on ess_frac outside (0, 1] or bounds that are not
    0 < lambda_min <= lambda_max < inf."""
    ess_frac, lo0, hi0 = float(ess_frac), float(lambda_min), float(lambda_max)
    if not 0.0 < ess_frac <= 1.0:
        raise ValueError("ess_lambda_ref: ess_frac must be in (0, 1]")
    if not 0.0 < lo0 <= hi0 < np.inf:
        raise ValueError("ess_lambda_ref: need 0 < lambda_min <= lambda_max < inf")
    c = np.asarray(costs, np.float64)
    single = c.ndim == 1
    c = c.reshape(-1, c.shape[-1])
    out = np.empty(c.shape[0])
    for b, row in enumerate(c):
        if not np.isfinite(row).any():
            out[b] = lam_default
            continue
        T = ess_target_ref(row, ess_frac)
        if ess_ref(row, lo0) >= T:
            out[b] = lo0
        elif ess_ref(row, hi0) < T:
            out[b] = hi0
        else:
            lo, hi = np.log(lo0), np.log(hi0)
            while True:
                mid = 0.5 * (lo + hi)
                if not lo < mid < hi:
                    break
                if ess_ref(row, np.exp(mid)) >= T:
                    hi = mid
                else:
                    lo = mid
            out[b] = np.exp(hi)
    return float(out[0]) if single else out


def ar1_precision(H: int, rho: float) -> np.ndarray:
    """P [H, H], the inverse of the unit-variance AR(1) covariance C[t, s] = rho^|t-s|: tridiagonal,
    1/(1 - rho^2) * tridiag(-rho; [1, 1 + rho^2, ..., 1 + rho^2, 1]; -rho) for H >= 2 and [1] for H == 1."""
    H, rho = int(H), float(rho)
    if H < 1 or not 0.0 <= rho < 1.0:
        raise ValueError("ar1_precision: need H >= 1 and rho in [0, 1)")
    if H == 1:
        return np.ones((1, 1))
    d = np.full(H, 1.0 + rho * rho)
    d[0] = d[-1] = 1.0
    P = np.diag(d) - rho * (np.eye(H, k=1) + np.eye(H, k=-1))
    return P / (1.0 - rho * rho)


def control_term_ref(U, noise, sigma_u, rho: float, gamma: float, Sinv=None):
    """The control-cost term in float64 (include/mppi.h mppi_set_control_cost): U [B, nu, H] (or [nu, H]), noise
    [B, nu, H, K] (or [nu, H, K]), sigma_u [nu] (or a scalar: every actuator's), rho in [0, 1), gamma >= 0 ->
    (term [B, K], lin [B, nu, H], majorant [B, nu, H]).

        lin  = gamma / sigma_u^2 * P U      along t, P = ar1_precision(H, rho); a frozen actuator (sigma_u == 0): 0
        term = sum_{u,t} lin * noise        every row, lin == 0 included: a non-finite noise entry makes its sample's
                                            term non-finite (0 * inf = NaN), as on the device
        majorant = gamma / sigma_u^2 * |P| |U|: the absolute-value bound of lin that the fp32 rule's rounding error is
                   stated against (csrc/control_cost.h: |lin_f32 - lin| <= 8 * 2^-24 * majorant)

    Sinv [nu, nu] (default None): the inverse of a cross-actuator covariance (mppi_set_noise_cov); sigma_u is then not
    read and
        lin[u]      = gamma * sum_v Sinv[u][v] (P U[v])
        majorant[u] = gamma * sum_v |Sinv[u][v]| (|P| |U[v]|)      (csrc/control_cost.h: (nu + 8) * 2^-24 * majorant)
    With Sinv = diag(1 / sigma_u^2) this is the per-actuator form above.

    ValueError on gamma negative or non-finite, rho outside [0, 1), negative or non-finite sigma_u, or shapes that do
    not agree."""
    U = np.asarray(U, np.float64)
    e = np.asarray(noise, np.float64)
    single = U.ndim == 2
    if U.ndim not in (2, 3) or e.ndim != U.ndim + 1:
        raise ValueError("control_term_ref: U must be [B, nu, H] (or [nu, H]) and noise [B, nu, H, K] (or [nu, H, K])")
    if single:
        U, e = U[None], e[None]
    B, nu, H = U.shape
    if e.shape[:3] != (B, nu, H):
        raise ValueError(f"control_term_ref: noise must be [{B}, {nu}, {H}, K], got {list(e.shape)}")
    gamma, rho = float(gamma), float(rho)
    if not 0.0 <= gamma < np.inf:
        raise ValueError("control_term_ref: gamma must be finite and >= 0")
    if not 0.0 <= rho < 1.0:
        raise ValueError("control_term_ref: rho must be in [0, 1)")
    P = ar1_precision(H, rho)
    if Sinv is not None:
        Si = np.asarray(Sinv, np.float64)
        if Si.shape != (nu, nu) or not np.all(np.isfinite(Si)):
            raise ValueError(f"control_term_ref: Sinv must be [{nu}, {nu}] and finite")
        lin = gamma * np.einsum("uv,ts,bvs->but", Si, P, U)
        majorant = gamma * np.einsum("uv,ts,bvs->but", np.abs(Si), np.abs(P), np.abs(U))
    else:
        s = np.asarray(sigma_u, np.float64)
        s = np.full(nu, float(s)) if s.ndim == 0 else s.ravel()
        if s.size != nu or not (np.all(np.isfinite(s)) and np.all(s >= 0.0)):
            raise ValueError(f"control_term_ref: sigma_u must be {nu} finite entries >= 0")
        scale = np.zeros(nu)
        scale[s > 0.0] = gamma / s[s > 0.0] ** 2
        lin = scale[None, :, None] * np.einsum("ts,bus->but", P, U)
        majorant = scale[None, :, None] * np.einsum("ts,bus->but", np.abs(P), np.abs(U))
    with np.errstate(invalid="ignore"):  # (a non-finite noise entry makes its sample's term non-finite, as on the device)
        term = np.einsum("but,butk->bk", lin, e)
    if single:
        return term[0], lin[0], majorant[0]
    return term, lin, majorant


def project_noise_ref(U, noise, lo=None, hi=None):
    """The projection of mppi_set_control_bounds in float32 (csrc/ctrl_bounds.h), bitwise what the device computes:
    U [B, nu, H] (or [nu, H]), noise [B, nu, H, K] (or [nu, H, K]), lo / hi scalars or [nu] (None: that side unbounded).
    With s = U + eps (one float32 add):  s < lo: eps' = lo - U;  s > hi: eps' = hi - U;  else eps' = eps, untouched
    (a NaN s lands here).  Returns (eps' float32, same shape as noise; counts uint32 [B, nu] (or [nu]): the projected
    elements per actuator).  lo > hi or a NaN bound raises ValueError."""
    U = np.asarray(U, np.float32)
    eps = np.asarray(noise, np.float32)
    single = U.ndim == 2
    if single:
        U, eps = U[None], eps[None]
    if U.ndim != 3 or eps.ndim != 4 or eps.shape[:3] != U.shape:
        raise ValueError("project_noise_ref: need U [B, nu, H] and noise [B, nu, H, K]")
    nu = U.shape[1]

    def side(v, default, name):
        if v is None:
            return np.full(nu, default, np.float32)
        a = np.asarray(v, np.float32)
        a = np.full(nu, a, np.float32) if a.ndim == 0 else a.ravel()
        if a.size != nu:
            raise ValueError(f"project_noise_ref: {name} must be a scalar or have nu = {nu} entries")
        return a

    lo, hi = side(lo, -np.inf, "lo"), side(hi, np.inf, "hi")
    if not (lo <= hi).all():  # (a NaN fails the comparison)
        raise ValueError("project_noise_ref: need lo <= hi, neither a NaN, for every actuator")
    Ue, lo_e, hi_e = U[..., None], lo[None, :, None, None], hi[None, :, None, None]
    with np.errstate(invalid="ignore", over="ignore"):
        s = (Ue + eps).astype(np.float32)
        below, above = s < lo_e, s > hi_e
        out = np.where(below, (lo_e - Ue).astype(np.float32), np.where(above, (hi_e - Ue).astype(np.float32), eps))
    counts = (below | above).sum(axis=(2, 3)).astype(np.uint32)
    out = out.astype(np.float32, copy=False)
    return (out[0], counts[0]) if single else (out, counts)


def rate_term_ref(U, noise, r, u_prev=None, ctrl_clamp: float = 0.0):
    """The control-rate cost term in float64 (include/mppi.h mppi_set_rate_cost; csrc/rate_cost.h): U [B, nu, H] (or
    [nu, H]), noise [B, nu, H, K] (or [nu, H, K]) as the rollout sees it, r a scalar or [nu] (>= 0), u_prev None (no
    anchor) or [B, nu] (or [nu]), ctrl_clamp as in the config (<= 0: none) -> term [B, K] (or [K]).

        v    = float32(U + noise), then clipped to +-ctrl_clamp     formed in float32 exactly as the device forms it
        d    = v[t] - v[t-1], v[-1] = u_prev                        t = 0 only with u_prev; float64 from here on
        term = sum_u r[u] sum_t d^2

    Every row enters: a non-finite U + noise on any row (a row with r == 0, an unanchored t = 0 and a sum the clamp
    would have made finite included) makes its sample's term NaN, as on the device.  ValueError on shapes that do not
    agree, or r negative, non-finite or of the wrong size."""
    U = np.asarray(U, np.float32)
    eps = np.asarray(noise, np.float32)
    single = U.ndim == 2
    if U.ndim not in (2, 3) or eps.ndim != U.ndim + 1:
        raise ValueError("rate_term_ref: U must be [B, nu, H] (or [nu, H]) and noise [B, nu, H, K] (or [nu, H, K])")
    if single:
        U, eps = U[None], eps[None]
    B, nu, H = U.shape
    if eps.shape[:3] != (B, nu, H):
        raise ValueError(f"rate_term_ref: noise must be [{B}, {nu}, {H}, K], got {list(eps.shape)}")
    w = np.asarray(r, np.float64)
    w = np.full(nu, float(w)) if w.ndim == 0 else w.ravel()
    if w.size != nu or not (np.all(np.isfinite(w)) and np.all(w >= 0.0)):
        raise ValueError(f"rate_term_ref: r must be {nu} finite entries >= 0")
    clamp = float(ctrl_clamp)
    with np.errstate(invalid="ignore", over="ignore"):
        s = (U[..., None] + eps).astype(np.float32)
        v = np.clip(s, np.float32(-clamp), np.float32(clamp)) if clamp > 0.0 else s
        v = np.where(np.isfinite(s), v, np.nan).astype(np.float64)
        if u_prev is None:
            first = v[:, :, :1] - v[:, :, :1]  # 0, or NaN for a non-finite row
        else:
            up = np.asarray(u_prev, np.float32).astype(np.float64).reshape(B, nu)
            first = v[:, :, :1] - up[:, :, None, None]
        d = np.concatenate([first, v[:, :, 1:] - v[:, :, :-1]], axis=2)
        term = np.einsum("u,butk->bk", w, d * d)
    return term[0] if single else term


def elite_select_ref(costs, n_elite: int):
    """Elite truncation (include/mppi.h mppi_set_elites; csrc/elite_select.h): costs [B, K] (or [K]) float32, the costs
    the softmin would otherwise weigh -> (idx [B, n_elite] int32, count [B] int32, tau [B] float32, ecost [B, K] float32)
    (or the row's own for a [K] input).

        F     = the finite costs, m = min(n_elite, |F|)
        E     = the first m of F in a STABLE ascending sort: cost first, the lower k on equal cost (-0.0 == +0.0)
        idx   = E in ascending k, -1 behind it;  count = m
        tau   = the m-th smallest cost (+ 0.0, so a zero reads +0.0), +inf when m == 0
        ecost = the cost bit for bit on E, +inf elsewhere

    ValueError unless 1 <= n_elite <= K."""
    c = np.asarray(costs, np.float32)
    single = c.ndim == 1
    if c.ndim not in (1, 2):
        raise ValueError("elite_select_ref: costs must be [B, K] or [K]")
    c = c[None] if single else c
    B, K = c.shape
    n_elite = int(n_elite)
    if not 1 <= n_elite <= K:
        raise ValueError(f"elite_select_ref: n_elite must be in 1..K = {K}")
    idx = np.full((B, n_elite), -1, np.int32)
    count = np.zeros(B, np.int32)
    tau = np.full(B, np.inf, np.float32)
    ecost = np.full((B, K), np.inf, np.float32)
    for b in range(B):
        fin = np.flatnonzero(np.isfinite(c[b]))
        order = fin[np.argsort(c[b, fin], kind="stable")]  # (-0.0 < +0.0 is false: equal, the lower k first)
        m = min(n_elite, fin.size)
        members = np.sort(order[:m])
        idx[b, :m] = members
        count[b] = m
        if m:
            tau[b] = c[b, order[m - 1]] + np.float32(0.0)
        ecost[b, members] = c[b, members]
    return (idx[0], count[0], tau[0], ecost[0]) if single else (idx, count, tau, ecost)


def keep_store_ref(U, noise, costs, n_keep: int, shift: bool = False, ctrl_clamp: float = 0.0):
    """The store of mppi_set_elite_keep in float32 (csrc/elite_keep.h), bitwise what the device computes: U [B, nu, H]
    (or [nu, H]) the nominal the rollout perturbed, noise [B, nu, H, K] (or [nu, H, K]) as the rollout saw it, costs
    [B, K] (or [K]) what the softmin would weigh ahead of any elite masking ->
    (v [B, nu, H, n_keep] float32, kcost [B, n_keep] float32, idx [B, n_keep] int32, count [B] int32, steps [B] int32).

        idx, count   = elite_select_ref(costs, n_keep): the n_keep best finite costs by (cost, k), in ascending k
        steps        = H - shift
        v[u, t, j]   = float32(U[u, t+shift] + noise[u, t+shift, idx[j]]) for t < steps, j < count, clamped to
                       +-ctrl_clamp when ctrl_clamp > 0 as csrc/rate_cost.h clamps (c + (s - s): a non-finite sum stays
                       non-finite); +0.0 everywhere else
        kcost[j]     = costs[idx[j]] bit for bit, +inf for j >= count

    ValueError on shapes that do not agree or n_keep outside 1..K."""
    U = np.asarray(U, np.float32)
    eps = np.asarray(noise, np.float32)
    c = np.asarray(costs, np.float32)
    single = U.ndim == 2
    if single:
        U, eps, c = U[None], eps[None], c[None]
    if U.ndim != 3 or eps.ndim != 4 or eps.shape[:3] != U.shape or c.shape != (U.shape[0], eps.shape[3]):
        raise ValueError("keep_store_ref: need U [B, nu, H], noise [B, nu, H, K] and costs [B, K]")
    B, nu, H = U.shape
    K = eps.shape[3]
    n_keep = int(n_keep)
    if not 1 <= n_keep <= K:
        raise ValueError(f"keep_store_ref: n_keep must be in 1..K = {K}")
    idx, count, _, _ = elite_select_ref(c, n_keep)
    sh = 1 if shift else 0
    steps = np.full(B, H - sh, np.int32)
    v = np.zeros((B, nu, H, n_keep), np.float32)
    kcost = np.full((B, n_keep), np.inf, np.float32)
    clamp = np.float32(ctrl_clamp)
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(B):
            m = int(count[b])
            kcost[b, :m] = c[b, idx[b, :m]]
            if m == 0 or H - sh == 0:
                continue
            s = (U[b][:, sh:, None] + eps[b][:, sh:, :][:, :, idx[b, :m]]).astype(np.float32)
            if clamp > 0:
                s = (np.fmin(clamp, np.fmax(-clamp, s)) + (s - s)).astype(np.float32)
            v[b, :, :H - sh, :m] = s
    return (v[0], kcost[0], idx[0], count[0], steps[0]) if single else (v, kcost, idx, count, steps)


def keep_inject_ref(U, noise, v, count, steps):
    """The injection of mppi_set_elite_keep in float32 (csrc/elite_keep.h), bitwise what the device computes: U
    [B, nu, H] (or [nu, H]) the nominal the solve will perturb, noise [B, nu, H, K] (or [nu, H, K]), v [B, nu, H, n_keep]
    and count / steps [B] (or the row's own) as keep_store_ref returns them -> the noise the rollout sees,

        eps[u, t, j] = float32(v[u, t, j] - U[u, t])     for j < count, t < steps

    and every other element the input's, bit for bit (a copy: the input is not written).  ValueError on shapes that do
    not agree, count outside 0..n_keep or steps outside 0..H."""
    U = np.asarray(U, np.float32)
    out = np.array(noise, np.float32, copy=True)
    v = np.asarray(v, np.float32)
    single = U.ndim == 2
    if single:
        U, out, v = U[None], out[None], v[None]
    count = np.atleast_1d(np.asarray(count, np.int64))
    steps = np.atleast_1d(np.asarray(steps, np.int64))
    if (U.ndim != 3 or out.ndim != 4 or v.ndim != 4 or out.shape[:3] != U.shape or v.shape[:3] != U.shape
            or count.shape != (U.shape[0],) or steps.shape != (U.shape[0],)):
        raise ValueError("keep_inject_ref: need U [B, nu, H], noise [B, nu, H, K], v [B, nu, H, n_keep], count and "
                         "steps [B]")
    B, nu, H = U.shape
    K, n_keep = out.shape[3], v.shape[3]
    if n_keep > K or ((count < 0) | (count > n_keep)).any() or ((steps < 0) | (steps > H)).any():
        raise ValueError("keep_inject_ref: need n_keep <= K, count in 0..n_keep and steps in 0..H")
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(B):
            m, st = int(count[b]), int(steps[b])
            if m and st:
                out[b, :, :st, :m] = (v[b, :, :st, :m] - U[b, :, :st, None]).astype(np.float32)
    return out[0] if single else out


# ---- weighted cross moments (MPPI_FLAG_CROSS; csrc/cross_moments.h)

def softmin_weights_ref(costs, lam: float = 1.0, norm_eps: float = 0.0) -> np.ndarray:
    """costs [B, K] -> the normalised softmin weights w [B, K] of solve_stats_ref (float64; 0 on non-finite costs and
    for a solve without a finite cost)."""
    c = np.asarray(costs, np.float64)
    c = c.reshape(-1, c.shape[-1])
    w = np.zeros(c.shape)
    for b in range(c.shape[0]):
        fin = np.isfinite(c[b])
        if fin.any():
            wt = np.zeros(c.shape[1])
            wt[fin] = np.exp(-(c[b][fin] - c[b][fin].min()) / lam)
            w[b] = wt / (wt.sum() + norm_eps)
    return w


def cross_moments_ref(costs, noise, lam: float = 1.0, norm_eps: float = 0.0, absolute: bool = False) -> np.ndarray:
    """costs [B, K], noise [B, nu, H, K] -> eps_mx [B, nu, nu] in float64.  absolute: the same sum over |e_u e_v|, the
    scale the fp32 summation's error is measured against (off-diagonal terms cancel)."""
    w = softmin_weights_ref(costs, lam, norm_eps)
    e = np.asarray(noise, np.float64)
    e = e.reshape(w.shape[0], -1, e.shape[-2], w.shape[1])
    if absolute:
        e = np.abs(e)
    return np.einsum("bk,buhk,bvhk->buv", w, e, e) / e.shape[2]


def _fma32_vec(a, b, c):
    """fmaf(a, b, c) elementwise on float32 arrays, exactly: the product of two floats is exact in float64, the sum is
    formed in float64 rounded TO ODD (the TwoSum residual decides), and rounding that to float32 is then the single
    rounding of the exact a * b + c (53 >= 24 + 2 bits)."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    with np.errstate(all="ignore"):
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        odd = (s.view(np.int64) & 1) != 0
        fix = np.isfinite(s) & (err != 0.0) & ~odd
        toward = np.where(err > 0.0, np.inf, -np.inf)
        s = np.where(fix, np.nextafter(s, toward), s)
        return s.astype(np.float32)


_BUTTERFLY = [np.arange(64) ^ o for o in (32, 16, 8, 4, 2, 1)]


def _wave_sum32(v):
    """wave_sum of csrc/wave_reduce.h over the last axis (64 lanes): the butterfly of offsets 32, 16, ..., 1 in float32;
    every lane ends with the same bits, lane 0 is returned."""
    v = np.asarray(v, np.float32)
    for perm in _BUTTERFLY:
        v = v + v[..., perm]
    return v[..., 0]


def moment_cells(H: int, Kp: int):
    """(nwc, L, nseg): the cells of one noise row (csrc/cross_moments.h moment_cells): wave-chunks of 256 k, at most 16
    horizon segments of L steps."""
    nwc = (Kp // 4 + 63) // 64
    smax = min(H, 16)
    L = (H + smax - 1) // smax
    return nwc, L, (H + L - 1) // L


def cross_moments_f32(w, noise) -> np.ndarray:
    """w [B, K] float32 (the normalised weights, as the device holds them), noise [B, nu, H, K] float32 -> eps_mx
    [B, nu, nu] float32 by the cell scheme of csrc/cross_moments.h, operation by operation: per cell (256 k x L steps)
    and lane one chain p = w_i * e_u_i; acc = fmaf(p, e_v_i, acc) in t order and x, y, z, w within a step, the wave's
    butterfly, then the finish pass over the cells and the division by float32(H).  Bitwise equal to the device and to
    the header through g++."""
    w = np.ascontiguousarray(w, np.float32)
    e = np.ascontiguousarray(noise, np.float32)
    B, K = w.shape
    e = e.reshape(B, -1, e.shape[-2], K)
    nu, H = e.shape[1], e.shape[2]
    Kp = (K + 63) // 64 * 64
    nwc, L, nseg = moment_cells(H, Kp)
    nq = Kp // 4
    # lanes beyond the row's last quad: weight 0 on the row's last quad (the device's clamp)
    q = np.minimum(np.arange(nwc * 64), nq - 1)
    act = np.arange(nwc * 64) < nq
    wp = np.zeros((B, Kp), np.float32)
    wp[:, :K] = w
    ep = np.zeros((B, nu, H, Kp), np.float32)
    ep[..., :K] = e
    wl = np.where(act[None, :, None], wp.reshape(B, nq, 4)[:, q], np.float32(0.0))   # [B, lanes, 4]
    el = ep.reshape(B, nu, H, nq, 4)[:, :, :, q]                                # [B, nu, H, lanes, 4]
    iu, iv = np.tril_indices(nu)
    npair = iu.size
    part = np.zeros((B, npair, nwc, nseg), np.float32)
    for s in range(nseg):
        acc = np.zeros((B, npair, nwc * 64), np.float32)
        for t in range(s * L, min(H, (s + 1) * L)):
            for i in range(4):
                et = el[:, :, t, :, i]                                          # [B, nu, lanes]
                p = wl[:, None, :, i] * et
                acc = _fma32_vec(p[:, iu], et[:, iv], acc)
        part[:, :, :, s] = _wave_sum32(acc.reshape(B, npair, nwc, 64))
    cells = part.reshape(B, npair, nwc * nseg)
    ncell = nwc * nseg
    lanes = np.zeros((B, npair, 64), np.float32)
    for i0 in range(0, ncell, 64):
        n = min(64, ncell - i0)
        lanes[:, :, :n] = lanes[:, :, :n] + cells[:, :, i0:i0 + n]
    m = _wave_sum32(lanes) / np.float32(H)
    mx = np.zeros((B, nu, nu), np.float32)
    mx[:, iu, iv] = m
    mx[:, iv, iu] = m
    return mx


# ---- the adapted covariance (mppi_set_noise_cov_adapt; csrc/noise_cov_adapt.h)

def _check_cov_adapt(rate, sigma_min, sigma_max):
    if not 0.0 <= float(rate) <= 1.0:
        raise ValueError("adapt_noise_cov: rate must be in [0, 1]")
    if not (0.0 < sigma_min <= sigma_max and np.isfinite(sigma_max)):
        raise ValueError("adapt_noise_cov: need 0 < sigma_min <= sigma_max < inf")


def adapt_noise_cov(Sigma, eps_mx, rate: float, sigma_min: float = 1e-3, sigma_max: float = 10.0) -> np.ndarray:
    """One step of the sampling covariance towards the noise that won the last solve(s), in float64: Sigma [nu, nu],
    eps_mx [B, nu, nu] (or [nu, nu]) the weighted cross moments of Engine.cross_moments -> the new Sigma.  Pure.

        S1 = (1 - rate) Sigma + rate mean_b eps_mx
        s = sqrt(diag S1);  c = clip(s, sigma_min, sigma_max);  Sigma' = diag(c / s) S1 diag(c / s)

    The clip is a congruence: it moves the standard deviations into the limits and keeps every correlation and the
    positive definiteness.  ValueError on bad settings or shapes, or a diagonal of S1 that is not finite and > 0."""
    _check_cov_adapt(rate, sigma_min, sigma_max)
    S = np.asarray(Sigma, np.float64)
    M = np.asarray(eps_mx, np.float64)
    if S.ndim != 2 or S.shape[0] != S.shape[1] or M.shape[-2:] != S.shape or M.ndim not in (2, 3):
        raise ValueError("adapt_noise_cov: Sigma must be [nu, nu] and eps_mx [B, nu, nu] or [nu, nu]")
    S1 = (1.0 - rate) * S + rate * M.reshape(-1, *S.shape).mean(axis=0)
    d = np.diag(S1)
    if not (np.all(np.isfinite(d)) and np.all(d > 0.0)):
        raise ValueError("adapt_noise_cov: the blended diagonal must be finite and > 0")
    s = np.sqrt(d)
    g = np.clip(s, sigma_min, sigma_max) / s
    return S1 * np.outer(g, g)  # (symmetric to the bit)


def _cov_factor_full(S):
    """csrc/noise_cov.h cov_factor in Python doubles, operation by operation: S [nu, nu] float32 (only its lower
    triangle is read) -> (L, Sinv, sigma_u) float32, or None where a pivot is not > 0 and finite or an entry of the
    inverse leaves float32."""
    nu = S.shape[0]
    Ld = [[0.0] * nu for _ in range(nu)]
    for u in range(nu):
        for v in range(u + 1):
            a = float(S[u, v])
            for j in range(v):
                p = Ld[u][j] * Ld[v][j]
                a = a - p
            if u == v:
                if not (a > 0.0 and np.isfinite(a)):
                    return None
                Ld[u][u] = float(np.sqrt(a))
            else:
                Ld[u][v] = a / Ld[v][v]
    Wd = [[0.0] * nu for _ in range(nu)]
    for c in range(nu):
        for r in range(c, nu):
            a = 1.0 if r == c else 0.0
            for j in range(c, r):
                p = Ld[r][j] * Wd[j][c]
                a = a - p
            Wd[r][c] = a / Ld[r][r]
    Sinv = np.zeros((nu, nu), np.float32)
    with np.errstate(over="ignore"):
        for u in range(nu):
            for v in range(u + 1):
                a = 0.0
                for j in range(u, nu):
                    p = Wd[j][u] * Wd[j][v]
                    a = a + p
                f = np.float32(a)
                if not np.isfinite(f):
                    return None
                Sinv[u, v] = Sinv[v, u] = f
    L = np.array(Ld, np.float64).astype(np.float32)
    sig = np.sqrt(np.diag(S).astype(np.float64)).astype(np.float32)
    return L, Sinv, sig


def adapt_noise_cov_f32(Sigma, eps_mx, rate, sigma_min=1e-3, sigma_max=10.0, n_finite=None):
    """The device's step (csrc/noise_cov_adapt.h), float32 operation by operation and the factor in doubles as
    noise.cov_factor runs it: Sigma [nu, nu] float32 (symmetric bit for bit, positive definite), eps_mx [B, nu, nu]
    float32, n_finite [B] or None -> (Sigma, L, Sinv, sigma_u, status), all float32 and bitwise what the device holds
    after the step.  status 1: the law moved; 0: some solve had no finite cost, nothing changed; -1: the step was
    rejected (a blended scale not finite or not > 0, a pivot not > 0 and finite, an inverse beyond float32), nothing
    changed.

        Mbar = sequential float32 sum over b, / float32(B);   S1 = fmaf(rate, Mbar, (1 - rate) * Sigma)   (v <= u)
        s_u = sqrt(S1[u][u]);  c_u = min(max(s_u, sigma_min), sigma_max);  g_u = c_u / s_u
        S2[u][v] = (S1[u][v] * g_u) * g_v (v < u, mirrored);  S2[u][u] = S1[u][u] if c_u == s_u else c_u * c_u"""
    from .noise import cov_factor
    _check_cov_adapt(rate, sigma_min, sigma_max)
    f = np.float32
    S = np.ascontiguousarray(Sigma, np.float32)
    nu = S.shape[0]
    M = np.ascontiguousarray(eps_mx, np.float32).reshape(-1, nu, nu)
    B = M.shape[0]

    def held(status):
        L, Sinv, sig = _cov_factor_full(S)
        return S.copy(), L, Sinv, sig, status

    if n_finite is not None and np.any(np.asarray(n_finite).reshape(-1) == 0):
        return held(0)
    rate, lo, hi = f(rate), f(sigma_min), f(sigma_max)
    with np.errstate(all="ignore"):
        acc = np.zeros((nu, nu), np.float32)
        for b in range(B):
            acc = acc + M[b]
        Mbar = acc / f(B)
        keep = f(1.0) - rate
        S1 = _fma32_vec(np.full((nu, nu), rate, np.float32), Mbar, keep * S)
        s = np.sqrt(np.diag(S1)).astype(np.float32)
        if not (np.all(np.isfinite(s)) and np.all(s > 0.0)):
            return held(-1)
        c = np.minimum(np.maximum(s, lo), hi).astype(np.float32)
        g = (c / s).astype(np.float32)
        S2 = np.zeros((nu, nu), np.float32)
        for u in range(nu):
            for v in range(u):
                S2[u, v] = S2[v, u] = f(f(S1[u, v] * g[u]) * g[v])
            S2[u, u] = S1[u, u] if c[u] == s[u] else f(c[u] * c[u])
    full = _cov_factor_full(S2)
    if full is None:
        return held(-1)
    L, Sinv, sig = full
    if np.all(np.isfinite(S2)):
        assert np.array_equal(L.view(np.uint32), cov_factor(S2).view(np.uint32))  # one factor, two statements
    return S2, L, Sinv, sig, 1


# ---- weighted per-step moments (MPPI_FLAG_STEP_MOMENTS; csrc/step_moments.h) and the refit of the per-step scales
# ---- (mppi_set_noise_steps_adapt; csrc/step_law.h)

def step_moments_ref(costs, noise, lam: float = 1.0, norm_eps: float = 0.0, w=None):
    """costs [B, K], noise [B, nu, H, K] -> (m1, m2), each [B, nu, H] in float64:
    m1 = sum_k w_k eps, m2 = sum_k w_k eps^2 with the softmin weights of solve_stats_ref -- or with the given weights
    w [B, K] (costs is then not read: pass None)."""
    w = softmin_weights_ref(costs, lam, norm_eps) if w is None else np.asarray(w, np.float64)
    w = w.reshape(-1, w.shape[-1])
    e = np.asarray(noise, np.float64)
    e = e.reshape(w.shape[0], -1, e.shape[-2], w.shape[1])
    return np.einsum("bk,buhk->buh", w, e), np.einsum("bk,buhk->buh", w, e * e)


def step_moments_f32(w, noise):
    """w [B, K] float32 (the normalised weights, as the device holds them), noise [B, nu, H, K] float32 -> (m1, m2),
    each [B, nu, H] float32, by the cell scheme of csrc/step_moments.h, operation by operation: per wave-chunk of 256 k
    and lane the chains a1 = fmaf(w_i, e_i, a1) and p = w_i * e_i; a2 = fmaf(p, e_i, a2) over the lane's quad in the
    order x, y, z, w, the wave's butterfly, then the chunks added in ascending order from 0.  Bitwise equal to the
    device and to the header through g++."""
    w = np.ascontiguousarray(w, np.float32)
    e = np.ascontiguousarray(noise, np.float32)
    B, K = w.shape
    e = e.reshape(B, -1, e.shape[-2], K)
    nu, H = e.shape[1], e.shape[2]
    Kp = (K + 63) // 64 * 64
    nq = Kp // 4
    nwc = (nq + 63) // 64
    # lanes beyond the row's last quad: weight 0 on the row's last quad (the device's clamp)
    q = np.minimum(np.arange(nwc * 64), nq - 1)
    act = np.arange(nwc * 64) < nq
    wp = np.zeros((B, Kp), np.float32)
    wp[:, :K] = w
    ep = np.zeros((B, nu, H, Kp), np.float32)
    ep[..., :K] = e
    wl = np.where(act[None, :, None], wp.reshape(B, nq, 4)[:, q], np.float32(0.0))[:, None, None]  # [B, 1, 1, lanes, 4]
    el = ep.reshape(B, nu, H, nq, 4)[:, :, :, q]                                                   # [B, nu, H, lanes, 4]
    wl = np.broadcast_to(wl, el.shape)
    a1 = np.zeros(el.shape[:-1], np.float32)
    a2 = np.zeros(el.shape[:-1], np.float32)
    with np.errstate(all="ignore"):
        for i in range(4):
            a1 = _fma32_vec(wl[..., i], el[..., i], a1)
            p = wl[..., i] * el[..., i]
            a2 = _fma32_vec(p, el[..., i], a2)
        c1 = _wave_sum32(a1.reshape(B, nu, H, nwc, 64))
        c2 = _wave_sum32(a2.reshape(B, nu, H, nwc, 64))
        m1 = np.zeros((B, nu, H), np.float32)
        m2 = np.zeros((B, nu, H), np.float32)
        for wc in range(nwc):
            m1 = m1 + c1[..., wc]
            m2 = m2 + c2[..., wc]
    return m1, m2


def _check_steps_adapt(rate, sigma_min, sigma_max):
    if not 0.0 <= float(rate) <= 1.0:
        raise ValueError("adapt_noise_steps: rate must be in [0, 1]")
    if not (0.0 < sigma_min <= sigma_max and np.isfinite(sigma_max)):
        raise ValueError("adapt_noise_steps: need 0 < sigma_min <= sigma_max < inf")


def _shift_steps(S, fill):
    """The table moved one step along the horizon: S[..., t] <- S[..., t + 1], the last cell the per-actuator fill."""
    out = np.empty_like(S)
    out[..., :-1] = S[..., 1:]
    out[..., -1] = np.broadcast_to(np.asarray(fill, S.dtype), S.shape[:-1])
    return out


def adapt_noise_steps(table, m1, m2, rate: float, sigma_min: float = 1e-3, sigma_max: float = 10.0,
                      centred: bool = True, shift: bool = False, fill=None, n_finite=None) -> np.ndarray:
    """One refit of the per-step scales in float64 (the rule of mppi_set_noise_steps_adapt): table, m1, m2 [B, nu, H]
    (or [nu, H]) -> the new table.  Pure.  Per solve, no batch mean:

        v  = m2 - m1^2 if centred else m2, clipped below at 0
        S' = clip(sqrt((1 - rate) S^2 + rate v), sigma_min, sigma_max)
        shift: S[t] <- S'[t + 1], S[H - 1] <- fill [nu] (a scalar: every actuator's; required with shift)

    n_finite [B] (default: all finite): a solve with 0 is only shifted.  ValueError on bad settings or shapes."""
    _check_steps_adapt(rate, sigma_min, sigma_max)
    S = np.asarray(table, np.float64)
    a, b = np.asarray(m1, np.float64), np.asarray(m2, np.float64)
    if S.ndim not in (2, 3) or a.shape != S.shape or b.shape != S.shape:
        raise ValueError("adapt_noise_steps: table, m1 and m2 must all be [B, nu, H] or [nu, H]")
    single = S.ndim == 2
    if single:
        S, a, b = S[None], a[None], b[None]
    if shift and fill is None:
        raise ValueError("adapt_noise_steps: shift needs the fill (sigma_u)")
    v = np.maximum(b - a * a if centred else b, 0.0)
    new = np.clip(np.sqrt((1.0 - rate) * S * S + rate * v), sigma_min, sigma_max)
    if n_finite is not None:
        dead = np.asarray(n_finite).reshape(-1)[:S.shape[0]] == 0
        new[dead] = S[dead]
    if shift:
        f = np.asarray(fill, np.float64)
        new = _shift_steps(new, np.full(S.shape[1], float(f)) if f.ndim == 0 else f.reshape(1, -1))
    return new[0] if single else new


def adapt_noise_steps_f32(table, m1, m2, rate, sigma_min=1e-3, sigma_max=10.0, centred=True, shift=False, fill=None,
                          n_finite=None) -> np.ndarray:
    """The device's refit (csrc/step_law.h, mppi_set_noise_steps_adapt) restated in numpy float32, operation by
    operation: table, m1, m2 [B, nu, H] float32, n_finite [B] or None, fill [nu] (or a scalar; read with shift only) ->
    the table after one step, bitwise what step_adapt_kernel leaves.

        n_finite[b] == 0: no cell of solve b is refit
        v   = fmaf(-m1, m1, m2) if centred else m2;   a non-finite v leaves the cell;   v = v if v > 0 else 0
        var = fmaf(rate, v, (1 - rate) * (S * S));    S' = min(max(sqrt(var), sigma_min), sigma_max)
              (a non-finite var or root leaves the cell)
        shift: S[t] <- S'[t + 1], S[H - 1] <- fill[u]

    adapt_noise_steps is the same rule in float64 (it raises on invalid input, this one follows the kernel)."""
    f = np.float32
    S = np.array(table, np.float32, copy=True)
    a, b = np.asarray(m1, np.float32), np.asarray(m2, np.float32)
    single = S.ndim == 2
    if single:
        S, a, b = S[None], a[None], b[None]
    rate, lo, hi = f(rate), f(sigma_min), f(sigma_max)
    with np.errstate(all="ignore"):
        v = _fma32_vec(-a, a, b) if centred else b.copy()
        ok = np.isfinite(v)
        v = np.where(v > 0.0, v, f(0.0)).astype(np.float32)
        keep = f(f(1.0) - rate)
        old = (keep * (S * S).astype(np.float32)).astype(np.float32)
        var = _fma32_vec(np.full(S.shape, rate, np.float32), v, old)
        r = np.sqrt(var, dtype=np.float32)
        ok &= np.isfinite(var) & np.isfinite(r)
        r = np.where(r < lo, lo, r)
        r = np.where(r > hi, hi, r).astype(np.float32)
    if n_finite is not None:
        ok &= (np.asarray(n_finite).reshape(-1)[:S.shape[0]] != 0)[:, None, None]
    new = np.where(ok, r, S).astype(np.float32)
    if shift:
        fl = np.asarray(fill, np.float32)
        new = _shift_steps(new, np.full(S.shape[1], fl, np.float32) if fl.ndim == 0 else fl.reshape(1, -1))
    return new[0] if single else new


def iter_best_ref(U, noise, costs, it: int = 0, stored=None, ctrl_clamp: float = 0.0):
    """The best-sample tracking of mppi_set_iterations in float32 (csrc/iter_best.h), bitwise what the device computes:
    U [B, nu, H] (or [nu, H]) the nominal the rollout perturbed, noise [B, nu, H, K] (or [nu, H, K]) as the rollout saw
    it, costs [B, K] (or [K]) what the softmin would weigh ahead of any elite masking ->
    (v [B, nu, H] float32, cost [B] float32, k [B] int32, iter [B] int32).

        stored None  the step's first iteration: the stored best is reset to (v = +0.0, cost = +inf, k = -1, iter = -1)
        stored       else the (v, cost, k, iter) carried in (copied, never written)
        k*           = the lowest k attaining the minimum over the finite costs (-0.0 equals +0.0); none finite: no
                       candidate
        accepted iff costs[k*] < cost, strict in float32; then cost = costs[k*] bit for bit, k = k*, iter = it and
        v[u, t]      = float32(U[u, t] + noise[u, t, k*]), clamped to +-ctrl_clamp when ctrl_clamp > 0 as
                       csrc/rate_cost.h clamps (c + (s - s): a non-finite sum stays non-finite)

    ValueError on shapes that do not agree."""
    U = np.asarray(U, np.float32)
    eps = np.asarray(noise, np.float32)
    c = np.asarray(costs, np.float32)
    single = U.ndim == 2
    if single:
        U, eps, c = U[None], eps[None], c[None]
    if U.ndim != 3 or eps.ndim != 4 or eps.shape[:3] != U.shape or c.shape != (U.shape[0], eps.shape[3]):
        raise ValueError("iter_best_ref: need U [B, nu, H], noise [B, nu, H, K] and costs [B, K]")
    B, nu, H = U.shape
    if stored is None:
        v = np.zeros((B, nu, H), np.float32)
        cost = np.full(B, np.inf, np.float32)
        k = np.full(B, -1, np.int32)
        bi = np.full(B, -1, np.int32)
    else:
        v = np.array(stored[0], np.float32).reshape(B, nu, H)
        cost = np.array(stored[1], np.float32).reshape(B)
        k = np.array(stored[2], np.int32).reshape(B)
        bi = np.array(stored[3], np.int32).reshape(B)
    clamp = np.float32(ctrl_clamp)
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(B):
            fin = np.isfinite(c[b])
            if not fin.any():
                continue
            ks = int(np.argmin(np.where(fin, c[b], np.float32(np.inf))))  # the first occurrence: the lowest k
            if not c[b, ks] < cost[b]:
                continue
            cost[b], k[b], bi[b] = c[b, ks], ks, it
            s = (U[b] + eps[b][:, :, ks]).astype(np.float32)
            if clamp > 0:
                s = (np.fmin(clamp, np.fmax(-clamp, s)) + (s - s)).astype(np.float32)
            v[b] = s
    return (v[0], cost[0], k[0], bi[0]) if single else (v, cost, k, bi)


def icem_population(K: int, n_iter: int, gamma: float, k_min: int) -> np.ndarray:
    """iCEM's sample budget per inner iteration, N_i = max(N / gamma^i, k_min), as mppi_population_icem computes it
    (csrc/population.h pop_icem) -> int32 [n_iter], the table Engine.set_population takes:

        d = 1.0;  for i < n_iter:  K_it[i] = max(k_min, int(K / d));  d *= gamma

    in double, a division, a truncation and a product per entry -- correctly rounded operations only, no pow -- so the
    table equals the C helper's on any host.  ValueError unless gamma >= 1, 1 <= k_min <= K and 1 <= n_iter <= 16."""
    K, n_iter, k_min, gamma = int(K), int(n_iter), int(k_min), float(gamma)
    if not gamma >= 1.0 or K < 1 or k_min < 1 or k_min > K or n_iter < 1 or n_iter > 16:
        raise ValueError("icem_population: need gamma >= 1, 1 <= k_min <= K and n_iter in [1, 16]")
    out = np.empty(n_iter, np.int32)
    d = 1.0
    for i in range(n_iter):
        out[i] = max(k_min, int(float(K) / d))
        d *= gamma
    return out


ENSEMBLE_MODES = {"mean": 0, "mean_std": 1, "worst": 2}  # MPPI_ENS_* (include/mppi.h)


def ensemble_combine_f32(member_costs, mode="mean", kappa: float = 0.0):
    """The combining rule of a dynamics-model ensemble (mppi_set_ensemble; csrc/ensemble.h) as the device takes it, float32
    operation by operation -> (costs, sd), each of member_costs' shape without its first axis, bit for bit the device's.

    member_costs [n, ...] float32, 2 <= n <= 8, the members' costs of every sample; r = float32(1) / float32(n):

        any member not finite:  cost = +inf, sd = +inf
        s = c_0;  s = s + c_e  ascending;  m = s * r;  every member bit for bit c_0: m = c_0
        q = +0;   q = fmaf(c_e - m, c_e - m, q)  ascending;  sd = sqrt(q * r)
        "mean": cost = m;  "mean_std": cost = fmaf(kappa, sd, m);  "worst": cost = the max, +0 above -0
        a non-finite cost becomes +inf, a non-finite sd becomes +inf"""
    m_id = ENSEMBLE_MODES.get(mode, mode)
    if isinstance(m_id, bool) or m_id not in ENSEMBLE_MODES.values():
        raise ValueError(f"ensemble_combine_f32: mode must be one of {sorted(ENSEMBLE_MODES)}")
    c = np.asarray(member_costs, np.float32)
    if c.ndim < 1 or not 2 <= c.shape[0] <= 8:
        raise ValueError("ensemble_combine_f32: member_costs must be [n, ...] with 2 <= n <= 8")
    kappa = np.float32(kappa)
    if not np.isfinite(kappa):
        raise ValueError("ensemble_combine_f32: kappa must be finite")
    n = c.shape[0]
    r = np.float32(1.0) / np.float32(n)
    inf = np.float32(np.inf)
    with np.errstate(all="ignore"):
        fin = np.isfinite(c).all(axis=0)
        s = c[0].copy()
        mx = c[0].copy()
        for e in range(1, n):
            s = (s + c[e]).astype(np.float32)
            # the larger; of two zeros, +0
            mx = np.where(mx < c[e], c[e], np.where(c[e] < mx, mx, np.where(np.signbit(mx), c[e], mx)))
        u = np.ascontiguousarray(c).view(np.uint32)
        same = (u == u[0]).all(axis=0)  # n equal numbers: their mean is that number
        m = np.where(same, c[0], (s * r).astype(np.float32)).astype(np.float32)
        q = np.zeros_like(m)
        for e in range(n):
            d = (c[e] - m).astype(np.float32)
            q = _fma32_vec(d, d, q)
        sd = np.sqrt((q * r).astype(np.float32)).astype(np.float32)
        if m_id == 0:
            cost = m
        elif m_id == 1:
            cost = _fma32_vec(np.broadcast_to(kappa, sd.shape).astype(np.float32), sd, m)
        else:
            cost = mx.astype(np.float32)
        cost = np.where(fin & np.isfinite(cost), cost, inf).astype(np.float32)
        sd = np.where(fin & np.isfinite(sd), sd, inf).astype(np.float32)
    return cost, sd
