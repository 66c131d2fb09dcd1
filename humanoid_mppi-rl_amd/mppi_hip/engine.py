"""Thin object wrapper over one C-ABI handle (one device, one stream)."""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, field, fields

import numpy as np

from . import _lib as L

_KINDS_COST = {"cartpole": L.COST_CARTPOLE, "cartpole_est": L.COST_CARTPOLE_EST, "humanoid_v3": L.COST_HUMANOID_V3,
               "humanoid_v1": L.COST_HUMANOID_V1, "quad_jl": L.COST_QUAD_JL, "quad_est": L.COST_QUAD_EST}
# MPPI_ENS_* (include/mppi.h): how an ensemble's member costs become one cost per sample
ENSEMBLE_MODES = {"mean": 0, "mean_std": 1, "worst": 2}


@dataclass
class Config:
    """mppi_config as a dataclass; see include/mppi.h for field meaning."""
    nx: int
    nu: int
    H: int
    K: int
    max_batch: int = 1
    lambda_: float = 1.0
    sigma: float = 1.0
    ctrl_clamp: float = 0.0
    U_clamp: float = 0.0
    norm_eps: float = 0.0
    shift_fill: float = 0.1
    terminal_weight: float = 10.0
    update_mode: int = L.UPDATE_ADD
    precision: int = L.PREC_BF16

    @classmethod
    def preset(cls, name: str, **overrides) -> "Config":
        c = L.preset_config(name)
        kw = {f.name: getattr(c, f.name) for f in fields(cls)}
        kw.update(overrides)
        return cls(**kw)

    def to_c(self) -> L.mppi_config:
        c = L.mppi_config()
        for f in fields(self):
            setattr(c, f.name, getattr(self, f.name))
        return c


def _f32(a, shape=None):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float32))
    if shape is not None and a.shape != tuple(shape):
        a = a.reshape(shape)
    return a


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


@dataclass
class SolveResult:
    U: np.ndarray
    costs: np.ndarray | None = None
    weights: np.ndarray | None = None
    u0: np.ndarray | None = None
    status: int = 0
    stats: dict | None = None  # solve(..., stats=True): Engine.stats of this solve


class Engine:
    def __init__(self, config: Config, device: int = 0):
        self.lib = L.load()
        self.config = config
        h = ctypes.c_void_p()
        L.check(self.lib.mppi_create(ctypes.byref(config.to_c()), device, ctypes.byref(h)))
        self._h = h
        self.device = device

    # -- lifecycle
    def close(self):
        if getattr(self, "_h", None):
            self.lib.mppi_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- setup
    def load_dynamics(self, kind: int, blob: bytes | None = None):
        if blob is None:
            L.check(self.lib.mppi_load_dynamics(self._h, kind, None, 0))
        else:
            buf = ctypes.create_string_buffer(blob, len(blob))
            L.check(self.lib.mppi_load_dynamics(self._h, kind, buf, len(blob)))
        return self

    def set_cost(self, kind, params=None):
        kind = _KINDS_COST.get(kind, kind)
        if params is None:
            L.check(self.lib.mppi_set_cost(self._h, kind, None, 0))
        else:
            p = _f32(params).ravel()
            L.check(self.lib.mppi_set_cost(self._h, kind, p.ctypes.data_as(L._fp), int(p.size)))
        return self

    def set_noise_model(self, sigma_u=None, rho: float = 0.0):
        """The sampling law of the device noise (mppi_set_noise_model): per-actuator standard deviations sigma_u [nu]
        (None = config.sigma for all) and the AR(1) correlation rho in [0, 1) along the horizon (noise.ar1_filter
        states the law).  (None, 0.0) restores the default white noise and its code path."""
        p = None
        if sigma_u is not None:
            s = _f32(sigma_u).ravel()
            if s.size != self.config.nu:
                raise ValueError(f"set_noise_model: sigma_u must have nu = {self.config.nu} entries, got {s.size}")
            p = s.ctypes.data_as(L._fp)
        L.check(self.lib.mppi_set_noise_model(self._h, p, ctypes.c_float(rho)))
        return self

    def noise_model(self) -> tuple[np.ndarray, float, bool]:
        """(sigma_u [nu], rho, active) of the handle's sampling law (mppi_get_noise_model).  With set_noise_adapt on
        it is the live device law after every enqueued solve (waits for the stream)."""
        s = np.empty(self.config.nu, np.float32)
        rho, active = ctypes.c_float(), ctypes.c_int()
        L.check(self.lib.mppi_get_noise_model(self._h, s.ctypes.data_as(L._fp), ctypes.byref(rho),
                                              ctypes.byref(active)))
        return s, float(rho.value), bool(active.value)

    def set_noise_adapt(self, rate: float, sigma_min: float = 1e-3, sigma_max: float = 10.0, rho_max: float = 0.95):
        """Adapt the sampling law on the device behind every solve (mppi_set_noise_adapt; the rule is
        stats.adapt_noise_model_f32): rate in (0, 1] enables, 0 disables and keeps the law as it stands.  Chained
        solves and graph streams adapt step by step with no host round trip.  Destroys captured graphs, as
        set_noise_model does."""
        L.check(self.lib.mppi_set_noise_adapt(self._h, ctypes.c_float(rate), ctypes.c_float(sigma_min),
                                              ctypes.c_float(sigma_max), ctypes.c_float(rho_max)))
        return self

    def noise_adapt(self) -> tuple[float, float, float, float]:
        """(rate, sigma_min, sigma_max, rho_max) of mppi_get_noise_adapt; rate 0.0 while adaptation is off."""
        v = [ctypes.c_float() for _ in range(4)]
        L.check(self.lib.mppi_get_noise_adapt(self._h, *(ctypes.byref(x) for x in v)))
        return tuple(float(x.value) for x in v)

    def set_noise_knots(self, n_knots: int, order: int = 1):
        """Knot-parameterised sampling noise (mppi_set_noise_knots; noise.knot_table / noise.knot_filter state the
        law): the device noise is drawn at n_knots knots along the horizon (1..H) and interpolated, order 0 (hold),
        1 (linear) or 3 (Catmull-Rom).  n_knots = 0 disables and keeps sigma_u and rho.  Makes the noise model active;
        destroys captured graphs, as set_noise_model does.  Not together with set_control_cost or set_noise_adapt."""
        L.check(self.lib.mppi_set_noise_knots(self._h, int(n_knots), int(order)))
        return self

    def noise_knots(self) -> tuple[int, int, np.ndarray | None, np.ndarray | None]:
        """(n_knots, order, idx [H, 4] int32, w [H, 4] float32) of the handle's knot law (mppi_get_noise_knots);
        (0, 0, None, None) while off."""
        H = self.config.H
        idx, w = np.zeros((H, 4), np.int32), np.zeros((H, 4), np.float32)
        n, order = ctypes.c_int(), ctypes.c_int()
        L.check(self.lib.mppi_get_noise_knots(self._h, ctypes.byref(n), ctypes.byref(order), _ptr(idx), _ptr(w)))
        if n.value == 0:
            return 0, 0, None, None
        return int(n.value), int(order.value), idx, w

    def set_noise_basis(self, M):
        """Horizon-basis sampling noise (mppi_set_noise_basis; noise.basis_filter states the law, noise.colored_basis
        builds iCEM's power-law table): the device noise of one (b, u, k) is M [H, R] (float32, 1 <= R <= min(H, 128))
        applied along the horizon to R white normals, scaled by sigma_u.  None disables and keeps sigma_u.  Makes the
        noise model active; destroys captured graphs, as set_noise_model does.  Not together with rho != 0,
        set_noise_knots, set_noise_cov, set_noise_adapt or set_control_cost."""
        if M is None:
            L.check(self.lib.mppi_set_noise_basis(self._h, 0, None))
            return self
        A = _f32(M)
        H = self.config.H
        if A.ndim != 2 or A.shape[0] != H or A.shape[1] < 1:
            raise ValueError(f"set_noise_basis: M must be [{H}, R] with R >= 1, got {list(A.shape)}")
        L.check(self.lib.mppi_set_noise_basis(self._h, int(A.shape[1]), _ptr(A)))
        return self

    def noise_basis(self) -> np.ndarray | None:
        """M [H, R] float32 of the handle's basis law as set, bitwise (mppi_get_noise_basis); None while off."""
        n = ctypes.c_int()
        L.check(self.lib.mppi_get_noise_basis(self._h, ctypes.byref(n), None))
        if n.value == 0:
            return None
        A = np.zeros((self.config.H, n.value), np.float32)
        L.check(self.lib.mppi_get_noise_basis(self._h, ctypes.byref(n), _ptr(A)))
        return A

    def set_noise_cov(self, Sigma):
        """Cross-actuator sampling covariance (mppi_set_noise_cov; noise.cov_factor / noise.cov_filter state the law):
        the device noise of one step is drawn with the full covariance Sigma [nu, nu] (float32: symmetric bit for bit,
        positive definite), eps[:, t, k] = L e[:, t, k] with Sigma = L L^T and e the handle's unit-variance AR(1) rows.
        None disables and keeps sigma_u = sqrt(diag Sigma) and rho.  Makes the noise model active; destroys captured
        graphs, as set_noise_model does.  Not together with set_noise_knots or set_noise_adapt."""
        if Sigma is None:
            L.check(self.lib.mppi_set_noise_cov(self._h, None))
            return self
        S = _f32(Sigma)
        nu = self.config.nu
        if S.shape != (nu, nu):
            raise ValueError(f"set_noise_cov: Sigma must be [{nu}, {nu}], got {list(S.shape)}")
        L.check(self.lib.mppi_set_noise_cov(self._h, _ptr(S)))
        return self

    def noise_cov(self) -> tuple[np.ndarray, np.ndarray, np.ndarray] | None:
        """(Sigma, L, Sinv), each [nu, nu] float32, of the handle's covariance (mppi_get_noise_cov): Sigma as given,
        its Cholesky factor (bitwise noise.cov_factor(Sigma)) and the inverse the control-cost term uses; None while
        off."""
        nu = self.config.nu
        S, Lf, Si = (np.zeros((nu, nu), np.float32) for _ in range(3))
        active = ctypes.c_int()
        L.check(self.lib.mppi_get_noise_cov(self._h, _ptr(S), _ptr(Lf), _ptr(Si), ctypes.byref(active)))
        return (S, Lf, Si) if active.value else None

    def set_noise_cov_adapt(self, rate: float, sigma_min: float = 1e-3, sigma_max: float = 10.0):
        """Adapt the full sampling covariance on the device behind every solve (mppi_set_noise_cov_adapt; the rule is
        stats.adapt_noise_cov_f32): Sigma moves towards the batch mean of the weighted cross moments, its standard
        deviations are clipped to [sigma_min, sigma_max] with the correlations kept, and L and Sigma^-1 are re-factored
        on the device.  rate in (0, 1] enables (needs set_noise_cov first), 0 disables and keeps the law as it
        stands.  Chained solves and graph streams adapt step by step with no host round trip.  Destroys captured
        graphs, as set_noise_adapt does."""
        L.check(self.lib.mppi_set_noise_cov_adapt(self._h, float(rate), float(sigma_min), float(sigma_max)))
        return self

    def noise_cov_adapt(self) -> tuple[float, float, float, int]:
        """(rate, sigma_min, sigma_max, rejects) of mppi_get_noise_cov_adapt; rate 0.0 while adaptation is off; rejects:
        the steps the device refused (a non-finite or rank-deficient blend) since it was enabled."""
        v = [ctypes.c_float() for _ in range(3)]
        r = ctypes.c_uint64()
        L.check(self.lib.mppi_get_noise_cov_adapt(self._h, *(ctypes.byref(x) for x in v), ctypes.byref(r)))
        return v[0].value, v[1].value, v[2].value, int(r.value)

    def noise_cov_law(self, step: int = 0) -> np.ndarray:
        """The Sigma [nu, nu] the adapting solve `step` drew its noise from (mppi_get_noise_cov_law; waits for the
        stream): step 0 after a plain or chained solve, 0..n_solves-1 after graph_launch."""
        nu = self.config.nu
        S = np.zeros((nu, nu), np.float32)
        L.check(self.lib.mppi_get_noise_cov_law(self._h, step, _ptr(S)))
        return S

    def set_noise_steps(self, sigma):
        """A sampling scale per solve, actuator and horizon step (mppi_set_noise_steps; noise.steps_filter states the
        law): eps[b, u, t, k] = sigma[b, u, t] * e[t] with e the handle's unit-variance AR(1) row -- the distribution
        of CEM / iCEM.  sigma [B, nu, H] float32 (1 <= B <= max_batch; slot b takes row b mod B), or [nu, H], which
        broadcasts one table to every solve; entries finite and >= 0.  None disables and keeps sigma_u and rho.  While
        on, sigma_u of set_noise_model is the fill a step entering the horizon starts with.  Makes the noise model
        active; a change destroys captured graphs, as set_noise_model does.  Not together with set_noise_knots,
        set_noise_basis, set_noise_cov, set_noise_adapt or set_control_cost.  Needs nu <= 32."""
        if sigma is None:
            L.check(self.lib.mppi_set_noise_steps(self._h, 0, None))
            return self
        c = self.config
        S = _f32(sigma)
        if S.ndim == 2:
            S = S[None]
        if S.ndim != 3 or S.shape[1:] != (c.nu, c.H):
            raise ValueError(f"set_noise_steps: sigma must be [B, {c.nu}, {c.H}] or [{c.nu}, {c.H}], "
                             f"got {list(S.shape)}")
        S = np.ascontiguousarray(S)
        L.check(self.lib.mppi_set_noise_steps(self._h, int(S.shape[0]), _ptr(S)))
        return self

    def noise_steps(self, B: int = 1) -> np.ndarray | None:
        """The live table [B, nu, H] float32 of the handle's per-step scales (mppi_get_noise_steps; waits for the
        stream: with set_noise_steps_adapt on, after every enqueued solve's refit); None while off."""
        c = self.config
        S = np.zeros((int(B), c.nu, c.H), np.float32)
        active = ctypes.c_int()
        L.check(self.lib.mppi_get_noise_steps(self._h, int(B), _ptr(S), ctypes.byref(active)))
        return S if active.value else None

    def set_noise_steps_adapt(self, rate: float, sigma_min: float = 1e-3, sigma_max: float = 10.0,
                              centred: bool = True):
        """Refit the per-step scales on the device behind every solve, each solve's table from its own per-step
        moments, and shift it along the horizon with the nominal (mppi_set_noise_steps_adapt; the rule is
        stats.adapt_noise_steps_f32): CEM's variance update with momentum.  rate in (0, 1] enables (needs
        set_noise_steps first), 0 disables and keeps the table as it stands.  centred: the variance about the weighted
        mean (CEM; with set_elites, of the elites about their mean), else the moment about the nominal.  Chained
        solves and graph streams refit step by step with no host round trip.  Destroys captured graphs, as
        set_noise_adapt does."""
        L.check(self.lib.mppi_set_noise_steps_adapt(self._h, float(rate), float(sigma_min), float(sigma_max),
                                                    int(bool(centred))))
        return self

    def noise_steps_adapt(self) -> tuple[float, float, float, bool]:
        """(rate, sigma_min, sigma_max, centred) of mppi_get_noise_steps_adapt; rate 0.0 while the refit is off."""
        v = [ctypes.c_float() for _ in range(3)]
        cen = ctypes.c_int()
        L.check(self.lib.mppi_get_noise_steps_adapt(self._h, *(ctypes.byref(x) for x in v), ctypes.byref(cen)))
        return float(v[0].value), float(v[1].value), float(v[2].value), bool(cen.value)

    def noise_eval(self, B: int, seed: int) -> np.ndarray:
        """The noise [B, nu, H, K] (float32) the handle's generator draws for the by-value key `seed` under the law in
        effect (mppi_noise_eval): a solve's noise for that key, ahead of bounds and kept elites.  Drops a prefetched
        noise (key sequence unchanged); U and every stored state stay."""
        c = self.config
        out = np.empty((int(B), c.nu, c.H, c.K), np.float32)
        L.check(self.lib.mppi_noise_eval(self._h, int(B), ctypes.c_uint64(int(seed) & (2**64 - 1)), _ptr(out)))
        return out

    def noise_law(self, step: int = 0) -> tuple[np.ndarray, float]:
        """(sigma_u [nu], rho) the adapting solve `step` drew its noise from (mppi_get_noise_law; waits for the
        stream): step 0 after a plain or chained solve, 0..n_solves-1 after graph_launch."""
        s = np.empty(self.config.nu, np.float32)
        rho = ctypes.c_float()
        L.check(self.lib.mppi_get_noise_law(self._h, step, s.ctypes.data_as(L._fp), ctypes.byref(rho)))
        return s, float(rho.value)

    # -- ESS targeting (mppi_set_ess_target; mppi_hip.stats.ess_lambda_ref states the rule)
    def set_ess_target(self, ess_frac: float, lambda_min: float = 1e-3, lambda_max: float = 1e3):
        """Choose the softmin temperature on the device, per solve, so that the solve's own costs give the effective
        sample size max(1, ess_frac * n_finite), within [lambda_min, lambda_max] (mppi_set_ess_target): ess_frac in
        (0, 1] enables, 0 disables and config.lambda_ runs again.  Works in every stream form with no host round trip;
        the analytic cartpole then takes three launches per solve instead of one.  Any change destroys captured graphs;
        a prefetched noise is kept."""
        L.check(self.lib.mppi_set_ess_target(self._h, ctypes.c_float(ess_frac), ctypes.c_float(lambda_min),
                                             ctypes.c_float(lambda_max)))
        return self

    def ess_target(self) -> tuple[float, float, float]:
        """(ess_frac, lambda_min, lambda_max) of mppi_get_ess_target; ess_frac 0.0 while targeting is off."""
        v = [ctypes.c_float() for _ in range(3)]
        L.check(self.lib.mppi_get_ess_target(self._h, *(ctypes.byref(x) for x in v)))
        return tuple(float(x.value) for x in v)

    def lambdas(self, B: int = 1, step: int = 0) -> np.ndarray:
        """lambda [B] the targeting solve `step` updated with (mppi_get_lambda; waits for the stream): step 0 after a
        plain or chained solve, 0..n_solves-1 after graph_launch."""
        out = np.empty(B, np.float32)
        L.check(self.lib.mppi_get_lambda(self._h, B, step, _ptr(out)))
        return out

    def lambda_eval(self, costs) -> np.ndarray:
        """The search kernel on host costs [B, K] (or [K]; non-finite entries allowed) -> lambda [B] (mppi_lambda_eval).
        Needs targeting enabled; no dynamics or cost need be loaded."""
        costs = _f32(costs).reshape(-1, self.config.K)
        out = np.empty(costs.shape[0], np.float32)
        L.check(self.lib.mppi_lambda_eval(self._h, costs.shape[0], _ptr(costs), _ptr(out)))
        return out

    # -- the control-cost term (mppi_set_control_cost; mppi_hip.stats.control_term_ref states the definitions)
    def set_control_cost(self, gamma: float):
        """Add the control-cost term of information-theoretic MPPI to the costs the softmin weighs
        (mppi_set_control_cost): gamma * sum U Sigma^-1 eps with Sigma the covariance of the law that drew the solve's
        noise.  A finite gamma > 0 (cost units, absolute) enables, 0 disables.  Works in every stream form; the `costs`
        output stays the rollout's.  The analytic cartpole leaves its fused one-launch form while it is on.  Any change
        destroys captured graphs; a prefetched noise is kept."""
        L.check(self.lib.mppi_set_control_cost(self._h, ctypes.c_float(gamma)))
        return self

    def control_cost(self) -> float:
        """gamma of mppi_get_control_cost; 0.0 while the term is off."""
        g = ctypes.c_float()
        L.check(self.lib.mppi_get_control_cost(self._h, ctypes.byref(g)))
        return float(g.value)

    def control_term(self, B: int = 1) -> tuple[np.ndarray, np.ndarray]:
        """(term [B, K], lin [B, nu, H]) of the last solve enqueued with the term on (mppi_get_control_term; waits for
        the stream) -- after graph_launch the chain's last solve."""
        c = self.config
        term = np.empty((B, c.K), np.float32)
        lin = np.empty((B, c.nu, c.H), np.float32)
        L.check(self.lib.mppi_get_control_term(self._h, B, _ptr(term), _ptr(lin)))
        return term, lin

    def control_term_eval(self, U, noise) -> tuple[np.ndarray, np.ndarray]:
        """The term's kernels on host arrays U [B, nu, H] and noise [B, nu, H, K] with the handle's current law and
        gamma -> (term [B, K], lin [B, nu, H]) (mppi_control_term_eval).  Needs the term enabled; no dynamics or cost
        need be loaded."""
        c = self.config
        U = _f32(U).reshape(-1, c.nu, c.H)
        B = U.shape[0]
        nz = _f32(noise).reshape(B, c.nu, c.H, c.K)
        term = np.empty((B, c.K), np.float32)
        lin = np.empty((B, c.nu, c.H), np.float32)
        L.check(self.lib.mppi_control_term_eval(self._h, B, _ptr(U), _ptr(nz), _ptr(term), _ptr(lin)))
        return term, lin

    # -- per-actuator control bounds (mppi_set_control_bounds; mppi_hip.stats.project_noise_ref states the rule)
    def _bound(self, v, name):
        if v is None:
            return None
        a = np.asarray(v, dtype=np.float32)
        a = np.full(self.config.nu, a, np.float32) if a.ndim == 0 else np.ascontiguousarray(a).ravel()
        if a.size != self.config.nu:
            raise ValueError(f"set_control_bounds: {name} must be a scalar or have nu = {self.config.nu} entries, "
                             f"got {a.size}")
        return a

    def set_control_bounds(self, lo=None, hi=None):
        """Keep every sampled control U + eps and the nominal U inside the box [lo[u], hi[u]] (mppi_set_control_bounds):
        the solve's noise is projected on the device ahead of the rollout (eps' = clip(U + eps, lo, hi) - U), U and u0
        are clipped behind the update.  lo, hi: scalars or [nu] (a model's actuator_ctrlrange columns); None leaves
        that side unbounded, (None, None) disables.  Works in every stream form; costs, weights, the control-cost term
        and the statistics describe the projected noise.  Any change destroys captured graphs; a prefetched noise is
        kept.  Needs nu <= 32."""
        lo, hi = self._bound(lo, "lo"), self._bound(hi, "hi")
        L.check(self.lib.mppi_set_control_bounds(self._h, None if lo is None else lo.ctypes.data_as(L._fp),
                                                 None if hi is None else hi.ctypes.data_as(L._fp)))
        return self

    def control_bounds(self) -> tuple[np.ndarray, np.ndarray, bool]:
        """(lo [nu], hi [nu], active) of mppi_get_control_bounds; -inf / +inf while the bounds are off."""
        lo, hi = np.empty(self.config.nu, np.float32), np.empty(self.config.nu, np.float32)
        active = ctypes.c_int()
        L.check(self.lib.mppi_get_control_bounds(self._h, lo.ctypes.data_as(L._fp), hi.ctypes.data_as(L._fp),
                                                 ctypes.byref(active)))
        return lo, hi, bool(active.value)

    def bound_counts(self, B: int = 1) -> np.ndarray:
        """counts [B, nu] (uint32): the (t, k) noise elements of each actuator the last enqueued bounded solve
        projected (mppi_get_bound_counts; waits for the stream) -- after graph_launch the chain's last solve."""
        out = np.empty((B, self.config.nu), np.uint32)
        L.check(self.lib.mppi_get_bound_counts(self._h, B, _ptr(out)))
        return out

    def bounds_eval(self, U, noise) -> tuple[np.ndarray, np.ndarray]:
        """The projection kernel alone on host arrays U [B, nu, H] and noise [B, nu, H, K] with the handle's box ->
        (projected noise [B, nu, H, K], counts [B, nu]) (mppi_bounds_eval).  Needs the bounds set; no dynamics or cost
        need be loaded."""
        c = self.config
        U = _f32(U).reshape(-1, c.nu, c.H)
        B = U.shape[0]
        nz = _f32(noise).reshape(B, c.nu, c.H, c.K)
        out = np.empty_like(nz)
        counts = np.empty((B, c.nu), np.uint32)
        L.check(self.lib.mppi_bounds_eval(self._h, B, _ptr(U), _ptr(nz), _ptr(out), _ptr(counts)))
        return out, counts

    # -- the control-rate cost term (mppi_set_rate_cost; mppi_hip.stats.rate_term_ref states the definitions)
    def set_rate_cost(self, weights, anchor: bool = True):
        """Add a penalty on the rate of the sampled controls to the costs the softmin weighs (mppi_set_rate_cost):
        sum_u r[u] sum_t (v[u, t] - v[u, t-1])^2 with v = clamp(U + eps) the control the rollout applied and, with
        `anchor`, v[u, -1] the control applied the step before (set_prev_control, or the u0 of the last shift solve).
        weights: a scalar (every actuator's) or [nu], finite, >= 0, not all zero; None disables.  Works in every stream
        form; the `costs` output stays the rollout's.  The analytic cartpole leaves its fused one-launch form while it
        is on.  Any change destroys captured graphs; a prefetched noise is kept.  Needs nu <= 32."""
        if weights is None:
            L.check(self.lib.mppi_set_rate_cost(self._h, None, 0))
            return self
        r = np.asarray(weights, dtype=np.float32)
        r = np.full(self.config.nu, r, np.float32) if r.ndim == 0 else np.ascontiguousarray(r).ravel()
        if r.size != self.config.nu:
            raise ValueError(f"set_rate_cost: weights must be a scalar or have nu = {self.config.nu} entries, "
                             f"got {r.size}")
        L.check(self.lib.mppi_set_rate_cost(self._h, r.ctypes.data_as(L._fp), int(bool(anchor))))
        return self

    def rate_cost(self) -> tuple[np.ndarray, bool, bool]:
        """(weights [nu], anchor, active) of mppi_get_rate_cost; zeros and False while the term is off."""
        r = np.empty(self.config.nu, np.float32)
        anchor, active = ctypes.c_int(), ctypes.c_int()
        L.check(self.lib.mppi_get_rate_cost(self._h, r.ctypes.data_as(L._fp), ctypes.byref(anchor),
                                            ctypes.byref(active)))
        return r, bool(anchor.value), bool(active.value)

    def set_prev_control(self, u):
        """The control applied the step before, u [B, nu] (or [nu]) -> the handle's u_prev (mppi_set_prev_control):
        what the anchored rate term differences t = 0 against.  Data, not a setting: captured graphs stay."""
        u = _f32(u).reshape(-1, self.config.nu)
        L.check(self.lib.mppi_set_prev_control(self._h, u.shape[0], _ptr(u)))
        return self

    def prev_control(self, B: int = 1) -> np.ndarray:
        """The handle's u_prev [B, nu] (mppi_get_prev_control; waits for the stream): zeros until set, then what was
        set or the u0 of the last shift solve made with the anchored term."""
        out = np.empty((B, self.config.nu), np.float32)
        L.check(self.lib.mppi_get_prev_control(self._h, B, _ptr(out)))
        return out

    def rate_term(self, B: int = 1) -> np.ndarray:
        """term [B, K] of the last solve enqueued with the term on (mppi_get_rate_term; waits for the stream) -- after
        graph_launch the chain's last solve."""
        term = np.empty((B, self.config.K), np.float32)
        L.check(self.lib.mppi_get_rate_term(self._h, B, _ptr(term)))
        return term

    def rate_term_eval(self, U, noise, u_prev=None) -> np.ndarray:
        """The term's kernel on host arrays U [B, nu, H], noise [B, nu, H, K] (as the rollout would see it: no
        projection here) and u_prev [B, nu] (None: the handle's) with the handle's weights, anchor and ctrl_clamp ->
        term [B, K] (mppi_rate_term_eval).  Needs the term enabled; no dynamics or cost need be loaded."""
        c = self.config
        U = _f32(U).reshape(-1, c.nu, c.H)
        B = U.shape[0]
        nz = _f32(noise).reshape(B, c.nu, c.H, c.K)
        up = None if u_prev is None else _f32(u_prev).reshape(B, c.nu)
        term = np.empty((B, c.K), np.float32)
        L.check(self.lib.mppi_rate_term_eval(self._h, B, _ptr(U), _ptr(nz), None if up is None else _ptr(up),
                                             _ptr(term)))
        return term

    # -- elite truncation (mppi_set_elites; mppi_hip.stats.elite_select_ref states the rule)
    def set_elites(self, n_elite: int):
        """Weigh only the n_elite best samples of each solve (mppi_set_elites): the selection runs on the device behind
        the rollout and the cost terms, exact and with ties admitted by ascending k; every other sample's weight is 0.
        n_elite in 1..K enables, 0 disables.  n_elite with a large lambda is CEM's elite mean, with set_ess_target a
        scale-free softmin over the elites, n_elite = K today's MPPI.  Works in every stream form; the `costs` output
        stays the rollout's.  The analytic cartpole leaves its fused one-launch form while it is on.  Any change
        destroys captured graphs; a prefetched noise is kept."""
        L.check(self.lib.mppi_set_elites(self._h, int(n_elite)))
        return self

    def elites(self) -> int:
        """n_elite of mppi_get_elites; 0 while off."""
        n = ctypes.c_int()
        L.check(self.lib.mppi_get_elites(self._h, ctypes.byref(n)))
        return int(n.value)

    def elite_set(self, B: int = 1) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(idx [B, n_elite] int32 in ascending k, -1 behind count; count [B]; tau [B]) of the last solve enqueued with
        elites (mppi_get_elite_set; waits for the stream) -- after graph_launch the chain's last solve."""
        n = self.elites()
        idx = np.empty((B, max(n, 1)), np.int32)
        count = np.empty(B, np.int32)
        tau = np.empty(B, np.float32)
        L.check(self.lib.mppi_get_elite_set(self._h, B, _ptr(idx), _ptr(count), _ptr(tau)))
        return idx, count, tau

    def elites_eval(self, costs) -> tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """The selection kernel on host costs [B, K] (or [K]; ties, NaN and +-inf allowed) with the handle's n_elite ->
        (idx [B, n_elite], count [B], tau [B], ecost [B, K]) (mppi_elites_eval).  Needs elites enabled; no dynamics or
        cost need be loaded."""
        costs = _f32(costs).reshape(-1, self.config.K)
        B, n = costs.shape[0], self.elites()
        idx = np.empty((B, max(n, 1)), np.int32)
        count = np.empty(B, np.int32)
        tau = np.empty(B, np.float32)
        ecost = np.empty((B, self.config.K), np.float32)
        L.check(self.lib.mppi_elites_eval(self._h, B, _ptr(costs), _ptr(idx), _ptr(count), _ptr(tau), _ptr(ecost)))
        return idx, count, tau, ecost

    # -- keep / shift elites (mppi_set_elite_keep; mppi_hip.stats.keep_store_ref / keep_inject_ref state the rule)
    def set_elite_keep(self, n_keep: int):
        """Carry the n_keep best sampled control sequences of each solve into the next one (mppi_set_elite_keep; iCEM's
        keep / shift elites): gathered on the device behind the rollout and the cost terms, time-shifted when the solve
        shifts, and injected into the first columns of the next solve's noise ahead of its bounds projection and
        rollout.  n_keep in 1..K enables, 0 disables.  Works in every stream form with no host round trip; the first
        solve with the feature on is bit for bit the solve without it.  The analytic cartpole leaves its fused
        one-launch form while it is on.  Any change destroys captured graphs and empties the stored set; a prefetched
        noise is kept."""
        L.check(self.lib.mppi_set_elite_keep(self._h, int(n_keep)))
        return self

    def elite_keep(self) -> int:
        """n_keep of mppi_get_elite_keep; 0 while off."""
        n = ctypes.c_int()
        L.check(self.lib.mppi_get_elite_keep(self._h, ctypes.byref(n)))
        return int(n.value)

    def kept(self, B: int = 1) -> tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """(v [B, nu, H, n_keep], kcost [B, n_keep], idx [B, n_keep] int32, count [B] int32, steps [B] int32): the set
        stored by the last solve enqueued, or written by set_kept (mppi_get_kept; waits for the stream) -- the planned
        candidate sequences and their costs.  After set_kept, kcost is +inf and idx -1."""
        c, n = self.config, max(self.elite_keep(), 1)
        v = np.empty((B, c.nu, c.H, n), np.float32)
        kcost = np.empty((B, n), np.float32)
        idx = np.empty((B, n), np.int32)
        count = np.empty(B, np.int32)
        steps = np.empty(B, np.int32)
        L.check(self.lib.mppi_get_kept(self._h, B, _ptr(v), _ptr(kcost), _ptr(idx), _ptr(count), _ptr(steps)))
        return v, kcost, idx, count, steps

    def _kept_args(self, who, B, v, count, steps):
        c, n = self.config, self.elite_keep()
        v = _f32(v)
        if n == 0 or v.size != B * c.nu * c.H * n:
            raise ValueError(f"{who}: v must be [B, nu, H, n_keep] = [{B}, {c.nu}, {c.H}, {n}] with the feature on")
        count = np.ascontiguousarray(np.asarray(count, np.int32)).ravel()
        steps = np.ascontiguousarray(np.asarray(steps, np.int32)).ravel()
        if count.size != B or steps.size != B:
            raise ValueError(f"{who}: count and steps must have B = {B} entries")
        return v.reshape(B, c.nu, c.H, n), count, steps

    def set_kept(self, v, count=None, steps=None, B: int | None = None):
        """Write the stored set of slots 0..B (mppi_set_kept): v [B, nu, H, n_keep] candidate control sequences, count
        [B] in 0..n_keep (default: n_keep) and steps [B] in 0..H (default: H) -- seeds the next solve with sequences of
        the caller's, or restores a saved set.  v None empties slots 0..B (B default 1).  Data, not a setting: captured
        graphs stay and their first solve injects this set."""
        c = self.config
        if v is None:
            L.check(self.lib.mppi_set_kept(self._h, 1 if B is None else int(B), None, None, None))
            return self
        n = self.elite_keep()
        v = _f32(v)
        if B is None:
            B = v.size // max(c.nu * c.H * max(n, 1), 1)
        B = int(B)
        count = np.full(B, n, np.int32) if count is None else count
        steps = np.full(B, c.H, np.int32) if steps is None else steps
        v, count, steps = self._kept_args("set_kept", B, v, count, steps)
        L.check(self.lib.mppi_set_kept(self._h, B, _ptr(v), _ptr(count), _ptr(steps)))
        return self

    def keep_store_eval(self, U, noise, costs, shift: bool = False):
        """The selection + gather kernels on host arrays U [B, nu, H], noise [B, nu, H, K] (as the rollout saw it) and
        costs [B, K] (NaN, +-inf and ties allowed) with the handle's n_keep and ctrl_clamp -> (v, kcost, idx, count,
        steps) as kept() (mppi_keep_store_eval).  The handle's stored set is untouched.  Needs the feature enabled; no
        dynamics or cost need be loaded."""
        c, n = self.config, max(self.elite_keep(), 1)
        U = _f32(U).reshape(-1, c.nu, c.H)
        B = U.shape[0]
        nz = _f32(noise).reshape(B, c.nu, c.H, c.K)
        costs = _f32(costs).reshape(B, c.K)
        v = np.empty((B, c.nu, c.H, n), np.float32)
        kcost = np.empty((B, n), np.float32)
        idx = np.empty((B, n), np.int32)
        count = np.empty(B, np.int32)
        steps = np.empty(B, np.int32)
        L.check(self.lib.mppi_keep_store_eval(self._h, B, _ptr(U), _ptr(nz), _ptr(costs), int(bool(shift)), _ptr(v),
                                              _ptr(kcost), _ptr(idx), _ptr(count), _ptr(steps)))
        return v, kcost, idx, count, steps

    def keep_inject_eval(self, U, noise, v, count, steps) -> np.ndarray:
        """The inject kernel on host arrays U [B, nu, H], noise [B, nu, H, K], v [B, nu, H, n_keep], count and steps
        [B] -> the noise the rollout would see [B, nu, H, K] (mppi_keep_inject_eval).  The handle's stored set is
        untouched.  Needs the feature enabled; no dynamics or cost need be loaded."""
        c = self.config
        U = _f32(U).reshape(-1, c.nu, c.H)
        B = U.shape[0]
        nz = _f32(noise).reshape(B, c.nu, c.H, c.K)
        v, count, steps = self._kept_args("keep_inject_eval", B, v, count, steps)
        out = np.empty_like(nz)
        L.check(self.lib.mppi_keep_inject_eval(self._h, B, _ptr(U), _ptr(nz), _ptr(v), _ptr(count), _ptr(steps),
                                               _ptr(out)))
        return out

    # -- inner iterations per control step (mppi_set_iterations; mppi_hip.stats.iter_best_ref states the tracking's rule)
    def set_iterations(self, n_iter: int, return_best: bool = False, add_mean: bool = False):
        """Refine the distribution n_iter (1..16) times per control step on the device (mppi_set_iterations; CEM / iCEM
        proper): a step -- one solve, one chained solve, one solve of a captured graph -- is bit for bit n_iter
        consecutive solves on the same state, all but the last without shift and env step, each with a fresh noise key
        and a statistics slot of its own (Engine.stats(B, step=it)).  return_best: the step executes the first control
        of the best sample seen during the step (u0, the rate anchor, the env step and the trajectory record see it; U
        is unchanged).  add_mean: the step's last iteration enters the nominal itself as a candidate.  While any of the
        three is on, the best sampled sequence of the step is tracked on the device (Engine.best).  Injected noise with
        n_iter > 1 and u0_before with n_iter > 1 or return_best are refused.  Any change destroys captured graphs; a
        prefetched noise is kept."""
        for name, v in (("return_best", return_best), ("add_mean", add_mean)):
            if v not in (0, 1, False, True):
                raise ValueError(f"set_iterations: {name} must be a bool")
        L.check(self.lib.mppi_set_iterations(self._h, int(n_iter), int(bool(return_best)), int(bool(add_mean))))
        return self

    def iterations(self) -> tuple[int, bool, bool]:
        """(n_iter, return_best, add_mean) of mppi_get_iterations; (1, False, False) by default."""
        n, rb, am = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        L.check(self.lib.mppi_get_iterations(self._h, ctypes.byref(n), ctypes.byref(rb), ctypes.byref(am)))
        return int(n.value), bool(rb.value), bool(am.value)

    def best(self, B: int = 1) -> tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """(v [B, nu, H], cost [B], k [B] int32, iter [B] int32): the best sampled control sequence of the last control
        step enqueued -- the planned trajectory -- with its cost, its sample index and the iteration that drew it
        (mppi_get_best; waits for the stream).  k = iter = -1, cost = +inf, v = 0 when no sample of the step was
        finite."""
        c = self.config
        v = np.empty((B, c.nu, c.H), np.float32)
        cost = np.empty(B, np.float32)
        k = np.empty(B, np.int32)
        it = np.empty(B, np.int32)
        L.check(self.lib.mppi_get_best(self._h, B, _ptr(v), _ptr(cost), _ptr(k), _ptr(it)))
        return v, cost, k, it

    def iter_best_eval(self, U, noise, costs, it: int = 0, stored=None):
        """The tracking kernel on host arrays U [B, nu, H], noise [B, nu, H, K] (as the rollout saw it) and costs
        [B, K] (NaN, +-inf and ties allowed) with the handle's ctrl_clamp -> (v, cost, k, iter) as best()
        (mppi_iter_best_eval).  stored None: the step's first iteration (the stored best is reset); else the (v, cost,
        k, iter) carried in.  The handle's stored best is untouched; no dynamics or cost need be loaded."""
        c = self.config
        U = _f32(U).reshape(-1, c.nu, c.H)
        B = U.shape[0]
        nz = _f32(noise).reshape(B, c.nu, c.H, c.K)
        costs = _f32(costs).reshape(B, c.K)
        if stored is None:
            v = np.empty((B, c.nu, c.H), np.float32)
            cost = np.empty(B, np.float32)
            k = np.empty(B, np.int32)
            bi = np.empty(B, np.int32)
        else:
            v = _f32(stored[0]).reshape(B, c.nu, c.H).copy()
            cost = _f32(stored[1]).reshape(B).copy()
            k = np.ascontiguousarray(np.asarray(stored[2], np.int32)).reshape(B).copy()
            bi = np.ascontiguousarray(np.asarray(stored[3], np.int32)).reshape(B).copy()
        L.check(self.lib.mppi_iter_best_eval(self._h, B, _ptr(U), _ptr(nz), _ptr(costs), int(stored is None), int(it),
                                             _ptr(v), _ptr(cost), _ptr(k), _ptr(bi)))
        return v, cost, k, bi

    # -- population-size decay (mppi_set_population; mppi_hip.stats.icem_population computes iCEM's schedule)
    def set_population(self, schedule):
        """A sample count per inner iteration (mppi_set_population; iCEM's shrinking budget): iteration i of every control
        step draws, rolls out and weighs schedule[i] samples and is bit for bit the solve of an engine created with
        K = schedule[i], the state handed over from iteration to iteration.  len(schedule) must equal n_iter of
        set_iterations, schedule[0] == K, every entry in [1, K] and >= n_elite, n_keep (n_keep + 1 with add_mean).
        None turns it off; a schedule of K throughout is the feature off.  costs / weights of a solve and the [B, K]
        read-outs then hold the last iteration's samples in their first schedule[-1] entries per row.  Any change
        destroys captured graphs and drops a prefetched noise (key sequence unchanged)."""
        if schedule is None:
            L.check(self.lib.mppi_set_population(self._h, None, 0))
            return self
        tab = np.ascontiguousarray(np.asarray(schedule, np.int64).reshape(-1))
        if tab.size and (np.abs(tab) >= 2**31).any():
            raise ValueError("set_population: entries must fit int32")
        tab = tab.astype(np.int32)
        L.check(self.lib.mppi_set_population(self._h, _ptr(tab), int(tab.size)))
        return self

    def population(self):
        """The schedule of set_population as a tuple of ints, or None while it is off (mppi_get_population)."""
        tab = np.zeros(16, np.int32)
        n = ctypes.c_int(0)
        L.check(self.lib.mppi_get_population(self._h, _ptr(tab), ctypes.byref(n)))
        return tuple(int(v) for v in tab[: n.value]) if n.value else None

    def iter_rollout_kernel(self, it: int) -> str:
        """The kernel iteration `it` of the last control step's rollout was routed to (mppi_iter_rollout_kernel); ""
        outside [0, n_iter) or before any solve."""
        return (self.lib.mppi_iter_rollout_kernel(self._h, int(it)) or b"").decode()

    # -- dynamics-model ensembles (mppi_set_ensemble; mppi_hip.stats.ensemble_combine_f32 restates the rule)
    def load_member(self, e: int, kind: int, blob: bytes | None = None):
        """Member e >= 1 of an ensemble (mppi_load_member): any blob load_dynamics accepts for this config, of member 0's
        kind; members are loaded densely and a loaded e is replaced.  Member 0 is what load_dynamics loaded."""
        if blob is None:
            L.check(self.lib.mppi_load_member(self._h, int(e), kind, None, 0))
        else:
            buf = ctypes.create_string_buffer(blob, len(blob))
            L.check(self.lib.mppi_load_member(self._h, int(e), kind, buf, len(blob)))
        return self

    def set_ensemble(self, n: int, mode="mean", kappa: float = 0.0, env_member: int = 0):
        """Roll every sample under members 0..n-1 and combine their costs per sample on the device (mppi_set_ensemble):
        mode "mean", "mean_std" (mean + kappa * population std; kappa < 0 is an optimism bonus) or "worst" (the max).
        n == 1 turns it off (loaded members stay).  env_member steps the environment.  Any change destroys captured
        graphs and drops a prefetched noise (key sequence unchanged)."""
        m = ENSEMBLE_MODES.get(mode, mode)
        if isinstance(m, bool) or not isinstance(m, (int, np.integer)) or int(m) not in ENSEMBLE_MODES.values():
            raise ValueError(f"set_ensemble: mode must be one of {sorted(ENSEMBLE_MODES)}")
        L.check(self.lib.mppi_set_ensemble(self._h, int(n), int(m), float(kappa), int(env_member)))
        return self

    def ensemble(self) -> dict:
        """The setting in effect and the number of members loaded, member 0 included (mppi_get_ensemble)."""
        n, mode, env, loaded = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
        kappa = ctypes.c_float(0.0)
        L.check(self.lib.mppi_get_ensemble(self._h, ctypes.byref(n), ctypes.byref(mode), ctypes.byref(kappa),
                                           ctypes.byref(env), ctypes.byref(loaded)))
        names = {v: k for k, v in ENSEMBLE_MODES.items()}
        return {"n": n.value, "mode": names[mode.value], "kappa": float(kappa.value), "env_member": env.value,
                "n_loaded": loaded.value}

    def member_costs(self, e: int, B: int = 1) -> np.ndarray:
        """Member e's costs [B, K] of the last solve with the ensemble on (mppi_get_member_costs): bit for bit the costs
        of an engine that loaded that member alone."""
        out = np.zeros((int(B), self.config.K), np.float32)
        L.check(self.lib.mppi_get_member_costs(self._h, int(B), int(e), _ptr(out)))
        return out

    def ensemble_spread(self, B: int = 1) -> np.ndarray:
        """The members' population std per sample [B, K] of the last solve with the ensemble on
        (mppi_get_ensemble_spread)."""
        out = np.zeros((int(B), self.config.K), np.float32)
        L.check(self.lib.mppi_get_ensemble_spread(self._h, int(B), _ptr(out)))
        return out

    def ensemble_eval(self, member_costs, mode="mean", kappa: float = 0.0):
        """The combining kernel on host arrays member_costs [n, B, K] (NaN and +-inf allowed) -> (costs, sd), [B, K] each
        (mppi_ensemble_eval).  The handle's state is untouched; no dynamics or cost need be loaded."""
        c = self.config
        mc = _f32(member_costs)
        if mc.ndim == 2:
            mc = mc[:, None, :]
        if mc.ndim != 3 or mc.shape[2] != c.K:
            raise ValueError("ensemble_eval: member_costs must be [n, B, K]")
        m = ENSEMBLE_MODES.get(mode, mode)
        if isinstance(m, bool) or not isinstance(m, (int, np.integer)) or int(m) not in ENSEMBLE_MODES.values():
            raise ValueError(f"ensemble_eval: mode must be one of {sorted(ENSEMBLE_MODES)}")
        n, B = mc.shape[0], mc.shape[1]
        mc = np.ascontiguousarray(mc)
        costs = np.zeros((B, c.K), np.float32)
        sd = np.zeros((B, c.K), np.float32)
        L.check(self.lib.mppi_ensemble_eval(self._h, B, n, int(m), float(kappa), _ptr(mc), _ptr(costs), _ptr(sd)))
        return costs, sd

    # -- host-memory solve
    def solve(self, x0, U, noise=None, seed: int = 0, ctx=None, shift: bool = False, u0_before: bool = False,
              want_costs: bool = True, want_weights: bool = False, colmajor: bool = False,
              raise_nonfinite: bool = False, stats: bool = False, cross: bool = False,
              step_moments: bool = False) -> SolveResult:
        """One batched solve. x0 [B,nx] (or [nx]); U [B,nu,H] (or [nu,H]); noise None (device Philox) or
        [B,nu,H,K] (or [nu,H,K]). Returns the updated (and optionally shifted) U plus diagnostics.
        stats: also compute the solve's statistics on the device (MPPI_FLAG_STATS) into SolveResult.stats.
        cross: the statistics plus the weighted cross moments (MPPI_FLAG_CROSS): SolveResult.stats["eps_mx"] [B,nu,nu].
        step_moments: the statistics plus the weighted per-step moments (MPPI_FLAG_STEP_MOMENTS):
        SolveResult.stats["step_m1"], ["step_m2"] [B,nu,H]."""
        c = self.config
        single = np.ndim(x0) == 1
        x0 = _f32(x0).reshape(-1, c.nx)
        B = x0.shape[0]
        Uo = _f32(U).reshape(B, c.H, c.nu) if colmajor else _f32(U).reshape(B, c.nu, c.H)
        Uo = Uo.copy()
        nz = None
        if noise is not None:
            nz = _f32(noise).reshape(B, c.K, c.H, c.nu) if colmajor else _f32(noise).reshape(B, c.nu, c.H, c.K)
        cx = None if ctx is None else _f32(ctx).reshape(B, L.CTX_MAX)
        costs = np.empty((B, c.K), np.float32) if want_costs else None
        weights = np.empty((B, c.K), np.float32) if want_weights else None
        u0 = np.empty((B, c.nu), np.float32)
        io = L.mppi_io(_ptr(x0), _ptr(Uo), _ptr(nz), _ptr(costs), _ptr(weights), _ptr(u0), _ptr(cx))
        flags = (L.FLAG_SHIFT if shift else 0) | (L.FLAG_U0_BEFORE if u0_before else 0) | (
            L.FLAG_COLMAJOR if colmajor else 0) | (L.FLAG_STATS if stats else 0) | (L.FLAG_CROSS if cross else 0) | (
            L.FLAG_STEP_MOMENTS if step_moments else 0)
        rc = self.lib.mppi_solve_ex(self._h, B, ctypes.byref(io), ctypes.c_uint64(seed), flags)
        if rc != L.MPPI_E_NONFINITE or raise_nonfinite:
            L.check(rc)
        sq = (lambda a: a[0]) if single else (lambda a: a)
        last = self.iterations()[0] - 1 if stats or cross or step_moments else 0  # the step's last iteration's slot
        st = {k: sq(v) for k, v in self.stats(B, last).items()} if stats or cross or step_moments else None
        if cross:
            st["eps_mx"] = sq(self.cross_moments(B, last))
        if step_moments:
            m1, m2 = self.step_moments(B, last)
            st["step_m1"], st["step_m2"] = sq(m1), sq(m2)
        return SolveResult(U=sq(Uo), costs=None if costs is None else sq(costs),
                           weights=None if weights is None else sq(weights), u0=sq(u0), status=rc, stats=st)

    # -- device-memory solve (pointers are integers, e.g. torch tensor .data_ptr())
    def solve_device(self, B: int, x0_ptr: int, U_ptr: int | None = None, noise_ptr: int | None = None, seed: int = 0,
                     costs_ptr: int | None = None, u0_ptr: int | None = None, ctx_ptr: int | None = None,
                     weights_ptr: int | None = None, shift: bool = False, resident_U: bool = False,
                     asynchronous: bool = True, env_step: bool = False, seed_counter: bool = False,
                     chain: bool = False, stats: bool = False, cross: bool = False,
                     step_moments: bool = False) -> int:
        """stats: also compute the solve's statistics (MPPI_FLAG_STATS; read with Engine.stats);
        cross: the statistics plus the weighted cross moments (MPPI_FLAG_CROSS; read with Engine.cross_moments);
        step_moments: the statistics plus the per-step moments (MPPI_FLAG_STEP_MOMENTS; read with Engine.step_moments);
        env_step: advance x0 in place by one dynamics step with u0 (MPPI_FLAG_ENV_STEP);
        seed_counter: noise key = seed + the handle's device counter (MPPI_FLAG_SEED_COUNTER);
        chain: a chained solve (MPPI_FLAG_CHAIN: the previous chained solve's reduce generated this one's noise;
        2 launches, bitwise equal to plain counter solves)."""
        io = L.mppi_io(x0_ptr, U_ptr, noise_ptr, costs_ptr, weights_ptr, u0_ptr, ctx_ptr)
        flags = self._dev_flags(shift, resident_U, env_step) | (L.FLAG_ASYNC if asynchronous else 0) | (
            L.FLAG_SEED_COUNTER if seed_counter else 0) | (L.FLAG_CHAIN if chain else 0) | (
            L.FLAG_STATS if stats else 0) | (L.FLAG_CROSS if cross else 0) | (
            L.FLAG_STEP_MOMENTS if step_moments else 0)
        return L.check(self.lib.mppi_solve_ex(self._h, B, ctypes.byref(io), ctypes.c_uint64(seed), flags))

    @staticmethod
    def _dev_flags(shift, resident_U, env_step):
        return L.FLAG_DEVICE | (L.FLAG_SHIFT if shift else 0) | (L.FLAG_RESIDENT_U if resident_U else 0) | (
            L.FLAG_ENV_STEP if env_step else 0)

    # -- receding-horizon stream as one hipGraph (mppi_graph_capture / mppi_graph_launch)
    def graph_capture(self, B: int, n_solves: int, x0_ptr: int, U_ptr: int | None = None, u0_ptr: int | None = None,
                      ctx_ptr: int | None = None, costs_ptr: int | None = None, seed: int = 0, shift: bool = True,
                      resident_U: bool = False, env_step: bool = True, stats: bool = False, cross: bool = False,
                      step_moments: bool = False):
        return self.graph_capture_traj(B, n_solves, x0_ptr, U_ptr, u0_ptr, ctx_ptr, costs_ptr, seed, shift,
                                       resident_U, env_step, stats=stats, cross=cross, step_moments=step_moments)

    def graph_capture_traj(self, B: int, n_solves: int, x0_ptr: int, U_ptr: int | None = None,
                           u0_ptr: int | None = None, ctx_ptr: int | None = None, costs_ptr: int | None = None,
                           seed: int = 0, shift: bool = True, resident_U: bool = False, env_step: bool = True,
                           traj_x_ptr: int | None = None, traj_u_ptr: int | None = None, stats: bool = False,
                           cross: bool = False, step_moments: bool = False):
        """Capture n_solves chained solves; with traj_*_ptr (device [n][B][nx] / [n][B][nu]) the env steps log
        the (state, control) trajectory.  stats: solve i also writes its statistics, Engine.stats(B, step=i); cross:
        and its weighted cross moments, Engine.cross_moments(B, step=i); step_moments: and its per-step moments,
        Engine.step_moments(B, step=i)."""
        io = L.mppi_io(x0_ptr, U_ptr, None, costs_ptr, None, u0_ptr, ctx_ptr)
        self._graph_io = io  # the graph holds these device pointers
        flags = self._dev_flags(shift, resident_U, env_step) | (L.FLAG_STATS if stats else 0) | (
            L.FLAG_CROSS if cross else 0) | (L.FLAG_STEP_MOMENTS if step_moments else 0)
        L.check(self.lib.mppi_graph_capture_traj(self._h, B, ctypes.byref(io), ctypes.c_uint64(seed), flags,
                                                 n_solves, traj_x_ptr, traj_u_ptr))
        return self

    def graph_launch(self, sync: bool = False) -> int:
        return L.check(self.lib.mppi_graph_launch(self._h, int(sync)))

    def set_seed_counter(self, value: int = 0):
        L.check(self.lib.mppi_set_seed_counter(self._h, ctypes.c_uint64(value)))

    def get_seed_counter(self) -> int:
        """The device noise-key counter after every enqueued solve (waits for the stream): with get_U, the warm-start
        state of a receding-horizon stream (checkpoint / resume)."""
        v = ctypes.c_uint64(0)
        L.check(self.lib.mppi_get_seed_counter(self._h, ctypes.byref(v)))
        return int(v.value)

    # -- solve diagnostics (MPPI_FLAG_STATS; mppi_hip.stats.solve_stats_ref states the definitions)
    def _stats_dict(self, rec, m2, m11) -> dict:
        out = {n: rec[n].copy() for n in rec.dtype.names}
        if m2 is not None:
            out["eps_m2"], out["eps_m11"] = m2, m11
        return out

    def stats(self, B: int = 1, step: int = 0) -> dict:
        """The statistics of the last solve made with stats=True (mppi_get_stats; waits for the stream): the fields of
        mppi_solve_stats as arrays [B], plus eps_m2 and eps_m11 [B, nu].  step: 0 after a plain or chained solve,
        0..n_solves-1 after graph_launch of a graph captured with stats=True."""
        rec = np.zeros(B, np.dtype(L.STATS_DTYPE))
        m2 = np.zeros((B, self.config.nu), np.float32)
        m11 = np.zeros((B, self.config.nu), np.float32)
        L.check(self.lib.mppi_get_stats(self._h, B, step, _ptr(rec), _ptr(m2), _ptr(m11)))
        return self._stats_dict(rec, m2, m11)

    def stats_eval(self, costs, noise=None) -> dict:
        """The same kernels on host arrays (mppi_stats_eval): costs [B, K] (or [K]; non-finite entries allowed), noise
        None or [B, nu, H, K]; the dictionary of Engine.stats, without the moments when noise is None.  Uses the
        handle's lambda_ and norm_eps; no dynamics or cost need be loaded."""
        c = self.config
        costs = _f32(costs).reshape(-1, c.K)
        B = costs.shape[0]
        nz = None if noise is None else _f32(noise).reshape(B, c.nu, c.H, c.K)
        rec = np.zeros(B, np.dtype(L.STATS_DTYPE))
        m2 = None if nz is None else np.zeros((B, c.nu), np.float32)
        m11 = None if nz is None else np.zeros((B, c.nu), np.float32)
        L.check(self.lib.mppi_stats_eval(self._h, B, _ptr(costs), _ptr(nz), _ptr(rec), _ptr(m2), _ptr(m11)))
        return self._stats_dict(rec, m2, m11)

    # -- weighted cross moments (MPPI_FLAG_CROSS; mppi_hip.stats.cross_moments_ref states the definition)
    def cross_moments(self, B: int = 1, step: int = 0) -> np.ndarray:
        """eps_mx [B, nu, nu] of the last solve made with cross=True (mppi_get_cross_moments; waits for the stream):
        1/H sum_t sum_k w_k eps_u eps_v, symmetric, its diagonal eps_m2 bit for bit.  step as for Engine.stats."""
        nu = self.config.nu
        mx = np.zeros((B, nu, nu), np.float32)
        L.check(self.lib.mppi_get_cross_moments(self._h, B, step, _ptr(mx)))
        return mx

    def cross_moments_eval(self, costs, noise) -> np.ndarray:
        """The same kernels on host arrays (mppi_cross_moments_eval): costs [B, K] (or [K]), noise [B, nu, H, K] ->
        eps_mx [B, nu, nu].  Uses the handle's lambda_ and norm_eps; no dynamics or cost need be loaded; touches no
        solve state."""
        c = self.config
        costs = _f32(costs).reshape(-1, c.K)
        B = costs.shape[0]
        nz = _f32(noise).reshape(B, c.nu, c.H, c.K)
        mx = np.zeros((B, c.nu, c.nu), np.float32)
        L.check(self.lib.mppi_cross_moments_eval(self._h, B, _ptr(costs), _ptr(nz), _ptr(mx)))
        return mx

    # -- weighted per-step moments (MPPI_FLAG_STEP_MOMENTS; mppi_hip.stats.step_moments_ref states the definition)
    def step_moments(self, B: int = 1, step: int = 0) -> tuple[np.ndarray, np.ndarray]:
        """(m1, m2), each [B, nu, H] float32, of the last solve made with step_moments=True or with
        set_noise_steps_adapt on (mppi_get_step_moments; waits for the stream): sum_k w_k eps and sum_k w_k eps^2 per
        actuator and horizon step.  step as for Engine.stats."""
        c = self.config
        m1 = np.zeros((B, c.nu, c.H), np.float32)
        m2 = np.zeros((B, c.nu, c.H), np.float32)
        L.check(self.lib.mppi_get_step_moments(self._h, B, step, _ptr(m1), _ptr(m2)))
        return m1, m2

    def step_moments_eval(self, costs, noise) -> tuple[np.ndarray, np.ndarray]:
        """The same kernels on host arrays (mppi_step_moments_eval): costs [B, K] (or [K]), noise [B, nu, H, K] ->
        (m1, m2) [B, nu, H].  Uses the handle's lambda_ and norm_eps; no dynamics or cost need be loaded; touches no
        solve state and never refits."""
        c = self.config
        costs = _f32(costs).reshape(-1, c.K)
        B = costs.shape[0]
        nz = _f32(noise).reshape(B, c.nu, c.H, c.K)
        m1 = np.zeros((B, c.nu, c.H), np.float32)
        m2 = np.zeros((B, c.nu, c.H), np.float32)
        L.check(self.lib.mppi_step_moments_eval(self._h, B, _ptr(costs), _ptr(nz), _ptr(m1), _ptr(m2)))
        return m1, m2

    def device_stats(self) -> dict:
        """Device pointers of the statistics' buffers (mppi_device_stats), slot-major with max_batch as the batch
        pitch, for consumers on the stream."""
        a, b, c = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        L.check(self.lib.mppi_device_stats(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return dict(stats=a.value, eps_m2=b.value, eps_m11=c.value)

    def x3_layer1(self) -> tuple[int, float]:
        """(products, probe_rel_err) of the split CA's layer 1 (mppi_x3_layer1): 2 or 3 once the first solve's probe
        ran (0 otherwise or not a split CA), and the probe's max relative cost difference between the two forms (-1: no
        probe ran)."""
        n, e = ctypes.c_int(), ctypes.c_float()
        L.check(self.lib.mppi_x3_layer1(self._h, ctypes.byref(n), ctypes.byref(e)))
        return n.value, float(e.value)

    def x3_f16(self) -> tuple[int, float]:
        """(form, probe_rel_err) of the split CA's fp16 form (mppi_x3_f16): 2 = on with the one-product last layer, 1 =
        on with the two-product one, 0 = off for this handle's horizon (also before the first solve and after
        set_cost, which resets the probe); and the probe's max relative cost difference between the fp16 form and three
        products, the larger of its runs on fc_wave32_x3p_kernel and fc_rollout_kernel_x3h, each where it can hold the
        shape (-1: no probe ran)."""
        n, e = ctypes.c_int(), ctypes.c_float()
        L.check(self.lib.mppi_x3_f16(self._h, ctypes.byref(n), ctypes.byref(e)))
        return int(n.value), float(e.value)

    def rollout_kernel(self) -> str:
        """The kernel the last solve's rollout was routed to (mppi_rollout_kernel)."""
        return (self.lib.mppi_rollout_kernel(self._h) or b"").decode()

    def gen_route(self) -> str:
        """Where the last chained solve generated the next solve's noise (mppi_gen_route): "overlap" (a second stream,
        beside the rollout), "fused" (inside the reduce) or "" before the first chained solve."""
        return (self.lib.mppi_gen_route(self._h) or b"").decode()

    def reduce_regen(self) -> int:
        """The eighths of its noise the last solve's reduce regenerated from the noise's key instead of reading them
        (mppi_reduce_regen); 0 when it read everything.  MPPI_REDUCE_REGEN=0 turns it off, 1..7 force a share."""
        return int(self.lib.mppi_reduce_regen(self._h))

    def noise_beside_eval(self, B: int, seed: int) -> np.ndarray:
        """The noise [B, nu, H, K] (float32) the overlap route's generator draws for the by-value key `seed`
        (mppi_noise_beside_eval): the default law's, bitwise noise_eval's with no noise model set."""
        c = self.config
        out = np.empty((int(B), c.nu, c.H, c.K), np.float32)
        L.check(self.lib.mppi_noise_beside_eval(self._h, int(B), ctypes.c_uint64(int(seed) & (2**64 - 1)), _ptr(out)))
        return out

    def set_stream(self, stream_handle: int | None):
        L.check(self.lib.mppi_set_stream(self._h, stream_handle))

    def sync(self):
        L.check(self.lib.mppi_sync(self._h))

    def get_U(self, B: int = 1) -> np.ndarray:
        out = np.empty((B, self.config.nu, self.config.H), np.float32)
        L.check(self.lib.mppi_get_U(self._h, B, _ptr(out)))
        return out

    def set_U(self, U, B: int | None = None):
        U = _f32(U).reshape(-1, self.config.nu, self.config.H)
        L.check(self.lib.mppi_set_U(self._h, U.shape[0] if B is None else B, _ptr(U)))

    def profile(self, enable: bool = True):
        L.check(self.lib.mppi_profile(self._h, int(enable)))

    def kernel_time(self, name: str) -> tuple[int, float]:
        n, ms = ctypes.c_int(), ctypes.c_double()
        L.check(self.lib.mppi_kernel_time(self._h, name.encode(), ctypes.byref(n), ctypes.byref(ms)))
        return n.value, ms.value

    def kernel_clock(self, enable: bool = True):
        """Reset and (re)start the rollout launch clock (mppi_kernel_clock): device wall-clock stamps of every
        rollout launch enqueued or captured from now on, read with kernel_clock_read()."""
        L.check(self.lib.mppi_kernel_clock(self._h, int(enable)))

    def kernel_clock_read(self) -> tuple[int, float, float]:
        """(launches, total_us, max_us) of the stamped rollout launches since the last reset."""
        n, tot, mx = ctypes.c_int(), ctypes.c_double(), ctypes.c_double()
        L.check(self.lib.mppi_kernel_clock_read(self._h, ctypes.byref(n), ctypes.byref(tot), ctypes.byref(mx)))
        return n.value, tot.value, mx.value

    def device_buffers(self) -> dict:
        dU, du0, dc = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        L.check(self.lib.mppi_device_buffers(self._h, ctypes.byref(dU), ctypes.byref(du0), ctypes.byref(dc)))
        return dict(U=dU.value, u0=du0.value, costs=dc.value)
