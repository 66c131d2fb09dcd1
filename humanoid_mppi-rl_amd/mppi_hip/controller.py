"""Drop-in mirror of the reference controller API, backed by the HIP engine.

The reference scripts keep their state in module globals (U_global, K, T, lambda, sigma) next to a MuJoCo
model; the functions below keep the same names, argument meaning and update semantics, with the globals
gathered into an MPPIModel:

  rollout(model, data, U, noise) -> costs[K]     src/cartpole_mppi.py:59-85, src/Humanoid_mppi_v3.jl:128-152
  mppi_step(model, data)                          src/cartpole_mppi.py:88-98, src/Humanoid_mppi_v3.jl:154-171
  mppi_controller(model, data)                    src/cartpole_mppi.py:101-106, src/Humanoid_mppi_v3.jl:173-179
  mppi_update(model, data)                        src/mppi.jl:83-99 / src/quadruped_datacollection.py:166-187
  rollout_learned_model_batched(model, state, U, noise, device=None) -> costs
                                                  src/cartpole_mppi_estimator.py:61-121

`data` is anything with numpy attributes qpos, qvel, ctrl (a mujoco.MjData, or SimData below).  For the humanoid
costs the reference reads the REAL environment's kinematics (data.xpos, data.cvel) on every call
(src/Humanoid_mppi_v3.jl:53-99, src/Humanoid_mppi.jl:89-106); when `data` carries them, mppi_step /
mppi_controller build the per-solve context row from them on every call, as the reference does.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from . import _lib as L
from .engine import ENSEMBLE_MODES, Config, Engine
from .nets import cross_attention_blob, feature_attention_blob, mlp_blob
from .noise import ar1_filter, basis_filter, colored_basis, knot_filter, steps_filter
from .stats import adapt_noise_model

# default cost of each preset (the reference script it mirrors)
PRESET_COST = {"cartpole_py": "cartpole", "cartpole_jl": "cartpole", "cartpole_collect": "cartpole",
               "quad_mppi_jl": "quad_jl", "humanoid_v3": "humanoid_v3", "humanoid_v1": "humanoid_v1",
               "humanoid_collect_v2": "humanoid_v3", "cartpole_est": "cartpole_est", "quad_est": "quad_est"}


@dataclass
class SimData:
    """Minimal stand-in for mujoco.MjData: the fields the controllers read and write."""
    qpos: np.ndarray
    qvel: np.ndarray
    ctrl: np.ndarray
    xpos: np.ndarray | None = None
    cvel: np.ndarray | None = None


class MPPIModel:
    """The reference script's module-level state for one controller, plus the engine handle.

    dynamics: "cartpole" (analytic mj_step restatement), ("cross_attention", state_dict[, dims dict]),
              ("feature_attention", state_dict[, dims dict]) or ("mlp", state_dict[, dims dict]); or an ensemble of one
              kind, ("mlp_ensemble", [state_dict, ...][, dims dict]) and so on (ensemble_mode below).
    noise:    "device" -> Philox on the GPU (seeded, advances per call);
              "numpy"  -> np.random.randn(nu,T,K)*sigma from numpy's global RNG, exactly the reference's draw
                          (src/cartpole_mppi.py:89), injected into the engine.
    noise_sigma, noise_rho: the sampling law (Engine.set_noise_model): per-actuator standard deviations [nu] (None =
              the preset's sigma) and AR(1) correlation along the horizon; both noise modes sample the same law.
    noise_knots: None (default), n_knots or (n_knots, order): knot-parameterised noise (Engine.set_noise_knots) -- the
              law above drawn at n_knots knots along the horizon and interpolated, order 0 (hold), 1 (linear, the
              default) or 3 (Catmull-Rom); both noise modes sample the same law.  Not together with adapt_noise or
              control_cost.
    noise_basis: None (default), an [H, R] array or ("colored", beta[, n_basis]): horizon-basis noise
              (Engine.set_noise_basis) -- the table applied along the horizon to R white normals per sample, scaled by
              noise_sigma; ("colored", beta) is noise.colored_basis(H, beta), iCEM's power-law noise.  Both noise modes
              sample the same law.  Not together with noise_knots, noise_rho != 0, adapt_noise or control_cost.
    noise_steps: None (default) or a table of sampling scales [nu, H] (Engine.set_noise_steps): one standard deviation
              per actuator AND horizon step, CEM's distribution, over the AR(1) row of noise_rho; noise_sigma is then
              the scale a step entering the horizon starts with.  Both noise modes sample the same law (the numpy mode
              reads the engine's live table).  Not together with noise_knots, noise_basis, adapt_noise or control_cost.
    adapt_steps: above 0 (needs noise_steps), the engine refits the table behind every solve from the solve's own
              per-step moments, about the weighted mean, and shifts it with the nominal (Engine.set_noise_steps_adapt
              with this rate and adapt_limits[:2] = (sigma_min, sigma_max)): with n_elite, CEM's variance update.
    adapt_noise: above 0, mppi_step / mppi_controller request the solve's statistics (Engine.solve(stats=True)) and
              after each step move the law towards the weighted moments of the noise that won
              (stats.adapt_noise_model with this rate and adapt_limits = (sigma_min, sigma_max, rho_max)), through
              Engine.set_noise_model.  The moments are about the nominal U.
    adapt_on: "host" (default): the loop above -- statistics read back, the next law computed in numpy and set through
              Engine.set_noise_model per step (which destroys captured graphs).  "device": Engine.set_noise_adapt, the
              same rule in fp32 in a kernel behind each solve's statistics; no statistics are requested and no law is
              set per step, chained solves and graph streams on the engine adapt step by step and stay captured, and
              noise_sigma / noise_rho read the engine's live law.
    ess_target: above 0, the engine chooses the softmin temperature per solve so that the solve's own costs give the
              effective sample size max(1, ess_target * n_finite), within lambda_limits = (lambda_min, lambda_max)
              (Engine.set_ess_target); 0 (default) keeps the preset's lambda.
    control_cost: above 0, the engine adds the control-cost term of information-theoretic MPPI, gamma = control_cost
              (cost units, absolute; Williams' choice is lambda * (1 - alpha)), to the costs the softmin weighs
              (Engine.set_control_cost); 0 (default) weighs the rollout's costs alone.
    u_min, u_max: per-actuator control bounds, scalars or [nu] (a MuJoCo model's actuator_ctrlrange columns); the
              engine keeps every sampled control and the nominal inside the box (Engine.set_control_bounds).  None
              (default) leaves that side unbounded; both None: no bounds.
    rate_cost, rate_anchor: per-actuator weights, a scalar or [nu] (finite, >= 0, not all zero), of a penalty on the
              rate of the sampled controls, sum_u r[u] sum_t (v[u, t] - v[u, t-1])^2, added to the costs the softmin
              weighs (Engine.set_rate_cost).  With rate_anchor (default) the first control is differenced against the
              control the environment applied last: mppi_step / mppi_controller pass data.ctrl to the engine before
              each solve.  None (default): no term.
    n_elite:  weigh only the n_elite best samples of each solve (Engine.set_elites), an int in 1..K: with a large
              lambda_ CEM's elite mean, with ess_target a scale-free softmin over the elites.  0 (default): every
              sample is weighed.
    n_keep:   carry the n_keep best sampled control sequences of each solve into the next one (Engine.set_elite_keep;
              iCEM's keep / shift elites), an int in 1..K: mppi_controller's shifting solves carry them time-shifted,
              mppi_step's as they are.  0 (default): every solve starts from fresh noise alone.
    n_iter, return_best, add_mean: refine the distribution n_iter (1..16) times per control step on the device
              (Engine.set_iterations; CEM / iCEM proper); return_best executes the first control of the best sample of
              the step instead of the mean's, add_mean enters the nominal as a candidate in the last iteration.  Needs
              device noise when n_iter > 1 and excludes u0_before when n_iter > 1 or return_best.  (1, False, False)
              (default): one solve per step.
    ensemble_mode, ensemble_kappa: with dynamics = ("mlp_ensemble", [sd0, sd1, ...][, dims]) -- likewise
              "cross_attention_ensemble", "feature_attention_ensemble", and "cartpole_ensemble" with parameter sets of 10
              floats -- every sample is rolled under each of the 2..8 members and the members' costs are combined per
              sample on the device (Engine.load_member, Engine.set_ensemble; the PE of PETS): "mean" (default),
              "mean_std" (mean + ensemble_kappa * population std; a negative kappa is an optimism bonus) or "worst".
    """

    def __init__(self, preset: str = "cartpole_py", dynamics="cartpole", cost: str | None = None, device: int = 0,
                 noise: str = "device", seed: int = 0, precision: int = L.PREC_BF16, ctx=None,
                 body_ids: dict | None = None, u0_before: bool = False, noise_sigma=None, noise_rho: float = 0.0,
                 adapt_noise: float = 0.0, adapt_limits=(1e-3, 10.0, 0.95), adapt_on: str = "host", ess_target: float = 0.0,
                 lambda_limits=(1e-3, 1e3), control_cost: float = 0.0, u_min=None, u_max=None, rate_cost=None,
                 rate_anchor: bool = True, n_elite: int = 0, n_keep: int = 0, noise_knots=None, noise_basis=None,
                 noise_steps=None, adapt_steps: float = 0.0, n_iter: int = 1, return_best: bool = False,
                 add_mean: bool = False, ensemble_mode: str = "mean", ensemble_kappa: float = 0.0, **overrides):
        """body_ids: 0-based MuJoCo body ids of HUMANOID_BODIES (default: src/humanoid.xml's, HUMANOID_BODY_IDS)
        for the per-call humanoid context; u0_before: apply U[:,0] before the update
        (src/quadruped_datacollection.py:170, MPPI_FLAG_U0_BEFORE)."""
        self.ess_target = float(ess_target)
        if not 0.0 <= self.ess_target <= 1.0:  # (NaN included)
            raise ValueError("MPPIModel: ess_target must be in [0, 1]")
        try:
            self.lambda_limits = tuple(float(v) for v in lambda_limits)
        except TypeError:
            raise ValueError("MPPIModel: lambda_limits must be (lambda_min, lambda_max)") from None
        if len(self.lambda_limits) != 2 or not (0.0 < self.lambda_limits[0] <= self.lambda_limits[1] < np.inf):
            raise ValueError("MPPIModel: lambda_limits needs 0 < lambda_min <= lambda_max < inf")
        self.control_cost = float(control_cost)
        if not 0.0 <= self.control_cost < np.inf:  # (NaN included)
            raise ValueError("MPPIModel: control_cost must be finite and >= 0")
        self.u_min, self.u_max = self._check_bounds(u_min, u_max)
        self.rate_cost = self._check_rate(rate_cost)
        self.rate_anchor = bool(rate_anchor)
        if isinstance(n_elite, bool) or not isinstance(n_elite, (int, np.integer)) or n_elite < 0:
            raise ValueError("MPPIModel: n_elite must be an int in 1..K (0: off)")
        self.n_elite = int(n_elite)
        if isinstance(n_keep, bool) or not isinstance(n_keep, (int, np.integer)) or n_keep < 0:
            raise ValueError("MPPIModel: n_keep must be an int in 1..K (0: off)")
        self.n_keep = int(n_keep)
        if isinstance(n_iter, bool) or not isinstance(n_iter, (int, np.integer)) or not 1 <= n_iter <= 16:
            raise ValueError("MPPIModel: n_iter must be an int in 1..16")
        if not isinstance(return_best, (bool, np.bool_)) or not isinstance(add_mean, (bool, np.bool_)):
            raise ValueError("MPPIModel: return_best and add_mean must be bools")
        if n_iter > 1 and noise != "device":
            raise ValueError("MPPIModel: n_iter > 1 needs noise = 'device' (one injected array cannot serve n iterations)")
        if u0_before and (n_iter > 1 or return_best):
            raise ValueError("MPPIModel: u0_before excludes n_iter > 1 and return_best")
        self.n_iter, self.return_best, self.add_mean = int(n_iter), bool(return_best), bool(add_mean)
        if ensemble_mode not in ENSEMBLE_MODES:
            raise ValueError(f"MPPIModel: ensemble_mode must be one of {sorted(ENSEMBLE_MODES)}")
        self.ensemble_mode, self.ensemble_kappa = ensemble_mode, float(ensemble_kappa)
        if not np.isfinite(self.ensemble_kappa):
            raise ValueError("MPPIModel: ensemble_kappa must be finite")
        self.preset = preset
        self.body_ids = dict(HUMANOID_BODY_IDS if body_ids is None else body_ids)
        self.u0_before = bool(u0_before)
        self.config = Config.preset(preset, precision=precision, **overrides)
        if self.n_elite > self.config.K:
            raise ValueError(f"MPPIModel: n_elite must be an int in 1..K = {self.config.K} (0: off)")
        if self.n_keep > self.config.K:
            raise ValueError(f"MPPIModel: n_keep must be an int in 1..K = {self.config.K} (0: off)")
        if self.rate_cost is not None and self.rate_cost.size not in (1, self.config.nu):
            raise ValueError(f"MPPIModel: rate_cost must be a scalar or have nu = {self.config.nu} entries")
        self.engine = Engine(self.config, device)
        if isinstance(dynamics, str) and dynamics == "cartpole":
            self.engine.load_dynamics(L.DYN_CARTPOLE)
        else:
            kind, sd = dynamics[0], dynamics[1]
            dims = dynamics[2] if len(dynamics) > 2 else {}

            def blob_of(kind, sd):
                if kind == "cross_attention":
                    return cross_attention_blob(sd, **dims)
                if kind == "mlp":
                    return mlp_blob(sd, state_dim=self.config.nx, action_dim=self.config.nu, **dims)
                if kind == "feature_attention":
                    d = {"hidden_dim": np.asarray(sd["feature_encoding.0.weight"]).shape[0], **dims}
                    return feature_attention_blob(sd, state_dim=self.config.nx, action_dim=self.config.nu, **d)
                if kind == "cartpole":  # a parameter set: the 10 floats of mppi_load_dynamics, or None for the defaults
                    return L.DYN_CARTPOLE, None if sd is None else np.asarray(sd, np.float32).reshape(10).tobytes()
                raise ValueError(f"unknown dynamics {kind!r}")

            if isinstance(kind, str) and kind.endswith("_ensemble"):
                members = list(sd)
                if not 2 <= len(members) <= 8:
                    raise ValueError("MPPIModel: an ensemble takes 2..8 members")
                for e, m in enumerate(members):
                    k, blob = blob_of(kind[:-len("_ensemble")], m)
                    if e == 0:
                        self.engine.load_dynamics(k, blob)
                    else:
                        self.engine.load_member(e, k, blob)
                self.engine.set_ensemble(len(members), self.ensemble_mode, self.ensemble_kappa)
            else:
                self.engine.load_dynamics(*blob_of(kind, sd))
        self.cost = cost or PRESET_COST[preset]
        self.engine.set_cost(self.cost, ctx)
        # the humanoid goal (ctx[0:3]) the per-call real-env context keeps: the caller's, when one was given
        self.target = tuple(float(v) for v in np.asarray(ctx, np.float64).ravel()[:3]) if ctx is not None \
            else HUMANOID_TARGET
        self.U_global = np.zeros((self.config.nu, self.config.H))
        self.adapt_on = adapt_on
        if adapt_on not in ("host", "device"):
            raise ValueError('MPPIModel: adapt_on must be "host" or "device"')
        self.adapt_noise = float(adapt_noise)
        self.adapt_limits = tuple(float(v) for v in adapt_limits)
        if not 0.0 <= self.adapt_noise <= 1.0:
            raise ValueError("MPPIModel: adapt_noise must be in [0, 1]")
        self.noise_sigma = None if noise_sigma is None else np.asarray(noise_sigma, np.float64).ravel()
        self.noise_rho = float(noise_rho)
        if self._noise_sigma is not None or self._noise_rho != 0.0:
            self.engine.set_noise_model(self._noise_sigma, self._noise_rho)
        if noise_knots is not None:
            n_knots, order = (noise_knots, 1) if np.isscalar(noise_knots) else noise_knots
            if self.adapt_noise > 0.0 or self.control_cost > 0.0:
                raise ValueError("MPPIModel: noise_knots does not go together with adapt_noise or control_cost")
            self.engine.set_noise_knots(int(n_knots), int(order))
        self._noise_basis = None
        if noise_basis is not None:
            if noise_knots is not None or self._noise_rho != 0.0 or self.adapt_noise > 0.0 or self.control_cost > 0.0:
                raise ValueError("MPPIModel: noise_basis does not go together with noise_knots, noise_rho != 0, "
                                 "adapt_noise or control_cost")
            self.noise_basis = noise_basis
        self.adapt_steps = float(adapt_steps)
        if not 0.0 <= self.adapt_steps <= 1.0:
            raise ValueError("MPPIModel: adapt_steps must be in [0, 1]")
        self._steps_on = noise_steps is not None
        if noise_steps is not None:
            if noise_knots is not None or noise_basis is not None or self.adapt_noise > 0.0 or self.control_cost > 0.0:
                raise ValueError("MPPIModel: noise_steps does not go together with noise_knots, noise_basis, "
                                 "adapt_noise or control_cost")
            self.engine.set_noise_steps(np.asarray(noise_steps, np.float32).reshape(self.config.nu, self.config.H))
            if self.adapt_steps > 0.0:
                self.engine.set_noise_steps_adapt(self.adapt_steps, self.adapt_limits[0], self.adapt_limits[1])
        elif self.adapt_steps > 0.0:
            raise ValueError("MPPIModel: adapt_steps needs noise_steps")
        if self.device_adapt:
            self.engine.set_noise_adapt(self.adapt_noise, *self.adapt_limits)
        if self.ess_target > 0.0:
            self.engine.set_ess_target(self.ess_target, *self.lambda_limits)
        if self.control_cost > 0.0:
            self.engine.set_control_cost(self.control_cost)
        if self.u_min is not None or self.u_max is not None:
            for name, v in (("u_min", self.u_min), ("u_max", self.u_max)):
                if v is not None and v.size not in (1, self.config.nu):
                    raise ValueError(f"MPPIModel: {name} must be a scalar or have nu = {self.config.nu} entries")
            self.engine.set_control_bounds(None if self.u_min is None else np.broadcast_to(self.u_min, self.config.nu),
                                           None if self.u_max is None else np.broadcast_to(self.u_max, self.config.nu))
        if self.rate_cost is not None:
            self.engine.set_rate_cost(np.broadcast_to(self.rate_cost, self.config.nu), self.rate_anchor)
        if self.n_elite > 0:
            self.engine.set_elites(self.n_elite)
        if self.n_keep > 0:
            self.engine.set_elite_keep(self.n_keep)
        if self.n_iter > 1 or self.return_best or self.add_mean:
            self.engine.set_iterations(self.n_iter, self.return_best, self.add_mean)
        self.noise = noise
        self.seed = int(seed)
        self.calls = 0
        self.last = None  # SolveResult of the last mppi_step (costs, weights) for inspection

    @staticmethod
    def _check_bounds(u_min, u_max):
        """u_min / u_max as float32 vectors (or None): no NaN, u_min <= u_max where both are given."""
        out = []
        for name, v in (("u_min", u_min), ("u_max", u_max)):
            if v is None:
                out.append(None)
                continue
            try:
                a = np.asarray(v, dtype=np.float32).ravel()
            except (TypeError, ValueError):
                raise ValueError(f"MPPIModel: {name} must be a scalar or a sequence of numbers") from None
            if a.size == 0 or np.isnan(a).any():
                raise ValueError(f"MPPIModel: {name} must be non-empty and hold no NaN")
            out.append(a)
        lo, hi = out
        if lo is not None and hi is not None:
            if lo.size != hi.size and 1 not in (lo.size, hi.size):
                raise ValueError("MPPIModel: u_min and u_max must have matching sizes")
            if (lo > hi).any():
                raise ValueError("MPPIModel: u_min must be <= u_max for every actuator")
        return lo, hi

    @staticmethod
    def _check_rate(rate_cost):
        """rate_cost as a float32 vector (or None): finite, every entry >= 0, not all zero."""
        if rate_cost is None:
            return None
        try:
            a = np.asarray(rate_cost, dtype=np.float32).ravel()
        except (TypeError, ValueError):
            raise ValueError("MPPIModel: rate_cost must be a scalar or a sequence of numbers") from None
        if a.size == 0 or not np.isfinite(a).all() or (a < 0.0).any() or not (a > 0.0).any():
            raise ValueError("MPPIModel: rate_cost must be finite, every entry >= 0 and at least one > 0")
        return a

    @property
    def device_adapt(self) -> bool:
        """The engine adapts the law itself (adapt_on="device" with adapt_noise > 0)."""
        return getattr(self, "adapt_on", "host") == "device" and getattr(self, "adapt_noise", 0.0) > 0.0

    # the sampling law: the host's copy, or (device adaptation) the engine's live law
    @property
    def noise_sigma(self):
        if self.device_adapt:
            return self.engine.noise_model()[0].astype(np.float64)
        return self._noise_sigma

    @noise_sigma.setter
    def noise_sigma(self, v):
        self._noise_sigma = v

    @property
    def noise_rho(self):
        if self.device_adapt:
            return float(self.engine.noise_model()[1])
        return self._noise_rho

    @noise_rho.setter
    def noise_rho(self, v):
        self._noise_rho = v

    @property
    def noise_knots(self):
        """(n_knots, order) of the engine's knot law (Engine.noise_knots), or None while it is off."""
        n, order = self.engine.noise_knots()[:2]
        return (n, order) if n > 0 else None

    @noise_knots.setter
    def noise_knots(self, v):
        n_knots, order = (0, 0) if v is None else ((v, 1) if np.isscalar(v) else v)
        self.engine.set_noise_knots(int(n_knots), int(order))

    @property
    def noise_basis(self):
        """M [H, R] (float32) of the engine's basis law as it was set here, or None while it is off."""
        return getattr(self, "_noise_basis", None)

    @noise_basis.setter
    def noise_basis(self, v):
        if v is None:
            self.engine.set_noise_basis(None)
            self._noise_basis = None
            return
        if isinstance(v, tuple) and len(v) in (2, 3) and isinstance(v[0], str) and v[0] == "colored":
            v = colored_basis(self.config.H, *v[1:])
        M = np.ascontiguousarray(np.asarray(v, np.float32))
        if M.ndim != 2 or M.shape[0] != self.config.H or not 1 <= M.shape[1] <= self.config.H:
            raise ValueError(f"MPPIModel: noise_basis must be [H = {self.config.H}, R] with 1 <= R <= H")
        self.engine.set_noise_basis(M)
        self._noise_basis = M

    @property
    def noise_steps(self):
        """The engine's live table of per-step scales [nu, H] (Engine.noise_steps), or None while it is off."""
        if not getattr(self, "_steps_on", False):
            return None
        S = self.engine.noise_steps(1)
        return None if S is None else S[0]

    @property
    def K(self):
        return self.config.K

    @property
    def T(self):
        return self.config.H

    def draw_noise(self):
        c = self.config
        if self.noise == "numpy":
            z = np.random.randn(c.nu, c.H, c.K)
            if self.noise_steps is not None:
                return steps_filter(z, self.noise_steps, self.noise_rho)
            if self.noise_basis is not None:
                return basis_filter(z, self.noise_basis,
                                    c.sigma if self.noise_sigma is None else self.noise_sigma).astype(np.float64)
            if self.noise_knots is not None:
                return knot_filter(z, *self.noise_knots, rho=self.noise_rho,
                                   sigma_u=c.sigma if self.noise_sigma is None else self.noise_sigma).astype(np.float64)
            if self.noise_sigma is None and self.noise_rho == 0.0:
                return z * c.sigma
            return ar1_filter(z, self.noise_rho, c.sigma if self.noise_sigma is None else self.noise_sigma)
        return None

    def adapt(self, stats: dict):
        """Move the sampling law towards the moments of one solve's statistics (adapt_noise > 0)."""
        c = self.config
        sig = np.full(c.nu, c.sigma) if self.noise_sigma is None else self.noise_sigma
        lo, hi, rho_max = self.adapt_limits
        self.noise_sigma, self.noise_rho = adapt_noise_model(sig, self.noise_rho, stats["eps_m2"], stats["eps_m11"],
                                                             self.adapt_noise, lo, hi, rho_max)
        self.engine.set_noise_model(self.noise_sigma, self.noise_rho)

    def next_seed(self) -> int:
        # (iteration i of a step draws key seed + i: consecutive steps never share a key)
        self.calls += getattr(self, "n_iter", 1)
        return (self.seed << 32) ^ self.calls

    def close(self):
        self.engine.close()


HUMANOID_TARGET = (2.0, 0.0, 1.28)  # const Position, src/Humanoid_mppi_v3.jl:12
HUMANOID_BODIES = ("shin_left", "shin_right", "foot_left", "foot_right")
# MuJoCo body ids of src/humanoid.xml (world = 0, then the <body> elements depth-first: torso 1, head 2,
# waist_lower 3, pelvis 4, thigh_right 5, shin_right 6, foot_right 7, thigh_left 8, shin_left 9, foot_left 10, ...;
# 18 bodies).  tests/test_host.py checks them against the XML when the reference tree is present.
HUMANOID_BODY_IDS = {"shin_left": 9, "shin_right": 6, "foot_left": 10, "foot_right": 7}


def humanoid_body_ids(mjmodel) -> dict:
    """0-based MuJoCo body ids (what MuJoCo.body(model, name).id returns), via the mujoco Python bindings."""
    import mujoco
    return {n: mujoco.mj_name2id(mjmodel, mujoco.mjtObj.mjOBJ_BODY, n) for n in HUMANOID_BODIES}


def humanoid_context(data, body_ids: dict, target=HUMANOID_TARGET) -> np.ndarray:
    """Per-solve context row (MPPI_CTX_MAX floats) for MPPI_COST_HUMANOID_V3 from the REAL environment's data.

    src/Humanoid_mppi_v3.jl:53-99 reads the global `data` (not the rollout copy), so these terms are constant
    over all k and t of one solve: [tx, ty, tz, swing_foot_x, swing_knee_x, const, 0, 0] with
    const = -0.15*swing_vx + 2*clr^2 [clr < 0.05] + 0.5*lat^2 [lat < 0].
    get_body_vx (:20-23) indexes the flat cvel buffer at 6*id-5+3 (1-based) with a 0-based id, i.e. it reads
    the linear-x velocity of body id-1; that behaviour is kept here.
    """
    cvel = np.asarray(data.cvel, np.float64).ravel()
    xpos = np.asarray(data.xpos, np.float64).reshape(-1, 3)

    def vx(bid):
        return cvel[6 * bid - 5 + 3 - 1]

    il, ir = body_ids["shin_left"], body_ids["shin_right"]
    if vx(il) > vx(ir):
        swing, stance, knee = body_ids["foot_left"], body_ids["foot_right"], il
    else:
        swing, stance, knee = body_ids["foot_right"], body_ids["foot_left"], ir
    const = -0.15 * vx(swing)
    clearance = xpos[swing, 2] - xpos[stance, 2]
    if clearance < 0.05:
        const += 2.0 * clearance ** 2
    lateral = xpos[body_ids["foot_left"], 1] - xpos[body_ids["foot_right"], 1]
    if lateral < 0:
        const += 0.5 * lateral ** 2
    ctx = np.zeros(L.CTX_MAX)
    ctx[:6] = [target[0], target[1], target[2], xpos[swing, 0], xpos[knee, 0], const]
    return ctx


def humanoid_v1_context(data, body_ids: dict, target=HUMANOID_TARGET) -> np.ndarray:
    """Per-solve context row for MPPI_COST_HUMANOID_V1 (src/Humanoid_mppi.jl:31-121) from the REAL environment's
    data.xpos: [2, 0, 1.28, left_foot_x, right_foot_x, 0.01 (right_z - left_z), 0.1 |left_y - right_y|, 0].
    The kernel picks the swing side per rollout step (t % 100 < 50: left swings, :76-87)."""
    xpos = np.asarray(data.xpos, np.float64).reshape(-1, 3)
    fl, fr = xpos[body_ids["foot_left"]], xpos[body_ids["foot_right"]]
    ctx = np.zeros(L.CTX_MAX)
    ctx[:7] = [target[0], target[1], target[2], fl[0], fr[0], 0.01 * (fr[2] - fl[2]), 0.1 * abs(fl[1] - fr[1])]
    return ctx


def env_context(model: "MPPIModel", data):
    """The per-call cost context the reference reads from the real environment, or None (engine default) when the
    cost has no real-env terms or `data` does not carry the kinematics (xpos / cvel).  The goal position ctx[0:3] is
    the model's (MPPIModel(ctx=...) at construction, else HUMANOID_TARGET), not replaced per call."""
    target = getattr(model, "target", HUMANOID_TARGET)
    if model.cost == "humanoid_v3" and getattr(data, "xpos", None) is not None and \
            getattr(data, "cvel", None) is not None:
        return humanoid_context(data, model.body_ids, target)
    if model.cost == "humanoid_v1" and getattr(data, "xpos", None) is not None:
        return humanoid_v1_context(data, model.body_ids, target)
    return None


def _state(data) -> np.ndarray:
    return np.concatenate([np.asarray(data.qpos, np.float64).ravel(), np.asarray(data.qvel, np.float64).ravel()])


def rollout(model: MPPIModel, data, U, noise) -> np.ndarray:
    """costs[K] of the K perturbed sequences U + noise[:, :, k] from data's state (no U update)."""
    state = _state(data)
    res = model.engine.solve(state, np.asarray(U), noise=np.asarray(noise), want_costs=True)
    return res.costs.astype(np.float64)


def rollout_learned_model_batched(model: MPPIModel, state, U, noise, device=None) -> np.ndarray:
    """Estimator form (src/cartpole_mppi_estimator.py:61): same as rollout() but takes the state vector."""
    if hasattr(noise, "detach"):
        noise = noise.detach().cpu().numpy()
    res = model.engine.solve(np.asarray(state, np.float64), np.asarray(U), noise=np.asarray(noise), want_costs=True)
    return res.costs.astype(np.float64)


def _device_adapt(model) -> bool:
    return bool(getattr(model, "device_adapt", False))


def _stats_kw(model) -> dict:
    """stats=True for the solve of a model that adapts its sampling law; nothing otherwise (the solve call of a model
    that does not adapt is what it always was)."""
    return {"stats": True} if getattr(model, "adapt_noise", 0.0) > 0.0 and not _device_adapt(model) else {}


def _pass_prev_control(model, data):
    """With the anchored rate term on, the control the environment applied last (data.ctrl) becomes the engine's
    previous control ahead of the solve; a model without the term makes no call."""
    if getattr(model, "rate_cost", None) is not None and getattr(model, "rate_anchor", False):
        model.engine.set_prev_control(np.asarray(data.ctrl, np.float32).ravel())


def _adapt(model, res):
    if getattr(model, "adapt_noise", 0.0) > 0.0 and res.status == L.MPPI_OK and not _device_adapt(model):
        model.adapt(res.stats)


def mppi_step(model: MPPIModel, data, ctx=None):
    """noise -> rollout -> softmin -> U_global update (add or replace per preset), in place.  ctx None: built from
    data's real-env kinematics for the humanoid costs (env_context), as the reference reads them per call."""
    ctx = env_context(model, data) if ctx is None else ctx
    noise = model.draw_noise()
    _pass_prev_control(model, data)
    res = model.engine.solve(_state(data), model.U_global, noise=noise, seed=model.next_seed(), ctx=ctx,
                             want_costs=True, want_weights=True, **_stats_kw(model))
    model.U_global = res.U.astype(np.float64)
    model.last = res
    _adapt(model, res)
    return res


def mppi_controller(model: MPPIModel, data, ctx=None):
    """mppi_step, then data.ctrl = U[:,0] and the receding-horizon shift (fill = preset's 0.1 or 0)."""
    ctx = env_context(model, data) if ctx is None else ctx
    noise = model.draw_noise()
    _pass_prev_control(model, data)
    res = model.engine.solve(_state(data), model.U_global, noise=noise, seed=model.next_seed(), ctx=ctx,
                             want_costs=True, want_weights=True, shift=True, u0_before=model.u0_before,
                             **_stats_kw(model))
    model.U_global = res.U.astype(np.float64)
    model.last = res
    _adapt(model, res)
    data.ctrl[:] = res.u0
    return res


mppi_update = mppi_controller  # src/mppi.jl:83-99 names the same step mppi_update!
