"""Per-sample isolation of the feature-attention (FA) rollouts that pack several samples into one MFMA tile or one
attention (tests/fa_isolation_cases.py holds the grid and the inputs).  Needs an MI355X.

Per case, four properties:
  a. the packed form agrees with the reference at all: fp32 against the float64 oracle at rtol 1e-4, bf16 against the
     bf16-rounding oracle at rtol 1e-2 (test_fa_wide_bf16's bar), or, for the cases fa_isolation_cases marks `dist`, in
     test_fa_small_net_layers_bf16's distribution form (median < 1e-4, 95th percentile < 3e-2, max < 5e-2);
  b. finite isolation: another finite noise column for one sample leaves every other cost of both solves bitwise;
  c. non-finite isolation: one NaN or +inf noise element costs exactly that sample (cost +inf, weight 0), every other
     cost bitwise, status 0, the weights the softmin of the clean costs with the victim at +inf;
  d. truncation invariance: the same noise columns at K = 1 and K = G + 1 (sample 0 alone in its workgroup, beside the
     absent slots' pad rows) give bitwise the first costs of the full solve.
Every solve asserts the kernel mppi_rollout_kernel names (fa_small_kernel, fa_rollout_kernel, fa_layered).

What (c) found.  No neighbour ever moved: the feature encoding's ReLU is an fmaxf, which turns a NaN (or the NaN that
+inf becomes in the encoding's LayerNorm) into 0, so a non-finite token enters the net as its bare position embedding
and the shared tiles (0 x NaN in P V would poison them) only ever hold finite values.  But the same laundering hid the
sample from its own cost: where the running cost does not read the dirty actuator (the cartpole cost reads actuator 0
only) the victim came back with a finite cost and a positive weight.  Before the rollouts' cost threads set the cost of
a sample with a non-finite control to +inf, (c) failed on small-L6-4layers, general-D128-4heads and
general-D128-8heads (the three cases with two actuators and the cartpole cost), NaN and +inf alike, at the first
victim: cost 25.1, 37.0 and 8.13 instead of +inf.  The other cases passed untouched.

(a) in distribution form: small-L6-4layers (4 seeded layers: median 1.8e-6, 95th percentile 9.4e-3, max 2.1e-2 over
the 71 samples of solve 1) and general-D128-8heads (median 5.5e-6, max 1.2e-2, 2 of 71 samples past 1e-2), the
profile test_fa_small_net_layers_bf16 documents.  Every other case holds rtol 1e-2 (fp32: 1e-4; measured 6.7e-6).
"""
import numpy as np
import pytest

import fa_isolation_cases as C
from oracle import mppi_ref as R
from oracle import nets_ref as N

pytestmark = pytest.mark.gpu

NAMES = [c.name for c in C.CASES]


@pytest.fixture(scope="module")
def M(gpu_available):
    import mppi_hip
    return mppi_hip


class _Rollout:
    """An engine of one case at K samples (the case's own K by default), closed on exit; solve() takes noise
    [B, nu, H, K] and checks the kernel the rollout was routed to."""

    def __init__(self, M, monkeypatch, case, K=None):
        from mppi_hip.nets import feature_attention_blob
        if case.form == "layered":  # read when the net is loaded (the workspace) and per launch
            monkeypatch.setenv("MPPI_FA_LAYERED", "1")
        else:
            monkeypatch.delenv("MPPI_FA_LAYERED", raising=False)
        self.case, self.K = case, case.K if K is None else K
        self.eng = M.Engine(M.Config(nx=case.nx, nu=case.nu, H=C.H, K=self.K, lambda_=C.LAM, sigma=C.SIGMA,
                                     precision=case.precision, max_batch=C.B, terminal_weight=C.TERMINAL_WEIGHT))
        try:
            self.eng.load_dynamics(*feature_attention_blob(C.weights(case.name), case.nx, case.nu, case.D,
                                                           num_heads=case.heads))
            self.eng.set_cost(case.cost)
        except Exception:
            self.eng.close()
            raise

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.eng.close()

    def solve(self, noise):
        i = C.inputs(self.case.name)
        res = self.eng.solve(i["x0"], i["U0"], noise=np.ascontiguousarray(noise[..., :self.K]), want_weights=True)
        kern = self.eng.rollout_kernel()
        assert kern == self.case.kernel, (self.case.name, kern)
        return res


def _ctx(case):
    return np.array(R.QUAD_GOAL) if case.cost == "quad_est" else None


@pytest.mark.parametrize("name", NAMES)
def test_packed_form_matches_the_oracle(M, monkeypatch, name):
    case, i = C.BY_NAME[name], C.inputs(name)
    with _Rollout(M, monkeypatch, case) as r:
        res = r.solve(i["noise"])
    assert res.status == 0 and np.isfinite(res.costs).all()
    pre = R.Preset("t", K=case.K, H=C.H, lam=C.LAM, sigma=C.SIGMA, terminal_weight=C.TERMINAL_WEIGHT)
    fp32 = case.precision == 0
    dyn = N.fa_dynamics(C.weights(name), case.nx, nheads=case.heads, precision="fp64" if fp32 else "bf16")
    for b in range(C.B):
        ref = R.mppi_solve(pre, dyn, R.COSTS[case.cost], i["x0"][b], i["U0"][b], i["noise"][b], ctx=_ctx(case),
                           dtype=np.float64 if fp32 else np.float32)
        rel = np.abs(res.costs[b] - ref["costs"]) / np.abs(ref["costs"])
        print(f"FA-ISOLATION {name} solve {b} ({r.case.kernel}, G = {case.G}, K = {case.K}): rel err median "
              f"{np.median(rel):.2e} q95 {np.quantile(rel, 0.95):.2e} max {rel.max():.2e}")
        if case.dist:
            assert np.median(rel) < 1e-4 and np.quantile(rel, 0.95) < 3e-2 and rel.max() < 5e-2, (
                np.median(rel), np.quantile(rel, 0.95), rel.max())
        else:
            np.testing.assert_allclose(res.costs[b], ref["costs"], rtol=1e-4 if fp32 else 1e-2)
        w_own = R.softmin_weights(res.costs[b].astype(np.float64), C.LAM)
        np.testing.assert_allclose(res.weights[b], w_own, atol=1e-5)


def _others_bitwise(case, got, clean, k, what):
    """Every cost but sample k of the victim solve has the clean solve's bits."""
    keep = np.ones((C.B, case.K), bool)
    keep[C.VICTIM_SOLVE, k] = False
    diff = np.argwhere((C.bits(got) != C.bits(clean)) & keep)
    assert len(diff) == 0, (f"{case.name} {what}, victim {k} of solve {C.VICTIM_SOLVE} (G = {case.G}): "
                            f"{len(diff)} other costs moved, (solve, sample) {diff[:16].tolist()}: "
                            f"{got[tuple(diff[0])]!r} from {clean[tuple(diff[0])]!r}")


@pytest.mark.parametrize("name", NAMES)
def test_finite_sample_moves_only_itself(M, monkeypatch, name):
    case, b = C.BY_NAME[name], C.VICTIM_SOLVE
    with _Rollout(M, monkeypatch, case) as r:
        clean = r.solve(C.inputs(name)["noise"])
        assert np.isfinite(clean.costs).all()
        for k in case.victims:
            got = r.solve(C.finite_dirty(name, k))
            _others_bitwise(case, got.costs, clean.costs, k, "finite")
            assert np.isfinite(got.costs[b, k]) and got.costs[b, k] != clean.costs[b, k], (name, k)


@pytest.mark.parametrize("bad", [np.nan, np.inf], ids=["nan", "inf"])
@pytest.mark.parametrize("name", NAMES)
def test_nonfinite_sample_costs_exactly_one_sample(M, monkeypatch, name, bad):
    case, b = C.BY_NAME[name], C.VICTIM_SOLVE
    with _Rollout(M, monkeypatch, case) as r:
        clean = r.solve(C.inputs(name)["noise"])
        assert np.isfinite(clean.costs).all() and clean.status == 0
        for k in case.victims:
            got = r.solve(C.nonfinite_dirty(name, k, bad))
            assert got.costs[b, k] == np.inf and got.weights[b, k] == 0.0, (name, k, got.costs[b, k], got.weights[b, k])
            _others_bitwise(case, got.costs, clean.costs, k, "nan" if bad != bad else "inf")
            assert got.status == 0
            for s in range(C.B):
                c = clean.costs[s].astype(np.float64)
                if s == b:
                    c[k] = np.inf
                np.testing.assert_allclose(got.weights[s], R.softmin_weights(c, C.LAM), atol=1e-5)


@pytest.mark.parametrize("name", NAMES)
def test_truncated_solve_keeps_the_first_costs(M, monkeypatch, name):
    case, noise = C.BY_NAME[name], C.inputs(name)["noise"]
    with _Rollout(M, monkeypatch, case) as r:
        full = r.solve(noise)
    for K in (1, case.G + 1):
        with _Rollout(M, monkeypatch, case, K=K) as r:
            got = r.solve(noise)
        assert got.costs.shape == (C.B, K)
        np.testing.assert_array_equal(C.bits(got.costs), C.bits(full.costs[:, :K]), err_msg=f"{name} K = {K}")
