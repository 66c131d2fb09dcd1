"""Solve diagnostics on the device (MPPI_FLAG_STATS, mppi_get_stats, mppi_stats_eval; csrc/kernels_stats.hip) against
their float64 statement mppi_hip.stats.solve_stats_ref, in every solve form, and bit for bit beside the same solves
without the flag."""
import ctypes
import math

import numpy as np
import pytest

from conftest import golden, golden_sd

pytestmark = pytest.mark.gpu

FLOATS = ("cost_min", "cost_max", "cost_mean", "cost_std", "cost_weighted", "ess", "entropy", "free_energy")
INTS = ("n_finite", "k_best")
INF = float("inf")


@pytest.fixture(scope="module")
def M(gpu_available):
    import mppi_hip
    return mppi_hip


def _bare(M, B, nu, H, K, lam=1.0, norm_eps=0.0):
    """An engine with nothing loaded: all mppi_stats_eval needs."""
    return M.Engine(M.Config(nx=4, nu=nu, H=H, K=K, max_batch=B, lambda_=lam, norm_eps=norm_eps))


def _setup(M, kind, K, H, B, **over):
    """(engine, x0 [B,nx] f32, U0 [B,nu,H] f32): the analytic cartpole (the fused-epilogue path), or the CrossAttention
    humanoid net of tests/golden in bf16 (rollout + reduce)."""
    rs = np.random.RandomState(11)
    if kind == "cartpole":
        eng = M.Engine(M.Config.preset("cartpole_py", K=K, H=H, max_batch=B, **over))
        eng.load_dynamics(1).set_cost("cartpole")
        x0 = np.stack([[0.0, 0.2 + 0.3 * b, 0.0, 0.0] for b in range(B)])
        nu = 1
    else:
        eng = M.Engine(M.Config.preset("humanoid_v3", K=K, H=H, max_batch=B, **over))
        eng.load_dynamics(*M.cross_attention_blob(golden_sd("ca_humanoid_weights.npz"))).set_cost("humanoid_v3")
        x0 = golden("g5_ca_humanoid_fwd.npz")["x0_stride20"][:B]
        nu = 21
    U0 = 0.1 * rs.randn(B, nu, H)
    return eng, np.ascontiguousarray(x0, np.float32), U0.astype(np.float32)


def _same_stats(a, b):
    assert a.keys() == b.keys()
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def _check_against_ref(got, ref):
    """The issue's bars: every float rtol 1e-4 (atol 1e-6 on the moments only), the integers exactly."""
    for n in INTS:
        np.testing.assert_array_equal(got[n], ref[n], err_msg=n)
    for n in FLOATS:
        fin = np.isfinite(ref[n]) & (ref[n] != 0.0)
        print(n, "max rel err", float(np.max(np.abs(got[n][fin] / ref[n][fin] - 1.0), initial=0.0)))
        np.testing.assert_allclose(got[n], ref[n], rtol=1e-4, atol=0.0, err_msg=n)
    for n in ("eps_m2", "eps_m11"):
        if n in ref:
            print(n, "max abs err", float(np.max(np.abs(got[n] - ref[n]))))
            np.testing.assert_allclose(got[n], ref[n], rtol=1e-4, atol=1e-6, err_msg=n)


# ------------------------------------------------------------------------------------------ 1. mppi_stats_eval

# (B, nu, H, K).  K = 2500: three 1024-sample blocks of the direct form (ten 256-sample wave-chunks), the last partial.
# H = 150: horizon segments longer than one load tile (L = 10 > 8); H = 100: L = 7, 15 segments.
SHAPES = [(1, 1, 1, 1), (1, 1, 2, 30), (3, 2, 7, 75), (2, 3, 100, 30), (1, 21, 5, 1100), (1, 2, 9, 2500),
          (1, 1, 150, 70)]


def _case(B, nu, H, K):
    rs = np.random.RandomState(1000 * B + 100 * nu + H + K)
    costs = (100.0 + 5.0 * rs.randn(B, K)).astype(np.float32)
    noise = rs.randn(B, nu, H, K).astype(np.float32)
    if K >= 8:  # non-finite entries at k = 0, at K - 1 and in the middle of some rows
        costs[0, 0], costs[0, K // 2] = np.nan, np.inf
        costs[B - 1, K - 1] = -np.inf
        costs[B - 1, K // 3] = np.nan
    return costs, noise


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stats_eval_against_the_reference(M, shape, monkeypatch):
    """Every shape under each forced form of the moment kernel and twice under the default routing: each run holds the
    reference's bars, repeats are bitwise equal, the forms agree to rtol 1e-6."""
    from mppi_hip.stats import solve_stats_ref
    B, nu, H, K = shape
    costs, noise = _case(*shape)
    ref = solve_stats_ref(costs, noise, 1.0, 0.0)
    eng = _bare(M, B, nu, H, K)
    runs = {}
    for knob in ("direct", "seg", None, "again"):
        if knob in ("direct", "seg"):
            monkeypatch.setenv("MPPI_STATS_FORM", knob)
        else:
            monkeypatch.delenv("MPPI_STATS_FORM", raising=False)
        runs[knob] = eng.stats_eval(costs, noise)
        _check_against_ref(runs[knob], ref)
    _same_stats(runs[None], runs["again"])
    for n in FLOATS + ("eps_m2", "eps_m11"):
        np.testing.assert_allclose(runs["direct"][n], runs["seg"][n], rtol=1e-6, atol=0.0, err_msg=n)
    only = eng.stats_eval(costs)  # noise = NULL: the struct alone, the same values
    assert "eps_m2" not in only
    for n in FLOATS + INTS:
        np.testing.assert_array_equal(only[n], runs[None][n], err_msg=n)
    eng.close()


def test_stats_eval_honours_lambda_and_norm_eps(M):
    from mppi_hip.stats import solve_stats_ref
    B, nu, H, K = 2, 2, 6, 200
    costs, noise = _case(B, nu, H, K)
    eng = _bare(M, B, nu, H, K, lam=7.5, norm_eps=0.25)
    _check_against_ref(eng.stats_eval(costs, noise), solve_stats_ref(costs, noise, 7.5, 0.25))
    eng.close()


# ------------------------------------------------------------------------------------------ 2. no finite cost

def test_all_costs_non_finite(M):
    """The defined read-out (include/mppi.h), return code MPPI_OK, and a finite solve beside it untouched."""
    from mppi_hip import _lib as L
    B, nu, H, K = 2, 2, 5, 70
    costs, noise = _case(B, nu, H, K)
    costs[0] = np.resize(np.array([np.nan, np.inf, -np.inf], np.float32), K)
    eng = _bare(M, B, nu, H, K)
    rec = np.zeros(B, np.dtype(L.STATS_DTYPE))
    m2, m11 = np.ones((B, nu), np.float32), np.ones((B, nu), np.float32)
    rc = eng.lib.mppi_stats_eval(eng._h, B, costs.ctypes.data_as(ctypes.c_void_p),
                                 noise.ctypes.data_as(ctypes.c_void_p), rec.ctypes.data_as(ctypes.c_void_p),
                                 m2.ctypes.data_as(ctypes.c_void_p), m11.ctypes.data_as(ctypes.c_void_p))
    assert rc == L.MPPI_OK
    assert rec["n_finite"][0] == 0 and rec["k_best"][0] == -1
    for n in ("ess", "entropy", "cost_std", "cost_weighted"):
        assert rec[n][0] == 0.0, n
    for n in ("cost_min", "cost_max", "cost_mean", "free_energy"):
        assert rec[n][0] == INF, n
    assert np.all(m2[0] == 0.0) and np.all(m11[0] == 0.0)
    assert rec["n_finite"][1] == K - 2 and np.all(m2[1] > 0.0)
    eng.close()


# ------------------------------------------------------------------------------------------ 3. a solve with the flag

@pytest.mark.parametrize("kind", ["cartpole", "ca"])
def test_flagged_solve_equals_eval_and_changes_nothing(M, kind):
    """Injected noise, B = 2: the statistics of the solve are mppi_stats_eval of its returned costs and that noise, and
    U, u0, costs and weights are bitwise those of the same solve without the flag."""
    from mppi_hip.stats import solve_stats_ref
    K, H, B = 150, 9, 2
    eng, x0, U0 = _setup(M, kind, K, H, B)
    nu = eng.config.nu
    noise = (eng.config.sigma * np.random.RandomState(5).randn(B, nu, H, K)).astype(np.float32)
    eng.profile(True)
    r1 = eng.solve(x0, U0, noise=noise, want_weights=True, shift=True, stats=True)
    assert eng.kernel_time("stats")[0] == 1
    eng.profile(False)
    assert r1.stats["eps_m2"].shape == (B, nu) and r1.stats["ess"].shape == (B,)
    _same_stats(r1.stats, eng.stats(B))
    ev = eng.stats_eval(r1.costs, noise)
    _same_stats(r1.stats, ev)
    _same_stats(r1.stats, eng.stats(B))  # the evaluation has its own slot: the solve's statistics stay readable
    _check_against_ref(r1.stats, solve_stats_ref(r1.costs, noise, eng.config.lambda_, eng.config.norm_eps))
    ref, _, _ = _setup(M, kind, K, H, B)
    r0 = ref.solve(x0, U0, noise=noise, want_weights=True, shift=True)
    assert r0.stats is None
    for n in ("U", "u0", "costs", "weights"):
        np.testing.assert_array_equal(getattr(r1, n), getattr(r0, n), err_msg=n)
    eng.close()
    ref.close()


# ------------------------------------------------------------------------------------------ 4. zero noise

@pytest.mark.parametrize("kind", ["cartpole", "ca"])
def test_zero_noise_gives_uniform_weights(M, kind):
    K, H, B = 100, 6, 2
    eng, x0, U0 = _setup(M, kind, K, H, B)
    nu = eng.config.nu
    r = eng.solve(x0, U0, noise=np.zeros((B, nu, H, K), np.float32), stats=True)
    assert np.all(r.costs == r.costs[:, :1])  # every sample rolled out the nominal U
    st = r.stats
    assert np.all(st["ess"] == np.float32(K))
    assert np.all(st["entropy"] == np.float32(math.log(K)))
    assert np.all(st["k_best"] == 0) and np.all(st["n_finite"] == K)
    assert np.all(st["eps_m2"] == 0.0) and np.all(st["eps_m11"] == 0.0)
    assert np.all(st["cost_std"] == 0.0) and np.array_equal(st["cost_min"], st["cost_max"])
    eng.close()


# ------------------------------------------------------------------------------------------ 5. the device law

def test_device_law_is_recovered_from_the_moments(M):
    """Uniform weights (lambda = 1e9) over H * K = 64 * 4096 draws per solve of the device's AR(1) law: a standard
    error near 0.002, bars of ten."""
    K, H, B = 4096, 64, 2
    eng, x0, U0 = _setup(M, "cartpole", K, H, B, lambda_=1e9)
    eng.set_noise_model([0.5], 0.8)
    st = eng.solve(x0, U0, seed=0x1234, stats=True).stats
    sig = np.sqrt(st["eps_m2"].astype(np.float64))
    rho = st["eps_m11"].astype(np.float64) / st["eps_m2"]
    print("sigma", sig.ravel(), "rho", rho.ravel(), "ess", st["ess"])
    assert np.all(np.abs(sig / 0.5 - 1.0) < 0.02)
    assert np.all(np.abs(rho - 0.8) < 0.02)
    eng.close()


# ------------------------------------------------------------------------------------------ 6. streams

def _snap(torch, *ts):
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in ts)


@pytest.mark.parametrize("kind", ["cartpole", "ca"])
def test_streams_give_the_plain_solves_statistics(M, kind):
    """Three chained solves and a three-solve graph (SHIFT | ENV_STEP), both with the flag: per step the statistics of
    three plain counter solves with the flag from the same start, bitwise; the U (and x0, u0) sequences are bitwise
    those of the same streams without the flag; the seed counters agree."""
    import torch
    K, H, B, n, seed = 128, 8, 2, 3, 9
    dev = torch.device("cuda")
    stats, seqs, ctrs = {}, {}, {}
    for mode in ("plain", "chain", "graph"):
        for flag in (True, False):
            eng, x0, U0 = _setup(M, kind, K, H, B)
            eng.set_stream(torch.cuda.current_stream().cuda_stream)
            tx, tU = torch.from_numpy(x0).to(dev), torch.from_numpy(U0).to(dev)
            tu0 = torch.zeros(B, U0.shape[1], device=dev)
            st, seq = [], []
            if mode == "graph":
                eng.graph_capture(B, n, tx.data_ptr(), tU.data_ptr(), tu0.data_ptr(), seed=seed, stats=flag)
                eng.graph_launch(sync=True)
                seq.append(_snap(torch, tx, tU, tu0))
                if flag:
                    st = [eng.stats(B, step=i) for i in range(n)]
            else:
                for _ in range(n):
                    eng.solve_device(B, tx.data_ptr(), tU.data_ptr(), None, seed=seed, u0_ptr=tu0.data_ptr(),
                                     shift=True, env_step=True, seed_counter=mode == "plain", chain=mode == "chain",
                                     stats=flag)
                    seq.append(_snap(torch, tx, tU, tu0))
                    if flag:
                        st.append(eng.stats(B))
            ctrs[mode, flag] = eng.get_seed_counter()
            stats[mode, flag], seqs[mode, flag] = st, seq
            eng.close()
    assert set(ctrs.values()) == {n}
    for mode in ("chain", "graph"):
        assert len(stats[mode, True]) == n
        for got, want in zip(stats[mode, True], stats["plain", True]):
            _same_stats(got, want)
    for mode in ("plain", "chain", "graph"):
        for got, want in zip(seqs[mode, True], seqs[mode, False]):
            for a, b in zip(got, want):
                np.testing.assert_array_equal(a, b)
    for a, b in zip(seqs["graph", True][-1], seqs["plain", True][-1]):  # (and the streams are the plain loop)
        np.testing.assert_array_equal(a, b)
    steps = stats["plain", True]
    assert not np.array_equal(steps[0]["cost_mean"], steps[1]["cost_mean"])  # the slots hold different solves


# ------------------------------------------------------------------------------------------ 7. errors

def test_get_stats_errors_and_survival(M):
    import torch
    from mppi_hip import _lib as L
    K, H, B, n = 128, 8, 2, 3
    eng, x0, U0 = _setup(M, "cartpole", K, H, 3)
    lib = eng.lib
    rec = np.zeros(3, np.dtype(L.STATS_DTYPE))
    p = rec.ctypes.data_as(ctypes.c_void_p)
    eng.solve(x0[:B], U0[:B], seed=1)  # a solve without the flag does not count
    assert lib.mppi_get_stats(eng._h, B, 0, p, None, None) == L.MPPI_E_STATE
    assert b"mppi_get_stats" in lib.mppi_last_error()
    eng.solve(x0[:B], U0[:B], seed=1, stats=True)
    assert lib.mppi_get_stats(eng._h, B, 0, p, None, None) == L.MPPI_OK
    assert lib.mppi_get_stats(eng._h, 1, 0, None, None, None) == L.MPPI_OK  # every pointer may be NULL
    for B_bad, step_bad in ((3, 0), (0, 0), (B, 1), (B, -1)):
        assert lib.mppi_get_stats(eng._h, B_bad, step_bad, p, None, None) == L.MPPI_E_ARG, (B_bad, step_bad)
    ptrs = eng.device_stats()
    assert all(ptrs.values())
    # a graph of n solves: steps 0..n-1; destroying it (mppi_set_noise_model) leaves the statistics readable
    dev = torch.device("cuda")
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    tx, tU = torch.from_numpy(x0[:B]).to(dev), torch.from_numpy(U0[:B]).to(dev)
    tu0 = torch.zeros(B, 1, device=dev)
    eng.graph_capture(B, n, tx.data_ptr(), tU.data_ptr(), tu0.data_ptr(), seed=3, stats=True)
    eng.graph_launch(sync=True)
    before = [eng.stats(B, step=i) for i in range(n)]
    assert lib.mppi_get_stats(eng._h, B, n, p, None, None) == L.MPPI_E_ARG
    assert lib.mppi_get_stats(eng._h, 3, 0, p, None, None) == L.MPPI_E_ARG
    eng.set_noise_model([0.6], 0.8)
    with pytest.raises(M.MPPIError) as ei:
        eng.graph_launch(sync=True)
    assert ei.value.code == L.MPPI_E_STATE
    for i in range(n):
        _same_stats(eng.stats(B, step=i), before[i])
    eng.close()


# ------------------------------------------------------------------------------------------ 8. the adaptive model

def test_model_adapts_its_sampling_law(M):
    """MPPIModel(adapt_noise=r): after a step the engine's law is adapt_noise_model of that step's statistics."""
    from mppi_hip.stats import adapt_noise_model
    m = M.MPPIModel("cartpole_py", K=256, adapt_noise=0.5, noise_rho=0.3, seed=4)
    d = M.SimData(qpos=np.array([0.0, 0.3]), qvel=np.zeros(2), ctrl=np.zeros(1))
    res = M.mppi_step(m, d)
    assert res.stats is not None and res.stats["eps_m2"].shape == (1,)
    sig, rho = adapt_noise_model([m.config.sigma], 0.3, res.stats["eps_m2"], res.stats["eps_m11"], 0.5, 1e-3, 10.0, 0.95)
    got = m.engine.noise_model()
    np.testing.assert_allclose(got[0], sig, rtol=1e-6)
    assert got[1] == pytest.approx(rho, rel=1e-6) and got[2] is True
    assert not np.array_equal(got[0], [m.config.sigma])
    plain = M.MPPIModel("cartpole_py", K=256, seed=4)
    assert M.mppi_step(plain, d).stats is None and plain.engine.noise_model()[2] is False
    m.close()
    plain.close()
