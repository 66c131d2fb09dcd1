"""The sampling law on the device (mppi_set_noise_model: per-actuator sigma, AR(1) along the horizon) against its
host restatement (mppi_hip.noise.ar1_filter over tests/philox_ref.device_noise), and in every stream form."""
import ctypes

import numpy as np
import pytest

from oracle import mppi_ref as R
from philox_ref import device_noise

pytestmark = pytest.mark.gpu

MLP_NX, MLP_NU = 10, 3


@pytest.fixture(scope="module")
def M(gpu_available):
    import mppi_hip
    return mppi_hip


def _setup(M, kind, K, H, B):
    """(engine, x0 [B,nx] f32, U0 [B,nu,H] f32): the analytic cartpole, or a seeded MLP (nu = 3, fp32, quad_est)."""
    rs = np.random.RandomState(11)
    if kind == "cartpole":
        eng = M.Engine(M.Config.preset("cartpole_py", K=K, H=H, max_batch=B))
        eng.load_dynamics(1).set_cost("cartpole")
        x0 = np.stack([[0.0, 0.2 + 0.3 * b, 0.0, 0.0] for b in range(B)])
        nu = 1
    else:
        from mppi_hip.nets import mlp_blob, synthetic_mlp
        sd = synthetic_mlp(MLP_NX, MLP_NU, seed=0)
        eng = M.Engine(M.Config(nx=MLP_NX, nu=MLP_NU, H=H, K=K, max_batch=B, lambda_=1.0, sigma=0.5, precision=0))
        eng.load_dynamics(*mlp_blob(sd, MLP_NX, MLP_NU))
        eng.set_cost("quad_est")
        x0 = 0.3 * rs.randn(B, MLP_NX)
        nu = MLP_NU
    U0 = 0.1 * rs.randn(B, nu, H)
    return eng, x0.astype(np.float32), U0.astype(np.float32)


@pytest.fixture(params=["direct", "lds"])
def path(request, monkeypatch):
    """Both generators of the active model (MPPI_NOISE_AR1, read per launch): noise_ar1_kernel, which the default
    routing takes for grids that fill the chip, and noise_ar1_lds_kernel for the small ones."""
    monkeypatch.setenv("MPPI_NOISE_AR1", request.param)
    return request.param


def _same(a, b):
    assert np.array_equal(a.costs, b.costs)
    assert np.array_equal(a.U, b.U)
    assert np.array_equal(a.u0, b.u0)


# ------------------------------------------------------------------------------------------ 1. identity

@pytest.mark.parametrize("kind", ["cartpole", "mlp"])
def test_default_valued_model_is_the_white_noise_bitwise(M, kind, path):
    """rho = 0 with every sigma_u == cfg.sigma runs the new kernel and reproduces the default noise value for value;
    the reset (None, 0) goes back to the default path."""
    K, H, B, seed = 130, 7, 2, 0x5151_0000_0007
    ref, x0, U0 = _setup(M, kind, K, H, B)
    r0 = ref.solve(x0, U0, seed=seed)
    eng, _, _ = _setup(M, kind, K, H, B)
    nu = eng.config.nu
    assert eng.noise_model()[2] is False
    eng.set_noise_model([eng.config.sigma] * nu, 0.0)
    s, rho, active = eng.noise_model()
    assert active is True and rho == 0.0 and np.array_equal(s, np.full(nu, eng.config.sigma, np.float32))
    _same(eng.solve(x0, U0, seed=seed), r0)
    eng.set_noise_model(None, 0.0)
    assert eng.noise_model()[2] is False
    _same(eng.solve(x0, U0, seed=seed), r0)
    ref.close()
    eng.close()


# ------------------------------------------------------------------------------------------ 2. the law

@pytest.mark.parametrize("H", [1, 7])
def test_device_law_equals_injected_reference(M, H, path):
    """Device AR(1) noise == ar1_filter over the numpy Philox normals, injected into a second engine.  K = 130 is no
    multiple of 4 (padded lanes).  The tolerances of test_cartpole_device_philox_noise, the same comparison: the fp32
    recursion adds at most about 1 / (1 - rho) = 10 roundings of 2^-24."""
    from mppi_hip.noise import ar1_filter
    K, B, rho, sig, seed = 130, 2, 0.9, [0.7], 0x1234_5678_9ABC
    eng, x0, U0 = _setup(M, "cartpole", K, H, B)
    eng.set_noise_model(sig, rho)
    r1 = eng.solve(x0, U0, seed=seed, want_weights=True)
    noise = ar1_filter(device_noise(seed, B, 1, H, K, 1.0), rho, sig)
    inj, _, _ = _setup(M, "cartpole", K, H, B)
    r2 = inj.solve(x0, U0, noise=noise, want_weights=True)
    print("max rel cost diff", float(np.max(np.abs(r1.costs - r2.costs) / np.abs(r2.costs))),
          "max U diff", float(np.max(np.abs(r1.U - r2.U))))
    np.testing.assert_allclose(r1.costs, r2.costs, rtol=2e-5)
    np.testing.assert_allclose(r1.U, r2.U, atol=2e-5)
    white, _, _ = _setup(M, "cartpole", K, H, B)  # ... and it is another law than the default
    assert not np.array_equal(white.solve(x0, U0, seed=seed).costs, r1.costs)
    for e in (eng, inj, white):
        e.close()


def test_both_generators_agree_bitwise_where_the_routing_changes(M, monkeypatch):
    """B * nu * Kp / 256 = 1024 waves (8 cartpole solves of K = 32768) is where the default routing goes from
    noise_ar1_lds_kernel to noise_ar1_kernel on a 256-CU device: the default and each forced kernel give the same
    solve bit for bit (several blocks along k in both), and it is the injected reference's."""
    from mppi_hip.noise import ar1_filter
    K, H, B, rho, sig, seed = 32768, 3, 8, 0.9, [0.7], 0xBEEF
    eng, x0, U0 = _setup(M, "cartpole", K, H, B)
    eng.set_noise_model(sig, rho)
    res = {}
    for knob in (None, "direct", "lds"):
        if knob:
            monkeypatch.setenv("MPPI_NOISE_AR1", knob)
        res[knob] = eng.solve(x0, U0, seed=seed)
    _same(res[None], res["direct"])
    _same(res[None], res["lds"])
    monkeypatch.delenv("MPPI_NOISE_AR1")
    eng.set_noise_model(None, 0.0)
    noise = ar1_filter(device_noise(seed, B, 1, H, K, 1.0), rho, sig)
    r2 = eng.solve(x0, U0, noise=noise)
    np.testing.assert_allclose(res[None].costs, r2.costs, rtol=2e-5)
    np.testing.assert_allclose(res[None].U, r2.U, atol=2e-5)
    eng.close()


# ------------------------------------------------------------------------------------------ 3. actuator mapping

def test_sigma_u_reaches_its_own_actuator(M, path):
    """nu = 3 with three different sigmas: costs against the injected reference at test_mlp_dynamics' fp32 bar, and
    U_new - U0 = sum_k w_k eps[u, t, k] of the REFERENCE noise with the engine's own weights (_check_solve's bar): a
    swapped or shared sigma index is off by the ratio of the sigmas."""
    from mppi_hip.noise import ar1_filter
    K, H, B, rho, sig, seed = 96, 5, 2, 0.5, [0.1, 0.5, 1.0], 77
    eng, x0, U0 = _setup(M, "mlp", K, H, B)
    eng.set_noise_model(sig, rho)
    r1 = eng.solve(x0, U0, seed=seed, want_weights=True)
    noise = ar1_filter(device_noise(seed, B, MLP_NU, H, K, 1.0), rho, sig)
    inj, _, _ = _setup(M, "mlp", K, H, B)
    r2 = inj.solve(x0, U0, noise=noise, want_weights=True)
    np.testing.assert_allclose(r1.costs, r2.costs, rtol=1e-4, atol=1e-7)
    pre = R.Preset("t", K=K, H=H, lam=1.0, sigma=0.5)
    for b in range(B):
        U_own = R.update_U(pre, U0[b].astype(np.float64), noise[b], r1.weights[b].astype(np.float64))
        np.testing.assert_allclose(r1.U[b], U_own, atol=1e-5)
        dU = np.abs(r1.U[b] - U0[b]).max(axis=1)
        assert dU[0] < dU[2]  # (the update of the sigma 0.1 actuator is the small one)
    eng.close()
    inj.close()


# ------------------------------------------------------------------------------------------ 4. streams

def _model_for(kind):
    return (None, 0.7) if kind == "cartpole" else ([0.2, 0.5, 0.8], 0.7)


def _plain(eng, B, tx, tU, tu0, seed, n):
    for _ in range(n):
        eng.solve_device(B, tx.data_ptr(), tU.data_ptr(), None, seed=seed, u0_ptr=tu0.data_ptr(), shift=True,
                         env_step=True, seed_counter=True)


def _snap(torch, *ts):
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in ts)


@pytest.mark.parametrize("kind", ["cartpole", "mlp"])
def test_streams_with_the_model_active_equal_plain_solves(M, kind, path):
    """A captured graph launched twice, and a loop of chained solves, are bitwise equal in (x0, U, u0) to the same
    number of plain counter solves; the trajectory log of a graph stream holds the plain loop's controls."""
    import torch
    from mppi_hip.trajectory import run_stream
    K, H, B, n, seed = 128, 8, 2, 5, 9
    dev = torch.device("cuda")
    outs = {}
    plain_u0 = []
    for mode in ("plain", "graph", "chain", "white"):
        eng, x0, U0 = _setup(M, kind, K, H, B)
        if mode != "white":
            eng.set_noise_model(*_model_for(kind))
        eng.set_stream(torch.cuda.current_stream().cuda_stream)
        tx, tU = torch.from_numpy(x0).to(dev), torch.from_numpy(U0).to(dev)
        tu0 = torch.zeros(B, U0.shape[1], device=dev)
        snaps = []
        if mode in ("plain", "white"):
            for i in range(2 * n):
                _plain(eng, B, tx, tU, tu0, seed, 1)
                if mode == "plain":
                    plain_u0.append(_snap(torch, tu0)[0])
                if i + 1 in (n, 2 * n):
                    snaps.append(_snap(torch, tx, tU, tu0))
        elif mode == "graph":
            eng.graph_capture(B, n, tx.data_ptr(), tU.data_ptr(), tu0.data_ptr(), seed=seed)
            for _ in range(2):
                eng.graph_launch(sync=True)
                snaps.append(_snap(torch, tx, tU, tu0))
        else:
            for i in range(2 * n):
                eng.solve_device(B, tx.data_ptr(), tU.data_ptr(), None, seed=seed, u0_ptr=tu0.data_ptr(), shift=True,
                                 env_step=True, chain=True)
                if i + 1 in (n, 2 * n):
                    snaps.append(_snap(torch, tx, tU, tu0))
        assert eng.get_seed_counter() == 2 * n
        outs[mode] = snaps
        eng.close()
    for mode in ("graph", "chain"):
        for got, want in zip(outs[mode], outs["plain"]):
            for a, b in zip(got, want):
                np.testing.assert_array_equal(a, b)
    assert not np.array_equal(outs["white"][0][1], outs["plain"][0][1])  # the model is in effect in the stream
    # trajectory logging (mppi_graph_capture_traj) with the model active
    eng, x0, U0 = _setup(M, kind, K, H, B)
    eng.set_noise_model(*_model_for(kind))
    states, actions, U_end = run_stream(eng, x0, U0, n, seed=seed, launches=2)
    np.testing.assert_array_equal(states[0], x0)
    np.testing.assert_array_equal(actions, np.stack(plain_u0))
    np.testing.assert_array_equal(U_end, outs["plain"][1][1])
    eng.close()


@pytest.mark.parametrize("kind", ["cartpole", "mlp"])
def test_graph_launches_mixed_with_plain_solves_model_active(M, kind):
    """The interleaving plan of test_graph_noise_prefetch_mixed_with_plain_solves (odd and even stream lengths, a
    re-capture, plain solves between) with the model active: the key sequence of a loop of plain solves, bitwise."""
    import torch
    K, H, B = 128, 8, 2
    dev = torch.device("cuda")
    plan = [("graph", 3), ("plain", 1), ("graph", 2), ("graph", 2), ("plain", 2), ("graph", 3)]
    outs = []
    for mode in ("loop", "mixed"):
        eng, x0, U0 = _setup(M, kind, K, H, B)
        eng.set_noise_model(*_model_for(kind))
        eng.set_stream(torch.cuda.current_stream().cuda_stream)
        tx, tU = torch.from_numpy(x0).to(dev), torch.from_numpy(U0).to(dev)
        tu0 = torch.zeros(B, U0.shape[1], device=dev)
        captured = None
        for what, n in plan:
            if mode == "loop" or what == "plain":
                _plain(eng, B, tx, tU, tu0, 5, n)
            else:
                if captured != n:  # re-capture only when the stream length changes
                    eng.graph_capture(B, n, tx.data_ptr(), tU.data_ptr(), tu0.data_ptr(), seed=5)
                    captured = n
                eng.graph_launch(sync=False)
        outs.append(_snap(torch, tx, tU, tu0))
        eng.close()
    for a, b in zip(outs[0], outs[1]):
        np.testing.assert_array_equal(a, b)


# ------------------------------------------------------------------------------------------ 5. invalidation

def test_set_noise_model_invalidates_graphs_and_keeps_the_key(M):
    import torch
    from mppi_hip import _lib as L
    K, H, B, n, seed = 128, 8, 2, 3, 21
    dev = torch.device("cuda")
    outs = []
    for mode in ("loop", "graph"):
        eng, x0, U0 = _setup(M, "cartpole", K, H, B)
        eng.set_stream(torch.cuda.current_stream().cuda_stream)
        tx, tU = torch.from_numpy(x0).to(dev), torch.from_numpy(U0).to(dev)
        tu0 = torch.zeros(B, 1, device=dev)
        if mode == "loop":  # n solves of the default law, then n of the model
            _plain(eng, B, tx, tU, tu0, seed, n)
            eng.set_noise_model([0.6], 0.8)
            _plain(eng, B, tx, tU, tu0, seed, n)
        else:
            eng.graph_capture(B, n, tx.data_ptr(), tU.data_ptr(), tu0.data_ptr(), seed=seed)
            eng.graph_launch(sync=True)  # leaves a prefetched noise of the default law: the counter is one ahead
            before = eng.get_seed_counter()
            eng.set_noise_model([0.6], 0.8)
            assert eng.get_seed_counter() == before == n  # the same logical key
            with pytest.raises(M.MPPIError) as ei:
                eng.graph_launch(sync=True)
            assert ei.value.code == L.MPPI_E_STATE and "mppi_graph_capture first" in str(ei.value)
            eng.graph_capture(B, n, tx.data_ptr(), tU.data_ptr(), tu0.data_ptr(), seed=seed)
            eng.graph_launch(sync=True)
        assert eng.get_seed_counter() == 2 * n
        outs.append(_snap(torch, tx, tU, tu0))
        eng.close()
    for a, b in zip(outs[0], outs[1]):
        np.testing.assert_array_equal(a, b)


# ------------------------------------------------------------------------------------------ 6. argument errors

def test_bad_arguments_are_refused_and_leave_the_model(M):
    from mppi_hip import _lib as L
    eng = M.Engine(M.Config(nx=MLP_NX, nu=MLP_NU, H=4, K=16))
    lib, fp = eng.lib, L._fp

    def call(sig, rho):
        p = None if sig is None else np.asarray(sig, np.float32).ctypes.data_as(fp)
        return lib.mppi_set_noise_model(eng._h, p, ctypes.c_float(rho))

    good = [0.1, 0.5, 1.0]
    bad = [(good, 1.0), (good, -0.1), (None, 1.0), (good, float("nan")), ([0.1, -0.5, 1.0], 0.5),
           ([0.1, float("nan"), 1.0], 0.5), ([float("inf"), 0.5, 1.0], 0.5), ([0.1, 0.5, -float("inf")], 0.0)]
    for state in ("default", "set"):
        if state == "set":
            eng.set_noise_model(good, 0.5)
        want = eng.noise_model()
        for sig, rho in bad:
            assert call(sig, rho) == L.MPPI_E_ARG, (sig, rho)
            assert b"mppi_set_noise_model" in lib.mppi_last_error()
            got = eng.noise_model()
            assert np.array_equal(got[0], want[0]) and got[1:] == want[1:], (sig, rho)
    s, rho, active = eng.noise_model()
    assert active and rho == 0.5 and np.array_equal(s, np.asarray(good, np.float32))
    assert call([0.0, 0.0, 0.0], 0.0) == L.MPPI_OK  # sigma 0 (a frozen actuator) is allowed
    eng.close()
    wide = M.Engine(M.Config(nx=4, nu=40, H=2, K=16))  # the model travels as a kernel argument: nu <= 32
    assert wide.lib.mppi_set_noise_model(wide._h, None, ctypes.c_float(0.5)) == L.MPPI_E_UNSUPPORTED
    assert wide.lib.mppi_set_noise_model(wide._h, None, ctypes.c_float(0.0)) == L.MPPI_OK
    assert wide.noise_model()[2] is False
    wide.close()
