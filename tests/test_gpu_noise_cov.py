"""The cross-actuator sampling covariance on the device (mppi_set_noise_cov, noise_cov_kernel) against its host
restatement (mppi_hip.noise.cov_filter over the device's own normals, read through mppi_noise_eval), bitwise, in every
stream form, with the control-cost term under the law, and the setter's contract.  (noise_cov_kernel has one form: no
env knob to go through.)"""
import ctypes

import numpy as np
import pytest

from conftest import PKG
from cov_cases import B, HS, K, NUS, RHOS, bits, build_lin_host, sigma_of
from test_gpu_noise_model import MLP_NU, MLP_NX, _setup

pytestmark = pytest.mark.gpu
U32 = 2.0 ** -24


@pytest.fixture(scope="module")
def M(gpu_available):
    import mppi_hip
    return mppi_hip


@pytest.fixture(scope="module")
def lin_host(tmp_path_factory):
    import os
    return build_lin_host(tmp_path_factory.mktemp("cov_lin"), os.path.join(PKG, "csrc"))


def _bare(M, nu, H, sigma=1.0, Kb=K):
    """an engine that only draws noise (mppi_noise_eval and mppi_control_term_eval need no dynamics)"""
    return M.Engine(M.Config(nx=4 if nu == 1 else MLP_NX, nu=nu, H=H, K=Kb, max_batch=B, lambda_=1.0, sigma=sigma,
                             precision=0))


def _same(a, b):
    assert np.array_equal(a.costs, b.costs)
    assert np.array_equal(a.U, b.U)
    assert np.array_equal(a.u0, b.u0)


def _law(eng, S, rho):
    """the covariance S with the AR(1) correlation rho on a handle"""
    eng.set_noise_cov(S)
    if rho > 0.0:
        eng.set_noise_model(None, rho)
    return eng


# ------------------------------------------------------------------------------------------ 6. the law, bitwise

@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("nu", NUS)
def test_device_law_equals_cov_filter_bitwise(M, nu, H):
    """z = the device's own normals (the default law with cfg.sigma = 1); with the covariance on the same handle the
    generator gives cov_filter(z, L, rho), bit for bit, L as the handle reports it = cov_factor(Sigma)."""
    from mppi_hip.noise import cov_factor, cov_filter
    seed = 0x5EED_0000_0200 + 64 * nu + H
    eng = _bare(M, nu, H)
    assert eng.noise_cov() is None
    z = eng.noise_eval(B, seed)
    assert z.shape == (B, nu, H, K) and np.all(np.isfinite(z))
    S = sigma_of(nu)
    S64 = S.astype(np.float64)
    for rho in RHOS:  # (ascending: rho = 0 is what enabling on the default law gives)
        _law(eng, S, rho)
        Sg, Lg, Sinv = eng.noise_cov()
        assert np.array_equal(bits(Sg), bits(S)) and np.array_equal(bits(Lg), bits(cov_factor(S)))
        inv = np.linalg.inv(S64)
        assert np.abs(Sinv - inv).max() <= 1e-5 * np.linalg.cond(S64) * np.abs(inv).max()
        s, r, active = eng.noise_model()
        assert active is True and r == np.float32(rho)
        assert np.array_equal(bits(s), bits(np.sqrt(np.diag(S64)).astype(np.float32)))
        got = eng.noise_eval(B, seed)
        want = cov_filter(z, Lg, rho, is_factor=True)
        bad = int(np.count_nonzero(bits(got) != bits(want)))
        print(f"nu {nu} H {H} rho {rho}: {bad} of {got.size} differ")
        assert bad == 0, rho
    assert not np.array_equal(eng.noise_eval(B, seed + 1), got)
    eng.close()


def test_device_law_with_several_blocks_along_k(M):
    """K = 1100 (Kp = 1152: 288 k-quads, five blocks of 64 along k, the last with 32 live lanes) at config #4's width."""
    from mppi_hip.noise import cov_filter
    nu, H, Kb, seed = 21, 7, 1100, 0xB10C
    eng = _bare(M, nu, H, Kb=Kb)
    z = eng.noise_eval(B, seed)
    _law(eng, sigma_of(nu), 0.9)
    got = eng.noise_eval(B, seed)
    assert np.array_equal(bits(got), bits(cov_filter(z, eng.noise_cov()[1], 0.9, is_factor=True)))
    eng.close()


# ------------------------------------------------------------------------------------------ 7. identity and return

@pytest.mark.parametrize("rho", RHOS)
@pytest.mark.parametrize("kind", ["cartpole", "mlp"])
def test_identity_covariance_is_the_unit_model_bitwise(M, kind, rho):
    """Sigma = I: the solve of set_noise_model(ones, rho); after disabling, the model stays active with
    sigma_u = sqrt(diag Sigma) and the old rho."""
    H, seed = 7, 0x7171_0000_0005
    ref, x0, U0 = _setup(M, kind, K, H, B)
    nu = ref.config.nu
    ref.set_noise_model(np.ones(nu, np.float32), rho)
    r0 = ref.solve(x0, U0, seed=seed)
    eng, _, _ = _setup(M, kind, K, H, B)
    _law(eng, np.eye(nu, dtype=np.float32), rho)
    _same(eng.solve(x0, U0, seed=seed), r0)
    S = sigma_of(nu)  # (another law in between: other costs)
    eng.set_noise_cov(S)
    assert not np.array_equal(eng.solve(x0, U0, seed=seed).costs, r0.costs)
    eng.set_noise_cov(None)
    assert eng.noise_cov() is None
    s, r, active = eng.noise_model()
    assert active is True and r == np.float32(rho)
    assert np.array_equal(bits(s), bits(np.sqrt(np.diag(S.astype(np.float64))).astype(np.float32)))
    ref.set_noise_model(s, rho)
    _same(eng.solve(x0, U0, seed=seed), ref.solve(x0, U0, seed=seed))
    eng.set_noise_cov(None)  # off -> off
    ref.close()
    eng.close()


# ------------------------------------------------------------------------------------------ 8. injected == device

@pytest.mark.parametrize("kind", ["cartpole", "mlp"])
def test_injected_noise_eval_equals_the_device_solve(M, kind):
    H, seed = 7, 0xD00D_0000_0021
    eng, x0, U0 = _setup(M, kind, K, H, B)
    _law(eng, sigma_of(eng.config.nu), 0.9)
    r1 = eng.solve(x0, U0, seed=seed, want_weights=True)
    noise = eng.noise_eval(B, seed)
    inj, _, _ = _setup(M, kind, K, H, B)
    r2 = inj.solve(x0, U0, noise=noise, want_weights=True)
    _same(r1, r2)
    assert np.array_equal(r1.weights, r2.weights)
    assert np.array_equal(eng.solve(x0, U0, seed=seed).costs, r1.costs)  # the evaluation left the handle as it was
    eng.close()
    inj.close()


# ------------------------------------------------------------------------------------------ 9. stream forms

def _snap(torch, *ts):
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in ts)


@pytest.mark.parametrize("extras", [False, True], ids=["cov", "cov+bounds+keep+ctrl"])
def test_stream_forms_agree_bitwise(M, extras):
    """n = 3 solves with SHIFT and ENV_STEP as plain counter solves, chained solves, one captured graph and the
    trajectory-logging capture: x, U, u0, the last solve's costs and the seed counter, bit for bit; once more with
    control bounds, n_keep = 4 and the control-cost term on (the passes behind the generator, and lin under the law)."""
    import torch
    H, n, seed = 7, 3, 77
    dev = torch.device("cuda")
    outs = {}
    for mode in ("plain", "chain", "graph", "traj", "no_cov"):
        eng, x0, U0 = _setup(M, "mlp", K, H, B)
        nu = eng.config.nu
        S = sigma_of(nu)
        if mode != "no_cov":
            _law(eng, S, 0.9)
        else:  # the same scales and rho, independent actuators
            eng.set_noise_model(np.sqrt(np.diag(S.astype(np.float64))).astype(np.float32), 0.9)
        if extras:
            eng.set_control_bounds(-0.3, 0.4)
            eng.set_elite_keep(4)
            eng.set_control_cost(0.5)
        eng.set_stream(torch.cuda.current_stream().cuda_stream)
        tx, tU = torch.from_numpy(x0).to(dev), torch.from_numpy(U0).to(dev)
        tu0, tc = torch.zeros(B, nu, device=dev), torch.zeros(B, K, device=dev)
        if mode in ("plain", "chain", "no_cov"):
            for _ in range(n):
                eng.solve_device(B, tx.data_ptr(), tU.data_ptr(), None, seed=seed, costs_ptr=tc.data_ptr(),
                                 u0_ptr=tu0.data_ptr(), shift=True, env_step=True, seed_counter=mode != "chain",
                                 chain=mode == "chain")
        elif mode == "graph":
            eng.graph_capture(B, n, tx.data_ptr(), tU.data_ptr(), tu0.data_ptr(), costs_ptr=tc.data_ptr(), seed=seed)
            eng.graph_launch(sync=True)
        else:
            trx, tru = torch.empty(n, B, eng.config.nx, device=dev), torch.empty(n, B, nu, device=dev)
            eng.graph_capture_traj(B, n, tx.data_ptr(), tU.data_ptr(), tu0.data_ptr(), costs_ptr=tc.data_ptr(),
                                   seed=seed, traj_x_ptr=trx.data_ptr(), traj_u_ptr=tru.data_ptr())
            eng.graph_launch(sync=True)
            assert np.array_equal(_snap(torch, tru)[0][-1], _snap(torch, tu0)[0])
        counter = eng.get_seed_counter()
        assert counter == n
        outs[mode] = _snap(torch, tx, tU, tu0, tc) + (counter,)
        eng.close()
    for mode in ("chain", "graph", "traj"):
        for a, b in zip(outs[mode], outs["plain"]):
            np.testing.assert_array_equal(a, b)
    assert not np.array_equal(outs["no_cov"][1], outs["plain"][1])  # the covariance is in effect in the stream


# ------------------------------------------------------------------------------------------ 10. the control-cost term

def _check_term(term, lin, nz):
    """the term against the float64 sum of the device's own lin: the bar of tests/test_gpu_control_cost.py"""
    n = lin.shape[1] * lin.shape[2]
    l64, e64 = lin.astype(np.float64), nz.astype(np.float64)
    want = np.einsum("buh,buhk->bk", l64, e64)
    maj = np.einsum("buh,buhk->bk", np.abs(l64), np.abs(e64))
    err = np.abs(term.astype(np.float64) - want)
    assert np.all(err <= n * U32 / (1 - n * U32) * maj)


@pytest.mark.parametrize("nu", NUS)
def test_control_term_eval_under_the_law(M, lin_host, nu):
    """lin of ctrl_lin_kernel equals the host header's cov form bit for bit and meets its bound against float64; the
    term meets the bar of the per-actuator term."""
    from mppi_hip.stats import control_term_ref
    gamma = np.float32(0.7)
    rs = np.random.RandomState(500 + nu)
    S = sigma_of(nu)
    for H in HS:
        eng = _bare(M, nu, H)
        eng.set_control_cost(float(gamma))
        U = (0.5 * rs.randn(B, nu, H)).astype(np.float32)
        nz = rs.randn(B, nu, H, K).astype(np.float32)
        for rho in RHOS:
            _law(eng, S, rho)
            Sinv = eng.noise_cov()[2]
            term, lin = eng.control_term_eval(U, nz)
            want = lin_host(Sinv, U, gamma, rho)
            assert np.array_equal(bits(lin), bits(want)), (nu, H, rho)
            _, lin64, A = control_term_ref(U, nz, None, float(np.float32(rho)), float(gamma), Sinv=Sinv)
            assert np.all(np.abs(lin.astype(np.float64) - lin64) <= (nu + 8) * U32 * A), (nu, H, rho)
            _check_term(term, lin, nz)
        eng.close()


def test_a_diagonal_covariance_gives_the_per_actuator_coefficients(M):
    """Sigma = diag(sigma_u^2) with square roots exact in fp32: lin within (nu + 8) roundings of the per-actuator
    form's, and the same noise as the per-actuator model."""
    from mppi_hip.stats import control_term_ref
    nu, H, gamma, rho = 3, 7, 0.7, 0.9
    sig = np.float32([0.5, 0.25, 2.0])
    rs = np.random.RandomState(12)
    U = (0.5 * rs.randn(B, nu, H)).astype(np.float32)
    nz = rs.randn(B, nu, H, K).astype(np.float32)
    ref = _bare(M, nu, H)
    ref.set_noise_model(sig, rho)
    ref.set_control_cost(gamma)
    lin_u = ref.control_term_eval(U, nz)[1]
    eng = _bare(M, nu, H)
    eng.set_control_cost(gamma)
    _law(eng, np.diag(sig * sig), rho)
    assert np.array_equal(eng.noise_model()[0], sig)
    lin_c = eng.control_term_eval(U, nz)[1]
    A = control_term_ref(U, nz, sig.astype(np.float64), float(np.float32(rho)), float(np.float32(gamma)))[2]
    assert np.all(np.abs(lin_c.astype(np.float64) - lin_u.astype(np.float64)) <= (nu + 8) * U32 * A)
    assert np.array_equal(eng.noise_eval(B, 9), ref.noise_eval(B, 9))
    ref.close()
    eng.close()


def test_a_solve_weighs_costs_plus_the_term_under_the_law(M, lin_host):
    """Through a solve: lin is the host header's on the solve's U, the term is the kernels' on the solve's noise, and a
    covariance enabled while the term is on takes effect in the next solve."""
    H, seed, gamma, rho = 7, 0xC0DE, 0.5, 0.9
    eng, x0, U0 = _setup(M, "mlp", K, H, B)
    S = sigma_of(eng.config.nu)
    eng.set_noise_model(np.sqrt(np.diag(S.astype(np.float64))).astype(np.float32), rho)
    eng.set_control_cost(gamma)
    r_u = eng.solve(x0, U0, seed=seed)
    lin_u = eng.control_term(B)[1]
    eng.set_noise_cov(S)  # while the term is on
    r_c = eng.solve(x0, U0, seed=seed, want_weights=True)
    term, lin = eng.control_term(B)
    assert np.array_equal(bits(lin), bits(lin_host(eng.noise_cov()[2], U0, gamma, rho)))
    assert not np.array_equal(lin, lin_u) and not np.array_equal(r_c.U, r_u.U)
    nz = eng.noise_eval(B, seed)
    ev = eng.control_term_eval(U0, nz)
    assert np.array_equal(ev[0], term) and np.array_equal(ev[1], lin)
    _check_term(term, lin, nz)
    off, _, _ = _setup(M, "mlp", K, H, B)  # the term moves the weights
    _law(off, S, rho)
    assert not np.array_equal(off.solve(x0, U0, seed=seed, want_weights=True).weights, r_c.weights)
    off.close()
    eng.close()


# ------------------------------------------------------------------------------------------ 11. the setter's contract

def test_bad_arguments_are_refused_and_change_nothing(M):
    from mppi_hip import _lib as L
    nu, H = MLP_NU, 7
    eng = _bare(M, nu, H, sigma=0.5)
    lib = eng.lib
    S = sigma_of(nu)
    bad = []
    for i, v in (((2, 2), np.nan), ((0, 1), np.inf), ((1, 1), 0.0)):
        m = S.copy()
        m[i] = v
        if i[0] != i[1]:
            m[i[::-1]] = v
        bad.append(m)
    m = S.copy()
    m[0, 1] = np.nextafter(m[0, 1], np.float32(10))  # asymmetric by one ulp
    bad.append(m)
    bad.append(np.float32([[1, 2, 0], [2, 1, 0], [0, 0, 1]]))  # indefinite
    for state in ("off", "on"):
        if state == "on":
            _law(eng, S, 0.5)
        want_c, want_m = eng.noise_cov(), eng.noise_model()
        for m in bad:
            assert lib.mppi_set_noise_cov(eng._h, m.ctypes.data_as(ctypes.c_void_p)) == L.MPPI_E_ARG, m
            assert b"mppi_set_noise_cov" in lib.mppi_last_error()
            got_c, got_m = eng.noise_cov(), eng.noise_model()
            assert got_m[1:] == want_m[1:] and np.array_equal(got_m[0], want_m[0])
            assert (got_c is None) == (want_c is None)
            if want_c is not None:
                assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(got_c, want_c))
        with pytest.raises(ValueError):
            eng.set_noise_cov(np.eye(nu + 1, dtype=np.float32))
    # enabling on the default law made the model active with rho = 0
    fresh = _bare(M, nu, H, sigma=0.5)
    assert fresh.noise_model()[2] is False
    fresh.set_noise_cov(S)
    s, rho, active = fresh.noise_model()
    assert active is True and rho == 0.0 and np.array_equal(s, np.sqrt(np.diag(S.astype(np.float64))).astype(np.float32))
    # mppi_set_noise_model while the covariance is on
    f = ctypes.c_float
    assert lib.mppi_set_noise_model(fresh._h, None, f(0.0)) == L.MPPI_E_STATE
    assert b"mppi_set_noise_cov" in lib.mppi_last_error()
    sig = np.ones(nu, np.float32)
    assert lib.mppi_set_noise_model(fresh._h, sig.ctypes.data_as(L._fp), f(0.5)) == L.MPPI_E_STATE
    assert b"mppi_set_noise_cov" in lib.mppi_last_error()
    assert fresh.noise_cov() is not None and fresh.noise_model()[1] == 0.0 and np.array_equal(fresh.noise_model()[0], s)
    fresh.set_noise_model(None, 0.5)  # rho alone: the covariance and its scales stay
    assert fresh.noise_cov() is not None and fresh.noise_model()[1] == 0.5 and np.array_equal(fresh.noise_model()[0], s)
    fresh.set_noise_cov(None)
    fresh.set_noise_model(None, 0.0)  # allowed once it is off
    assert fresh.noise_model()[2] is False and fresh.noise_cov() is None
    fresh.close()
    eng.close()
    wide = M.Engine(M.Config(nx=4, nu=40, H=2, K=16))  # a covariance is an active model: nu <= 32
    eye = np.eye(40, dtype=np.float32)
    assert wide.lib.mppi_set_noise_cov(wide._h, eye.ctypes.data_as(ctypes.c_void_p)) == L.MPPI_E_UNSUPPORTED
    assert wide.lib.mppi_set_noise_cov(wide._h, None) == L.MPPI_OK
    assert wide.noise_model()[2] is False and wide.noise_cov() is None
    wide.close()


def test_knots_and_adaptation_are_refused_in_both_orders(M):
    from mppi_hip import _lib as L
    H, seed = 7, 0xC0FFEE
    f = ctypes.c_float
    eng, x0, U0 = _setup(M, "mlp", K, H, B)
    lib = eng.lib
    S = sigma_of(eng.config.nu)
    Sp = S.ctypes.data_as(ctypes.c_void_p)
    # the covariance first: knots and adaptation are refused, the law and the next solve stay
    _law(eng, S, 0.9)
    r0 = eng.solve(x0, U0, seed=seed)
    assert lib.mppi_set_noise_knots(eng._h, 3, 1) == L.MPPI_E_UNSUPPORTED
    err = lib.mppi_last_error()
    assert b"mppi_set_noise_knots" in err and b"mppi_set_noise_cov" in err
    assert lib.mppi_set_noise_adapt(eng._h, f(0.3), f(1e-3), f(10.0), f(0.95)) == L.MPPI_E_UNSUPPORTED
    err = lib.mppi_last_error()
    assert b"mppi_set_noise_adapt" in err and b"mppi_set_noise_cov" in err
    assert eng.noise_knots()[0] == 0 and eng.noise_adapt()[0] == 0.0 and eng.noise_cov() is not None
    _same(eng.solve(x0, U0, seed=seed), r0)
    assert lib.mppi_set_noise_knots(eng._h, 0, 0) == L.MPPI_OK  # (turning either off is no pair)
    assert lib.mppi_set_noise_adapt(eng._h, f(0.0), f(1e-3), f(10.0), f(0.95)) == L.MPPI_OK
    eng.close()
    # knots first
    eng, _, _ = _setup(M, "mlp", K, H, B)
    eng.set_noise_model(None, 0.9)
    eng.set_noise_knots(3, 1)
    r0 = eng.solve(x0, U0, seed=seed)
    assert lib.mppi_set_noise_cov(eng._h, Sp) == L.MPPI_E_UNSUPPORTED
    err = lib.mppi_last_error()
    assert b"mppi_set_noise_knots" in err and b"mppi_set_noise_cov" in err
    assert eng.noise_cov() is None and eng.noise_knots()[:2] == (3, 1)
    _same(eng.solve(x0, U0, seed=seed), r0)
    eng.close()
    # adaptation first (rate 0.3 moves the law behind every solve: the same two solves on a second handle)
    res = []
    for refuse in (False, True):
        eng, _, _ = _setup(M, "mlp", K, H, B)
        eng.set_noise_model(None, 0.9)
        eng.set_noise_adapt(0.3)
        first = eng.solve(x0, U0, seed=seed)
        if refuse:
            assert lib.mppi_set_noise_cov(eng._h, Sp) == L.MPPI_E_UNSUPPORTED
            err = lib.mppi_last_error()
            assert b"mppi_set_noise_adapt" in err and b"mppi_set_noise_cov" in err
            assert eng.noise_cov() is None and eng.noise_adapt()[0] == np.float32(0.3)
        res.append((first, eng.solve(x0, U0, seed=seed)))
        eng.close()
    _same(res[0][0], res[1][0])
    _same(res[0][1], res[1][1])


def test_a_change_destroys_graphs_and_keeps_the_key(M):
    """n solves of the AR(1) model, then n under a covariance enabled mid-stream: a loop of plain solves against a graph
    stream whose prefetched noise the change drops.  The value already in effect keeps the graph."""
    import torch
    from mppi_hip import _lib as L
    H, n, seed = 7, 3, 21
    dev = torch.device("cuda")
    outs = []
    for mode in ("loop", "graph"):
        eng, x0, U0 = _setup(M, "mlp", K, H, B)
        nu = eng.config.nu
        S = sigma_of(nu)
        eng.set_noise_model(np.full(nu, 0.6, np.float32), 0.8)
        eng.set_stream(torch.cuda.current_stream().cuda_stream)
        tx, tU = torch.from_numpy(x0).to(dev), torch.from_numpy(U0).to(dev)
        tu0 = torch.zeros(B, nu, device=dev)

        def plain():
            for _ in range(n):
                eng.solve_device(B, tx.data_ptr(), tU.data_ptr(), None, seed=seed, u0_ptr=tu0.data_ptr(), shift=True,
                                 env_step=True, seed_counter=True)

        if mode == "loop":
            plain()
            eng.set_noise_cov(S)
            plain()
            plain()
        else:
            eng.graph_capture(B, n, tx.data_ptr(), tU.data_ptr(), tu0.data_ptr(), seed=seed)
            eng.graph_launch(sync=True)  # leaves a prefetched noise of the old law: the device counter is one ahead
            before = eng.get_seed_counter()
            eng.set_noise_cov(S)
            assert eng.get_seed_counter() == before == n  # the same logical key
            with pytest.raises(M.MPPIError) as ei:
                eng.graph_launch(sync=True)
            assert ei.value.code == L.MPPI_E_STATE
            eng.graph_capture(B, n, tx.data_ptr(), tU.data_ptr(), tu0.data_ptr(), seed=seed)
            eng.graph_launch(sync=True)
            eng.set_noise_cov(S.copy())  # the value in effect, bitwise: the graph and its prefetched noise stay
            assert eng.get_seed_counter() == 2 * n
            eng.graph_launch(sync=True)
        assert eng.get_seed_counter() == 3 * n
        outs.append(_snap(torch, tx, tU, tu0))
        eng.close()
    for a, b in zip(outs[0], outs[1]):
        np.testing.assert_array_equal(a, b)


# ------------------------------------------------------------------------------------------ 12. off is off

@pytest.mark.parametrize("kind", ["cartpole", "mlp"])
def test_launches_per_solve(M, kind):
    """A handle that never enables the law, and one that enabled and disabled it, launch the kernels of the AR(1)
    model; with the law on the launch counts are the same (one generator, no second pass), and the control-cost term
    adds its own launches only."""
    H = 7
    names = ("noise", "rollout", "elites", "keep", "lambda", "bounds", "ctrl_cost", "reduce", "stats")

    def counts(e, x0, U0):
        e.profile(True)  # (resets the counters)
        e.solve(x0, U0, seed=3)
        got = {k: e.kernel_time(k)[0] for k in names}
        e.profile(False)
        return got

    never, x0, U0 = _setup(M, kind, K, H, B)
    default = counts(never, x0, U0)
    never.set_noise_model(None, 0.9)
    ar1 = counts(never, x0, U0)
    eng, _, _ = _setup(M, kind, K, H, B)
    assert counts(eng, x0, U0) == default
    _law(eng, sigma_of(eng.config.nu), 0.9)
    assert counts(eng, x0, U0) == ar1
    eng.set_noise_cov(None)
    assert counts(eng, x0, U0) == ar1
    eng.set_noise_model(None, 0.0)
    assert counts(eng, x0, U0) == default
    never.close()
    eng.close()
