"""Knot-parameterised sampling noise on the device (mppi_set_noise_knots, noise_knot_kernel) against its host
restatement (mppi_hip.noise.knot_filter over the device's own normals, read through mppi_noise_eval), bitwise, and in
every stream form."""
import ctypes

import numpy as np
import pytest

from knot_cases import B, HS, K, ORDERS, RHOS, bits, knot_counts, sigma_u
from test_gpu_noise_model import MLP_NU, MLP_NX, _setup

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def M(gpu_available):
    import mppi_hip
    return mppi_hip


def _bare(M, nu, H, sigma=1.0):
    """an engine that only draws noise (mppi_noise_eval needs no dynamics)"""
    return M.Engine(M.Config(nx=4 if nu == 1 else MLP_NX, nu=nu, H=H, K=K, max_batch=B, lambda_=1.0, sigma=sigma,
                             precision=0))


def _same(a, b):
    assert np.array_equal(a.costs, b.costs)
    assert np.array_equal(a.U, b.U)
    assert np.array_equal(a.u0, b.u0)


# ------------------------------------------------------------------------------------------ 5. the law, bitwise

@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("nu", [1, MLP_NU])
def test_device_law_equals_knot_filter_bitwise(M, nu, H):
    """z = the device's own normals (the default law with cfg.sigma = 1); with a knot law on the same handle the
    generator gives knot_filter(z), bit for bit: every order, P in {1, 2, 3, H}, rho in {0, 0.9}, non-uniform sigma_u.
    (noise_knot_kernel has one form: no env knob to go through.)"""
    from mppi_hip.noise import knot_filter, knot_table
    seed = 0x5EED_0000_0100 + H
    eng = _bare(M, nu, H)
    z = eng.noise_eval(B, seed)
    assert z.shape == (B, nu, H, K) and z.dtype == np.float32 and np.all(np.isfinite(z))
    sig = sigma_u(nu)
    for P in knot_counts(H):
        for order in ORDERS:
            for rho in RHOS:
                eng.set_noise_model(sig, rho)
                eng.set_noise_knots(P, order)
                n, o, idx, w = eng.noise_knots()
                tid, tw = knot_table(H, P, order)
                assert (n, o) == (P, order) and np.array_equal(idx, tid) and np.array_equal(bits(w), bits(tw))
                got = eng.noise_eval(B, seed)
                want = knot_filter(z, P, order, rho, sig)
                bad = int(np.count_nonzero(bits(got) != bits(want)))
                print(f"nu {nu} H {H} P {P} order {order} rho {rho}: {bad} of {got.size} differ")
                assert bad == 0, (P, order, rho)
    # the evaluation under the other laws: AR(1) without knots, and the default law again
    eng.set_noise_knots(0)
    assert eng.noise_knots() == (0, 0, None, None)
    assert np.array_equal(bits(eng.noise_eval(B, seed)), bits(knot_filter(z, H, 1, RHOS[-1], sig)))
    eng.set_noise_model(None, 0.0)
    assert np.array_equal(bits(eng.noise_eval(B, seed)), bits(z))
    assert not np.array_equal(eng.noise_eval(B, seed + 1), z)
    eng.close()


def test_device_law_with_several_blocks_along_k(M):
    """K = 1100 (Kp = 1152: 288 k-quads, two blocks of 256 threads, the second partly idle) and B nu = 6 rows: the
    same bitwise comparison where the grid has more than one block in both directions."""
    from mppi_hip.noise import knot_filter
    H, P, Kb, seed = 9, 3, 1100, 0xB10C
    eng = M.Engine(M.Config(nx=MLP_NX, nu=MLP_NU, H=H, K=Kb, max_batch=B, lambda_=1.0, sigma=1.0, precision=0))
    z = eng.noise_eval(B, seed)
    sig = sigma_u(MLP_NU)
    eng.set_noise_model(sig, 0.9)
    for order in ORDERS:
        eng.set_noise_knots(P, order)
        assert np.array_equal(bits(eng.noise_eval(B, seed)), bits(knot_filter(z, P, order, 0.9, sig))), order
    eng.close()


# ------------------------------------------------------------------------------------------ 6. identity

@pytest.mark.parametrize("kind", ["cartpole", "mlp"])
def test_all_knots_linear_is_the_ar1_model_bitwise(M, kind):
    """P == H with order 1 (and order 0): the solve of the AR(1) model, bit for bit; after disabling, the model without
    knots again (sigma_u and rho as they stood)."""
    H, seed, rho = 7, 0x7171_0000_0003, 0.9
    ref, x0, U0 = _setup(M, kind, K, H, B)
    sig = sigma_u(ref.config.nu)
    ref.set_noise_model(sig, rho)
    r0 = ref.solve(x0, U0, seed=seed)
    eng, _, _ = _setup(M, kind, K, H, B)
    eng.set_noise_model(sig, rho)
    for order in (1, 0):
        eng.set_noise_knots(H, order)
        assert eng.noise_knots()[:2] == (H, order)
        _same(eng.solve(x0, U0, seed=seed), r0)
    eng.set_noise_knots(2, 1)  # (another law in between: other costs)
    assert not np.array_equal(eng.solve(x0, U0, seed=seed).costs, r0.costs)
    eng.set_noise_knots(0)
    s, r, active = eng.noise_model()
    assert active is True and r == np.float32(rho) and np.array_equal(s, sig)
    _same(eng.solve(x0, U0, seed=seed), r0)
    ref.close()
    eng.close()


# ------------------------------------------------------------------------------------------ 7. injected == device

@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kind", ["cartpole", "mlp"])
def test_injected_noise_eval_equals_the_device_solve(M, kind, order):
    H, P, seed = 9, 3, 0xD00D_0000_0011
    eng, x0, U0 = _setup(M, kind, K, H, B)
    eng.set_noise_model(sigma_u(eng.config.nu), 0.9)
    eng.set_noise_knots(P, order)
    r1 = eng.solve(x0, U0, seed=seed, want_weights=True)
    noise = eng.noise_eval(B, seed)
    inj, _, _ = _setup(M, kind, K, H, B)
    r2 = inj.solve(x0, U0, noise=noise, want_weights=True)
    _same(r1, r2)
    assert np.array_equal(r1.weights, r2.weights)
    assert np.array_equal(eng.solve(x0, U0, seed=seed).costs, r1.costs)  # the evaluation left the handle as it was
    eng.close()
    inj.close()


# ------------------------------------------------------------------------------------------ 8. stream forms

def _snap(torch, *ts):
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in ts)


@pytest.mark.parametrize("extras", [False, True], ids=["knots", "knots+bounds+keep"])
@pytest.mark.parametrize("kind", ["cartpole", "mlp"])
def test_stream_forms_agree_bitwise(M, kind, extras):
    """n = 3 solves with SHIFT and ENV_STEP as plain counter solves, chained solves, one captured graph and the
    trajectory-logging capture: x, U, u0, the last solve's costs and the seed counter, bit for bit; once more with
    control bounds and n_keep = 4 on (the passes behind the generator)."""
    import torch
    H, P, order, n, seed = 9, 3, 3, 3, 77
    dev = torch.device("cuda")
    outs = {}
    for mode in ("plain", "chain", "graph", "traj", "no_knots"):
        eng, x0, U0 = _setup(M, kind, K, H, B)
        nu = eng.config.nu
        eng.set_noise_model(sigma_u(nu), 0.9)
        if mode != "no_knots":
            eng.set_noise_knots(P, order)
        if extras:
            eng.set_control_bounds(-0.3, 0.4)
            eng.set_elite_keep(4)
        eng.set_stream(torch.cuda.current_stream().cuda_stream)
        tx, tU = torch.from_numpy(x0).to(dev), torch.from_numpy(U0).to(dev)
        tu0, tc = torch.zeros(B, nu, device=dev), torch.zeros(B, K, device=dev)
        if mode in ("plain", "chain", "no_knots"):
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
    assert not np.array_equal(outs["no_knots"][1], outs["plain"][1])  # the knot law is in effect in the stream


# ------------------------------------------------------------------------------------------ 9. the setter's contract

def test_bad_arguments_are_refused_and_change_nothing(M):
    from mppi_hip import _lib as L
    H = 7
    eng = _bare(M, MLP_NU, H, sigma=0.5)
    lib = eng.lib
    bad = [(-1, 1), (H + 1, 1), (3, 2), (3, -1), (3, 4), (-3, 0), (H + 1, 7)]
    for state in ("off", "on"):
        if state == "on":
            eng.set_noise_model(sigma_u(MLP_NU), 0.5)
            eng.set_noise_knots(3, 3)
        want_k, want_m = eng.noise_knots(), eng.noise_model()
        for n, order in bad:
            assert lib.mppi_set_noise_knots(eng._h, n, order) == L.MPPI_E_ARG, (n, order)
            assert b"mppi_set_noise_knots" in lib.mppi_last_error()
            got_k, got_m = eng.noise_knots(), eng.noise_model()
            assert got_k[:2] == want_k[:2] and got_m[1:] == want_m[1:] and np.array_equal(got_m[0], want_m[0])
            if state == "on":
                assert np.array_equal(got_k[2], want_k[2]) and np.array_equal(bits(got_k[3]), bits(want_k[3]))
    # enabling on the default law made the model active with the default's values
    fresh = _bare(M, MLP_NU, H, sigma=0.5)
    assert fresh.noise_model()[2] is False
    fresh.set_noise_knots(3, 1)
    s, rho, active = fresh.noise_model()
    assert active is True and rho == 0.0 and np.array_equal(s, np.full(MLP_NU, 0.5, np.float32))
    # (NULL, 0) of mppi_set_noise_model is the default path: refused while a knot law is on, allowed once it is off
    assert lib.mppi_set_noise_model(fresh._h, None, ctypes.c_float(0.0)) == L.MPPI_E_STATE
    assert b"mppi_set_noise_knots" in lib.mppi_last_error()
    assert fresh.noise_knots()[:2] == (3, 1) and fresh.noise_model()[2] is True
    fresh.set_noise_model(None, 0.5)  # every other model keeps the knot law
    assert fresh.noise_knots()[:2] == (3, 1) and fresh.noise_model()[1] == 0.5
    fresh.set_noise_knots(0, 5)  # (0 disables whatever the order)
    fresh.set_noise_model(None, 0.0)
    assert fresh.noise_model()[2] is False and fresh.noise_knots()[0] == 0
    fresh.close()
    eng.close()
    wide = M.Engine(M.Config(nx=4, nu=40, H=2, K=16))  # a knot law is an active model: nu <= 32
    assert wide.lib.mppi_set_noise_knots(wide._h, 1, 1) == L.MPPI_E_UNSUPPORTED
    assert wide.lib.mppi_set_noise_knots(wide._h, 3, 1) == L.MPPI_E_ARG
    assert wide.lib.mppi_set_noise_knots(wide._h, 0, 0) == L.MPPI_OK
    assert wide.noise_model()[2] is False and wide.noise_knots()[0] == 0
    wide.close()


def test_a_change_destroys_graphs_and_keeps_the_key(M):
    """n solves of the AR(1) model, then n under a knot law enabled mid-stream: a loop of plain solves against a graph
    stream whose prefetched noise the change drops.  The value already in effect keeps the graph."""
    import torch
    from mppi_hip import _lib as L
    H, n, seed = 9, 3, 21
    dev = torch.device("cuda")
    outs = []
    for mode in ("loop", "graph"):
        eng, x0, U0 = _setup(M, "cartpole", K, H, B)
        eng.set_noise_model([0.6], 0.8)
        eng.set_stream(torch.cuda.current_stream().cuda_stream)
        tx, tU = torch.from_numpy(x0).to(dev), torch.from_numpy(U0).to(dev)
        tu0 = torch.zeros(B, 1, device=dev)

        def plain():
            for _ in range(n):
                eng.solve_device(B, tx.data_ptr(), tU.data_ptr(), None, seed=seed, u0_ptr=tu0.data_ptr(), shift=True,
                                 env_step=True, seed_counter=True)

        if mode == "loop":
            plain()
            eng.set_noise_knots(3, 1)
            plain()
            plain()
        else:
            eng.graph_capture(B, n, tx.data_ptr(), tU.data_ptr(), tu0.data_ptr(), seed=seed)
            eng.graph_launch(sync=True)  # leaves a prefetched noise of the old law: the device counter is one ahead
            before = eng.get_seed_counter()
            eng.set_noise_knots(3, 1)
            assert eng.get_seed_counter() == before == n  # the same logical key
            with pytest.raises(M.MPPIError) as ei:
                eng.graph_launch(sync=True)
            assert ei.value.code == L.MPPI_E_STATE
            eng.graph_capture(B, n, tx.data_ptr(), tU.data_ptr(), tu0.data_ptr(), seed=seed)
            eng.graph_launch(sync=True)
            eng.set_noise_knots(3, 1)  # the value in effect: the graph and its prefetched noise stay
            assert eng.get_seed_counter() == 2 * n
            eng.graph_launch(sync=True)
        assert eng.get_seed_counter() == 3 * n
        outs.append(_snap(torch, tx, tU, tu0))
        eng.close()
    for a, b in zip(outs[0], outs[1]):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("kind", ["cartpole", "mlp"])
def test_control_cost_and_adaptation_are_refused_in_both_orders(M, kind):
    from mppi_hip import _lib as L
    H, seed = 9, 0xC0FFEE
    eng, x0, U0 = _setup(M, kind, K, H, B)
    nu = eng.config.nu
    lib = eng.lib
    f = ctypes.c_float
    # knots first: the term and the adaptation are refused, the law and the next solve stay
    eng.set_noise_model(sigma_u(nu), 0.9)
    eng.set_noise_knots(3, 3)
    r0 = eng.solve(x0, U0, seed=seed)
    assert lib.mppi_set_control_cost(eng._h, f(0.5)) == L.MPPI_E_UNSUPPORTED
    err = lib.mppi_last_error()
    assert b"mppi_set_control_cost" in err and b"mppi_set_noise_knots" in err
    assert lib.mppi_set_noise_adapt(eng._h, f(0.3), f(1e-3), f(10.0), f(0.95)) == L.MPPI_E_UNSUPPORTED
    err = lib.mppi_last_error()
    assert b"mppi_set_noise_adapt" in err and b"mppi_set_noise_knots" in err
    assert eng.control_cost() == 0.0 and eng.noise_adapt()[0] == 0.0 and eng.noise_knots()[:2] == (3, 3)
    _same(eng.solve(x0, U0, seed=seed), r0)
    assert lib.mppi_set_control_cost(eng._h, f(0.0)) == L.MPPI_OK  # (turning either off is no pair)
    assert lib.mppi_set_noise_adapt(eng._h, f(0.0), f(1e-3), f(10.0), f(0.95)) == L.MPPI_OK
    eng.close()
    # the term first
    eng, _, _ = _setup(M, kind, K, H, B)
    eng.set_noise_model(sigma_u(nu), 0.9)
    eng.set_control_cost(0.5)
    r0 = eng.solve(x0, U0, seed=seed)
    assert lib.mppi_set_noise_knots(eng._h, 3, 3) == L.MPPI_E_UNSUPPORTED
    err = lib.mppi_last_error()
    assert b"mppi_set_noise_knots" in err and b"mppi_set_control_cost" in err
    assert eng.noise_knots()[0] == 0 and eng.control_cost() == 0.5
    _same(eng.solve(x0, U0, seed=seed), r0)
    eng.close()
    # adaptation first (rate 0.3 moves the law behind every solve: the same two solves on a second handle)
    res = []
    for refuse in (False, True):
        eng, _, _ = _setup(M, kind, K, H, B)
        eng.set_noise_model(sigma_u(nu), 0.9)
        eng.set_noise_adapt(0.3)
        first = eng.solve(x0, U0, seed=seed)
        if refuse:
            assert lib.mppi_set_noise_knots(eng._h, 3, 3) == L.MPPI_E_UNSUPPORTED
            err = lib.mppi_last_error()
            assert b"mppi_set_noise_knots" in err and b"mppi_set_noise_adapt" in err
            assert eng.noise_knots()[0] == 0 and eng.noise_adapt()[0] == np.float32(0.3)
        res.append((first, eng.solve(x0, U0, seed=seed)))
        eng.close()
    _same(res[0][0], res[1][0])
    _same(res[0][1], res[1][1])


# ------------------------------------------------------------------------------------------ 10. rank

def test_the_rows_of_a_three_knot_law_have_rank_three(M):
    H, P = 9, 3
    eng = _bare(M, MLP_NU, H)
    eng.set_noise_model(sigma_u(MLP_NU), 0.0)
    eng.set_noise_knots(P, 1)
    eps = eng.noise_eval(B, 5)
    # fp32 as drawn: the default tolerance is then fp32's (S.max * B nu K * 2^-23), above the interpolation's roundings
    rows = np.moveaxis(eps, 2, 0).reshape(H, -1)  # [H, B nu K]
    assert rows.dtype == np.float32 and np.linalg.matrix_rank(rows) == P
    eng.set_noise_knots(0)
    rows = np.moveaxis(eng.noise_eval(B, 5), 2, 0).reshape(H, -1)
    assert np.linalg.matrix_rank(rows) == H
    eng.close()
