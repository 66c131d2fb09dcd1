"""Horizon-basis sampling noise on the device (mppi_set_noise_basis, noise_basis_kernel) against its host restatement
(mppi_hip.noise.basis_filter over the device's own normals, read through mppi_noise_eval), bitwise, and in every stream
form."""
import ctypes

import numpy as np
import pytest

from basis_cases import B, BIG, HS, K, TAIL, TALL, WIDE, basis_counts, bits, sigma_u, sparse_table, table
from test_gpu_noise_model import MLP_NU, MLP_NX, _setup

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def M(gpu_available):
    import mppi_hip
    return mppi_hip


def _bare(M, nu, H, sigma=1.0, Kb=K):
    """an engine that only draws noise (mppi_noise_eval needs no dynamics)"""
    return M.Engine(M.Config(nx=4 if nu == 1 else MLP_NX, nu=nu, H=H, K=Kb, max_batch=B, lambda_=1.0, sigma=sigma,
                             precision=0))


def _same(a, b):
    assert np.array_equal(a.costs, b.costs)
    assert np.array_equal(a.U, b.U)
    assert np.array_equal(a.u0, b.u0)


def _tables(H, R):
    """the tables of one shape: random normals and, where R allows it, the coloured basis of beta = 1"""
    from mppi_hip.noise import colored_basis
    out = [("randn", table(H, R)), ("sparse", sparse_table(H, R))]
    if R == H or R % 2 == 1:
        out.append(("colored", colored_basis(H, 1.0, R)))
    return out


def _check_law(eng, z, seed, H, R, sig):
    from mppi_hip.noise import basis_filter
    for name, A in _tables(H, R):
        eng.set_noise_basis(A)
        back = eng.noise_basis()
        assert back.shape == (H, R) and np.array_equal(bits(back), bits(A))
        got = eng.noise_eval(B, seed)
        want = basis_filter(z, A, sig)
        bad = int(np.count_nonzero(bits(got) != bits(want)))
        print(f"nu {z.shape[1]} H {H} R {R} K {z.shape[3]} {name}: {bad} of {got.size} differ")
        assert bad == 0, (H, R, name)


@pytest.fixture(params=["mfma", "valu"])
def form(request, monkeypatch):
    """Both generators of the law (MPPI_NOISE_BASIS, read per launch): noise_basis_mfma_kernel, the default up to
    H = 128, and noise_basis_kernel, which longer horizons run."""
    if request.param == "valu":
        monkeypatch.setenv("MPPI_NOISE_BASIS", "valu")
    else:
        monkeypatch.delenv("MPPI_NOISE_BASIS", raising=False)
    return request.param


# ------------------------------------------------------------------------------------------ 1. the law, bitwise

@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("nu", [1, MLP_NU])
def test_device_law_equals_basis_filter_bitwise(M, form, nu, H):
    """z = the device's own normals (the default law with cfg.sigma = 1); with a basis law on the same handle the
    generator gives basis_filter(z), bit for bit: R in {1, 2, 3, H}, random and coloured tables, non-uniform sigma_u.
    Then the law is disabled: the rho = 0 model, and the default law again."""
    seed = 0x5EED_0000_0200 + H
    eng = _bare(M, nu, H)
    z = eng.noise_eval(B, seed)
    assert z.shape == (B, nu, H, K) and z.dtype == np.float32 and np.all(np.isfinite(z))
    sig = sigma_u(nu)
    eng.set_noise_model(sig, 0.0)
    for R in basis_counts(H):
        _check_law(eng, z, seed, H, R, sig)
    eng.set_noise_basis(None)
    assert eng.noise_basis() is None
    s, rho, active = eng.noise_model()
    assert active is True and rho == 0.0 and np.array_equal(s, sig)  # sigma_u as it stood
    assert np.array_equal(bits(eng.noise_eval(B, seed)), bits(sig[:, None, None] * z))
    eng.set_noise_model(None, 0.0)
    assert np.array_equal(bits(eng.noise_eval(B, seed)), bits(z))
    assert not np.array_equal(eng.noise_eval(B, seed + 1), z)
    eng.close()


@pytest.mark.parametrize("H,R", list(BIG) + [TAIL, TALL])
def test_device_law_at_the_worst_cases(M, form, H, R):
    """(64, 64): 64 KiB of LDS under noise_basis_kernel's block of 256 k; (128, 128): the same under a block of 128 k,
    the largest law and the MFMA form's 128 accumulators; a horizon whose last tile of steps is stored in part; and one
    past the MFMA form (either value of the knob runs noise_basis_kernel).  After the law an AR(1) model draws as
    before."""
    from mppi_hip.noise import ar1_filter_f32
    seed = 0xB16 + H
    eng = _bare(M, MLP_NU, H)
    z = eng.noise_eval(B, seed)
    sig = sigma_u(MLP_NU)
    eng.set_noise_model(sig, 0.0)
    _check_law(eng, z, seed, H, R, sig)
    eng.set_noise_basis(None)
    eng.set_noise_model(sig, 0.9)
    assert np.array_equal(bits(eng.noise_eval(B, seed)), bits(sig[:, None, None] * ar1_filter_f32(z, 0.9)))
    eng.close()


def test_device_law_with_several_blocks_along_k(M, form):
    """K = 1100 (Kp = 1152: five blocks of 256 k, the last one with two of its four waves past Kp) and B nu = 6 rows."""
    H, R, Kb = WIDE
    seed = 0xB10C
    eng = _bare(M, MLP_NU, H, Kb=Kb)
    z = eng.noise_eval(B, seed)
    sig = sigma_u(MLP_NU)
    eng.set_noise_model(sig, 0.0)
    _check_law(eng, z, seed, H, R, sig)
    eng.close()


# ------------------------------------------------------------------------------------------ 2. identity

@pytest.mark.parametrize("kind", ["cartpole", "mlp"])
def test_the_identity_table_is_the_white_model_bitwise(M, kind):
    """M = I: the solve of set_noise_model(sig, 0), bit for bit; after disabling, the same solve again."""
    H, seed = 7, 0x7171_0000_0004
    ref, x0, U0 = _setup(M, kind, K, H, B)
    sig = sigma_u(ref.config.nu)
    ref.set_noise_model(sig, 0.0)
    r0 = ref.solve(x0, U0, seed=seed)
    eng, _, _ = _setup(M, kind, K, H, B)
    eng.set_noise_model(sig, 0.0)
    eng.set_noise_basis(np.eye(H, dtype=np.float32))
    assert np.array_equal(eng.noise_basis(), np.eye(H, dtype=np.float32))
    _same(eng.solve(x0, U0, seed=seed), r0)
    eng.set_noise_basis(table(H, 2))  # (another law in between: other costs)
    assert not np.array_equal(eng.solve(x0, U0, seed=seed).costs, r0.costs)
    eng.set_noise_basis(None)
    s, r, active = eng.noise_model()
    assert active is True and r == 0.0 and np.array_equal(s, sig)
    _same(eng.solve(x0, U0, seed=seed), r0)
    ref.close()
    eng.close()


# ------------------------------------------------------------------------------------------ 3. injected == device

@pytest.mark.parametrize("kind", ["cartpole", "mlp"])
def test_injected_noise_eval_equals_the_device_solve(M, kind):
    H, R, seed = 9, 3, 0xD00D_0000_0012
    eng, x0, U0 = _setup(M, kind, K, H, B)
    eng.set_noise_model(sigma_u(eng.config.nu), 0.0)
    eng.set_noise_basis(table(H, R))
    r1 = eng.solve(x0, U0, seed=seed, want_weights=True)
    noise = eng.noise_eval(B, seed)
    inj, _, _ = _setup(M, kind, K, H, B)
    r2 = inj.solve(x0, U0, noise=noise, want_weights=True)
    _same(r1, r2)
    assert np.array_equal(r1.weights, r2.weights)
    assert np.array_equal(eng.solve(x0, U0, seed=seed).costs, r1.costs)  # the evaluation left the handle as it was
    eng.close()
    inj.close()


# ------------------------------------------------------------------------------------------ 4. stream forms

def _snap(torch, *ts):
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in ts)


@pytest.mark.parametrize("extras", [False, True], ids=["basis", "basis+bounds+keep"])
@pytest.mark.parametrize("kind", ["cartpole", "mlp"])
def test_stream_forms_agree_bitwise(M, kind, extras):
    """n = 3 solves with SHIFT and ENV_STEP as plain counter solves, chained solves, one captured graph and the
    trajectory-logging capture: x, U, u0, the last solve's costs and the seed counter, bit for bit; once more with
    control bounds and n_keep = 4 on (the passes behind the generator)."""
    import torch
    from mppi_hip.noise import colored_basis
    H, n, seed = 9, 3, 78
    A = colored_basis(H, 1.0, 5)
    dev = torch.device("cuda")
    outs = {}
    for mode in ("plain", "chain", "graph", "traj", "no_basis"):
        eng, x0, U0 = _setup(M, kind, K, H, B)
        nu = eng.config.nu
        eng.set_noise_model(sigma_u(nu), 0.0)
        if mode != "no_basis":
            eng.set_noise_basis(A)
        if extras:
            eng.set_control_bounds(-0.3, 0.4)
            eng.set_elite_keep(4)
        eng.set_stream(torch.cuda.current_stream().cuda_stream)
        tx, tU = torch.from_numpy(x0).to(dev), torch.from_numpy(U0).to(dev)
        tu0, tc = torch.zeros(B, nu, device=dev), torch.zeros(B, K, device=dev)
        if mode in ("plain", "chain", "no_basis"):
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
    assert not np.array_equal(outs["no_basis"][1], outs["plain"][1])  # the basis law is in effect in the stream


# ------------------------------------------------------------------------------------------ 5. the setter's contract

def test_a_change_destroys_graphs_and_keeps_the_key(M):
    """n solves of the white model, then n under a basis law enabled mid-stream: a loop of plain solves against a graph
    stream whose prefetched noise the change drops.  The table already in effect keeps the graph."""
    import torch
    from mppi_hip import _lib as L
    H, n, seed = 9, 3, 22
    A = table(H, 3)
    dev = torch.device("cuda")
    outs = []
    for mode in ("loop", "graph"):
        eng, x0, U0 = _setup(M, "cartpole", K, H, B)
        eng.set_noise_model([0.6], 0.0)
        eng.set_stream(torch.cuda.current_stream().cuda_stream)
        tx, tU = torch.from_numpy(x0).to(dev), torch.from_numpy(U0).to(dev)
        tu0 = torch.zeros(B, 1, device=dev)

        def plain():
            for _ in range(n):
                eng.solve_device(B, tx.data_ptr(), tU.data_ptr(), None, seed=seed, u0_ptr=tu0.data_ptr(), shift=True,
                                 env_step=True, seed_counter=True)

        if mode == "loop":
            plain()
            eng.set_noise_basis(A)
            plain()
            plain()
        else:
            eng.graph_capture(B, n, tx.data_ptr(), tU.data_ptr(), tu0.data_ptr(), seed=seed)
            eng.graph_launch(sync=True)  # leaves a prefetched noise of the old law: the device counter is one ahead
            before = eng.get_seed_counter()
            eng.set_noise_basis(A)
            assert eng.get_seed_counter() == before == n  # the same logical key
            with pytest.raises(M.MPPIError) as ei:
                eng.graph_launch(sync=True)
            assert ei.value.code == L.MPPI_E_STATE
            eng.graph_capture(B, n, tx.data_ptr(), tU.data_ptr(), tu0.data_ptr(), seed=seed)
            eng.graph_launch(sync=True)
            eng.set_noise_basis(A.copy())  # the table in effect: the graph and its prefetched noise stay
            assert eng.get_seed_counter() == 2 * n
            eng.graph_launch(sync=True)
        assert eng.get_seed_counter() == 3 * n
        outs.append(_snap(torch, tx, tU, tu0))
        eng.close()
    for a, b in zip(outs[0], outs[1]):
        np.testing.assert_array_equal(a, b)


def test_bad_arguments_are_refused_and_change_nothing(M):
    from mppi_hip import _lib as L
    H = 7
    eng = _bare(M, MLP_NU, H, sigma=0.5)
    lib = eng.lib
    ok = table(H, H + 1)  # (room for every R tried)
    ptr = ok.ctypes.data_as(ctypes.c_void_p)
    nan, inf = table(H, 3), table(H, 3)
    nan[4, 1], inf[6, 2] = np.nan, -np.inf
    bad = [(-1, ptr), (H + 1, ptr), (3, None), (3, nan.ctypes.data_as(ctypes.c_void_p)),
           (3, inf.ctypes.data_as(ctypes.c_void_p)), (200, ptr)]
    for state in ("off", "on"):
        if state == "on":
            eng.set_noise_model(sigma_u(MLP_NU), 0.0)
            eng.set_noise_basis(table(H, 3, seed=1))
        want_b, want_m = eng.noise_basis(), eng.noise_model()
        for n, p in bad:
            assert lib.mppi_set_noise_basis(eng._h, n, p) == L.MPPI_E_ARG, n
            assert b"mppi_set_noise_basis" in lib.mppi_last_error()
            got_b, got_m = eng.noise_basis(), eng.noise_model()
            assert got_m[1:] == want_m[1:] and np.array_equal(got_m[0], want_m[0])
            if state == "on":
                assert np.array_equal(bits(got_b), bits(want_b))  # bitwise as set
            else:
                assert got_b is None
    assert np.array_equal(bits(want_b), bits(table(H, 3, seed=1)))
    # enabling on the default law made the model active with the default's values
    fresh = _bare(M, MLP_NU, H, sigma=0.5)
    assert fresh.noise_model()[2] is False
    fresh.set_noise_basis(table(H, 3))
    s, rho, active = fresh.noise_model()
    assert active is True and rho == 0.0 and np.array_equal(s, np.full(MLP_NU, 0.5, np.float32))
    # (NULL, 0) of mppi_set_noise_model is the default path: refused while a basis is on, allowed once it is off
    assert lib.mppi_set_noise_model(fresh._h, None, ctypes.c_float(0.0)) == L.MPPI_E_STATE
    assert b"mppi_set_noise_basis" in lib.mppi_last_error()
    assert fresh.noise_basis() is not None and fresh.noise_model()[2] is True
    fresh.set_noise_model(sigma_u(MLP_NU), 0.0)  # new scales keep the basis
    assert np.array_equal(bits(fresh.noise_basis()), bits(table(H, 3)))
    assert np.array_equal(fresh.noise_model()[0], sigma_u(MLP_NU))
    assert lib.mppi_set_noise_basis(fresh._h, 0, None) == L.MPPI_OK  # (0 disables whatever M)
    fresh.set_noise_model(None, 0.0)
    assert fresh.noise_model()[2] is False and fresh.noise_basis() is None
    fresh.close()
    eng.close()
    # n_basis > 128 with H to match: not built
    big = _bare(M, 1, 130)
    A = table(130, 129)
    assert big.lib.mppi_set_noise_basis(big._h, 129, A.ctypes.data_as(ctypes.c_void_p)) == L.MPPI_E_UNSUPPORTED
    assert b"mppi_set_noise_basis" in big.lib.mppi_last_error()
    assert big.noise_basis() is None and big.noise_model()[2] is False
    big.close()
    wide = M.Engine(M.Config(nx=4, nu=40, H=2, K=16))  # a basis law is an active model: nu <= 32
    A = table(2, 1)
    assert wide.lib.mppi_set_noise_basis(wide._h, 1, A.ctypes.data_as(ctypes.c_void_p)) == L.MPPI_E_UNSUPPORTED
    assert wide.lib.mppi_set_noise_basis(wide._h, 3, A.ctypes.data_as(ctypes.c_void_p)) == L.MPPI_E_ARG
    assert wide.lib.mppi_set_noise_basis(wide._h, 0, None) == L.MPPI_OK
    assert wide.noise_model()[2] is False and wide.noise_basis() is None
    wide.close()


def _pairs(eng, sig):
    """(name, the other setter as a raw call returning its status, how to read that it is off)"""
    lib, h, f = eng.lib, eng._h, ctypes.c_float
    nu = eng.config.nu
    S = (np.diag(sig.astype(np.float64) ** 2) + 0.01).astype(np.float32)
    S = ((S + S.T) / 2).astype(np.float32)
    sp = sig.ctypes.data_as(ctypes.POINTER(f))
    return [
        ("mppi_set_noise_model", lambda: lib.mppi_set_noise_model(h, sp, f(0.5)), lambda: eng.noise_model()[1] == 0.0),
        ("mppi_set_noise_knots", lambda: lib.mppi_set_noise_knots(h, 3, 1), lambda: eng.noise_knots()[0] == 0),
        ("mppi_set_noise_cov", lambda: lib.mppi_set_noise_cov(h, S.ctypes.data_as(ctypes.c_void_p)),
         lambda: eng.noise_cov() is None),
        ("mppi_set_noise_cov_adapt", lambda: lib.mppi_set_noise_cov_adapt(h, f(0.3), f(1e-3), f(10.0)),
         lambda: eng.noise_cov_adapt()[0] == 0.0),
        ("mppi_set_noise_adapt", lambda: lib.mppi_set_noise_adapt(h, f(0.3), f(1e-3), f(10.0), f(0.95)),
         lambda: eng.noise_adapt()[0] == 0.0),
        ("mppi_set_control_cost", lambda: lib.mppi_set_control_cost(h, f(0.5)), lambda: eng.control_cost() == 0.0),
    ]


@pytest.mark.parametrize("kind", ["cartpole", "mlp"])
def test_every_refused_pair_in_both_orders(M, kind):
    from mppi_hip import _lib as L
    H, seed = 9, 0xC0FFEE
    A = table(H, 3)
    ap = A.ctypes.data_as(ctypes.c_void_p)
    # the basis first: every other setter is refused, the law and the next solve stay
    eng, x0, U0 = _setup(M, kind, K, H, B)
    sig = sigma_u(eng.config.nu)
    eng.set_noise_model(sig, 0.0)
    eng.set_noise_basis(A)
    r0 = eng.solve(x0, U0, seed=seed)
    for name, call, is_off in _pairs(eng, sig):
        assert call() == L.MPPI_E_UNSUPPORTED, name
        err = eng.lib.mppi_last_error()
        assert name.encode() in err and b"mppi_set_noise_basis" in err, err
        assert is_off() and np.array_equal(bits(eng.noise_basis()), bits(A)), name
        _same(eng.solve(x0, U0, seed=seed), r0)
    eng.close()
    # the other first (mppi_set_noise_cov_adapt needs its covariance, which then is the pair)
    for name, call, _ in _pairs(eng, sig):
        res = []
        for refuse in (False, True):
            eng, _, _ = _setup(M, kind, K, H, B)
            if name not in ("mppi_set_noise_cov", "mppi_set_noise_cov_adapt"):
                eng.set_noise_model(sig, 0.0)
            pairs = dict((p[0], p[1]) for p in _pairs(eng, sig))
            if name == "mppi_set_noise_cov_adapt":
                assert pairs["mppi_set_noise_cov"]() == L.MPPI_OK
            assert pairs[name]() == L.MPPI_OK, name
            first = eng.solve(x0, U0, seed=seed)
            if refuse:
                assert eng.lib.mppi_set_noise_basis(eng._h, 3, ap) == L.MPPI_E_UNSUPPORTED, name
                err = eng.lib.mppi_last_error()
                assert b"mppi_set_noise_basis" in err and name.encode() in err, err
                assert eng.noise_basis() is None
            res.append((first, eng.solve(x0, U0, seed=seed)))
            eng.close()
        _same(res[0][0], res[1][0])
        _same(res[0][1], res[1][1])


# ------------------------------------------------------------------------------------------ 6. rank

def test_the_rows_of_a_three_column_law_have_rank_three(M):
    H, R = 9, 3
    eng = _bare(M, MLP_NU, H)
    eng.set_noise_model(sigma_u(MLP_NU), 0.0)
    eng.set_noise_basis(table(H, R))
    eps = eng.noise_eval(B, 5)
    # fp32 as drawn: the default tolerance is then fp32's (S.max * B nu K * 2^-23), above the mix's roundings
    rows = np.moveaxis(eps, 2, 0).reshape(H, -1)  # [H, B nu K]
    assert rows.dtype == np.float32 and np.linalg.matrix_rank(rows) == R
    eng.set_noise_basis(None)
    rows = np.moveaxis(eng.noise_eval(B, 5), 2, 0).reshape(H, -1)
    assert np.linalg.matrix_rank(rows) == H
    eng.close()
