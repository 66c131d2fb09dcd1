"""The weighted cross moments on the device (MPPI_FLAG_CROSS, mppi_get_cross_moments, mppi_cross_moments_eval;
csrc/kernels_cross.hip) against the cell scheme's numpy restatement mppi_hip.stats.cross_moments_f32 (bitwise) and the
float64 statement cross_moments_ref, in both forms of the kernel, in every solve form, and bit for bit beside the same
solves without the flag."""
import ctypes

import numpy as np
import pytest

from cross_cases import B, FORMS, SHAPES, bits, case, exact_case, exact_want, shape_id

pytestmark = pytest.mark.gpu

MLP_NX, MLP_NU = 10, 3


@pytest.fixture(scope="module")
def M(gpu_available):
    import mppi_hip
    return mppi_hip


def _bare(M, nu, H, K, Bn=B, **kw):
    """An engine with nothing loaded: all mppi_cross_moments_eval needs."""
    return M.Engine(M.Config(nx=4, nu=nu, H=H, K=K, max_batch=Bn, lambda_=1.0, norm_eps=0.0, **kw))


def _mlp(M, K, H, Bn):
    """(engine, x0, U0): a seeded MLP (nu = 3, fp32, quad_est), as tests/test_gpu_noise_adapt.py"""
    from mppi_hip.nets import mlp_blob, synthetic_mlp
    rs = np.random.RandomState(11)
    eng = M.Engine(M.Config(nx=MLP_NX, nu=MLP_NU, H=H, K=K, max_batch=Bn, lambda_=1.0, sigma=0.5, precision=0))
    eng.load_dynamics(*mlp_blob(synthetic_mlp(MLP_NX, MLP_NU, seed=0), MLP_NX, MLP_NU))
    eng.set_cost("quad_est")
    return eng, (0.3 * rs.randn(Bn, MLP_NX)).astype(np.float32), (0.1 * rs.randn(Bn, MLP_NU, H)).astype(np.float32)


def _set_form(monkeypatch, form):
    if form is None:
        monkeypatch.delenv("MPPI_CROSS_FORM", raising=False)
    else:
        monkeypatch.setenv("MPPI_CROSS_FORM", form)


# ------------------------------------------------------------------------------------------ 1. mppi_cross_moments_eval

@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_eval_equals_the_cell_scheme_bitwise_in_every_form(M, shape, monkeypatch):
    """Costs whose device weights are known to the bit (cross_cases.exact_case): every MPPI_CROSS_FORM gives
    cross_moments_f32 bit for bit, a symmetric matrix, the diagonal of mppi_stats_eval's eps_m2, and the same again
    on a repeat.  Then random costs (weights through the device's __expf): the forms agree bit for bit with each
    other, the diagonal is eps_m2, and the float64 bar |got - ref| <= 1e-4 A + 1e-6 holds (printed with the achieved
    error; A = 1/H sum w |e_u e_v|)."""
    from mppi_hip.stats import cross_moments_ref
    nu, H, K = shape
    costs_x, _, noise = exact_case(*shape)
    costs_r, _ = case(*shape)
    want = exact_want(*shape)
    ref, A = cross_moments_ref(costs_r, noise), cross_moments_ref(costs_r, noise, absolute=True)
    eng = _bare(M, nu, H, K)
    rand = {}
    for form in FORMS + ("again",):
        _set_form(monkeypatch, None if form == "again" else form)
        got = eng.cross_moments_eval(costs_x, noise)
        assert np.array_equal(bits(got), bits(want)), form
        assert np.array_equal(bits(got), bits(got.transpose(0, 2, 1))), form
        m2 = eng.stats_eval(costs_x, noise)["eps_m2"]
        assert np.array_equal(bits(np.diagonal(got, axis1=1, axis2=2)), bits(m2)), form
        rand[form] = eng.cross_moments_eval(costs_r, noise)
        assert np.array_equal(bits(rand[form]), bits(rand[FORMS[0]])), form
        m2 = eng.stats_eval(costs_r, noise)["eps_m2"]
        assert np.array_equal(bits(np.diagonal(rand[form], axis1=1, axis2=2)), bits(m2)), form
        ratio = float((np.abs(rand[form] - ref) / (1e-4 * A + 1e-6)).max())
        print(shape, form, "max |got - ref| / (1e-4 A + 1e-6) =", ratio, "max |got - ref| =",
              float(np.abs(rand[form] - ref).max()))
        assert ratio <= 1.0, form
    eng.close()


def test_eval_honours_lambda_and_norm_eps_and_one_solve_of_a_larger_handle(M):
    from mppi_hip.stats import cross_moments_ref
    nu, H, K = 3, 7, 130
    costs, noise = case(nu, H, K)
    eng = M.Engine(M.Config(nx=4, nu=nu, H=H, K=K, max_batch=5, lambda_=7.5, norm_eps=0.25))
    got = eng.cross_moments_eval(costs, noise)
    ref, A = cross_moments_ref(costs, noise, 7.5, 0.25), cross_moments_ref(costs, noise, 7.5, 0.25, absolute=True)
    assert np.all(np.abs(got - ref) <= 1e-4 * A + 1e-6)
    one = eng.cross_moments_eval(costs[1], noise[1:2])  # B = 1 of max_batch = 5
    assert np.array_equal(bits(one[0]), bits(got[1]))
    eng.close()


# ------------------------------------------------------------------------------------------ 2. a solve with the flag

def test_flagged_solve_equals_eval_and_changes_nothing(M, monkeypatch):
    """Injected noise: the cross moments of the solve are mppi_cross_moments_eval of its returned costs and that noise
    (the evaluation has its own slot: the solve's stay readable), the statistics are those of stats=True, and U, u0,
    costs and weights are bitwise those of the same solve without the flag, which launches no cross kernel."""
    K, H, Bn = 150, 9, 2
    eng, x0, U0 = _mlp(M, K, H, Bn)
    noise = (0.5 * np.random.RandomState(5).randn(Bn, MLP_NU, H, K)).astype(np.float32)
    eng.profile(True)
    r1 = eng.solve(x0, U0, noise=noise, want_weights=True, shift=True, cross=True)
    assert eng.kernel_time("cross")[0] == 1 and eng.kernel_time("stats")[0] == 1
    mx = r1.stats["eps_mx"]
    assert mx.shape == (Bn, MLP_NU, MLP_NU)
    assert np.array_equal(bits(mx), bits(eng.cross_moments(Bn)))
    assert np.array_equal(bits(np.diagonal(mx, axis1=1, axis2=2)), bits(r1.stats["eps_m2"]))
    ev = eng.cross_moments_eval(r1.costs, noise)
    assert np.array_equal(bits(ev), bits(mx))
    assert np.array_equal(bits(eng.cross_moments(Bn)), bits(mx))
    r2 = eng.solve(x0, U0, noise=noise, want_weights=True, shift=True, stats=True)  # the flag alone: as before
    assert eng.kernel_time("cross")[0] == 2 and eng.kernel_time("stats")[0] == 3  # (the eval's pair, no third cross)
    eng.profile(False)
    assert "eps_mx" not in r2.stats
    for k, v in r2.stats.items():
        assert np.array_equal(r1.stats[k], v), k
    ref, _, _ = _mlp(M, K, H, Bn)
    r0 = ref.solve(x0, U0, noise=noise, want_weights=True, shift=True)
    for n in ("U", "u0", "costs", "weights"):
        np.testing.assert_array_equal(getattr(r1, n), getattr(r0, n), err_msg=n)
    eng.close()
    ref.close()


# ------------------------------------------------------------------------------------------ 3. streams

def _snap(torch, *ts):
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in ts)


def test_stream_forms_give_the_plain_solves_cross_moments(M):
    """Three plain counter solves, three chained solves, a three-solve graph and a trajectory-logging graph
    (SHIFT | ENV_STEP), with the flag: per step the same eps_mx bit for bit; the x0, U, u0 sequences and the costs are
    bitwise those of the same streams without the flag; the seed counters agree."""
    import torch
    K, H, Bn, n, seed = 128, 8, 2, 3, 9
    dev = torch.device("cuda")
    mxs, seqs, ctrs = {}, {}, {}
    for mode in ("plain", "chain", "graph", "traj"):
        for flag in (True, False):
            eng, x0, U0 = _mlp(M, K, H, Bn)
            eng.set_stream(torch.cuda.current_stream().cuda_stream)
            tx, tU = torch.from_numpy(x0).to(dev), torch.from_numpy(U0).to(dev)
            tu0, tc = torch.zeros(Bn, MLP_NU, device=dev), torch.zeros(Bn, K, device=dev)
            mx, seq = [], []
            if mode in ("graph", "traj"):
                trx, tru = torch.zeros(n, Bn, MLP_NX, device=dev), torch.zeros(n, Bn, MLP_NU, device=dev)
                eng.graph_capture_traj(Bn, n, tx.data_ptr(), tU.data_ptr(), tu0.data_ptr(), costs_ptr=tc.data_ptr(),
                                       seed=seed, cross=flag, traj_x_ptr=trx.data_ptr() if mode == "traj" else None,
                                       traj_u_ptr=tru.data_ptr() if mode == "traj" else None)
                eng.graph_launch(sync=True)
                seq.append(_snap(torch, tx, tU, tu0, tc))
                if flag:
                    mx = [eng.cross_moments(Bn, step=i) for i in range(n)]
            else:
                for _ in range(n):
                    eng.solve_device(Bn, tx.data_ptr(), tU.data_ptr(), None, seed=seed, u0_ptr=tu0.data_ptr(),
                                     costs_ptr=tc.data_ptr(), shift=True, env_step=True, seed_counter=mode == "plain",
                                     chain=mode == "chain", cross=flag)
                    seq.append(_snap(torch, tx, tU, tu0, tc))
                    if flag:
                        mx.append(eng.cross_moments(Bn))
            ctrs[mode, flag] = eng.get_seed_counter()
            mxs[mode, flag], seqs[mode, flag] = mx, seq
            eng.close()
    assert set(ctrs.values()) == {n}
    for mode in ("chain", "graph", "traj"):
        assert len(mxs[mode, True]) == n
        for got, want in zip(mxs[mode, True], mxs["plain", True]):
            assert np.array_equal(bits(got), bits(want)), mode
    for mode in ("plain", "chain", "graph", "traj"):
        for got, want in zip(seqs[mode, True], seqs[mode, False]):
            for a, b in zip(got, want):
                np.testing.assert_array_equal(a, b, err_msg=mode)
    for mode in ("graph", "traj"):  # (and the streams are the plain loop)
        for a, b in zip(seqs[mode, True][-1], seqs["plain", True][-1]):
            np.testing.assert_array_equal(a, b, err_msg=mode)
    steps = mxs["plain", True]
    assert not np.array_equal(steps[0], steps[1])  # the slots hold different solves
    assert np.all(np.abs(steps[0][:, 1, 0]) > 0.0)


# ------------------------------------------------------------------------------------------ 4. errors

def test_get_cross_moments_errors(M):
    from mppi_hip import _lib as L
    K, H, Bn = 128, 8, 2
    eng, x0, U0 = _mlp(M, K, H, 3)
    lib = eng.lib
    buf = np.zeros((3, MLP_NU, MLP_NU), np.float32)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    eng.solve(x0[:Bn], U0[:Bn], seed=1, stats=True)  # the statistics alone carry no cross moments
    assert lib.mppi_get_cross_moments(eng._h, Bn, 0, p) == L.MPPI_E_STATE
    assert b"mppi_get_cross_moments" in lib.mppi_last_error()
    eng.cross_moments_eval(np.ones((Bn, K), np.float32), np.ones((Bn, MLP_NU, H, K), np.float32))
    assert lib.mppi_get_cross_moments(eng._h, Bn, 0, p) == L.MPPI_E_STATE  # ... nor does an evaluation
    eng.solve(x0[:Bn], U0[:Bn], seed=1, cross=True)
    assert lib.mppi_get_cross_moments(eng._h, Bn, 0, p) == L.MPPI_OK
    assert lib.mppi_get_cross_moments(eng._h, Bn, 0, None) == L.MPPI_E_ARG
    for B_bad, step_bad in ((3, 0), (0, 0), (Bn, 1), (Bn, -1)):
        assert lib.mppi_get_cross_moments(eng._h, B_bad, step_bad, p) == L.MPPI_E_ARG, (B_bad, step_bad)
    c = np.ones((Bn, K), np.float32).ctypes.data_as(ctypes.c_void_p)
    for args in ((0, c, c, p), (4, c, c, p), (Bn, None, c, p), (Bn, c, None, p), (Bn, c, c, None)):
        assert lib.mppi_cross_moments_eval(eng._h, *args) == L.MPPI_E_ARG, args
        assert b"mppi_cross_moments_eval" in lib.mppi_last_error()
    eng.close()
    wide = _bare(M, 33, 2, 16, Bn=1)  # nu <= 32
    n = np.ones((1, 33, 2, 16), np.float32)
    out = np.zeros((1, 33, 33), np.float32)
    assert lib.mppi_cross_moments_eval(wide._h, 1, n.ctypes.data_as(ctypes.c_void_p), n.ctypes.data_as(ctypes.c_void_p),
                                       out.ctypes.data_as(ctypes.c_void_p)) == L.MPPI_E_UNSUPPORTED
    assert wide.stats_eval(np.ones((1, 16), np.float32), n)["eps_m2"].shape == (1, 33)  # the statistics have no limit
    wide.close()
