"""Keep / shift elites on the device (mppi_set_elite_keep): the gather and inject kernels against the numpy references,
exactly; the first solve bit for bit the solve without the feature; the exactness of the whole flow (a second solve
equals a keep-off solve fed the reference's injected noise), alone and composed with shift, bounds, the clamp, the cost
terms, ESS targeting and elites; every stream form against a loop of plain solves; save / restore; seeding; the best
cost never getting worse; and the state rules of the six entries."""
import ctypes

import numpy as np
import pytest

from elite_cases import FAMILIES, family
from keep_cases import hand_cases, hand_inject_cases, inputs, same_bits
from test_gpu_elites import FRAC, LIMITS, MLP_NU, MLP_NX, _setup, _snap

pytestmark = pytest.mark.gpu

K0, B0 = 130, 2            # Kp pads (192), and more than two 64-lane strides at n_keep = 130
N_KEEPS = (1, 17, 70, K0)  # not multiples of 4 or 64


@pytest.fixture(scope="module")
def M(gpu_available):
    import mppi_hip
    return mppi_hip


def _same(a, b, msg=""):
    assert same_bits(a, b), (msg, a, b)


def _same_kept(got, want, msg=""):
    """(v, kcost, idx, count, steps) exactly: bitwise v / kcost, integer idx / count / steps."""
    _same(got[0], want[0], (msg, "v"))
    _same(got[1], want[1], (msg, "kcost"))
    for name, g, w in zip(("idx", "count", "steps"), got[2:], want[2:]):
        assert np.array_equal(g, w), (msg, name, g, w)


def _unfuse(eng, kind):
    """The cartpole is compared in its unfused form on both sides (ESS targeting pinned to cfg.lambda), as
    tests/test_gpu_elites.py does: its fused one-launch form differs from reduce_kernel in the last bits."""
    if kind == "cartpole":
        eng.set_ess_target(FRAC, eng.config.lambda_, eng.config.lambda_)


# ------------------------------------------------------------------------------------------ 1. the store kernels

@pytest.mark.parametrize("rows", ["", "2", "8"], ids=["rows-auto", "rows-2", "rows-8"])
@pytest.mark.parametrize("H", [1, 8])
def test_keep_store_eval_equals_the_reference_exactly(M, monkeypatch, H, rows):
    """No rollout: keep_store_eval on the cost families of elite_cases.py x n_keep x both shifts, with and without the
    clamp, B = 2 with rows that differ; every rows-per-wave form of the gather (tiles that end inside and beyond a
    solve's rows), one to three 64-column strides.  v, kcost bit for bit, idx, count, steps as integers; two calls
    bitwise equal."""
    from mppi_hip.stats import keep_store_ref
    if rows:
        monkeypatch.setenv("MPPI_KEEP_ROWS", rows)
    for clamp in (0.0, 1.25):
        eng = M.Engine(M.Config(nx=4, nu=3, H=H, K=K0, max_batch=B0, ctrl_clamp=clamp))
        U, eps = inputs(B0, 3, H, K0, seed=H)
        for n_keep in N_KEEPS:
            eng.set_elite_keep(n_keep)
            assert eng.elite_keep() == n_keep
            for name in FAMILIES:
                c = family(name, K0)
                for shift in (False, True):
                    got = eng.keep_store_eval(U, eps, c, shift=shift)
                    _same_kept(got, keep_store_ref(U, eps, c, n_keep, shift=shift, ctrl_clamp=clamp),
                               (name, n_keep, shift, clamp))
            _same_kept(eng.keep_store_eval(U, eps, c, shift=True), got, "two calls")
        # a row without a finite cost: an empty set beside a full one; a non-finite noise entry is carried as it is
        c = family("gauss", K0)
        c[0] = np.nan
        e2 = eps.copy()
        e2[1, 0, 0, int(np.argmin(c[1]))] = np.inf
        got = eng.keep_store_eval(U, e2, c)
        _same_kept(got, keep_store_ref(U, e2, c, N_KEEPS[-1], ctrl_clamp=clamp), "no finite cost / inf noise")
        assert got[3].tolist() == [0, K0] and not got[0][0].any() and np.all(got[2][0] == -1)
        eng.close()


def test_keep_store_eval_on_the_selections_large_form(M):
    """K = 4100: elite_select_kernel's large form feeds the gather (Kp = 4160, 65 strides of 64 lanes at n_keep = K)."""
    from mppi_hip.stats import keep_store_ref
    K, H = 4100, 8
    eng = M.Engine(M.Config(nx=4, nu=3, H=H, K=K, max_batch=B0))
    U, eps = inputs(B0, 3, H, K)
    c = family("quantised", K)
    c[1, 7] = np.nan
    for n_keep in (70, K):
        eng.set_elite_keep(n_keep)
        _same_kept(eng.keep_store_eval(U, eps, c, shift=True), keep_store_ref(U, eps, c, n_keep, shift=True), n_keep)
    eng.close()


def test_keep_evals_on_the_hand_written_rows(M):
    from mppi_hip.stats import keep_inject_ref
    for name, U, eps, costs, n_keep, shift, clamp, v, kcost, idx, count, steps in hand_cases():
        eps = np.array(eps, np.float32)
        eng = M.Engine(M.Config(nx=4, nu=1, H=eps.shape[1], K=eps.shape[2], max_batch=2, ctrl_clamp=clamp))
        eng.set_elite_keep(n_keep)
        got = eng.keep_store_eval(np.array([U], np.float32), eps[None], np.array([costs], np.float32), shift=bool(shift))
        want = (np.array([v], np.float32), np.array([kcost], np.float32), np.array([idx], np.int32),
                np.array([count], np.int32), np.array([steps], np.int32))
        assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), name  # (-0.0 and +0.0 told apart)
        _same_kept(got, want, name)
        eng.close()
    for name, U, eps, v, count, steps, out in hand_inject_cases():
        eps = np.array(eps, np.float32)
        eng = M.Engine(M.Config(nx=4, nu=1, H=eps.shape[1], K=eps.shape[2], max_batch=2))
        eng.set_elite_keep(2)
        got = eng.keep_inject_eval(np.array([U], np.float32), eps[None], np.array([v], np.float32), [count], [steps])
        _same(got[0], np.array(out, np.float32), name)
        eng.close()


# ------------------------------------------------------------------------------------------ 2. the inject kernel

@pytest.mark.parametrize("rows", ["", "2", "8"], ids=["rows-auto", "rows-2", "rows-8"])
@pytest.mark.parametrize("H", [1, 8])
def test_keep_inject_eval_equals_the_reference_exactly(M, monkeypatch, H, rows):
    """keep_inject_eval against keep_inject_ref: count 0, steps 0, count = n_keep, ragged counts inside a 16-B quad and
    across 64-lane strides, per-b values that differ; columns >= count and rows >= steps come out bit for bit (NaN and
    infinities among them)."""
    from mppi_hip.stats import keep_inject_ref
    if rows:
        monkeypatch.setenv("MPPI_KEEP_ROWS", rows)
    eng = M.Engine(M.Config(nx=4, nu=3, H=H, K=K0, max_batch=B0))
    U, eps = inputs(B0, 3, H, K0, seed=20 + H)
    eps[0, 1, 0, 3], eps[1, 2, H - 1, 69], eps[0, 0, 0, K0 - 1] = np.nan, np.inf, -np.inf
    for n_keep in N_KEEPS:
        eng.set_elite_keep(n_keep)
        v = inputs(B0, 3, H, n_keep, seed=40)[1]
        counts = sorted({0, 1, n_keep // 2, max(n_keep - 1, 0), n_keep})
        for ca in counts:
            for cb in (counts[-1], counts[0]):
                for steps in ([H, H], [H - 1, 0], [0, H]):
                    got = eng.keep_inject_eval(U, eps, v, [ca, cb], steps)
                    _same(got, keep_inject_ref(U, eps, v, [ca, cb], steps), (n_keep, ca, cb, steps))
    eng.close()


# ------------------------------------------------------------------------------------------ 3. the first solve

@pytest.mark.parametrize("kind", ["cartpole", "mlp"])
def test_the_first_solve_is_the_solve_without_the_feature(M, kind):
    """costs, weights, U, u0 and the seed counter of the first solve with the feature on (device noise, seed counter)
    are bit for bit those without it: the inject kernel runs on an empty set."""
    import torch
    K, H, B, seed = K0, 8, B0, 5
    dev = torch.device("cuda")
    outs = []
    for n_keep in (0, 17):
        eng, x0, U0 = _setup(M, kind, K, H, B)
        _unfuse(eng, kind)
        eng.set_elite_keep(n_keep)
        eng.set_stream(torch.cuda.current_stream().cuda_stream)
        tx, tU = torch.from_numpy(x0).to(dev), torch.from_numpy(U0).to(dev)
        tu0, tc, tw = (torch.zeros(B, U0.shape[1], device=dev), torch.zeros(B, K, device=dev),
                       torch.zeros(B, K, device=dev))
        eng.solve_device(B, tx.data_ptr(), tU.data_ptr(), None, seed=seed, u0_ptr=tu0.data_ptr(),
                         costs_ptr=tc.data_ptr(), weights_ptr=tw.data_ptr(), shift=True, seed_counter=True)
        outs.append(_snap(torch, tU, tu0, tc, tw) + (eng.get_seed_counter(),))
        if n_keep:
            assert eng.kept(B)[3].tolist() == [n_keep] * B  # ... and it stored its own
        eng.close()
    for a, b, name in zip(outs[0][:4], outs[1][:4], ("U", "u0", "costs", "weights")):
        _same(a, b, name)
    assert outs[0][4] == outs[1][4] == 1


# ------------------------------------------------------------------------------------------ 4, 5. the whole flow

def _flow(M, kind, n_keep, H=8, shift=False, clamp=0.0, bounds=False, terms=False, ess=False, n_elite=0):
    """Two solves with injected noise.  Engine A has keep on and is fed noise1, then noise2; engine B has keep off and is
    fed noise1, then keep_inject_ref(noise2, the set kept by reference).  Both must give bitwise equal costs, weights, U
    and u0 on solve 2, and A's kept() after solve 1 must equal the reference."""
    from mppi_hip.stats import keep_inject_ref, keep_store_ref, project_noise_ref
    K, B = K0, B0
    kw = dict(ctrl_clamp=clamp) if clamp else {}
    engs = []
    for keep in (n_keep, 0):
        eng, x0, U0 = _setup(M, kind, K, H, B, **kw)
        sigma, nu = eng.config.sigma, U0.shape[1]
        if terms:
            eng.set_control_cost(0.05)
            eng.set_rate_cost(np.linspace(0.4, 0.2, nu), anchor=True)
        if bounds:
            eng.set_control_bounds(-0.6 * sigma, 0.5 * sigma)
        if ess:
            eng.set_ess_target(FRAC, *LIMITS)
        elif not (terms or n_elite):
            _unfuse(eng, kind)
        if n_elite:
            eng.set_elites(n_elite)
        eng.set_elite_keep(keep)
        engs.append(eng)
    A, Bn = engs
    rs = np.random.RandomState(17)
    nz1 = (sigma * rs.randn(B, nu, H, K)).astype(np.float32)
    nz2 = (sigma * rs.randn(B, nu, H, K)).astype(np.float32)
    x1 = x0 + np.float32(0.01)
    a1 = A.solve(x0, U0, noise=nz1, shift=shift, want_weights=True)
    b1 = Bn.solve(x0, U0, noise=nz1, shift=shift, want_weights=True)
    for name in ("costs", "weights", "U", "u0"):
        _same(getattr(a1, name), getattr(b1, name), ("solve 1", name))
    # the set by reference: the noise as the rollout saw it, the costs the softmin would weigh ahead of any masking
    seen = project_noise_ref(U0, nz1, -0.6 * sigma, 0.5 * sigma)[0] if bounds else nz1
    c = a1.costs
    if terms:
        c = ((c + A.control_term(B)[0]).astype(np.float32) + A.rate_term(B)).astype(np.float32)
    want = keep_store_ref(U0, seen, c, n_keep, shift=shift, ctrl_clamp=clamp)
    got = A.kept(B)
    _same_kept(got, want, "kept() after solve 1")
    assert np.all(want[3] == n_keep) and np.all(want[4] == H - int(shift))
    if n_elite == n_keep:  # the shared selection: the kept set is the elite set
        assert np.array_equal(got[2], A.elite_set(B)[0])
    elif n_elite:
        assert not np.array_equal(got[2][:, :min(n_keep, n_elite)], A.elite_set(B)[0][:, :min(n_keep, n_elite)])
    a2 = A.solve(x1, a1.U, noise=nz2, shift=shift, want_weights=True)
    inj = keep_inject_ref(b1.U, nz2, want[0], want[3], want[4])
    if H > int(shift):
        assert not same_bits(inj, nz2)
    b2 = Bn.solve(x1, b1.U, noise=inj, shift=shift, want_weights=True)
    for name in ("costs", "weights", "U", "u0"):
        _same(getattr(a2, name), getattr(b2, name), ("solve 2", name))
    plain = Bn.solve(x1, b1.U, noise=nz2, shift=shift)
    if H > int(shift):
        assert not same_bits(plain.U, a2.U), "the carried samples must move the solve"
    for e in engs:
        e.close()


@pytest.mark.parametrize("kind", ["cartpole", "mlp"])
@pytest.mark.parametrize("n_keep", N_KEEPS)
def test_the_flow_is_exact(M, kind, n_keep):
    _flow(M, kind, n_keep)


@pytest.mark.parametrize("kind", ["cartpole", "mlp"])
@pytest.mark.parametrize("case", ["shift-bounds-clamp", "terms-ess", "elites-shared", "elites-other", "all", "H1-shift"])
def test_the_flow_composes(M, kind, case):
    """shift, bounds (the projection runs behind the injection) and ctrl_clamp > 0; the control-cost term, the rate term
    and ESS targeting; elites with n_elite == n_keep (one selection serves both, identical set) and n_elite != n_keep;
    everything at once; H = 1 with shift (steps 0: the second solve is the plain one)."""
    kw = {"shift-bounds-clamp": dict(shift=True, bounds=True, clamp=0.45),
          "terms-ess": dict(shift=True, terms=True, ess=True),
          "elites-shared": dict(n_elite=17, ess=True),
          "elites-other": dict(n_elite=40, shift=True),
          "all": dict(shift=True, bounds=True, clamp=0.45, terms=True, ess=True, n_elite=17),
          "H1-shift": dict(H=1, shift=True)}[case]
    _flow(M, kind, 17, **kw)


# ------------------------------------------------------------------------------------------ 6. streams

def _run_form(M, torch, kind, form, n, seed, adapt, n_keep=17):
    """One stream form, n steps (device noise, shift + env step) with the feature on.  Returns the state after the n
    steps, the kept set, the law and the seed counter."""
    from mppi_hip.trajectory import run_stream
    K, H, B = K0, 8, B0
    dev = torch.device("cuda")
    eng, x0, U0 = _setup(M, kind, K, H, B)
    eng.set_elite_keep(n_keep)
    if n_keep == 0:
        _unfuse(eng, kind)
    if adapt:
        eng.set_noise_model(*(([0.6], 0.7) if kind == "cartpole" else ([0.2, 0.5, 0.8], 0.7)))
        eng.set_noise_adapt(0.3)
    out = {}
    if form == "traj":
        states, actions, U_end = run_stream(eng, x0, U0, n, seed=seed)
        out["traj"] = (states, actions)
        out["U"] = U_end
    else:
        eng.set_stream(torch.cuda.current_stream().cuda_stream)
        tx, tU = torch.from_numpy(x0).to(dev), torch.from_numpy(U0).to(dev)
        tu0 = torch.zeros(B, U0.shape[1], device=dev)
        if form == "graph":
            eng.graph_capture(B, n, tx.data_ptr(), tU.data_ptr(), tu0.data_ptr(), seed=seed)
            eng.graph_launch(sync=True)
        else:
            out["x_before"], out["u0_steps"], out["sets"] = [], [], []
            for i in range(n):
                if form == "plain":
                    out["x_before"].append(_snap(torch, tx)[0])
                eng.solve_device(B, tx.data_ptr(), tU.data_ptr(), None, seed=seed, u0_ptr=tu0.data_ptr(), shift=True,
                                 env_step=True, seed_counter=form == "plain", chain=form != "plain")
                if form == "plain":
                    out["u0_steps"].append(_snap(torch, tu0)[0])
                    if n_keep:
                        out["sets"].append(eng.kept(B))
        out["x"], out["U"], out["u0"] = _snap(torch, tx, tU, tu0)
    out["set"] = eng.kept(B) if n_keep else None
    out["law"] = eng.noise_model()[:2] if adapt else None
    out["ctr"] = eng.get_seed_counter()
    eng.close()
    return out


@pytest.mark.parametrize("kind", ["cartpole", "mlp"])
@pytest.mark.parametrize("adapt", [False, True], ids=["white", "adapting"])
def test_stream_forms_agree_bitwise(M, kind, adapt):
    """Plain counter solves, chained solves, a captured graph of 4 solves and graph_capture_traj via run_stream (shift +
    env step), on white and adapting noise: bitwise equal x0, U, u0, final kept set and adapted law, seed counter 4; the
    set every plain step leaves is full (so steps 2.. inject count > 0), and the stream is not the keep-off stream."""
    import torch
    n, seed = 4, 9
    outs = {f: _run_form(M, torch, kind, f, n, seed, adapt) for f in ("plain", "chain", "graph", "traj")}
    want = outs["plain"]
    for form, got in outs.items():
        assert got["ctr"] == n, form
        np.testing.assert_array_equal(got["U"], want["U"], err_msg=form)
        if form != "traj":
            np.testing.assert_array_equal(got["x"], want["x"], err_msg=form)
            np.testing.assert_array_equal(got["u0"], want["u0"], err_msg=form)
        _same_kept(got["set"], want["set"], (form, "the final kept set"))
        if adapt:
            _same(got["law"][0], want["law"][0], (form, "sigma_u"))
            _same(np.float32(got["law"][1]), np.float32(want["law"][1]), (form, "rho"))
    states, actions = outs["traj"]["traj"]
    np.testing.assert_array_equal(states, np.stack(want["x_before"]))
    np.testing.assert_array_equal(actions, np.stack(want["u0_steps"]))
    assert all(np.all(s[3] == 17) and np.all(s[4] == 7) for s in want["sets"])
    assert len({s[0].tobytes() for s in want["sets"]}) == n  # each step's set is its own
    off = _run_form(M, torch, kind, "plain", n, seed, adapt, n_keep=0)
    assert off["ctr"] == n and not np.array_equal(off["U"], want["U"])
    np.testing.assert_array_equal(off["u0_steps"][0], want["u0_steps"][0])  # the first step is the same


# ------------------------------------------------------------------------------------------ 7. host / ASYNC

def test_host_pointer_and_async_solves_agree_with_plain_device_solves(M):
    """Two host-pointer solves and two device solves (plain, then ASYNC) of the same inputs and keys: bitwise the same
    U, u0 and kept set -- the second solve of each pair runs on the first one's set."""
    import torch
    K, H, B, seed = K0, 8, B0, 4
    dev = torch.device("cuda")
    eng, x0, U0 = _setup(M, "mlp", K, H, B)
    eng.set_elite_keep(17)
    h1 = eng.solve(x0, U0, seed=seed, shift=True)
    host = eng.solve(x0, h1.U, seed=seed + 1, shift=True)
    host_set = eng.kept(B)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    for asynchronous in (False, True):
        eng.set_kept(None, B=B)  # the pair starts from an empty set, as the host pair did
        tx, tU = torch.from_numpy(x0).to(dev), torch.from_numpy(U0).to(dev)
        tu0 = torch.zeros(B, MLP_NU, device=dev)
        for i in range(2):
            eng.solve_device(B, tx.data_ptr(), tU.data_ptr(), None, seed=seed + i, u0_ptr=tu0.data_ptr(), shift=True,
                             asynchronous=asynchronous)
        got_set = eng.kept(B)  # (waits for the stream)
        U, u0 = _snap(torch, tU, tu0)
        _same(U, host.U, ("U", asynchronous))
        _same(u0, host.u0, ("u0", asynchronous))
        _same_kept(got_set, host_set, asynchronous)
    eng.close()


# ------------------------------------------------------------------------------------------ 8. save / restore

def test_save_and_restore(M):
    """2 steps, save (x, U, seed counter, law, u_prev, kept()), restore on a fresh handle with set_kept, 2 more: bit for
    bit 4 straight steps."""
    import torch
    K, H, B, seed = K0, 8, B0, 13
    dev = torch.device("cuda")

    def start():
        eng, x0, U0 = _setup(M, "mlp", K, H, B)
        eng.set_noise_model([0.2, 0.5, 0.8], 0.6)
        eng.set_rate_cost(0.3, anchor=True)
        eng.set_elite_keep(17)
        eng.set_stream(torch.cuda.current_stream().cuda_stream)
        return eng, x0, U0

    def steps(eng, tx, tU, tu0, n):
        for _ in range(n):
            eng.solve_device(B, tx.data_ptr(), tU.data_ptr(), None, seed=seed, u0_ptr=tu0.data_ptr(), shift=True,
                             env_step=True, seed_counter=True)
        return _snap(torch, tx, tU, tu0)

    eng, x0, U0 = start()
    t = (torch.from_numpy(x0).to(dev), torch.from_numpy(U0).to(dev), torch.zeros(B, MLP_NU, device=dev))
    x, U, _ = steps(eng, *t, 2)
    saved = dict(x=x, U=U, ctr=eng.get_seed_counter(), law=eng.noise_model()[:2], u_prev=eng.prev_control(B),
                 kept=eng.kept(B))
    want = steps(eng, *t, 2)
    want_set = eng.kept(B)
    eng.close()
    assert saved["ctr"] == 2 and np.all(saved["kept"][3] == 17)

    eng, _, _ = start()
    eng.set_noise_model(*saved["law"])
    eng.set_prev_control(saved["u_prev"])
    eng.set_seed_counter(saved["ctr"])
    v, _, _, count, st = saved["kept"]
    eng.set_kept(v, count, st)
    back = eng.kept(B)
    _same(back[0], v, "set_kept / kept round trip")
    assert np.isposinf(back[1]).all() and np.all(back[2] == -1)
    assert np.array_equal(back[3], count) and np.array_equal(back[4], st)
    t = (torch.from_numpy(saved["x"]).to(dev), torch.from_numpy(saved["U"]).to(dev),
         torch.zeros(B, MLP_NU, device=dev))
    got = steps(eng, *t, 2)
    for a, b, name in zip(got, want, ("x", "U", "u0")):
        _same(a, b, name)
    _same_kept(eng.kept(B), want_set, "the set after the restored steps")
    assert eng.get_seed_counter() == 4
    eng.close()


# ------------------------------------------------------------------------------------------ 9. seeding

@pytest.mark.parametrize("kind", ["cartpole", "mlp"])
def test_seeding_a_solve_with_candidates(M, kind):
    """set_kept with hand-made candidates, then one solve: columns 0..count of its costs are the costs of a keep-off
    solve given those perturbations by injected noise (the whole costs row is)."""
    from mppi_hip.stats import keep_inject_ref
    K, H, B, n_keep = K0, 8, B0, 17
    A, x0, U0 = _setup(M, kind, K, H, B)
    Bn = _setup(M, kind, K, H, B)[0]
    nu = U0.shape[1]
    A.set_elite_keep(n_keep)
    _unfuse(Bn, kind)
    rs = np.random.RandomState(23)
    V = (0.3 * rs.randn(B, nu, H, n_keep)).astype(np.float32)
    V[:, :, :, 0] = 0.0  # "do nothing" as a candidate
    count, steps = np.array([n_keep, n_keep - 3], np.int32), np.array([H, H - 2], np.int32)
    nz = (A.config.sigma * rs.randn(B, nu, H, K)).astype(np.float32)
    A.set_kept(V, count, steps)
    a = A.solve(x0, U0, noise=nz)
    inj = keep_inject_ref(U0, nz, V, count, steps)
    b = Bn.solve(x0, U0, noise=inj)
    for bb in range(B):
        _same(a.costs[bb, :count[bb]], b.costs[bb, :count[bb]], ("the seeded columns", bb))
    _same(a.costs, b.costs, "costs")
    assert not same_bits(a.costs, Bn.solve(x0, U0, noise=nz).costs)
    A.close()
    Bn.close()


# ------------------------------------------------------------------------------------------ 10. the best cost

def test_the_best_cost_does_not_get_worse(M):
    """Cartpole, fp32, no shift, fixed x0, ADD mode, terms off, 4 solves: min(costs) of solve i + 1 <= min(costs) of
    solve i * (1 + 1e-5) -- the best sample is carried, and the carried control differs from v by at most one rounding
    (the project's fp32 cartpole cost tolerance: SURVEY section 8d, measured <= 1.6e-6)."""
    K, H, B = K0, 8, B0
    eng, x0, U = _setup(M, "cartpole", K, H, B, precision=0)
    assert eng.config.update_mode == 0 and eng.config.precision == 0
    eng.set_elite_keep(17)
    best = None
    for i in range(4):
        res = eng.solve(x0, U, seed=100 + i)
        U = res.U
        cur = res.costs.min(axis=1).astype(np.float64)
        print("solve", i, "min costs", cur)
        if best is not None:
            assert np.all(cur <= best * (1.0 + 1e-5)), (i, cur, best)
        best = cur
    eng.close()


# ------------------------------------------------------------------------------------------ 11. state rules

def test_state_and_argument_errors(M):
    from mppi_hip import _lib as L
    K, H = 16, 4
    eng = M.Engine(M.Config(nx=MLP_NX, nu=MLP_NU, H=H, K=K, max_batch=2))
    U, eps = inputs(2, MLP_NU, H, K)
    c = np.ones((2, K), np.float32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    v3 = np.zeros((2, MLP_NU, H, 3), np.float32)
    one, four = np.array([1, 1], np.int32), np.array([H, H], np.int32)
    # the feature is off
    for call in (lambda: eng.kept(1), lambda: L.check(eng.lib.mppi_set_kept(eng._h, 1, None, None, None)),
                 lambda: L.check(eng.lib.mppi_keep_store_eval(eng._h, 2, p(U), p(eps), p(c), 0, *[None] * 5)),
                 lambda: L.check(eng.lib.mppi_keep_inject_eval(eng._h, 2, p(U), p(eps), p(v3), p(one), p(four),
                                                               p(eps.copy())))):
        with pytest.raises(M.MPPIError) as ei:
            call()
        assert ei.value.code == L.MPPI_E_STATE
    assert eng.lib.mppi_set_kept(eng._h, 1, None, None, None) == L.MPPI_E_STATE
    for state in (0, 5):
        eng.set_elite_keep(state)
        for bad in (-1, K + 1, 1 << 30):
            assert eng.lib.mppi_set_elite_keep(eng._h, bad) == L.MPPI_E_ARG, bad
            assert b"mppi_set_elite_keep" in eng.lib.mppi_last_error()
            assert eng.elite_keep() == state, "a refused value changes nothing"
    eng.set_elite_keep(K)  # the edges are allowed
    eng.set_elite_keep(3)
    with pytest.raises(M.MPPIError) as ei:  # enabling alone stores nothing
        eng.kept(1)
    assert ei.value.code == L.MPPI_E_STATE
    # set_kept: sizes are checked, a refused call writes nothing; B beyond the slots written is refused by the getter
    for count, steps in (([4, 1], [H, H]), ([-1, 1], [H, H]), ([1, 1], [H + 1, H]), ([1, 1], [H, -1])):
        rc = eng.lib.mppi_set_kept(eng._h, 2, p(v3), p(np.array(count, np.int32)), p(np.array(steps, np.int32)))
        assert rc == L.MPPI_E_ARG, (count, steps)
    assert eng.lib.mppi_set_kept(eng._h, 2, p(v3), None, None) == L.MPPI_E_ARG
    assert eng.lib.mppi_set_kept(eng._h, 3, p(v3), p(one), p(four)) == L.MPPI_E_ARG  # beyond max_batch
    with pytest.raises(M.MPPIError) as ei:
        eng.kept(1)
    assert ei.value.code == L.MPPI_E_STATE
    eng.set_kept(v3[:1] + 1.0, [2], [H - 1])
    got = eng.kept(1)
    assert got[3].tolist() == [2] and got[4].tolist() == [H - 1] and np.all(got[0] == 1.0)
    with pytest.raises(M.MPPIError) as ei:
        eng.kept(2)
    assert ei.value.code == L.MPPI_E_ARG
    eng.set_kept(None, B=1)  # emptied: readable, and empty
    got = eng.kept(1)
    assert got[3].tolist() == [0] and got[4].tolist() == [0] and not got[0].any()
    # the evaluations: beyond max_batch, bad sizes, optional outputs; they leave the stored set alone
    eng.set_kept(v3[:1] + 2.0, [3], [H])
    with pytest.raises(M.MPPIError) as ei:
        eng.keep_store_eval(np.zeros((3, MLP_NU, H)), np.zeros((3, MLP_NU, H, K)), np.ones((3, K)))
    assert ei.value.code == L.MPPI_E_ARG
    for count, steps in (([4, 1], [H, H]), ([1, 1], [H + 1, H])):
        with pytest.raises(M.MPPIError) as ei:
            eng.keep_inject_eval(U, eps, v3, count, steps)
        assert ei.value.code == L.MPPI_E_ARG
    cnt = np.zeros(2, np.int32)
    assert eng.lib.mppi_keep_store_eval(eng._h, 2, p(U), p(eps), p(c), 1, None, None, None, p(cnt), None) == L.MPPI_OK
    assert cnt.tolist() == [3, 3]
    assert eng.lib.mppi_keep_store_eval(eng._h, 2, None, p(eps), p(c), 1, *[None] * 5) == L.MPPI_E_ARG
    eng.keep_inject_eval(U, eps, v3, one, four)
    got = eng.kept(1)
    assert got[3].tolist() == [3] and np.all(got[0] == 2.0), "the evaluations have a slot of their own"
    # a change of n_keep empties the set; the value in effect keeps it
    eng.set_elite_keep(3)
    assert eng.kept(1)[3].tolist() == [3]
    eng.set_elite_keep(4)
    with pytest.raises(M.MPPIError) as ei:
        eng.kept(1)
    assert ei.value.code == L.MPPI_E_STATE
    eng.close()


def test_the_setter_destroys_graphs_keeps_the_prefetched_noise_and_empties_the_set(M):
    import torch
    from mppi_hip import _lib as L
    K, H, B, n, seed = K0, 8, B0, 3, 21
    dev = torch.device("cuda")

    def start():
        eng, x0, U0 = _setup(M, "mlp", K, H, B)
        eng.set_stream(torch.cuda.current_stream().cuda_stream)
        tx, tU = torch.from_numpy(x0).to(dev), torch.from_numpy(U0).to(dev)
        return eng, tx, tU, torch.zeros(B, MLP_NU, device=dev)

    def chain(eng, tx, tU, tu0, steps):
        for _ in range(steps):
            eng.solve_device(B, tx.data_ptr(), tU.data_ptr(), None, seed=seed, u0_ptr=tu0.data_ptr(), shift=True,
                             env_step=True, chain=True)
        return _snap(torch, tx, tU, tu0)

    eng, tx, tU, tu0 = start()
    eng.graph_capture(B, n, tx.data_ptr(), tU.data_ptr(), tu0.data_ptr(), seed=seed)
    eng.graph_launch(sync=True)  # leaves a prefetched noise: the device counter is one ahead
    assert eng.get_seed_counter() == n
    eng.set_elite_keep(17)
    assert eng.get_seed_counter() == n  # the key sequence is unchanged
    with pytest.raises(M.MPPIError) as ei:
        eng.graph_launch(sync=True)
    assert ei.value.code == L.MPPI_E_STATE and "mppi_graph_capture first" in str(ei.value)
    eng.graph_capture(B, n, tx.data_ptr(), tU.data_ptr(), tu0.data_ptr(), seed=seed)
    eng.graph_launch(sync=True)
    assert eng.get_seed_counter() == 2 * n
    first = eng.kept(B)
    assert first[0].shape == (B, MLP_NU, H, 17) and np.all(first[3] == 17) and np.all(first[4] == H - 1)
    eng.set_elite_keep(17)  # the same value: nothing changes, the graph and the set stay
    _same_kept(eng.kept(B), first, "a no-op keeps the set")
    eng.set_kept(first[0], first[3], first[4])  # data, allowed between launches: the graph stays
    eng.graph_launch(sync=True)
    eng.set_elite_keep(18)  # a change destroys it and empties the set
    with pytest.raises(M.MPPIError) as ei:
        eng.graph_launch(sync=True)
    assert ei.value.code == L.MPPI_E_STATE
    with pytest.raises(M.MPPIError) as ei:
        eng.kept(B)
    assert ei.value.code == L.MPPI_E_STATE
    eng.set_elite_keep(0)  # ... and so does disabling
    eng.graph_capture(B, n, tx.data_ptr(), tU.data_ptr(), tu0.data_ptr(), seed=seed)
    eng.set_elite_keep(0)  # off -> off: nothing to destroy
    eng.graph_launch(sync=True)
    eng.close()

    # a prefetched noise survives the setter: a chain with the feature switched on after two steps goes on with the
    # noise it would have drawn -- what plain counter solves with the same switch draw
    a = start()
    chain(*a, 2)
    a[0].set_elite_keep(17)
    got = chain(*a, 2)
    assert a[0].get_seed_counter() == 4
    eng_b, bx, bU, bu0 = start()
    for i in range(4):
        if i == 2:
            eng_b.set_elite_keep(17)
        eng_b.solve_device(B, bx.data_ptr(), bU.data_ptr(), None, seed=seed, u0_ptr=bu0.data_ptr(), shift=True,
                           env_step=True, seed_counter=True)
    want = _snap(torch, bx, bU, bu0)
    for x, y in zip(got, want):
        np.testing.assert_array_equal(x, y)
    _same_kept(a[0].kept(B), eng_b.kept(B))
    for e in (a[0], eng_b):
        e.close()


# ------------------------------------------------------------------------------------------ 12. launches

@pytest.mark.parametrize("kind", ["cartpole", "mlp"])
def test_launches_per_solve(M, kind):
    """With the feature off, kernel names and counts equal those of a handle that never touched it (the cartpole: its
    one fused launch, no reduce); with it on the launches are counted once per solve under "keep", and the cartpole
    takes its unfused form; with elites at the same n the selection is shared (one "elites" group, one "keep")."""
    K, H, B = K0, 7, B0
    eng, x0, U0 = _setup(M, kind, K, H, B)
    names = ("noise", "rollout", "elites", "keep", "lambda", "bounds", "reduce", "stats")

    def counts(e=eng):
        e.profile(True)  # (resets the counters)
        e.solve(x0, U0, seed=3)
        got = {k: e.kernel_time(k)[0] for k in names}
        assert e.kernel_time("keep")[1] >= 0.0
        e.profile(False)
        return got

    fused = kind == "cartpole"
    base = dict(noise=1, rollout=1, stats=0, bounds=0, elites=0, **{"lambda": 0})
    never = counts()
    assert never == dict(base, keep=0, reduce=0 if fused else 1)
    eng.set_elite_keep(13)
    assert counts() == dict(base, keep=1, reduce=1)
    assert counts() == dict(base, keep=1, reduce=1)  # (a solve that injects a stored set: the same launches)
    eng.set_elites(13)
    assert counts() == dict(base, keep=1, elites=1, reduce=1)
    eng.set_elites(0)
    eng.set_elite_keep(0)
    assert counts() == never
    eng.close()
