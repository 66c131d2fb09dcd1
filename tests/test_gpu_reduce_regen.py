"""The read-only reduce that regenerates part of the noise it sums from the noise's key (csrc/reduce_regen.h,
reduce_kernel<REGEN>): forced shares against share 0, bitwise, over chained solves on both routes of the next noise and
mixed; across a counter reset; and content the rule must refuse, which reports 0 and stays bitwise what it was.

Every case runs a seeded MLP (fp32, quad_est, no probe).  The shapes (B, nu, H, K) are the walk's edges: K = 96 is
fewer quads than lanes (Kp = 128: 32 quads, the clamped loads), K = 1024 exactly one tile of four quads per lane,
K = 1536 a second, partial tile, K = 100 is K < Kp (padded columns, weight 0), and B * nu = 168 >= 128 takes the
block-local form (LOCAL) instead of the ticketed one.

On the fused route (MPPI_GEN_OVERLAP=0) the reduce also draws the next noise and never regenerates by itself; a FORCED
share separates the two launches there, so every solve reports the forced share on either route."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NX = 10
SHAPES = [(2, 3, 5, 96), (3, 2, 4, 1024), (1, 21, 3, 1536), (2, 3, 4, 100), (8, 21, 2, 64)]  # (B, nu, H, K)
SHARES = (1, 3, 4, 7)
SEED = 0x0517_0000_0033
_cache = {}
_ids = lambda s: "B%d-nu%d-H%d-K%d" % s  # noqa: E731


@pytest.fixture(scope="module")
def M(gpu_available):
    import mppi_hip
    return mppi_hip


def _engine(M, shape):
    from mppi_hip.nets import mlp_blob, synthetic_mlp
    B, nu, H, K = shape
    eng = M.Engine(M.Config(nx=NX, nu=nu, H=H, K=K, max_batch=B, lambda_=1.0, sigma=0.5, precision=0))
    eng.load_dynamics(*mlp_blob(synthetic_mlp(NX, nu, seed=0), NX, nu))
    eng.set_cost("quad_est")
    rs = np.random.RandomState(11)
    x0 = (0.3 * rs.randn(B, NX)).astype(np.float32)
    U0 = (0.1 * rs.randn(B, nu, H)).astype(np.float32)
    return eng, x0, U0


class _Env:
    """MPPI_GEN_OVERLAP / MPPI_REDUCE_REGEN for one solve (both read per launch), restored on exit."""
    NAMES = ("MPPI_GEN_OVERLAP", "MPPI_REDUCE_REGEN")

    def __enter__(self):
        self.saved = {n: os.environ.get(n) for n in self.NAMES}
        return self

    def set(self, overlap, regen):
        for n, v in zip(self.NAMES, (overlap, regen)):
            if v is None:
                os.environ.pop(n, None)
            else:
                os.environ[n] = str(v)

    def __exit__(self, *a):
        for n, v in self.saved.items():
            if v is None:
                os.environ.pop(n, None)
            else:
                os.environ[n] = v


def _chain(M, shape, overlaps, regen, reset_at=None):
    """len(overlaps) chained solves (seed_counter, shift, chain) on one engine; overlaps[i] is MPPI_GEN_OVERLAP for
    solve i, regen MPPI_REDUCE_REGEN for all of them; reset_at: set_seed_counter(0) ahead of that solve.
    Per solve: (costs, weights, U, u0, the share reported)."""
    import torch
    B, nu, H, K = shape
    dev = torch.device("cuda:0")
    eng, x0, U0 = _engine(M, shape)
    tx, tU = torch.from_numpy(x0).to(dev), torch.from_numpy(U0).to(dev)
    tc, tw, tu0 = torch.zeros(B, K, device=dev), torch.zeros(B, K, device=dev), torch.zeros(B, nu, device=dev)
    torch.cuda.synchronize()
    out = []
    try:
        with _Env() as env:
            for i, ov in enumerate(overlaps):
                if reset_at is not None and i == reset_at:
                    eng.set_seed_counter(0)
                env.set(ov, regen)
                eng.solve_device(B, tx.data_ptr(), tU.data_ptr(), None, seed=SEED, costs_ptr=tc.data_ptr(),
                                 u0_ptr=tu0.data_ptr(), weights_ptr=tw.data_ptr(), shift=True, seed_counter=True,
                                 chain=True)
                share = eng.reduce_regen()
                eng.sync()
                out.append((tc.cpu().numpy(), tw.cpu().numpy(), tU.cpu().numpy(), tu0.cpu().numpy(), share))
    finally:
        eng.close()
    return out


def _share0(M, shape, overlaps, reset_at=None):
    """The share-0 sequence of a shape and route plan: computed once, shared, never written."""
    key = (shape, tuple(overlaps), reset_at)
    if key not in _cache:
        _cache[key] = _chain(M, shape, overlaps, "0", reset_at)
        for rec in _cache[key]:
            assert rec[4] == 0
            for a in rec[:4]:
                a.setflags(write=False)
    return _cache[key]


def _same(got, want, what):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        for name, a, b in zip(("costs", "weights", "U", "u0"), g[:4], w[:4]):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"{what}: solve {i} {name}"


@pytest.mark.parametrize("overlap", ["1", "0"], ids=["overlap", "fused"])
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_forced_shares_equal_share_0(M, shape, overlap):
    plan = [overlap] * 3
    want = _share0(M, shape, plan)
    assert all(np.isfinite(rec[0]).all() for rec in want) and not np.array_equal(want[0][2], want[-1][2])
    assert all(rec[1].sum() > 0.5 for rec in want)
    for share in SHARES:
        got = _chain(M, shape, plan, share)
        assert [rec[4] for rec in got] == [share] * 3, (share, [rec[4] for rec in got])
        _same(got, want, f"share {share}")


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_routes_mixed_from_solve_to_solve(M, shape):
    plan = ["1", "0", "0", "1"]
    want = _share0(M, shape, plan)
    for share in (3, 4):
        got = _chain(M, shape, plan, share)
        assert [rec[4] for rec in got] == [share] * 4, (share, [rec[4] for rec in got])
        _same(got, want, f"mixed, share {share}")


@pytest.mark.parametrize("overlap", ["1", "0"], ids=["overlap", "fused"])
def test_counter_reset_between_solves(M, overlap):
    """One solve, set_seed_counter(0), two solves: the prefetched noise of the old counter is drawn again, and the key
    the reduce regenerates from is the one recorded beside the buffer, not the counter's."""
    shape, plan = SHAPES[2], [overlap] * 3
    want = _share0(M, shape, plan, reset_at=1)
    got = _chain(M, shape, plan, 3, reset_at=1)
    assert [rec[4] for rec in got] == [3] * 3
    _same(got, want, "counter reset")


def _plain(M, shape, regen, setup=None, noise=None):
    """Two plain solves (the second from the first's U) with MPPI_REDUCE_REGEN=regen; (results, shares reported)."""
    eng, x0, U0 = _engine(M, shape)
    res, shares = [], []
    try:
        if setup:
            setup(eng)
        with _Env() as env:
            env.set(None, regen)
            U = U0
            for i in range(2):
                r = eng.solve(x0, U, noise=noise, seed=SEED + i, shift=True, want_weights=True)
                res.append(r)
                shares.append(eng.reduce_regen())
                U = r.U
    finally:
        eng.close()
    return res, shares


def _same_plain(got, want, what):
    for i, (g, w) in enumerate(zip(got, want)):
        for name in ("costs", "weights", "U", "u0"):
            a, b = getattr(g, name), getattr(w, name)
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"{what}: solve {i} {name}"


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[4]], ids=_ids)
def test_plain_solves_regenerate_when_forced(M, shape):
    """The positive control of the refusals below: the plain i.i.d. law on a plain solve is eligible."""
    want, s0 = _plain(M, shape, "0")
    got, s3 = _plain(M, shape, "3")
    assert s0 == [0, 0] and s3 == [3, 3]
    _same_plain(got, want, "plain")


def _ar1(eng):
    eng.set_noise_model([0.4] * eng.config.nu, 0.6)


def _bounds(eng):
    eng.set_control_bounds([-0.3] * eng.config.nu, [0.3] * eng.config.nu)


@pytest.mark.parametrize("what", ["injected", "ar1", "bounds"])
def test_ineligible_content_reads_everything_even_when_forced(M, what):
    shape = SHAPES[0]
    B, nu, H, K = shape
    noise = (0.5 * np.random.RandomState(3).randn(B, nu, H, K)).astype(np.float32) if what == "injected" else None
    setup = {"injected": None, "ar1": _ar1, "bounds": _bounds}[what]
    want, s0 = _plain(M, shape, "0", setup, noise)
    got, s7 = _plain(M, shape, "7", setup, noise)
    assert s0 == [0, 0] and s7 == [0, 0], (what, s7)
    _same_plain(got, want, what)
    if what != "injected":  # ... and it is another solve than the plain law's, which the same knob does regenerate
        plain, sp = _plain(M, shape, "7")
        assert sp == [7, 7] and not np.array_equal(plain[0].U, got[0].U)
