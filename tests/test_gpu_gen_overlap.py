"""The next solve's noise generated BESIDE the rollout (chained solves; csrc/gen_overlap.h, noise_beside_kernel): the
overlap route against the fused route (reduce_kernel<GEN>), bitwise, on the CrossAttention humanoid net in the split
mode; routes mixed from solve to solve; a stream switch between overlapped solves; the generator's noise against
noise_kernel's; and the rule's choice at the default benchmark line's shape.

The shapes are the generator's edges (one wave per block, kGenRows = 4 whole rows per block, one quad of four samples
per lane and pass): B=1 K=32 H=2 is less than one quad per lane (Kp = 64: 16 quads, a partial wave) and 42 rows (a last
block of two rows); B=3 K=96 H=5 is 315 rows, no multiple of the rows per block, and a partial wave; B=1 K=1056 H=3 is
more than four quads per lane with a tail (Kp = 1088: 272 quads)."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

SHAPES = [(1, 32, 2), (3, 96, 5), (1, 1056, 3)]  # (B, K, H)
N_SOLVES, SEED = 6, 0x0517_0000_0021
_cache = {}


@pytest.fixture(scope="module")
def M(gpu_available):
    import mppi_hip
    return mppi_hip


def _engine(M, B, K, H):
    sd = M.load_npz(os.path.join(GOLDEN, "ca_humanoid_weights.npz"))
    eng = M.Engine(M.Config.preset("humanoid_v3", K=K, H=H, precision=2, max_batch=B), device=0)
    eng.load_dynamics(*M.cross_attention_blob(sd)).set_cost("humanoid_v3")
    return eng


def _inputs(B, H):
    xs = np.load(os.path.join(GOLDEN, "g5_ca_humanoid_fwd.npz"))["x0_stride20"]
    x0 = xs[np.arange(B) % len(xs)].astype(np.float32)
    U0 = (0.1 * np.random.RandomState(5).randn(B, 21, H)).astype(np.float32)
    return x0, U0


def _run(M, shape, routes, switch_at=None):
    """One engine, len(routes) chained solves (seed_counter, shift, chain); routes[i] is MPPI_GEN_OVERLAP for solve i
    ("0" / "1" / None = the rule decides).  switch_at: before that solve the engine moves to a fresh stream.
    Returns per solve (costs, U, u0, seed counter, route reported)."""
    import torch
    B, K, H = shape
    dev = torch.device("cuda:0")
    eng = _engine(M, B, K, H)
    x0, U0 = _inputs(B, H)
    tx, tU = torch.from_numpy(x0).to(dev), torch.from_numpy(U0).to(dev)
    tc, tu0 = torch.zeros(B, K, device=dev), torch.zeros(B, 21, device=dev)
    torch.cuda.synchronize()
    keep, out, saved = [], [], os.environ.get("MPPI_GEN_OVERLAP")
    try:
        for i, r in enumerate(routes):
            if r is None:
                os.environ.pop("MPPI_GEN_OVERLAP", None)
            else:
                os.environ["MPPI_GEN_OVERLAP"] = r
            if switch_at is not None and i == switch_at:
                keep.append(torch.cuda.Stream(device=dev))
                eng.set_stream(keep[-1].cuda_stream)
            eng.solve_device(B, tx.data_ptr(), tU.data_ptr(), None, seed=SEED, costs_ptr=tc.data_ptr(),
                             u0_ptr=tu0.data_ptr(), shift=True, seed_counter=True, chain=True)
            route = eng.gen_route()
            ctr = eng.get_seed_counter()  # (waits for the stream)
            eng.sync()
            out.append((tc.cpu().numpy(), tU.cpu().numpy(), tu0.cpu().numpy(), ctr, route))
    finally:
        if saved is None:
            os.environ.pop("MPPI_GEN_OVERLAP", None)
        else:
            os.environ["MPPI_GEN_OVERLAP"] = saved
        eng.close()
    return out


def _fused(M, shape):
    """The all-fused sequence of a shape: computed once, shared, never written."""
    if shape not in _cache:
        _cache[shape] = _run(M, shape, ["0"] * N_SOLVES)
        for rec in _cache[shape]:
            for a in rec[:3]:
                a.setflags(write=False)
    return _cache[shape]


def _same(got, want, what):
    assert len(got) <= len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        for name, a, b in zip(("costs", "U", "u0"), g[:3], w[:3]):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"{what}: solve {i} {name}"
        assert g[3] == w[3] == i + 1, f"{what}: solve {i} seed counter {g[3]} vs {w[3]}"


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d-K%d-H%d" % s)
def test_forced_overlap_equals_forced_fused(M, shape):
    want = _fused(M, shape)
    assert all(rec[4] == "fused" for rec in want)
    assert all(np.isfinite(rec[0]).any() for rec in want) and not np.array_equal(want[0][1], want[-1][1])
    got = _run(M, shape, ["1"] * N_SOLVES)
    assert all(rec[4] == "overlap" for rec in got)
    _same(got, want, "overlap")


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d-K%d-H%d" % s)
def test_mixed_routes_neither_lose_nor_repeat_a_key(M, shape):
    routes = ["1", "1", "0", "1"]
    got = _run(M, shape, routes)
    assert [rec[4] for rec in got] == ["overlap", "overlap", "fused", "overlap"]
    _same(got, _fused(M, shape), "mixed")


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d-K%d-H%d" % s)
def test_stream_switch_between_overlapped_solves(M, shape):
    got = _run(M, shape, ["1"] * 4, switch_at=2)
    _same(got, _fused(M, shape), "stream switch")


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d-K%d-H%d" % s)
def test_generator_draws_noise_kernels_noise(M, shape):
    """noise_beside_kernel against noise_kernel for the same by-value key (neither needs dynamics), bit for bit; with
    MPPI_GEN_ROWS at 1 and at 7 (blocks of other sizes, other tails) as well as the default."""
    B, K, H = shape
    eng = M.Engine(M.Config.preset("humanoid_v3", K=K, H=H, precision=2, max_batch=B), device=0)
    saved = os.environ.get("MPPI_GEN_ROWS")
    try:
        want = eng.noise_eval(B, SEED + 3)
        assert np.isfinite(want).all() and want.std() > 0.1
        for rows in (None, "1", "7"):
            if rows is None:
                os.environ.pop("MPPI_GEN_ROWS", None)
            else:
                os.environ["MPPI_GEN_ROWS"] = rows
            got = eng.noise_beside_eval(B, SEED + 3)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), rows
    finally:
        if saved is None:
            os.environ.pop("MPPI_GEN_ROWS", None)
        else:
            os.environ["MPPI_GEN_ROWS"] = saved
        eng.close()


def test_rule_chooses_the_overlap_at_64_solves(M):
    """The default benchmark line's shape, B=64 K=1024 H=64 (a solve is half a millisecond): unforced, the route report
    says the rule chose the overlap, and the overlapped solves equal forced-fused ones bitwise.  The rule's size side is
    the noise of one batch in bytes (gen_overlap.h: past 128 MiB, where the reduce stops being latency-bound), so the
    horizon is the workload's: at H=2 the same batch has 11 MB of noise and the rule -- rightly -- keeps the fused route,
    which is asserted too.  The register side is asserted only where the routed kernel is the one the rule was built
    for."""
    shape = (64, 1024, 64)
    got = _run(M, shape, [None, None, None])
    small = _run(M, (64, 1024, 2), [None, None])
    assert [rec[4] for rec in small] == ["fused", "fused"]
    eng = _engine(M, *shape)
    try:
        x0, U0 = _inputs(64, 64)
        res = eng.solve(x0, U0, seed=1)
        assert np.isfinite(res.costs).any()
        kern = eng.rollout_kernel()
    finally:
        eng.close()
    want = _run(M, shape, ["0", "0", "0"])
    _same(got, want, "rule")
    if not kern.startswith("fc_wave32_x3p_kernel"):
        pytest.skip(f"the routed rollout kernel is {kern}, not fc_wave32_x3p_kernel: no register fit to assert")
    assert [rec[4] for rec in got] == ["overlap"] * 3, [rec[4] for rec in got]
