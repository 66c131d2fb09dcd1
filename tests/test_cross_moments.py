"""The weighted cross moments on the host (MPPI_FLAG_CROSS; no GPU needed): mppi_hip.stats.cross_moments_f32 against the
header csrc/cross_moments.h through g++ (bitwise), against the float64 statement cross_moments_ref, the consequences of
the cell scheme (the diagonal is eps_m2's chain, the matrix is symmetric), and the NULL-handle paths of the two
entries."""
import ctypes
import os

import numpy as np
import pytest

from conftest import PKG, REPO
from cross_cases import B, SHAPES, bits, build_host, case, exact_case, exact_want, host_cross, shape_id

ENTRIES = ("mppi_get_cross_moments", "mppi_cross_moments_eval")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("cross_moments")
    return build_host(d), d


def _weights_f32(costs):
    from mppi_hip.stats import softmin_weights_ref
    return softmin_weights_ref(costs).astype(np.float32)


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_numpy_restatement_equals_the_header_bitwise(host, shape):
    """random weights (the float64 softmin rounded to float32) and the exact-weight case the device test uses"""
    from mppi_hip.stats import cross_moments_f32
    costs, noise = case(*shape)
    w = _weights_f32(costs)
    got = cross_moments_f32(w, noise)
    assert got.dtype == np.float32 and got.shape == (B, shape[0], shape[0])
    assert np.array_equal(bits(got), bits(host_cross(*host, w, noise)))
    _, we, _ = exact_case(*shape)
    assert np.array_equal(bits(exact_want(*shape)), bits(host_cross(*host, we, noise)))


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_f32_scheme_holds_the_bar_against_float64(shape):
    """|got - ref| <= 1e-4 A[u][v] + 1e-6 with A = 1/H sum w |e_u e_v| in float64: the eps_m2 bar of
    tests/test_gpu_stats.py, taken on the absolute sum because off-diagonal terms cancel (on the diagonal it is that
    bar).  The weights enter both sides as the same float32 numbers, so the figure is the summation's alone."""
    from mppi_hip.stats import cross_moments_f32
    costs, noise = case(*shape)
    w = _weights_f32(costs)
    got = cross_moments_f32(w, noise).astype(np.float64)
    e = noise.astype(np.float64)
    ref = np.einsum("bk,buhk,bvhk->buv", w.astype(np.float64), e, e) / shape[1]
    A = np.einsum("bk,buhk,bvhk->buv", w.astype(np.float64), np.abs(e), np.abs(e)) / shape[1]
    ratio = float((np.abs(got - ref) / (1e-4 * A + 1e-6)).max())
    print(shape, "max |got - ref| / (1e-4 A + 1e-6) =", ratio)
    assert ratio <= 1.0


def test_ref_from_costs_matches_its_parts():
    """cross_moments_ref is the einsum over softmin_weights_ref; its diagonal is solve_stats_ref's eps_m2"""
    from mppi_hip.stats import cross_moments_ref, softmin_weights_ref, solve_stats_ref
    costs, noise = case(3, 7, 130)
    ref = cross_moments_ref(costs, noise, 2.0, 0.25)
    w = softmin_weights_ref(costs, 2.0, 0.25)
    e = noise.astype(np.float64)
    np.testing.assert_allclose(ref, np.einsum("bk,buhk,bvhk->buv", w, e, e) / 7, rtol=1e-13)
    np.testing.assert_allclose(np.diagonal(ref, axis1=1, axis2=2), solve_stats_ref(costs, noise, 2.0, 0.25)["eps_m2"],
                               rtol=1e-12)
    assert np.all(cross_moments_ref(costs, noise, absolute=True) >= np.abs(cross_moments_ref(costs, noise)))


@pytest.mark.parametrize("shape", [(3, 7, 130), (21, 33, 1030)], ids=shape_id)
def test_diagonal_is_the_m2_chain_and_the_matrix_is_symmetric(shape):
    """The diagonal pair (u, u) runs stats_row's expression: a one-actuator call on row u alone gives the same bits,
    whatever the other rows hold (what makes eps_mx[u][u] == eps_m2[u] on the device).  Mirrored, so symmetric."""
    from mppi_hip.stats import cross_moments_f32
    costs, noise = case(*shape)
    w = _weights_f32(costs)
    got = cross_moments_f32(w, noise)
    assert np.array_equal(bits(got), bits(got.transpose(0, 2, 1)))
    for u in (0, shape[0] - 1):
        alone = cross_moments_f32(w, noise[:, u:u + 1])
        assert np.array_equal(bits(alone[:, 0, 0]), bits(got[:, u, u]))


def test_zero_weights_and_pads_give_zero():
    from mppi_hip.stats import cross_moments_f32
    _, noise = case(3, 7, 130)
    assert not np.any(cross_moments_f32(np.zeros((B, 130), np.float32), noise))


def test_moment_cells_is_the_statistics_split():
    """the split of kernels_stats.hip: 256-k wave-chunks, at most 16 segments of ceil(H / 16) steps"""
    from mppi_hip.stats import moment_cells
    assert moment_cells(1, 64) == (1, 1, 1)
    assert moment_cells(7, 192) == (1, 1, 7)
    assert moment_cells(33, 1088) == (5, 3, 11)
    assert moment_cells(64, 1024) == (4, 4, 16)
    assert moment_cells(100, 64) == (1, 7, 15)
    assert moment_cells(150, 128) == (1, 10, 15)


def test_ctypes_prototypes_and_null_handles():
    from mppi_hip import _lib as L
    lib = L.load()
    for name, nargs in zip(ENTRIES, (4, 5)):
        assert name in L.EXPORTED
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == nargs, name
    assert L.FLAG_CROSS == 0x400
    buf = np.ones((3, 3), np.float32)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    assert lib.mppi_get_cross_moments(None, 1, 0, p) == L.MPPI_E_ARG
    assert b"mppi_get_cross_moments" in lib.mppi_last_error()
    assert lib.mppi_cross_moments_eval(None, 1, p, p, p) == L.MPPI_E_ARG
    assert b"mppi_cross_moments_eval" in lib.mppi_last_error()
    assert np.array_equal(buf, np.ones((3, 3), np.float32))
    assert lib.mppi_abi_version() == 4  # additive


def test_header_declares_the_entries_and_the_wrappers_exist():
    text = open(os.path.join(REPO, "include", "mppi.h")).read()
    for name in ENTRIES:
        assert f"int {name}(mppi_handle*" in text, name
    assert "#define MPPI_FLAG_CROSS 0x400" in text and "#define MPPI_ABI_VERSION 4" in text
    from mppi_hip import Engine
    for name in ("cross_moments", "cross_moments_eval"):
        assert callable(getattr(Engine, name))
    jl = open(os.path.join(PKG, "julia", "MPPIHip.jl")).read()
    for name in ENTRIES:
        assert f":{name}" in jl, name
