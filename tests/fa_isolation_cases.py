"""Inputs shared by tests/test_gpu_fa_isolation.py: the grid of feature-attention (FA) rollouts that pack several
samples into one MFMA tile or one attention, and the clean, finite-dirty and non-finite-dirty noise of every case.

Three kernels pack samples (csrc/kernels_fa_small.hip, kernels_fa.hip, kernels_fa_layered.hip):

  fa_small_kernel    16 // L samples per 16-row tile (bf16, hidden 64, 4 heads, <= 4 layers, L <= 16 tokens)
  fa_rollout_kernel  R // L samples per workgroup, R = 16 NT token rows (NT = 1, 2, 4 for L <= 16, 32, 64 at hidden
                     <= 128; hidden 512 always takes R = 64); attention on MFMA for bf16 at hidden >= 128, on VALU
                     otherwise
  fa_layered         one sample per attention workgroup, whose 64-token window reaches into the next samples' rows

Every case is B = 2 solves of H = 3 steps with injected noise; K is 70, or 71 where 70 is a multiple of the packing G,
so the last workgroup of a solve is partly empty.  Every row of the grid loaded (mppi_load_dynamics refused none).
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

B, H, SIGMA, LAM, TERMINAL_WEIGHT = 2, 3, 0.4, 1.0, 10.0
VICTIM_SOLVE, DIRTY_STEP = 1, 1  # the dirty sample lives in solve 1; its dirty element at the middle step


@dataclass(frozen=True)
class Case:
    name: str
    nx: int
    nu: int
    D: int
    heads: int
    layers: int
    precision: int  # 0: fp32, 1: bf16
    form: str       # "small" | "general" | "layered"
    seed: int
    # (a): this seeded multi-layer net amplifies single bf16 rounding flips (test_fa_small_net_layers_bf16's reason),
    # so its costs are held in distribution instead of at rtol 1e-2
    dist: bool = False

    @property
    def L(self) -> int:
        return self.nx + self.nu

    @property
    def rows(self) -> int:
        """Token rows of the unit that packs samples: the 16-row tile, the workgroup's R rows, the 64-token window."""
        if self.form == "small":
            return 16
        if self.form == "layered" or self.D == 512:
            return 64
        return 16 * (1 if self.L <= 16 else 2 if self.L <= 32 else 4)  # csrc/mppi_internal.h fa_nt_min

    @property
    def G(self) -> int:
        """Samples that share the unit (layered: the samples whose rows the window of one sample covers)."""
        return self.rows // self.L

    @property
    def K(self) -> int:
        return 71 if 70 % self.G == 0 else 70

    @property
    def kernel(self) -> str:
        """What mppi_rollout_kernel names after a solve of this case."""
        return {"small": "fa_small_kernel", "general": "fa_rollout_kernel", "layered": "fa_layered"}[self.form]

    @property
    def cost(self) -> str:
        return "cartpole" if self.nx == 4 else "quad_est"

    @property
    def victims(self) -> list[int]:
        """Sample 0, the middle slot of workgroup 0 (G >= 3), its last slot, the first of workgroup 1, sample K - 1."""
        G, v = self.G, {0, self.G - 1, self.G, self.K - 1}
        if G >= 3:
            v.add(G // 2)
        return sorted(v)

    @property
    def dirty_actuator(self) -> int:
        return self.nu // 2


CASES = [
    Case("small-L5-2layers", 4, 1, 64, 4, 2, 1, "small", 101),          # G = 3, one pad row
    Case("small-L6-4layers", 4, 2, 64, 4, 4, 1, "small", 102, dist=True),  # G = 2, four pad rows
    Case("general-D64-5layers-bf16", 4, 1, 64, 4, 5, 1, "general", 103),  # too deep for the small kernel; G = 3
    Case("general-D64-fp32", 4, 1, 64, 4, 2, 0, "general", 104),        # VALU attention, the control arm; G = 3
    Case("general-D128-4heads", 4, 2, 128, 4, 2, 1, "general", 105),    # MFMA attention, NT = 1; G = 2
    Case("general-D128-8heads", 4, 2, 128, 8, 2, 1, "general", 106, dist=True),
    Case("general-D512-4heads-L5", 4, 1, 512, 4, 2, 1, "general", 107),  # R = 64; G = 12
    Case("general-D512-8heads-L5", 4, 1, 512, 8, 2, 1, "general", 108),
    Case("general-D512-L21", 15, 6, 512, 4, 2, 1, "general", 109),      # G = 3, one pad row
    Case("general-D128-L49", 37, 12, 128, 4, 2, 1, "general", 110),     # NT = 4; G = 1, 15 pad rows
    Case("layered-L21", 15, 6, 512, 4, 2, 1, "layered", 111),           # the window covers 2 further samples
    Case("layered-L49", 37, 12, 512, 4, 2, 1, "layered", 112),          # 15 rows of the next sample, no whole one
]
BY_NAME = {c.name: c for c in CASES}


@functools.lru_cache(maxsize=None)
def weights(name: str) -> dict:
    """Seeded FA weights with the LayerNorm affines and the attention / out-proj biases moved off their init values, as
    tests/test_gpu_parity.py::_perturbed_fa."""
    from mppi_hip.nets import synthetic_feature_attention
    c = BY_NAME[name]
    sd = synthetic_feature_attention(c.nx, c.nu, c.D, num_heads=c.heads, attn_layers=c.layers, seed=c.seed)
    rs = np.random.RandomState(c.seed + 1)
    for k in list(sd):
        if k.endswith(("norm1.weight", "norm2.weight")) or k == "feature_encoding.1.weight":
            sd[k] = (1.0 + 0.2 * rs.randn(*sd[k].shape)).astype(np.float32)
        elif (k.endswith(("norm1.bias", "norm2.bias", "in_proj_bias", "out_proj.bias"))
              or k == "feature_encoding.1.bias"):
            sd[k] = (0.1 * rs.randn(*sd[k].shape)).astype(np.float32)
    return sd


@functools.lru_cache(maxsize=None)
def inputs(name: str) -> dict:
    """x0 [B, nx], U0 [B, nu, H], the clean noise [B, nu, H, K] and a second, independent draw `alt` of the same shape
    (float32, read-only)."""
    c = BY_NAME[name]
    rs = np.random.RandomState(c.seed + 7)
    out = dict(x0=(0.2 * rs.randn(B, c.nx)).astype(np.float32), U0=(0.1 * rs.randn(B, c.nu, H)).astype(np.float32),
               noise=(SIGMA * rs.randn(B, c.nu, H, c.K)).astype(np.float32),
               alt=(SIGMA * rs.randn(B, c.nu, H, c.K)).astype(np.float32))
    for a in out.values():
        a.setflags(write=False)
    return out


def finite_dirty(name: str, k: int) -> np.ndarray:
    """The clean noise with sample k of the victim solve replaced, whole column, by the other finite draw."""
    i = inputs(name)
    n = i["noise"].copy()
    n[VICTIM_SOLVE, :, :, k] = i["alt"][VICTIM_SOLVE, :, :, k]
    assert not np.array_equal(n, i["noise"])
    return n


def nonfinite_dirty(name: str, k: int, bad: float) -> np.ndarray:
    """The clean noise with one element of sample k of the victim solve set to `bad` (NaN or +inf): one actuator at the
    middle step, so in the reference the damage enters mid-rollout and stays in the sample's state rows."""
    c = BY_NAME[name]
    n = inputs(name)["noise"].copy()
    n[VICTIM_SOLVE, c.dirty_actuator, DIRTY_STEP, k] = bad
    return n


def bits(a) -> np.ndarray:
    """float32 array -> its bit patterns"""
    return np.ascontiguousarray(a, np.float32).view(np.uint32)
