"""Constructed inputs, the fp64 reference and the error metric of the attention kernels' own tests (CPU only; shared by
tests/test_attention_cases_cpu.py, tests/test_attention_edges_gpu.py and tools/attention_error.py).

The operation is the NonLocalBlock's attention, y = softmax(theta phi^T) g with NO 1/sqrt(d) (model.py:51-53).  Every constructor is
deterministic and returns fp32 ``qkv [B, T, 3 D]`` (theta | phi | g), D = 128 (csrc/attention.h, csrc/attention_h16.h) or 256
(csrc/attention256.h).  Image b of a case depends on (case, T, D, b) alone, so a batch's images all differ — a wrong (image, query block)
map shows — and image b is the same whatever the batch around it.

All three kernels work on 32-key tiles in base-2 logits with a LAZY running maximum: it moves only when a tile exceeds it by more than 8
log2 units, decided once per wave of 32 queries.  The cases aim at that:

benign            randn * 0.5.
one_hot           phi rows are random unit vectors, theta[q] = 100 phi[perm[q]] (the winner's logit is 100, the runner-up's below 60),
                  g[k, d] = (k' D + d) / 2^19 with k' = (k + 5 b) mod T — exact in fp32 and as hi + lo fp16.  Output row q is
                  g[perm[q]]: a wrong key or channel index in a V fragment or a swizzle is an O(1) error on a known element.
staircase_under   queries a e + noise, keys c_t e + noise (noise orthogonal to e): over the last min(T / 32, 16) tiles the logit climbs
staircase_over    by 7.5 / 8.5 log2 units PER TILE.  `over` rescales at every tile of the staircase in a single-stream kernel.  `under`
                  as stated cannot stay below the threshold for more than one tile (two steps are 15 > 8): a single-stream kernel
                  rescales at every SECOND staircase tile and runs the tiles between with P = 2^7.5.  The two-stream fp32 kernel sees
                  every other tile, steps of 15 / 17, and rescales at each tile of either staircase.
plateau_under     the threshold's worst case proper: the first tile of that region sits at level 0, every later one 7.5 log2 units
                  above it — no rescale after the first tile, P = 2^7.5 for up to 15 consecutive tiles.
late_spike_even   one dominant key (logit ~ +170 log2 units over every other) in the last even tile / the last odd tile / tile 0: in the
late_spike_odd    fp32 kernel's merge of its even and odd key streams one stream's factor is then exactly 0, in each direction.  (With
first_tile_spike  a single tile, T = 32 at D = 256, there is no odd tile and the spike of late_spike_odd sits in tile 0.)
all_negative      every logit in [-210, -190]: a running maximum that does not start at -inf (or at the first tile) gives 0 / 0.
uniform_rows      a few all-zero queries among benign ones: the output is the mean of g, small.

Metric (per query, so that large rows cannot hide small ones, and with no blow-up under cancellation):
    err_q = max_d |got - ref| / max_d sum_k P_qk |g_kd|          (denominator in fp64)
a case's error is the maximum over its queries, reported with the worst (image, query).
"""
from __future__ import annotations

import math

import numpy as np
import torch

CASES = ("benign", "one_hot", "staircase_under", "staircase_over", "plateau_under", "late_spike_even", "late_spike_odd",
         "first_tile_spike", "all_negative", "uniform_rows")
KT = 32                                  # keys per tile, every kernel
LN2 = math.log(2.0)
STAIR_STEP = {"staircase_under": 7.5, "staircase_over": 8.5, "plateau_under": 7.5}     # log2 units
STAIR_A = 8.0                            # the queries' component along e
SPIKE_A, SPIKE_C = 3.0, 40.0             # queries' component along e; the spike key's: logit 120 = 173 log2 units
UNIFORM_QUERIES = (3, 31, 32)            # and T - 1

# What the tests run (the issue's list; the d = 256 kernel also at 128 and 256 so that the CPU check at those T is inside its budget's range)
T_128 = (128, 256, 384, 1152)
T_128_BIG = 4096                         # benign and one_hot only, B = 1
T_256 = (32, 64, 96, 128, 256, 1152)
B_128, B_256 = 3, 2
BIG_CASES = ("benign", "one_hot")


def _gen(case: str, T: int, D: int, b: int) -> torch.Generator:
    return torch.Generator().manual_seed(1_000_003 * CASES.index(case) + 7919 * T + 31 * D + b)


def _unit(v: torch.Tensor) -> torch.Tensor:
    return v / v.norm(dim=-1, keepdim=True)


def _orth(x: torch.Tensor, e: torch.Tensor) -> torch.Tensor:
    """x with its component along the unit vector e removed (fp64 inside)."""
    xd, ed = x.double(), e.double()
    return (xd - (xd @ ed)[:, None] * ed).float()


def stair_tiles(T: int) -> int:
    return min(T // KT, 16)


def stair_levels(case: str, T: int) -> np.ndarray:
    """Per tile: the level (log2 units) of the logits of every query against that tile's keys."""
    nt, n = T // KT, stair_tiles(T)
    lv = np.zeros(nt)
    j = np.arange(n)
    lv[nt - n:] = STAIR_STEP[case] * (np.minimum(j, 1) if case == "plateau_under" else j)
    return lv


def spike_key(case: str, T: int, b: int) -> int:
    nt = T // KT
    if case == "first_tile_spike":
        tile = 0
    elif case == "late_spike_even":
        tile = (nt - 1) & ~1
    else:
        tile = nt - 1 if (nt - 1) & 1 else max(nt - 2, 0)
    return tile * KT + (13 + 7 * b) % KT


def one_hot_perm(T: int, D: int, b: int) -> torch.Tensor:
    return torch.randperm(T, generator=torch.Generator().manual_seed(424243 + 7919 * T + 31 * D + b))


def one_hot_expected(T: int, D: int, b: int) -> torch.Tensor:
    """g[perm[q]] of image b: the row the one_hot output must reproduce (fp32, exact)."""
    k = (one_hot_perm(T, D, b) + 5 * b) % T
    return ((k[:, None] * D + torch.arange(D)[None, :]).double() / 2.0 ** 19).float()


def _image(case: str, T: int, D: int, b: int) -> torch.Tensor:
    g = _gen(case, T, D, b)
    rn = lambda *s: torch.randn(*s, generator=g)
    if case in ("benign", "uniform_rows"):
        x = rn(T, 3 * D) * 0.5
        if case == "uniform_rows":
            for q in UNIFORM_QUERIES + (T - 1,):
                x[(q + b) % T, :D] = 0.0
        return x
    if case == "one_hot":
        phi = _unit(rn(T, D).double()).float()
        theta = 100.0 * phi[one_hot_perm(T, D, b)]
        k = (torch.arange(T) + 5 * b) % T
        gg = ((k[:, None] * D + torch.arange(D)[None, :]).double() / 2.0 ** 19).float()
        return torch.cat((theta, phi, gg), dim=1)
    e = _unit(rn(D).double()).float()
    if case in STAIR_STEP:
        lv = torch.from_numpy(stair_levels(case, T)).repeat_interleave(KT)            # [T], log2 units
        c = (lv * LN2 / STAIR_A).float()
        theta = STAIR_A * e[None, :] + _orth(rn(T, D) * 0.01, e)
        phi = c[:, None] * e[None, :] + _orth(rn(T, D) * 0.3, e)
        return torch.cat((theta, phi, rn(T, D) * 0.5), dim=1)
    if case in ("late_spike_even", "late_spike_odd", "first_tile_spike"):
        theta = SPIKE_A * e[None, :] + _orth(rn(T, D) * 0.2, e)
        phi = _orth(rn(T, D) * 0.5, e)
        phi[spike_key(case, T, b)] += SPIKE_C * e
        return torch.cat((theta, phi, rn(T, D) * 0.5), dim=1)
    if case == "all_negative":
        theta = 10.0 * e[None, :] + _orth(rn(T, D) * 0.2, e) * (128.0 / D) ** 0.5
        phi = -20.0 * e[None, :] + _orth(rn(T, D) * 0.5, e)
        return torch.cat((theta, phi, rn(T, D) * 0.5), dim=1)
    raise KeyError(case)


def make_case(case: str, B: int, T: int, D: int) -> torch.Tensor:
    assert D in (128, 256) and T % KT == 0 and T > 0 and B > 0
    return torch.stack([_image(case, T, D, b) for b in range(B)]).contiguous()


_REF_CACHE: dict = {}


def reference(case: str, B: int, T: int, D: int):
    """(qkv fp32, ref fp64 [B,T,D], scale fp64 [B,T]) — computed once per (case, B, T, D) and shared; callers leave them unchanged."""
    key = (case, B, T, D)
    if key not in _REF_CACHE:
        qkv = make_case(case, B, T, D)
        ref, scale = reference_of(qkv)
        _REF_CACHE[key] = (qkv, ref, scale)
    return _REF_CACHE[key]


def logits64(qkv: torch.Tensor) -> torch.Tensor:
    D = qkv.shape[2] // 3
    q, k, _ = (t.double() for t in qkv.split(D, dim=2))
    return q @ k.transpose(1, 2)


def reference_of(qkv: torch.Tensor):
    """fp64 softmax(theta phi^T) g and the metric's per-query scale max_d sum_k P_qk |g_kd|."""
    D = qkv.shape[2] // 3
    v = qkv[:, :, 2 * D:].double()
    refs, scales = [], []
    for b in range(qkv.shape[0]):                      # one image at a time: T x T doubles
        p = torch.softmax(logits64(qkv[b:b + 1])[0], -1)
        refs.append(p @ v[b])
        scales.append((p @ v[b].abs()).amax(dim=1))
    return torch.stack(refs), torch.stack(scales)


def case_error(got, ref: torch.Tensor, scale: torch.Tensor):
    """(err, image, query): the metric's maximum over a case's queries and where it is.  A non-finite output counts as infinite."""
    got = torch.as_tensor(np.asarray(got)) if not isinstance(got, torch.Tensor) else got
    e = (got.double() - ref).abs().amax(dim=2) / scale
    e = torch.where(torch.isfinite(e), e, torch.full_like(e, float("inf")))
    i = int(e.argmax())
    return float(e.flatten()[i]), i // e.shape[1], i % e.shape[1]


# ---- budgets -------------------------------------------------------------------------------------------------------------------------
# EMULATED[kernel][case] = the error of the kernel's arithmetic restated in float32 numpy (tools/attention_error.py), maximum over the
# tested T (profiles/attention_edges_emulation.txt has the figure of every T).  The budget is 3 x that — the factor
# tests/test_wino_conv2_gpu.py uses: the matrix cores fuse and order their sums differently from the emulation.  The figures come from the
# emulation alone, never from a kernel's output.  one_hot on the fp32 kernels has the fixed budget 1e-6: the row is expected back exactly.
EMULATED = {
    "f32": {"benign": 3.42e-6, "one_hot": 6.72e-31, "staircase_under": 1.23e-5, "staircase_over": 1.01e-5, "plateau_under": 4.33e-7, "late_spike_even": 0.0, "late_spike_odd": 0.0, "first_tile_spike": 0.0, "all_negative": 4.39e-5, "uniform_rows": 3.01e-6},
    "h16": {"benign": 4.51e-6, "one_hot": 4.90e-26, "staircase_under": 5.05e-6, "staircase_over": 5.18e-6, "plateau_under": 2.65e-7, "late_spike_even": 1.06e-7, "late_spike_odd": 8.89e-8, "first_tile_spike": 9.95e-8, "all_negative": 1.39e-5, "uniform_rows": 1.83e-6},
    "h16_pv1": {"benign": 7.29e-4, "one_hot": 4.88e-4, "staircase_under": 2.66e-4, "staircase_over": 2.40e-4, "plateau_under": 1.32e-4, "late_spike_even": 4.26e-4, "late_spike_odd": 3.84e-4, "first_tile_spike": 4.06e-4, "all_negative": 3.56e-4, "uniform_rows": 6.81e-4},
    "d256": {"benign": 6.27e-6, "one_hot": 4.08e-37, "staircase_under": 1.54e-5, "staircase_over": 1.42e-5, "plateau_under": 8.12e-7, "late_spike_even": 0.0, "late_spike_odd": 0.0, "first_tile_spike": 0.0, "all_negative": 5.70e-5, "uniform_rows": 6.27e-6},
}
ONE_HOT_F32_BUDGET = 1e-6


def budget(kernel: str, case: str) -> float:
    if case == "one_hot" and kernel in ("f32", "d256"):
        return ONE_HOT_F32_BUDGET
    return 3.0 * EMULATED[kernel][case]
