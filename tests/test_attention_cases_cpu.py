"""CPU: the constructed attention cases (tests/attention_cases.py) have the properties they claim, the float32 emulation of the three
kernels (tools/attention_error.py) stays within a third of every budget at T = 128 and 256, and the budgets can tell a broken kernel:
every planted defect of the emulation exceeds the budget of the cases named in DEFECT_SHOWS."""
import os
import sys

import numpy as np
import pytest
import torch

import attention_cases as ac

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
import attention_error as ae      # noqa: E402

LOG2E = 1.4426950408889634
SMALL_T = (128, 256)


def _tile_max(case, T, D, b=0):
    """fp64 base-2 logits of image b, maximum per (query, tile)."""
    qkv = ac.make_case(case, b + 1, T, D)[b:b + 1]
    return (ac.logits64(qkv)[0] * LOG2E).reshape(T, T // ac.KT, ac.KT).amax(dim=2)


@pytest.mark.parametrize("D", [128, 256])
def test_constructors_are_deterministic_and_every_image_differs(D):
    for case in ac.CASES:
        a, b = ac.make_case(case, 3, 128, D), ac.make_case(case, 3, 128, D)
        assert a.dtype == torch.float32 and a.shape == (3, 128, 3 * D) and torch.equal(a, b) and bool(torch.isfinite(a).all())
        assert torch.equal(ac.make_case(case, 1, 128, D)[0], a[0])
        for i, j in ((0, 1), (0, 2), (1, 2)):
            assert not torch.equal(a[i, :, :2 * D], a[j, :, :2 * D]), (case, i, j)
        assert float(a[..., :2 * D].abs().max()) * LOG2E < 6.0e4            # theta x log2 e and phi fit fp16


@pytest.mark.parametrize("T,D", [(128, 128), (1152, 128), (4096, 128), (1152, 256)])
def test_one_hot_gap_and_expected_rows(T, D):
    qkv = ac.make_case("one_hot", 1, T, D)
    s = ac.logits64(qkv)[0]
    top = s.topk(2, dim=1)
    assert torch.equal(top.indices[:, 0], ac.one_hot_perm(T, D, 0))
    assert float((top.values[:, 0] - 100.0).abs().max()) < 1e-4
    assert float((top.values[:, 0] - top.values[:, 1]).min()) >= 40.0
    want = ac.one_hot_expected(T, D, 0)
    g = qkv[0, :, 2 * D:]
    assert torch.equal(want, g[ac.one_hot_perm(T, D, 0)])
    hi = g.half().float()
    lo = (g - hi).half().float()
    assert torch.equal(hi + lo, g)                                            # exact as hi + lo fp16 planes
    if T <= 1152:
        _, ref, _ = ac.reference("one_hot", 1, T, D)
        assert float((ref[0] - want.double()).abs().max()) < 1e-15


@pytest.mark.parametrize("T,D", [(128, 128), (256, 128), (384, 128), (1152, 128), (32, 256), (96, 256)])
def test_spikes_sit_in_the_named_tile_and_stream(T, D):
    nt = T // ac.KT
    for b in (0, 1):
        for case, tile in (("first_tile_spike", 0), ("late_spike_even", (nt - 1) & ~1), ("late_spike_odd", nt - 1 if nt > 1 and (nt - 1) & 1 else max(nt - 2, 0))):
            key = ac.spike_key(case, T, b)
            assert key // ac.KT == tile
            if D == 128:
                assert tile % 2 == (1 if case == "late_spike_odd" else 0) and (case == "first_tile_spike" or tile >= nt - 2)
            s = ac.logits64(ac.make_case(case, b + 1, T, D)[b:b + 1])[0] * LOG2E
            assert bool((s.argmax(dim=1) == key).all())
            rest = s.clone()
            rest[:, key] = -float("inf")
            assert float((s[:, key] - rest.amax(dim=1)).min()) >= 60.0
    assert ac.spike_key("late_spike_odd", T, 0) != ac.spike_key("late_spike_odd", T, 1)


@pytest.mark.parametrize("T", SMALL_T)
def test_fp32_merge_factor_is_exactly_zero_in_each_direction(T):
    for case, dead in (("late_spike_even", "s1"), ("first_tile_spike", "s1"), ("late_spike_odd", "s0")):
        _, info = ae.emulate_f32(ac.make_case(case, 1, T, 128)[0].numpy())
        live = "s0" if dead == "s1" else "s1"
        assert float(np.abs(info[dead]).max()) == 0.0 and float(info[live].min()) == 1.0, case


@pytest.mark.parametrize("T,D", [(128, 128), (1152, 128), (32, 256), (1152, 256)])
def test_all_negative_logits(T, D):
    s = ac.logits64(ac.make_case("all_negative", 2, T, D))
    assert float(s.max()) <= -190.0 and float(s.min()) >= -210.0


def test_uniform_rows_average_g():
    qkv, ref, scale = ac.reference("uniform_rows", 2, 128, 128)
    for b in range(2):
        for q in ac.UNIFORM_QUERIES + (127,):
            row = (q + b) % 128
            assert float(qkv[b, row, :128].abs().max()) == 0.0
            assert float((ref[b, row] - qkv[b, :, 256:].double().mean(dim=0)).abs().max()) < 1e-15
            assert float(ref[b, row].abs().max()) < 0.25 < float(scale[b, row])


@pytest.mark.parametrize("T,D", [(128, 128), (256, 128), (1152, 128), (64, 256), (1152, 256)])
def test_staircase_steps(T, D):
    """The tile maxima of every query climb by the stated step, inside (7, 8) for `under` and (8.5 - 0.5, 9) for `over`."""
    n, nt = ac.stair_tiles(T), T // ac.KT
    for case, lo, hi in (("staircase_under", 7.0, 8.0), ("staircase_over", 8.0, 9.0)):
        d = _tile_max(case, T, D).diff(dim=1)[:, nt - n:]
        assert d.shape[1] == n - 1 and float(d.min()) > lo and float(d.max()) < hi, (case, float(d.min()), float(d.max()))
    m = _tile_max("plateau_under", T, D)[:, nt - n:]
    d0 = m[:, 1:] - m[:, :1]
    assert float(d0.min()) > 7.0 and float(d0.max()) < 8.0


@pytest.mark.parametrize("T", SMALL_T)
def test_emulated_rescale_counts_and_largest_p(T):
    """Single-stream kernels (h16, d256): `over` rescales at every staircase tile above the base, `under` at every second one with
    P = 2^7.5 between, the plateau never.  The fp32 kernel's two streams see steps of 15 / 17: every stream tile after its first
    rescales on both staircases; the plateau never."""
    n = ac.stair_tiles(T)
    assert n == T // ac.KT                                   # T <= 512: the staircase covers every tile
    want = {"staircase_over": n - 1, "staircase_under": (n - 1) // 2, "plateau_under": 0}
    for case in want:
        for kernel in ("h16", "h16_pv1", "d256"):
            _, (info,) = ae.emulate_batch(kernel, ac.make_case(case, 1, T, ae.KERNELS[kernel][0]).numpy())
            assert (info["rescales"] == want[case]).all(), (kernel, case, np.unique(info["rescales"]))
            if case == "staircase_over":
                assert float(info["pmax"].max()) < 2.0
            else:
                assert float(info["pmax"].min()) >= 2.0 ** 7 and float(info["pmax"].max()) <= 2.0 ** 8
        _, info = ae.emulate_f32(ac.make_case(case, 1, T, 128)[0].numpy())
        assert (info["rescales"] == (0 if case == "plateau_under" else n - 2)).all(), (case, np.unique(info["rescales"]))
        if case == "plateau_under":
            assert float(info["pmax"].min()) >= 2.0 ** 7 and float(info["pmax"].max()) <= 2.0 ** 8


def test_budget_table_is_complete():
    for kernel in ae.KERNELS:
        assert set(ac.EMULATED[kernel]) == set(ac.CASES), kernel
        for case in ac.CASES:
            want = 1e-6 if (case == "one_hot" and kernel in ("f32", "d256")) else 3 * ac.EMULATED[kernel][case]
            assert ac.budget(kernel, case) == want
    # the hi-planes-only P.V form is its own, much wider, class
    assert ac.budget("h16_pv1", "benign") > 100 * ac.budget("h16", "benign")


@pytest.mark.parametrize("kernel", list(ae.KERNELS))
@pytest.mark.parametrize("T", SMALL_T)
def test_emulation_stays_within_a_third_of_every_budget(kernel, T):
    for case in ac.CASES:
        err, img, q = ae.emulated_error(kernel, case, 1, T)
        assert err <= ac.budget(kernel, case) / 3, (kernel, case, T, err, img, q)


# Which cases a planted defect must push over its budget (kernel, case); found with T = 256, B = 1.
DEFECT_SHOWS = {
    "drop_last_tile": [("f32", "late_spike_odd"), ("f32", "one_hot"), ("f32", "benign"), ("h16", "late_spike_odd"), ("h16", "staircase_over"),
                       ("h16_pv1", "late_spike_odd"), ("d256", "late_spike_odd"), ("d256", "benign")],
    "merge_unscaled": [("f32", "late_spike_even"), ("f32", "first_tile_spike"), ("f32", "one_hot"), ("f32", "benign")],      # not late_spike_odd: there stream 1's factor IS 1
    "rescale_o_only": [("f32", "staircase_over"), ("f32", "staircase_under"), ("h16", "staircase_over"), ("h16", "staircase_under"),
                       ("h16_pv1", "staircase_over"), ("d256", "staircase_over")],
    "hi_only": [("h16", "benign"), ("h16", "uniform_rows"), ("h16", "all_negative")],
    "swap_g_rows": [("f32", "one_hot"), ("h16", "one_hot"), ("h16_pv1", "one_hot"), ("d256", "one_hot"), ("f32", "benign")],
}


@pytest.mark.parametrize("defect", list(DEFECT_SHOWS))
def test_planted_defects_exceed_the_budgets(defect):
    assert set(DEFECT_SHOWS) == set(ae.DEFECTS)
    for kernel, case in DEFECT_SHOWS[defect]:
        err, _, _ = ae.emulated_error(kernel, case, 1, 256, defect=defect)
        assert err > ac.budget(kernel, case), (defect, kernel, case, err, ac.budget(kernel, case))


@pytest.mark.parametrize("T", SMALL_T)
def test_hi_only_products_are_ten_budgets_away_on_benign(T):
    err, _, _ = ae.emulated_error("h16", "benign", 1, T, defect="hi_only")
    assert err >= 10 * ac.budget("h16", "benign"), (T, err)
