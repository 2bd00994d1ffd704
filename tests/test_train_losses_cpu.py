"""The host statement of train_step's reconstruction and gradient losses (blindshadowremoval_amd/train_losses.py) on constructed inputs
with closed-form answers, and what example_inputs promises.  No GPU."""
import numpy as np
import pytest

from blindshadowremoval_amd import train_losses as host

import train_losses_cases as cases

f32 = np.float32


@pytest.mark.parametrize("check", cases.ALL, ids=lambda c: c.__name__)
def test_constructed_case(check):
    check(host.step_losses)


def test_two_dilations_are_one_clipped_nine_by_nine_window():
    rng = np.random.default_rng(0)
    e = (rng.random((40, 40)) > 0.97).astype(f32)
    want = np.zeros_like(e)
    for y, x in zip(*np.nonzero(e)):
        want[max(y - 4, 0):y + 5, max(x - 4, 0):x + 5] = 1
    np.testing.assert_array_equal((host.dilate5(host.dilate5(e)) > 0).astype(f32), want)


@pytest.mark.parametrize("scale", host.SCALES)
def test_ramp_gradient_planes_are_constant_away_from_the_last_row_and_column(scale):
    S = 64
    yy, xx = np.meshgrid(np.arange(S, dtype=f32), np.arange(S, dtype=f32), indexing="ij")
    ramp = np.repeat(((yy / f32(64)) + (xx / f32(32)))[:, :, None], 3, axis=2).astype(f32)
    g = host.coarse_grad(ramp, scale)
    s = S // scale
    assert g.shape == (s, s, 3)
    np.testing.assert_allclose(g[:-1, :-1], 5.0 * scale * (1 / 64 + 1 / 32), rtol=1e-6)
    np.testing.assert_allclose(g[-1, :-1], 5.0 * scale / 32, rtol=1e-6)            # the last row has no dy
    np.testing.assert_allclose(g[:-1, -1], 5.0 * scale / 64, rtol=1e-6)            # the last column no dx
    assert g[-1, -1].tolist() == [0, 0, 0]
    full = host.img_grad(ramp, scale)
    edge = 0 if scale == 1 else (3 * scale) // 2
    assert full.shape == (S, S, 3)
    np.testing.assert_allclose(full[:S - 1 - edge, :S - 1 - edge], 5.0 * scale * (1 / 64 + 1 / 32), rtol=1e-6)


@pytest.mark.parametrize("S,B", [(32, 3), (64, 2), (256, 1)])
def test_example_inputs_hold_every_promised_area(S, B):
    img, gt, mask_sv, gs, con = host.example_inputs(S, B, seed=9)
    assert img.shape == gt.shape == mask_sv.shape == con.shape == (B, S, S, 3) and gs.shape == (B, S, S, 1)
    assert all(a.dtype == f32 and a.flags.c_contiguous for a in (img, gt, mask_sv, gs, con))
    e0 = host.edge0(mask_sv)
    mean_c, min_c = mask_sv.mean(axis=3), mask_sv.min(axis=3)
    for b in range(B):
        assert (mask_sv[b].max(axis=2) == 0).mean() > 0.25                              # an empty area
        between = (mean_c[b] > .01) & (min_c[b] <= .3)
        assert between.sum() >= S * S // 16 and (e0[b][between] == 1).all()            # an area between .01 and .3
        above = min_c[b] > .3
        assert above.sum() >= S * S // 16 and (e0[b][above] == 0).all()                # an area above .3 in all channels
        lit = mean_c[b] > .01
        pad = np.pad(lit, 1)
        neighbours = sum(pad[1 + dy:1 + dy + S, 1 + dx:1 + dx + S] for dy in (-1, 0, 1) for dx in (-1, 0, 1)) - lit
        assert (lit & (neighbours == 0) & (np.arange(S)[:, None] > 0) & (np.arange(S)[:, None] < S - 1)).sum() >= 1      # an isolated lit pixel
        assert lit[0, 0] and lit[S - 1, S - 1] and not lit[0, S - 1] and not lit[S - 1, 0]      # two opposite corners
        assert lit[S - 1].sum() >= S // 4                                                       # along one border
    # smooth with added noise: neighbouring pixels are close, and differ
    for a in (gt, img, gs, con):
        d = np.abs(np.diff(a, axis=2))
        assert 0 < np.median(d) < 0.1
    r = host.step_losses(img, gt, mask_sv, gs, con)
    assert 0 < r["bmaskgt"].mean() < 1 and 0 < r["mask_edge"].mean() < 1 and (r["losses"] > 0).all()


def test_shapes_and_sizes_are_checked():
    arrays = list(host.example_inputs(32, 1, 0))
    with pytest.raises(ValueError, match="32, 64, 128 or 256"):
        host.step_losses(*(np.zeros((1, 48, 48, c), f32) for c in (3, 3, 3, 1, 3)))
    with pytest.raises(ValueError, match="gs must be"):
        host.step_losses(arrays[0], arrays[1], arrays[2], arrays[4], arrays[4])


def test_the_package_exports_the_device_binding_lazily():
    import blindshadowremoval_amd
    assert "TrainLosses" in blindshadowremoval_amd.__all__
    from blindshadowremoval_amd import _lib
    assert "bsr_train_losses" in _lib.EXPORTS and "bsr_train_losses_scratch_bytes" in _lib.EXPORTS
    assert len(host.SUM_NAMES) == host.K == 18
