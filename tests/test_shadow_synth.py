"""The host statement of the shadow synthesis (blindshadowremoval_amd/shadow_synth.py) on its own: the two disc forms against each
other, the Gaussian's edges, the rules of our own, draw()'s ranges and the command-line entry.  No GPU."""
import os

import numpy as np
import pytest

from blindshadowremoval_amd import shadow_synth as host

from shadow_synth_cases import f32, inputs, largest_r, record


@pytest.mark.parametrize("r", [1, 2, 8, 11])
def test_fft_and_direct_disc_forms_agree(r):
    S = 32
    rng = np.random.default_rng(r)
    corners = np.zeros((S, S))
    corners[0, 0] = corners[0, -1] = corners[-1, 0] = corners[-1, -1] = 1.0
    for m in (rng.random((S, S)), (rng.random((S, S)) > 0.5).astype(np.float64), corners):
        a, b = host.apply_disc_filter_fft(m, r), host.apply_disc_filter_direct(m, r)
        assert np.abs(a - b).max() <= 1e-12
        assert np.abs(a[0] - b[0]).max() <= 1e-12 and np.abs(a[:, 0] - b[:, 0]).max() <= 1e-12
    w = float(host.create_disc_filter(r).max())
    # the one-pixel offset: a lit pixel (y, x) is the centre tap of output (y + 1, x + 1)
    single = np.zeros((S, S)); single[15, 17] = 1.0
    blur = host.apply_disc_filter_direct(single, r)
    ys, xs = np.nonzero(blur)
    assert (ys.min() + ys.max()) == 2 * 16 and (xs.min() + xs.max()) == 2 * 18 and blur[16, 18] > 0
    # the wrapped term: the lit pixel (S-1, S-1) (S-1, x) reaches output (0, x + 1) and nothing else of row 0
    edge = np.zeros((S, S)); edge[S - 1, 10] = 1.0
    assert np.isclose(host.apply_disc_filter_direct(edge, r)[0, 11], w) and host.apply_disc_filter_direct(edge, r)[0].sum() == pytest.approx(w)
    edge = np.zeros((S, S)); edge[10, S - 1] = 1.0
    assert np.isclose(host.apply_disc_filter_direct(edge, r)[11, 0], w)


def test_the_narrowest_gaussian_is_the_identity():
    x = np.random.default_rng(0).random((32, 32), dtype=f32)
    np.testing.assert_array_equal(host.gaussian_taps(f32(0.042)), np.array([0, 1, 0], f32))
    np.testing.assert_array_equal(host.gaussian_filter(x, f32(0.042)), x)


@pytest.mark.parametrize("S", [32, 64])
def test_radius_s_minus_one_passes_and_one_more_raises(S):
    r = largest_r(S)
    sigma = host.level_sigma(5, r)
    assert len(host.gaussian_taps(sigma)) == 2 * (S - 1) + 1
    x = np.random.default_rng(1).random((S, S), dtype=f32)
    y = host.gaussian_filter(x, sigma)
    assert y.shape == x.shape and np.isfinite(y).all() and x.min() <= y.min() and y.max() <= x.max()
    over = r
    while len(host.gaussian_taps(host.level_sigma(5, over))) == 2 * (S - 1) + 1:
        over = np.nextafter(over, f32(100))
    with pytest.raises(ValueError, match="REFLECT"):
        host.gaussian_filter(x, host.level_sigma(5, over))
    with pytest.raises(ValueError, match="REFLECT"):
        host.check_scale(over, S)
    with pytest.raises(ValueError, match="REFLECT"):
        host.pack_draws([record(np.random.default_rng(2), S, r=over)], S)
    host.check_scale(np.nextafter(f32(15), f32(0)), 256)          # the reference's full range fits at 256


def test_all_zero_gradients_give_the_empty_mask_status():
    rng = np.random.default_rng(3)
    arrays = inputs(32, 2, seed=3)
    for i, sv in enumerate((True, False)):
        d = record(rng, 32, sv=sv)
        for g in d.g_shadow + d.g_guide + d.g_bright:
            g[:] = 0
        res = host.process_item(*(a[i] for a in arrays), d)
        assert res["status"] == host.STATUS_EMPTY and not res["thre"].any()
        np.testing.assert_array_equal(res["img"], np.clip(arrays[1][i], 0, 1))
        assert not res["mask_sv"].any() and not res["mask_edge"].any()
    img, mask_sv, mask_edge, status = host.process_mask(*arrays, [record(rng, 32), d])
    assert status.tolist() == [host.STATUS_OK, host.STATUS_EMPTY] and img.shape == (2, 32, 32, 3) and img.dtype == f32


def test_draw_stays_in_the_references_ranges():
    rng = np.random.default_rng(4)
    seen_disc, seen_blur = set(), set()
    for i in range(1000):
        d = host.draw(rng, (32, 64, 128, 256)[i % 4])
        for u in (d.u_mask, d.u_ss, d.u_bright, d.u_sv):
            assert isinstance(u, np.float32) and 0 <= u < 1
        assert isinstance(d.disc_sz, np.int32) and 1 <= d.disc_sz <= 11 and isinstance(d.blur_size, np.int32) and d.blur_size in (1, 2)
        seen_disc.add(int(d.disc_sz)); seen_blur.add(int(d.blur_size))
        assert f32(0.05) <= d.p_shadow <= f32(0.85) and f32(0.05) <= d.p_guide <= f32(0.25) and f32(0.05) <= d.p_bright <= f32(0.25)
        assert isinstance(d.r, np.float32) and 1 <= d.r < 15
        assert d.gains.dtype == f32 and d.gains.shape == (6,) and (d.gains >= f32(1.1)).all() and (d.gains <= f32(1.5)).all()
        for gs, sides in ((d.g_shadow, (5, 9, 17, 33)), (d.g_guide, (3,)), (d.g_bright, (3, 5))):
            assert [g.shape for g in gs] == [(s, s, 2) for s in sides]
            for g in gs:
                assert g.dtype == f32 and np.abs((g ** 2).sum(axis=2) - 1).max() < 1e-6
    assert seen_disc == set(range(1, 12)) and seen_blur == {1, 2}
    assert host.pack_draws([d], 256).shape == (1, host.DRAW_WORDS)


def test_outputs_are_float32_in_range_and_consistent():
    rng = np.random.default_rng(5)
    arrays = inputs(64, 1, seed=5)
    for perlin in (True, False):
        res = host.process_item(*(a[0] for a in arrays), record(rng, 64, perlin=perlin))
        assert res["status"] == 0
        for k in ("img", "mask_sv", "mask_edge"):
            assert res[k].dtype == f32 and res[k].shape == (64, 64, 3) and np.isfinite(res[k]).all()
        assert 0 <= res["img"].min() and res["img"].max() <= 1 and 0 <= res["mask_sv"].min() and res["mask_sv"].max() <= 1
        np.testing.assert_array_equal(res["mask_edge"], np.abs(res["mask_sv"] - res["mask"]))
        assert -1 <= res["bright"].min() and res["bright"].max() <= 1          # min_val (1 + noise), capped: the noise is signed


def test_command_line_entry_writes_a_tree_the_test_loader_lists(tmp_path):
    from blindshadowremoval_amd.dataset import Dataset
    from blindshadowremoval_amd.pngio import read_rgb_u8, write_png
    rng = np.random.default_rng(6)
    S = 32
    # 68 landmarks spread over the crop (pixels): a ring and an inner grid
    ang = np.linspace(0, 2 * np.pi, 40, endpoint=False)
    lm = np.concatenate([np.stack([16 + 12 * np.cos(ang), 16 + 12 * np.sin(ang)], 1), rng.uniform(8, 24, (28, 2))]).astype(np.float32)
    src, dst = tmp_path / "src", tmp_path / "dst"
    for name in ("a", "b"):
        write_png(str(src / name / (name + ".png")), rng.integers(30, 220, (S, S, 3), dtype=np.uint8))
        np.save(str(src / name / (name + ".npy")), lm)
    assert host.main([str(src), str(dst), "--seed", "3", "--host", "--batch", "2"]) == 0

    class Config:
        DATA_DIR_TEST = [str(dst / "*")]
    names = Dataset(Config(), "test").name_list
    assert [os.path.basename(n) for n in names] == ["a.npy", "b.npy"]
    for name in ("a", "b"):
        shadowed, gt = read_rgb_u8(str(dst / name / (name + ".png"))), read_rgb_u8(str(dst / name / (name + "-gt.png")))
        mask = read_rgb_u8(str(dst / name / (name + "-mask.png")))
        assert shadowed.shape == gt.shape == mask.shape == (S, S, 3) and mask.any() and (shadowed != gt).any()
        np.testing.assert_array_equal(np.load(str(dst / name / (name + ".npy"))), lm)
