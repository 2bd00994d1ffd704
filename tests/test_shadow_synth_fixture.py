"""The host statement (blindshadowremoval_amd/shadow_synth.py) against tests/golden/shadow_synth_*.npz: the reference's own process_mask and
the utils.py functions it calls, executed from their source over a numpy TensorFlow stand-in by tools/make_shadow_synth_fixture.py with
every tf.random draw taken from a tape that also filled the ShadowDraws record stored beside the outputs.  The 16 branch combinations
at S = 64, three at S = 128.  No GPU."""
import glob
import os

import numpy as np
import pytest

from blindshadowremoval_amd import shadow_synth as host

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FILES = sorted(glob.glob(os.path.join(GOLDEN, "shadow_synth_*.npz")))


def cases():
    for path in FILES:
        z = np.load(path)
        ci = 0
        while "c%d_seed" % ci in z.files:
            yield os.path.basename(path), ci, z
            ci += 1


@pytest.fixture(scope="module")
def results():
    """Every fixture case run through the host statement once: [(label, fixture arrays of the case, host result, tolerance)]."""
    out = []
    for name, ci, z in cases():
        S = int(z["S"])
        d = host.unpack_draws(z["c%d_draws" % ci])
        arrays = [a[0] for a in host.example_inputs(S, 1, int(z["c%d_seed" % ci]))]
        tol = 4.0 * float(z["measured_max_diff"])
        assert 0 < tol <= 1e-4
        out.append(("%s case %d" % (name, ci), {k: z["c%d_%s" % (ci, k)] for k in ("perlin_map", "img", "mask_sv", "mask_edge", "combo")},
                    host.process_item(*arrays, d), tol))
    return out


def test_the_fixture_covers_the_sixteen_branch_combinations():
    assert len(FILES) == 7
    combos = {(int(z["S"]),) + tuple(int(v) for v in z["c%d_combo" % ci]) for _, ci, z in cases()}
    assert len({c[1:] for c in combos if c[0] == 64}) == 16 and len({c for c in combos if c[0] == 128}) == 3


def test_perlin_map_to_1e_5(results):
    seen = 0
    for label, fx, res, _ in results:
        if fx["combo"][0]:
            seen += 1
            err = float(np.abs(res["perlin_map"].astype(np.float64) - fx["perlin_map"]).max())
            assert err <= 1e-5, "%s: Perlin map differs by %.3g" % (label, err)
    assert seen == 10


def test_thresholded_mask_exactly(results):
    for label, fx, res, _ in results:
        if fx["combo"][0]:
            assert np.abs(fx["perlin_map"].astype(np.float64) - 0.15).min() > 1e-5, label          # what the tool asserted
            np.testing.assert_array_equal(res["thre"], (fx["perlin_map"] > np.float32(0.15)).astype(np.float32), err_msg=label)
            assert 0 < res["thre"].mean() < 1


def test_outputs_within_four_times_the_measured_difference(results):
    worst = 0.0
    for label, fx, res, tol in results:
        assert res["status"] == 0, label
        for k in ("img", "mask_sv", "mask_edge"):
            err = float(np.abs(res[k].astype(np.float64) - fx[k]).max())
            worst = max(worst, err)
            assert err <= tol, "%s: %s differs by %.3g, over %.3g" % (label, k, err, tol)
    print("shadow_synth fixture: max |host - reference| %.3g" % worst)


def test_face_darken_pieces_against_the_references():
    """apply_tone_curve(is_rgb=True), get_ctm_ls and apply_ctm of the reference are numpy already; the same float64 operations on the same
    float32 image, so 1e-6 covers the least-squares solver's freedom (values are below 2)."""
    z = np.load(os.path.join(GOLDEN, "shadow_synth_64_0.npz"))
    img, gain = z["tone_in"], z["tone_gain"]
    tone = host.apply_tone_curve_rgb(img, gain)
    assert np.abs(tone - z["tone_out"]).max() <= 1e-6
    cm = host.colour_matrix(img, tone)
    assert cm.shape == (3, 3) and np.abs(cm - z["tone_ctm"]).max() <= 1e-6
    assert np.abs(host.apply_ctm(img, cm) - z["tone_applied"]).max() <= 1e-6
    aug, dark, cm2 = host.face_darken(img, gain, gain)
    np.testing.assert_array_equal(aug, dark)
    assert np.abs(dark - z["tone_applied"]).max() <= 1e-6 and np.abs(cm2 - z["tone_ctm"]).max() <= 1e-6


def test_unpack_draws_inverts_pack_draws():
    d = host.draw(np.random.default_rng(0), 64)
    words = host.pack_draws([d], 64)[0]
    np.testing.assert_array_equal(host.pack_draws([host.unpack_draws(words)], 64)[0], words)


def test_a_constant_blend_guidance_selects_the_finest_level():
    """Rule 3: all-zero guidance gradients with a lit map — the reference divides 0 by 0; we take the r = blur_size level."""
    rng = np.random.default_rng(7)
    d = host.draw(rng, 32)
    d.u_mask, d.u_sv, d.u_ss, d.blur_size = np.float32(0.2), np.float32(0.9), np.float32(0.1), np.int32(2)
    for g in d.g_guide:
        g[:] = 0
    arrays = [a[0] for a in host.example_inputs(32, 1, 7)]
    res = host.process_item(*arrays, d)
    assert res["status"] == 0 and res["thre"].any() and np.isfinite(res["img"]).all()
    p0 = host.apply_disc_filter(res["thre"], 2)
    np.testing.assert_array_equal(res["mask"][:, :, 0], arrays[3][:, :, 0] * (p0 / p0.max()))
