"""The RGB baseline's UCB post-processing restatement (blindshadowremoval_amd/ucb_post_rgb.py) against the outputs of the reference's own
`FSRNet.test_step` of train_RGB_test.py (tests/golden/ucb_post_rgb_9156.npz, tools/make_ucb_post_rgb_fixture.py) on the same inputs."""
import hashlib
import os

import numpy as np
import pytest

from blindshadowremoval_amd.ucb_post import resize_bilinear
from blindshadowremoval_amd.ucb_post_rgb import strip_of, ucb_postprocess_rgb
from ucb_cases import GOLDEN, cases

FIX = np.load(os.path.join(GOLDEN, "ucb_post_rgb_9156.npz"))


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def test_fixture_is_small_and_complete():
    assert os.path.getsize(os.path.join(GOLDEN, "ucb_post_rgb_9156.npz")) < 700_000
    assert str(FIX["backend"]) == "standin" or str(FIX["backend"]).startswith("tf-")
    keys = [c[0] for c in cases()]
    assert len(keys) == 10
    for k in keys:
        assert {k + "_ssim", k + "_psnr", k + "_strip_sha256"} <= set(FIX.files)
    assert sorted(k[:-4] for k in FIX.files if k.endswith("_out")) == sorted(k for k in keys if k.endswith("a"))


@pytest.mark.parametrize("case", list(cases()), ids=lambda c: c[0])
def test_matches_reference_code(case):
    key, row, box, masks, con, _ = case
    losses, figs = ucb_postprocess_rgb(row[..., 0:3], row[..., 3:6], con, box, masks["face_hair"])
    assert len(figs) == 3 and all(f.shape == (1, 256, 256, 3) and f.dtype == np.float32 for f in figs)
    strip = strip_of(figs)
    assert strip.shape == (256, 768, 3) and strip.dtype == np.uint8
    assert _sha(strip) == str(FIX[key + "_strip_sha256"]), key                                   # byte-equal strip
    if key + "_out" in FIX.files:
        np.testing.assert_array_equal(figs[1][0].astype(np.float16), FIX[key + "_out"])         # the composite, as float16
    assert abs(losses["ssim"] - float(FIX[key + "_ssim"])) < 1e-5
    assert abs(losses["psnr"] - float(FIX[key + "_psnr"])) < 1e-5


def test_grey_and_three_channel_masks_agree():
    for key, row, box, masks, con, _ in list(cases())[::3]:
        l3, f3 = ucb_postprocess_rgb(row[..., 0:3], row[..., 3:6], con, box, masks["face_hair"])
        l1, f1 = ucb_postprocess_rgb(row[..., 0:3], row[..., 3:6], con, box, masks["face_hair"][:, :, 0:1])
        assert l1 == l3, key
        for a, b in zip(f1, f3):
            np.testing.assert_array_equal(a, b)


def test_prediction_is_not_clipped_before_the_composite():
    """con far outside [0, 1]: inside the mask the composite is clip(resize(con)), NOT resize(clip(con)); outside it is the input."""
    key, row, box, masks, _, _ = next(iter(cases()))
    yy, xx = np.mgrid[0:256, 0:256]
    con = np.where(((yy + xx) % 2 == 0)[..., None], np.float32(1.7), np.float32(-0.6)).repeat(3, axis=2).astype(np.float32)
    con[..., 1] += np.float32(0.3)
    losses, figs = ucb_postprocess_rgb(row[..., 0:3], row[..., 3:6], con, box, masks["face_hair"])
    size = int(np.asarray(box).reshape(4)[3] - np.asarray(box).reshape(4)[1])
    m = np.round(resize_bilinear(masks["face_hair"][:, :, 0:1].astype(np.float32), size))[..., 0]
    assert (m == 1).sum() > 1000 and (m == 0).sum() > 1000
    out = figs[1][0, :size, :size]
    want_in = np.clip(resize_bilinear(con, size), 0, 1)
    pre_clipped = resize_bilinear(np.clip(con, 0, 1), size)
    inside = m == 1
    np.testing.assert_array_equal(out[inside], want_in[inside])
    assert np.abs(out[inside] - pre_clipped[inside]).max() > 0.1               # a pre-clip would give other values
    np.testing.assert_array_equal(out[~inside], np.clip(figs[0][0, :size, :size][~inside], 0, 1))
    assert (figs[1][0, size:] == 0).all() and (figs[1][0, :, size:] == 0).all()
    assert np.isfinite(losses["ssim"]) and np.isfinite(losses["psnr"])


def test_bad_box_raises():
    key, row, box, masks, con, _ = next(iter(cases()))
    b = np.asarray(box, np.float32).reshape(4).copy()
    b[3] = b[1] + 300
    with pytest.raises(ValueError):
        ucb_postprocess_rgb(row[..., 0:3], row[..., 3:6], con, b, masks["face_hair"])
