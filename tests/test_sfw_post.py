"""sfw_post.py — the host statement of the GSC model's test_step_sfw after the generator call (/root/reference/train_test_GSC.py:799-838) —
against tests/golden/sfw_post_gsc.npz, produced by executing the reference's own test_step_sfw with sklearn.metrics
(tools/make_sfw_post_fixture.py) over the cases of tests/sfw_post_cases.py."""
import hashlib
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _fixture():
    return np.load(os.path.join(GOLDEN, "sfw_post_gsc.npz"))


@pytest.mark.parametrize("idx", range(6))
def test_sfw_post_matches_the_reference_step(idx):
    from blindshadowremoval_amd.sfw_post import sfw_postprocess, strip_of
    from sfw_post_cases import cases
    key, img, con, mask, dif, face = cases()[idx]
    z = _fixture()
    losses, figs = sfw_postprocess(img, con, mask, dif, face)
    assert list(losses) == ["ssim", "psnr", "auc"]
    assert abs(losses["ssim"] - float(z[key + "_ssim"])) <= 1e-4, key
    assert abs(losses["psnr"] - float(z[key + "_psnr"])) <= 1e-4, key
    assert abs(losses["auc"] - float(z[key + "_auc"])) <= 1e-12, key          # sklearn's trapezoids vs the exact rational
    assert np.float32(losses["auc"]) == z[key + "_auc_f32"]
    strip = strip_of(figs)
    assert strip.shape == (256, 1024, 3)
    assert hashlib.sha256(np.ascontiguousarray(strip).tobytes()).hexdigest() == str(z[key + "_strip_sha256"]), key


def test_sfw_post_cases_cover_the_edges():
    from sfw_post_cases import cases
    c = {k: (mask, (dif * face).astype(np.float32)) for k, _, _, mask, dif, face in cases()}
    p = c["ties"][1]
    assert (p == 0).mean() > 0.5
    p = c["negzero"][1]
    assert (np.signbit(p) & (p == 0)).any() and (~np.signbit(p) & (p == 0)).any()
    p = c["subnormal"][1]
    assert ((p != 0) & (np.abs(p) < np.finfo(np.float32).tiny)).sum() > 1000
    assert not (c["nopos"][0] == 2).any()
    assert (c["allface"][1] != 0).all()
    m = c["near2"][0]
    assert (m == 2).any() and ((np.abs(m - 2) < 1e-3) & (m != 2)).any()


def test_sfw_post_raises_on_non_finite_scores_and_video_figs():
    from blindshadowremoval_amd.sfw_post import sfw_score, sfw_video_figs
    from sfw_post_cases import cases
    _, img, con, mask, dif, face = cases()[0]
    bad = dif.copy()
    bad[5, 7, 0] = np.nan
    face1 = np.ones_like(face)
    with pytest.raises(ValueError):
        sfw_score(mask, bad, face1)
    figs = sfw_video_figs(img, con, dif, face)
    assert [f.shape for f in figs] == [(1, 256, 256, 3), (1, 256, 256, 3), (1, 256, 256, 1)]
    np.testing.assert_array_equal(figs[2][0], (dif * face) * np.float32(2))
