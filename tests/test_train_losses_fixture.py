"""The host statement (blindshadowremoval_amd/train_losses.py) against tests/golden/train_losses_{32,64}.npz: the reference's own find_edge,
l1_loss, l1_loss_yuv, get_img_grad and the loss statements of train_step, executed from their source over a numpy TensorFlow stand-in
by tools/make_train_losses_fixture.py.  The binary planes exactly; the dif_grad figure and the losses within 4 x the difference the tool
measured (the stand-in reduces in float32, the statement in float64), never above 1e-4.  No GPU."""
import os

import numpy as np
import pytest

from blindshadowremoval_amd import train_losses as host

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module", params=[(32, 3), (64, 2)], ids=["S32", "S64"])
def case(request):
    S, B = request.param
    z = np.load(os.path.join(GOLDEN, "train_losses_%d.npz" % S))
    assert int(z["S"]) == S and int(z["B"]) == B and os.path.getsize(os.path.join(GOLDEN, "train_losses_%d.npz" % S)) < 1 << 20
    arrays = host.example_inputs(S, B, int(z["seed"]))
    return z, arrays, host.step_losses(*arrays)


def test_no_pixel_sits_on_a_threshold(case):
    z, (img, gt, mask_sv, _, _), _ = case          # what the tool asserted before it kept the seed
    m = mask_sv.astype(np.float64)
    dif = host.gray(gt).astype(np.float64) - host.gray(img).astype(np.float64)
    assert min(np.abs(m.mean(axis=3) - .01).min(), np.abs(m - .01).min(), np.abs(m.min(axis=3) - .3).min(), np.abs(dif - .04).min()) > 1e-5


def test_binary_planes_exactly(case):
    z, _, res = case
    np.testing.assert_array_equal(res["mask_edge"], z["mask_edge"].astype(np.float32))
    np.testing.assert_array_equal(res["bmaskgt"], z["bmaskgt"].astype(np.float32))
    assert 0 < z["mask_edge"].mean() < 1 and 0 < z["bmaskgt"].mean() < 1


def test_dif_grad_plane_within_four_times_the_measured_difference(case):
    z, _, res = case
    tol = 4.0 * float(z["measured_max_diff"])
    assert 0 <= tol <= 1e-4
    err = float(np.abs(res["dif_grad"].astype(np.float64) - z["dif_grad"].astype(np.float64)).max())
    print("train_losses fixture S=%d: dif_grad max |host - reference| %.3g (allowed %.3g)" % (int(z["S"]), err, tol))
    assert z["dif_grad"].max() > 0.1 and err <= tol


def test_losses_within_four_times_the_measured_difference(case):
    z, _, res = case
    tol = 4.0 * float(z["measured_rel_diff"])
    assert 0 < tol <= 1e-4
    rel = np.abs(res["losses"].astype(np.float64) - z["losses"]) / np.abs(z["losses"])
    print("train_losses fixture S=%d: losses %s, relative |host - reference| %s (allowed %.3g)" % (int(z["S"]), res["losses"], rel, tol))
    assert (z["losses"] > 0).all() and (rel <= tol).all()
