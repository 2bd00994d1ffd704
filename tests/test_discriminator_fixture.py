"""The host statement blindshadowremoval_amd/discriminator.py held to the reference's own Discriminator, Conv, hinge_loss and train_step
statements, executed over the numpy TensorFlow stand-in by tools/make_discriminator_fixture.py (tests/golden/discriminator_*.npz: seeds,
the six logit maps as float32, the three losses, and the difference the tool measured).  Logits and losses agree within 4 x the
recorded measured difference, never above 1e-5 relative."""
import os

import numpy as np
import pytest

from blindshadowremoval_amd import discriminator as host
from blindshadowremoval_amd.weights import init_discriminator_weights

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.parametrize("S,B", [(32, 2), (64, 1)])
def test_host_statement_against_the_reference(S, B):
    fx = np.load(os.path.join(GOLDEN, "discriminator_%d.npz" % S))
    seed = int(fx["seed"])
    assert (int(fx["S"]), int(fx["B"])) == (S, B)
    logit_tol, loss_tol = 4 * float(fx["measured_logit_diff"]), 4 * float(fx["measured_loss_rel"])
    assert 0 < logit_tol <= 1e-5 and 0 < loss_tol <= 1e-5
    weights = init_discriminator_weights(seed)
    for k in (1, 2, 3):
        weights["discriminator_%d/conv2/conv/kernel" % k] *= np.float32(float(fx["head_gain"]))
    ours = host.gan_losses(weights, *host.example_inputs(S, B, seed))
    for k in (1, 2, 3):
        h = host.final_side(S, k)
        stored = np.concatenate([fx["real_%d" % k], fx["fake_%d" % k]]).astype(np.float64)
        assert stored.shape == ours["logits"][k - 1].shape == (2 * B, h, h) and fx["real_%d" % k].dtype == np.float32
        e = float(np.abs(ours["logits"][k - 1] - stored).max() / np.abs(stored).max())
        print("discriminator fixture S=%d d%d: logits scaled |host - reference| %.3g (allowed %.3g)" % (S, k, e, logit_tol))
        assert e <= logit_tol
    rel = np.abs(ours["losses"].astype(np.float64) - fx["losses"]) / np.abs(fx["losses"])
    print("discriminator fixture S=%d: losses host %s reference %s, relative %s (allowed %.3g)" % (S, ours["losses"], fx["losses"], rel, loss_tol))
    assert (rel <= loss_tol).all()
    assert np.abs(fx["losses"][0]) > 1e-3 and (fx["losses"][1:] > 0).all()
    if S == 64:          # the case with the head kernels x 8: the reference's max(0, .) clips a real and a fake logit there
        real = np.concatenate([fx["real_%d" % k].reshape(-1) for k in (1, 2, 3)])
        fake = np.concatenate([fx["fake_%d" % k].reshape(-1) for k in (1, 2, 3)])
        assert float(fx["head_gain"]) == 8.0 and (real > 1).any() and (real < 1).any() and (fake < -1).any() and (fake > -1).any()
