"""The host statement of d per_loss / d con_rgb against tests/golden/perceptual_grad_*.npz: torch autograd in float64 over the seeds of
perceptual_*.npz (tools/make_perceptual_grad_fixture.py).  The float64 gradient within 4 x the difference the tool measured and recorded,
never above 1e-9 of the largest magnitude; the float32 gradient within three float32 roundings of it (the fixture's one, the
statement's two: the gradient at the network's input, then the product with 255)."""
import os

import numpy as np
import pytest

from blindshadowremoval_amd import perceptual as host
from blindshadowremoval_amd.weights import init_vgg_weights

import perceptual_grad_cases as gcases


@pytest.mark.parametrize("S", (32, 64))
def test_host_statement_matches_the_autograd_fixture(golden_dir, S):
    case = np.load(os.path.join(golden_dir, "perceptual_grad_%d.npz" % S))
    forward = np.load(os.path.join(golden_dir, "perceptual_%d.npz" % S))
    B, seed = int(case["B"]), int(case["seed"])
    assert int(case["S"]) == S and B == gcases.FIXTURE_CASES[S] and (seed, B) == (int(forward["seed"]), int(forward["B"]))
    want = case["grad_f64"]
    assert want.shape == (B, S, S, 3) and want.dtype == np.float64 and case["grad"].dtype == np.float32
    assert case["grad"].tobytes() == want.astype(np.float32).tobytes()
    tol = 4 * float(case["measured_rel"])
    assert 0 < tol <= 1e-9
    r = host.per_loss_grad(init_vgg_weights(seed), *host.example_inputs(S, B, seed))
    scale = float(np.abs(want).max())
    diff = float(np.abs(gcases.statement_grad64(r) - want).max()) / scale
    print("perceptual grad fixture S=%d: statement against the fixture %.3g of the largest magnitude %.3g (recorded %.3g)" % (S, diff, scale, float(case["measured_rel"])))
    assert scale > 0 and diff <= tol
    assert r["grad"].dtype == np.float32 and (np.abs(r["grad"].astype(np.float64) - case["grad"]) <= 3 * 2.0 ** -24 * np.abs(want) + tol * scale).all()
    np.testing.assert_allclose(float(r["loss"][0]), float(forward["per"]), rtol=4 * float(forward["measured_mean_rel"]), atol=0)


def test_the_fixtures_hold_numbers_only(golden_dir):
    for S in (32, 64):
        path = os.path.join(golden_dir, "perceptual_grad_%d.npz" % S)
        assert os.path.getsize(path) < 256 * 1024
        with np.load(path) as z:
            assert sorted(z.files) == sorted(["seed", "B", "S", "backend", "grad", "grad_f64", "measured_rel"])
            assert float(z["measured_rel"]) == float(np.load(os.path.join(golden_dir, "perceptual_grad_32.npz"))["measured_rel"])
