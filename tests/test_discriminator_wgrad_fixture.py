"""discriminator.disc_grad against tests/golden/discriminator_wgrad_32.npz: torch autograd's float64
gradient of d_total_loss with respect to the 54 trainable variables, kept as float32 (tools/make_discriminator_wgrad_fixture.py).  Per
variable, on the scale of its largest magnitude: within 4 x the largest difference measured when the fixture was made, never above 1e-9,
plus 2^-24 for the fixture's rounding to float32 (half a unit in the last place of an element is at most that of the largest)."""
import os

import numpy as np

from blindshadowremoval_amd import discriminator as host
from blindshadowremoval_amd.weights import discriminator_variable_shapes, init_discriminator_weights

import discriminator_wgrad_cases as cases

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_statement_matches_the_autograd_fixture():
    S, B = cases.FIXTURE
    fx = dict(np.load(os.path.join(GOLDEN, "discriminator_wgrad_%d.npz" % S)))
    shapes = discriminator_variable_shapes()
    assert int(fx["batch"]) == B and sorted(n for n in fx if "/" in n) == sorted(cases.NAMES)
    for n in cases.NAMES:
        assert fx[n].dtype == np.float32 and fx[n].shape == shapes[n], n
    assert 0 < float(fx["diff"]) <= float(fx["measured"]) < cases.AUTOGRAD_CAP / 4
    bound = min(4 * float(fx["measured"]), cases.AUTOGRAD_CAP) + 2.0 ** -24
    w = init_discriminator_weights(int(fx["seeds"][0]))
    got = host.disc_grad(w, *host.example_inputs(S, B, int(fx["seeds"][1])))
    d, at = cases.worst_scaled_diff(got, fx)
    print("discriminator wgrad fixture S=%d B=%d: worst scaled difference %.3g at %s (bound %.3g, %.3g in float64 when made)" % (S, B, d, at, bound, float(fx["diff"])))
    assert d <= bound
