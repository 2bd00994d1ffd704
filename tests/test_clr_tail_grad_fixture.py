"""generator_grad.tail_grad against tests/golden/clr_tail_grad_16.npz: torch autograd's float64 gradient of <g_con, con_rgb> + <g_gs, gs>
with respect to the colour tail's ten variables, f and gs, kept as float32 (tools/make_clr_tail_grad_fixture.py).  Per output, on the
scale of its largest magnitude: within the CPU test's bound (4 x the largest difference measured when the fixture was made, never above
1e-9) plus 2^-24 for the fixture's rounding to float32."""
import os

import numpy as np

from blindshadowremoval_amd import generator_grad as host
from blindshadowremoval_amd.weights import generator_variable_shapes

import clr_tail_grad_cases as cases

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_statement_matches_the_autograd_fixture():
    H, W, B = cases.FIXTURE
    fx = dict(np.load(os.path.join(GOLDEN, "clr_tail_grad_%d.npz" % H)))
    shapes = generator_variable_shapes()
    assert tuple(fx["shape"]) == (H, W, B) and sorted(n for n in fx if "/" in n) == sorted(cases.NAMES)
    for n in cases.NAMES:
        assert fx[n].dtype == np.float32 and fx[n].shape == shapes[n], n
    assert fx["d_f"].shape == (B, H, W, 64) and fx["d_gs"].shape == (B, H, W, 1)
    assert 0 < float(fx["diff"]) <= float(fx["measured"]) < cases.AUTOGRAD_CAP / 4
    bound = min(4 * float(fx["measured"]), cases.AUTOGRAD_CAP) + 2.0 ** -24
    got = host.tail_grad(*cases.case(H, W, B, int(fx["seed"])))
    d, at = cases.worst_scaled_diff(got, fx)
    print("colour tail grad fixture H=%d W=%d B=%d: worst scaled difference %.3g at %s (bound %.3g, %.3g in float64 when made)"
          % (H, W, B, d, at, bound, float(fx["diff"])))
    assert d <= bound
