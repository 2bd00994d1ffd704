"""The host statement of the backward of res_stack/5's upper half against the committed autograd results
tests/golden/nonlocal_grad_2x4.npz, written by tools/make_nonlocal_grad_fixture.py: torch autograd in float64, stored as float32.  The
bound is the autograd test's (4 x the fixture's own `measured`, never above 1e-9) plus 2^-24, the rounding of the stored values."""
import os

import numpy as np

from blindshadowremoval_amd import generator_grad as host

import nonlocal_grad_cases as cases

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_statement_matches_the_committed_autograd_gradients():
    h, w, B = cases.FIXTURE
    fix = np.load(os.path.join(GOLDEN, "nonlocal_grad_%dx%d.npz" % (h, w)))
    assert tuple(fix["shape"]) == (h, w, B)
    want = {n: fix[n] for n in cases.OUTPUTS}
    wt, y3, xin, d_out = cases.case(h, w, B, int(fix["seed"]))
    res = host.nonlocal_grad(wt, y3, xin, d_out)
    bound = min(4 * float(fix["measured"]), cases.AUTOGRAD_CAP) + 2.0 ** -24
    d, at = cases.worst_scaled_diff(res, want)
    print("non-local grad fixture: worst scaled difference %.3g at %s (bound %.3g)" % (d, at, bound))
    assert all(want[n].dtype == np.float32 and want[n].shape == np.asarray(res[n]).shape for n in cases.OUTPUTS)
    assert d <= bound
