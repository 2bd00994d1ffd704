"""The host statement of the colour decoder's backward against the committed autograd results tests/golden/clr_decoder_grad_2x4.npz
(with clr_up1's kernel gradient in ..._k1a.npz and ..._k1b.npz: no committed file passes 1 MiB), written by
tools/make_clr_decoder_grad_fixture.py: torch autograd in float64, stored as float32.  The bound is the autograd test's (4 x the
fixture's own `measured`, never above 1e-9) plus 2^-24, the rounding of the stored values."""
import os

import numpy as np

from blindshadowremoval_amd import generator_grad as host

import clr_decoder_grad_cases as cases

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_statement_matches_the_committed_autograd_gradients():
    h, w, B = cases.FIXTURE
    stem = os.path.join(GOLDEN, "clr_decoder_grad_%dx%d" % (h, w))
    fix = np.load(stem + ".npz")
    assert tuple(fix["shape"]) == (h, w, B)
    want = {n: fix[n] for n in cases.OUTPUTS if n != "clr_up1/conv/kernel"}
    want["clr_up1/conv/kernel"] = np.concatenate([np.load(stem + "_k1a.npz")["k1a"], np.load(stem + "_k1b.npz")["k1b"]])
    wt, x, d_f = cases.case(h, w, B, int(fix["seed"]))
    res = host.decoder_grad(wt, x, d_f)
    bound = min(4 * float(fix["measured"]), cases.AUTOGRAD_CAP) + 2.0 ** -24
    d, at = cases.worst_scaled_diff(res, want)
    print("colour decoder grad fixture: worst scaled difference %.3g at %s (bound %.3g)" % (d, at, bound))
    assert all(want[n].dtype == np.float32 and want[n].shape == np.asarray(res[n]).shape for n in cases.OUTPUTS)
    assert d <= bound
