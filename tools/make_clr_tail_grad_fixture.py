"""Write tests/golden/clr_tail_grad_16.npz (H = 16, W = 32, B = 2): the gradient of <g_con, con_rgb> + <g_gs, gs> with respect to
each of the ten trainable variables of the generator's colour tail, to f and to gs, by torch autograd in float64
(tests/clr_tail_grad_cases.autograd_grads: F.conv2d, F.leaky_relu, the variables and the two inputs as leaves), from
clr_tail_grad_cases.case(H, W, B, INPUT_SEED).  The file holds the twelve gradients as float32 under their names, `diff` (the worst
scaled difference max |statement - autograd| / max |autograd| over the outputs of generator_grad.tail_grad measured here on that case)
and `measured` (the largest such difference over this case and clr_tail_grad_cases.AUTOGRAD_SIZES, which the tests take their bound from:
4 x measured, never above 1e-9).  No reference text is involved: the backward is pinned to the restatement of TensorFlow's gradient
definitions in generator_grad.tail_grad's docstring.

    python tools/make_clr_tail_grad_fixture.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from blindshadowremoval_amd import generator_grad as host                     # noqa: E402

import clr_tail_grad_cases as cases                                           # noqa: E402

INPUT_SEED = 1


def case(H, W, B):
    args = cases.case(H, W, B, INPUT_SEED)
    auto = cases.autograd_grads(*args)
    return auto, cases.worst_scaled_diff(host.tail_grad(*args), auto)[0]


def main():
    H, W, B = cases.FIXTURE
    auto, d = case(H, W, B)
    diffs = [d] + [case(*size)[1] for size in cases.AUTOGRAD_SIZES]
    path = os.path.join(ROOT, "tests", "golden", "clr_tail_grad_%d.npz" % H)
    np.savez_compressed(path, diff=np.float64(d), measured=np.float64(max(diffs)), seed=np.int64(INPUT_SEED), shape=np.array([H, W, B]),
                        **{n: auto[n].astype(np.float32) for n in cases.OUTPUTS})
    print("%s: diff %.3g, measured %.3g, %d bytes" % (path, d, max(diffs), os.path.getsize(path)))


if __name__ == "__main__":
    main()
