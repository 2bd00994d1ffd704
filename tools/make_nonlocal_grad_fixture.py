"""Write tests/golden/nonlocal_grad_2x4.npz (coarse h = 2, w = 4, B = 2): the gradient of <d_out, out> with respect to each of the ten
trainable variables of res_stack/5's non-local block, to y3 (`d_y3`) and to the block's input through the skip (`d_skip`), by torch
autograd in float64 (tests/nonlocal_grad_cases.autograd_grads: the reference's semantics written with torch.matmul, torch.softmax and
F.leaky_relu, the variables, y3 and xin as leaves), from nonlocal_grad_cases.case(h, w, B, INPUT_SEED).  The gradients are stored as
float32 under their names (0.5 MB: one file), with `diff` (the worst scaled difference max |statement - autograd| / max |autograd| over
the outputs of generator_grad.nonlocal_grad measured here on that case, d phi/bias on the scale of d theta/bias) and `measured` (the
largest such difference over this case, nonlocal_grad_cases.AUTOGRAD_SIZES and the C = 877 case, which the tests take their bound from:
4 x measured, never above 1e-9).  No reference text is involved: the backward is pinned to the restatement in
generator_grad.nonlocal_grad's docstring.

    python tools/make_nonlocal_grad_fixture.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from blindshadowremoval_amd import generator_grad as host                     # noqa: E402

import nonlocal_grad_cases as cases                                           # noqa: E402

INPUT_SEED = 1


def case(h, w, B, seed=INPUT_SEED, C=261):
    args = cases.case(h, w, B, seed, C)
    auto = cases.autograd_grads(*args)
    return auto, cases.worst_scaled_diff(host.nonlocal_grad(*args), auto)[0]


def main():
    h, w, B = cases.FIXTURE
    auto, d = case(h, w, B)
    diffs = [d] + [case(*size)[1] for size in cases.AUTOGRAD_SIZES] + [case(1, 4, 1, 2, 877)[1]]
    path = os.path.join(ROOT, "tests", "golden", "nonlocal_grad_%dx%d.npz" % (h, w))
    np.savez_compressed(path, diff=np.float64(d), measured=np.float64(max(diffs)), seed=np.int64(INPUT_SEED), shape=np.array([h, w, B]),
                        **{n: auto[n].astype(np.float32) for n in cases.OUTPUTS})
    size = os.path.getsize(path)
    assert size < (1 << 20), size
    print("%s: %d bytes" % (path, size))
    print("diff %.3g, measured %.3g" % (d, max(diffs)))


if __name__ == "__main__":
    main()
