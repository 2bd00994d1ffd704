"""Write tests/golden/clr_decoder_grad_2x4.npz and its two companions (coarse h = 2, w = 4, B = 2): the gradient of <d_f, f> with
respect to each of the twelve trainable variables of the generator's colour decoder and to x, by torch autograd in float64
(tests/clr_decoder_grad_cases.autograd_grads: F.conv_transpose2d, F.leaky_relu, the variables and x as leaves), from
clr_decoder_grad_cases.case(h, w, B, INPUT_SEED).  The gradients are stored as float32 under their names; the 1.9 MB they hold are
split so that no file passes 1 MiB: clr_up1's kernel gradient [3,3,128,261] lies in ..._k1a.npz (tap rows 0 and 1, `k1a`) and
..._k1b.npz (tap row 2, `k1b`), everything else in the main file, with `diff` (the worst scaled difference max |statement - autograd| /
max |autograd| over the outputs of generator_grad.decoder_grad measured here on that case) and `measured` (the largest such difference
over this case and clr_decoder_grad_cases.AUTOGRAD_SIZES, which the tests take their bound from: 4 x measured, never above 1e-9).  No
reference text is involved: the backward is pinned to the restatement of TensorFlow's gradient definitions in
generator_grad.decoder_grad's docstring.

    python tools/make_clr_decoder_grad_fixture.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from blindshadowremoval_amd import generator_grad as host                     # noqa: E402

import clr_decoder_grad_cases as cases                                        # noqa: E402

INPUT_SEED = 1
K1 = "clr_up1/conv/kernel"


def case(h, w, B):
    args = cases.case(h, w, B, INPUT_SEED)
    auto = cases.autograd_grads(*args)
    return auto, cases.worst_scaled_diff(host.decoder_grad(*args), auto)[0]


def main():
    h, w, B = cases.FIXTURE
    auto, d = case(h, w, B)
    diffs = [d] + [case(*size)[1] for size in cases.AUTOGRAD_SIZES]
    stem = os.path.join(ROOT, "tests", "golden", "clr_decoder_grad_%dx%d" % (h, w))
    k1 = auto[K1].astype(np.float32)
    np.savez_compressed(stem + ".npz", diff=np.float64(d), measured=np.float64(max(diffs)), seed=np.int64(INPUT_SEED), shape=np.array([h, w, B]),
                        **{n: auto[n].astype(np.float32) for n in cases.OUTPUTS if n != K1})
    np.savez_compressed(stem + "_k1a.npz", k1a=k1[:2])
    np.savez_compressed(stem + "_k1b.npz", k1b=k1[2:])
    for suffix in (".npz", "_k1a.npz", "_k1b.npz"):
        size = os.path.getsize(stem + suffix)
        assert size < (1 << 20), (suffix, size)
        print("%s: %d bytes" % (stem + suffix, size))
    print("diff %.3g, measured %.3g" % (d, max(diffs)))


if __name__ == "__main__":
    main()
