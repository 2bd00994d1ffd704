"""Write tests/golden/discriminator_grad_32.npz (B = 2) and discriminator_grad_64.npz (B = 1): d gen / d con_rgb through the three
discriminators by torch autograd in float64 (tests/discriminator_grad_cases.autograd_grad: F.conv2d on explicitly padded input,
F.leaky_relu, F.interpolate(bilinear, align_corners=False)), from init_discriminator_weights(WEIGHT_SEED) and
discriminator.example_inputs(S, B, INPUT_SEED).  Each file holds `grad32` (the gradient as float32), `grad64` (the float64 it came
from), `diff` (the scaled difference max |statement - autograd| / max |autograd| of discriminator.gen_grad measured here on that case)
and `measured` (the largest such difference over the fixtures' cases and discriminator_grad_cases.AUTOGRAD_SIZES, which the tests
take their bound from: 4 x measured, never above 1e-9).  No reference text is involved: the backward is pinned to the restatement of
TensorFlow's gradient definitions in discriminator.gen_grad's docstring.

    python tools/make_discriminator_grad_fixture.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from blindshadowremoval_amd import discriminator as host                      # noqa: E402
from blindshadowremoval_amd.weights import init_discriminator_weights        # noqa: E402

import discriminator_grad_cases as cases                                      # noqa: E402

WEIGHT_SEED, INPUT_SEED = 3, 1


def case(S, B):
    w = init_discriminator_weights(WEIGHT_SEED)
    gt, con, mask = host.example_inputs(S, B, INPUT_SEED)
    auto = cases.autograd_grad(w, gt, con, mask)
    return auto, cases.scaled_diff(host.gen_grad(w, gt, con, mask)["grad"], auto)


def main():
    made = {(S, B): case(S, B) for S, B in cases.FIXTURES}
    diffs = [d for _, d in made.values()] + [case(S, B)[1] for S, B in cases.AUTOGRAD_SIZES]
    for (S, B), (auto, d) in made.items():
        path = os.path.join(ROOT, "tests", "golden", "discriminator_grad_%d.npz" % S)
        np.savez_compressed(path, grad32=auto.astype(np.float32), grad64=auto, diff=np.float64(d), measured=np.float64(max(diffs)),
                            seeds=np.array([WEIGHT_SEED, INPUT_SEED]), batch=np.int64(B))
        print("%s: B=%d diff %.3g, measured %.3g, %d bytes" % (path, B, d, max(diffs), os.path.getsize(path)))


if __name__ == "__main__":
    main()
