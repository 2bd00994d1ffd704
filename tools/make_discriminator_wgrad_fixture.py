"""Write tests/golden/discriminator_wgrad_32.npz (S = 32, B = 2): d (disc_real + disc_fake) / d each of
the 54 trainable variables of the three discriminators by torch autograd in float64 (tests/discriminator_wgrad_cases.autograd_grads:
F.conv2d on explicitly padded input, F.leaky_relu, the hinge as relu, parameters as leaves), from
init_discriminator_weights(WEIGHT_SEED) and discriminator.example_inputs(S, B, INPUT_SEED).  The file holds the 54 gradients as
float32 under the variables' names, `diff` (the worst scaled difference max |statement - autograd| /
max |autograd| over the variables of discriminator.disc_grad measured here on that case) and `measured` (the largest such difference over
this case, discriminator_wgrad_cases.AUTOGRAD_SIZES and the hinge case, which the tests take their bound from: 4 x measured, never above
1e-9).  No reference text is involved: the backward is pinned to the restatement of TensorFlow's gradient definitions in
discriminator.disc_grad's docstring.

    python tools/make_discriminator_wgrad_fixture.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from blindshadowremoval_amd import discriminator as host                      # noqa: E402
from blindshadowremoval_amd.weights import init_discriminator_weights        # noqa: E402

import discriminator_cases as dcases                                          # noqa: E402
import discriminator_wgrad_cases as cases                                     # noqa: E402

WEIGHT_SEED, INPUT_SEED = 3, 1


def case(w, gt, con, mask):
    auto = cases.autograd_grads(w, gt, con, mask)
    return auto, cases.worst_scaled_diff(host.disc_grad(w, gt, con, mask), auto)[0]


def main():
    S, B = cases.FIXTURE
    w = init_discriminator_weights(WEIGHT_SEED)
    auto, d = case(w, *host.example_inputs(S, B, INPUT_SEED))
    diffs = [d] + [case(w, *host.example_inputs(s, b, INPUT_SEED))[1] for s, b in cases.AUTOGRAD_SIZES] + [case(*dcases.hinge_case())[1]]
    path = os.path.join(ROOT, "tests", "golden", "discriminator_wgrad_%d.npz" % S)
    np.savez_compressed(path, diff=np.float64(d), measured=np.float64(max(diffs)), seeds=np.array([WEIGHT_SEED, INPUT_SEED]), batch=np.int64(B),
                        **{n: auto[n].astype(np.float32) for n in cases.NAMES})
    print("%s: B=%d diff %.3g, measured %.3g, %d bytes" % (path, B, d, max(diffs), os.path.getsize(path)))


if __name__ == "__main__":
    main()
