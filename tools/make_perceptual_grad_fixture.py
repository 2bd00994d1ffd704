"""Generate tests/golden/perceptual_grad_32.npz (B = 2) and perceptual_grad_64.npz (B = 1): d per_loss / d con_rgb by torch autograd in
float64, for the seeds of perceptual_32.npz and perceptual_64.npz (400 + S; inputs perceptual.example_inputs(S, B, seed), variables
init_vgg_weights(seed)).  Runs on the CPU; no reference text is involved: the backward is pinned to the project's restatement of
TensorFlow's gradient definitions (blindshadowremoval_amd/perceptual.py), and this is its second, independent form — the same VGG19
stand-in written with torch's conv2d, relu, max_pool2d and abs, differentiated by their registered gradients
(tests/perceptual_grad_cases.torch_grad).

Each file holds the seed, B, S, the gradient as float32 (`grad`) and as the float64 it was rounded from (`grad_f64`: the host statement
is held to it far below float32's resolution), and `measured_rel`: the largest difference of the host statement from autograd, over
the two fixture cases and the sizes of tests/test_perceptual_grad_cpu.py, relative to the largest gradient magnitude of the case, with
torch on one thread and on eight (its float64 convolution sums in another order then).  The tests allow 4 x that, never above 1e-9.

Usage:  python tools/make_perceptual_grad_fixture.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from blindshadowremoval_amd import perceptual as host                          # noqa: E402
from blindshadowremoval_amd.weights import init_vgg_weights                    # noqa: E402

import perceptual_grad_cases as gcases                                         # noqa: E402


def main():
    import torch
    worst, done = 0.0, []
    for threads in (1, 8):
        torch.set_num_threads(threads)
        w = init_vgg_weights(21)
        for S, B in gcases.GRAD_SIZES:
            d, want = gcases.autograd_difference(w, *gcases.inputs(S, B))
            print("threads %d S=%d B=%d: |statement - autograd| %.3g of max |grad| %.3g" % (threads, S, B, d, np.abs(want).max()))
            worst = max(worst, d)
        for S, B in gcases.FIXTURE_CASES.items():
            seed = 400 + S
            d, want = gcases.autograd_difference(init_vgg_weights(seed), *host.example_inputs(S, B, seed))
            print("threads %d fixture S=%d B=%d seed %d: |statement - autograd| %.3g of max |grad| %.3g" % (threads, S, B, seed, d, np.abs(want).max()))
            worst = max(worst, d)
            if threads == 1:
                done.append({"seed": np.int64(seed), "B": np.int64(B), "S": np.int64(S), "backend": np.array("torch autograd float64"),
                             "grad": want.astype(np.float32), "grad_f64": want})
    assert 0 < worst <= 2.5e-10, worst
    for case in done:
        case["measured_rel"] = np.float64(worst)
        path = os.path.join(ROOT, "tests", "golden", "perceptual_grad_%d.npz" % int(case["S"]))
        np.savez_compressed(path, **case)
        print("wrote %s (%d bytes), measured_rel %.3g" % (path, os.path.getsize(path), worst))
        assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
