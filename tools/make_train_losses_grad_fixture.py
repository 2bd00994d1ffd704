"""Generate tests/golden/train_losses_grad_32.npz: torch autograd's float64 gradients of the reconstruction and gradient losses with
respect to gs and con_rgb, so that tests/test_train_losses_grad_fixture.py holds train_losses.step_losses_grad(f64=True) to them with
no torch in the loop.

The objective is tests/train_losses_grad_cases.torch_objective, the float64 restatement of the forward that shares no code with the
host statement (F.interpolate for both resizes, a max-pool for the dilations).  B = 2 items of side 32 from
train_losses.example_inputs(32, 2, seed); the seed is the first at which no difference that a sign is taken from lies within 1e-9 of 0
without being exactly 0 (train_losses_grad_cases.pick_seed), and only the seed is stored, not the inputs.  Stored: `seed`; `grad_gs`
[2,32,32,1] under the weights (1, 0, 0); `grad_con_recon_c` and `grad_con_grad` [2,32,32,3] under (0, 1, 0) and (0, 0, 1).  The
objective is linear in the weights, so every other weighting follows from these three.

Usage:  python tools/make_train_losses_grad_fixture.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from blindshadowremoval_amd import train_losses as host            # noqa: E402
import train_losses_grad_cases as cases                            # noqa: E402

S, B = 32, 2
OUT = os.path.join(ROOT, "tests", "golden", "train_losses_grad_32.npz")


def main():
    seed = cases.pick_seed(S, B)
    arrays = host.example_inputs(S, B, seed)
    grad_gs, zero = cases.autograd_grads(arrays, (1.0, 0.0, 0.0))
    assert not zero.any()
    _, recon_c = cases.autograd_grads(arrays, (0.0, 1.0, 0.0))
    _, grad = cases.autograd_grads(arrays, (0.0, 0.0, 1.0))
    np.savez(OUT, seed=np.int64(seed), S=np.int64(S), B=np.int64(B), grad_gs=grad_gs, grad_con_recon_c=recon_c, grad_con_grad=grad)
    print("wrote %s: seed %d, %d bytes" % (OUT, seed, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
