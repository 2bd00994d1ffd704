"""train_losses.step_losses_grad(f64=True) against tests/golden/train_losses_grad_32.npz: torch autograd's float64 gradients of a
restatement of the forward that shares no code with the statement (tools/make_train_losses_grad_fixture.py), with no torch in the loop.
The bar is the autograd test's: 1e-12 on the scale of the largest magnitude."""
import os

import numpy as np
import pytest

from blindshadowremoval_amd import train_losses as host

f32 = np.float32
BAR = 1e-12
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_losses_grad_32.npz")


@pytest.fixture(scope="module")
def golden():
    assert os.path.getsize(GOLDEN) < 200_000
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def scaled(got, ref):
    return float(np.abs(got - ref).max() / np.abs(ref).max())


def test_statement_against_the_stored_autograd_gradients(golden):
    S, B = int(golden["S"]), int(golden["B"])
    assert (S, B) == (32, 2) and golden["grad_gs"].dtype == golden["grad_con_grad"].dtype == np.float64
    arrays = host.example_inputs(S, B, int(golden["seed"]))
    for w, key, name in (((1, 0, 0), "grad_gs", "grad_gs"), ((0, 1, 0), "grad_con", "grad_con_recon_c"), ((0, 0, 1), "grad_con", "grad_con_grad")):
        got = host.step_losses_grad(*arrays, upstream=np.array(w, f32), f64=True)
        e = scaled(got[key], golden[name])
        print("train_losses grad fixture %s: scaled error %.3g, largest %.3g" % (name, e, np.abs(golden[name]).max()))
        assert got[key].shape == golden[name].shape and e <= BAR
    got = host.step_losses_grad(*arrays, upstream=np.array(host.G_TOTAL_WEIGHTS, f32), f64=True)
    w = host.G_TOTAL_WEIGHTS
    assert scaled(got["grad_gs"], w[0] * golden["grad_gs"]) <= BAR
    assert scaled(got["grad_con"], w[1] * golden["grad_con_recon_c"] + w[2] * golden["grad_con_grad"]) <= BAR
    assert scaled(got["d_recon_c"], w[1] * golden["grad_con_recon_c"]) <= BAR and scaled(got["d_grad"], w[2] * golden["grad_con_grad"]) <= BAR


def test_float32_signs_agree_with_the_fixture_on_its_seed(golden):
    """On the fixture's seed no sign turns under float32 rounding, so the float32-sign statement is the stored gradient rounded once."""
    arrays = host.example_inputs(int(golden["S"]), int(golden["B"]), int(golden["seed"]))
    got = host.step_losses_grad(*arrays)
    assert got["grad_gs"].dtype == f32 and scaled(got["grad_gs"].astype(np.float64), golden["grad_gs"]) <= 2.0 ** -23
    differs = np.abs(got["grad_con"].astype(np.float64) - (golden["grad_con_recon_c"] + golden["grad_con_grad"])) > 2.0 ** -23 * np.abs(golden["grad_con_grad"]).max()
    print("train_losses grad fixture: share of grad_con elements a turned sign moves %.4g%%" % (100 * differs.mean()))
    assert differs.mean() <= 1e-3
