"""The host statement of d d_total_loss / d the discriminators' variables (blindshadowremoval_amd/discriminator.py: disc_grad) against
torch autograd in float64, on the hinge case, on the closed forms of discriminator_wgrad_cases and against central finite differences
of the float64 objective d_total_f64 in extended precision; pack.pack_discriminators_wgrad against its un-pack and
weights.discriminator_trainable_names against the checkpoint inventory."""
import json
import os

import numpy as np
import pytest

from blindshadowremoval_amd import discriminator as host
from blindshadowremoval_amd import pack
from blindshadowremoval_amd.weights import (BN_EPS, N_LAYER_D, discriminator_trainable_names, discriminator_variable_shapes,
                                            init_discriminator_weights)

import discriminator_cases as dcases
import discriminator_wgrad_cases as cases

f32 = np.float32
LD = np.longdouble
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FD_SEED = 1


def host_run(weights, gt, con_rgb, mask_sv):
    acts = host.forward(weights, gt, con_rgb, mask_sv)
    return {"grads": host.disc_grad(weights, gt, con_rgb, mask_sv, acts=acts), "acts": acts, "dtype": np.float64}


def autograd_bound():
    measured = float(np.load(os.path.join(GOLDEN, "discriminator_wgrad_%d.npz" % cases.FIXTURE[0]))["measured"])
    return min(4 * measured, cases.AUTOGRAD_CAP)


@pytest.mark.parametrize("check", cases.CONSTRUCTED, ids=lambda c: c.__name__)
def test_constructed_case(check):
    check(host_run)


@pytest.mark.parametrize("S,B", cases.AUTOGRAD_SIZES)
def test_statement_matches_torch_autograd_in_float64(S, B):
    w = init_discriminator_weights(3)
    arrays = host.example_inputs(S, B, 1)
    res = host.disc_grad(w, *arrays)
    d, at = cases.worst_scaled_diff(res, cases.autograd_grads(w, *arrays))
    print("discriminator wgrad S=%d B=%d: statement against torch autograd, worst scaled difference %.3g at %s (bound %.3g)" % (S, B, d, at, autograd_bound()))
    assert d <= autograd_bound()
    shapes = discriminator_variable_shapes()
    for name in cases.NAMES:
        assert res[name].shape == shapes[name] and res[name].dtype == np.float64, name
        assert np.abs(res[name]).max() > 0 or name.endswith("conv2/conv/bias"), name          # all terms active: the head bias's seeds cancel
    for k in (1, 2, 3):
        sides = host.map_sides(S, k)
        assert res["d%d/out" % k].shape == (2 * B, sides[-1], sides[-1], 1)
        for i in range(N_LAYER_D):
            assert res["d%d/conv%d" % (k, i)].shape == (2 * B, sides[i + 1], sides[i + 1], host.DISC_CH[i])
    assert len(res) == 54 + 15


def test_the_hinge_case_pins_the_clip():
    """discriminator_cases.hinge_case: each of the six hinge terms has active and inactive logits, none within 1e-3 of +-1, so a
    statement that let every logit through, or none, or clipped the wrong side, misses autograd by far more than the bound."""
    args = dcases.hinge_case()
    B = args[1].shape[0]
    fwd = host.forward(*args)
    assert dcases.hinge_condition(host.logits_of(fwd), B)
    res = host.disc_grad(*args, acts=fwd)
    for k in (1, 2, 3):
        seed = res["d%d/out" % k]
        assert (seed[:B] <= 0).all() and (seed[:B] < 0).any() and (seed[:B] == 0).any()
        assert (seed[B:] >= 0).all() and (seed[B:] > 0).any() and (seed[B:] == 0).any()
    d, at = cases.worst_scaled_diff(res, cases.autograd_grads(*args))
    print("discriminator wgrad hinge case: statement against torch autograd, worst scaled difference %.3g at %s (bound %.3g)" % (d, at, autograd_bound()))
    assert d <= autograd_bound()


def test_a_hinge_term_of_exactly_zero_passes_nothing():
    """TensorFlow's Maximum(0., t) hands a tie to the constant: logits of exactly +1 on the real side and -1 on the fake side seed 0."""
    y = np.array([[[1.0]], [[0.5]], [[-1.0]], [[-0.5]]], f32)                 # rows: real, real, fake, fake
    seed = host.hinge_seed(y, 2, f32(0.25))[..., 0]
    np.testing.assert_array_equal(seed.reshape(-1), [0.0, -0.25, 0.0, 0.25])


def test_logits_and_acts_given_are_those_of_the_own_forward():
    w = init_discriminator_weights(3)
    arrays = host.example_inputs(32, 2, 1)
    fwd = host.forward(w, *arrays)
    own, given = host.disc_grad(w, *arrays), host.disc_grad(w, *arrays, acts=fwd, logits=host.logits_of(fwd))
    assert sorted(own) == sorted(given) and all(own[n].tobytes() == given[n].tobytes() for n in own)


def test_d_total_f64_is_disc_real_plus_disc_fake():
    w = init_discriminator_weights(3)
    gt, con, mask = host.example_inputs(32, 2, 1)
    losses = host.gan_losses(w, gt, con, mask)["losses"]
    want = float(losses[1]) + float(losses[2])
    assert abs(host.d_total_f64(w, gt, con, mask) - want) <= 1e-6 * max(1.0, abs(want))


@pytest.mark.parametrize("S,B,FD_STEP", ((32, 2, 1e-6), (32, 1, 1e-6)))
def test_central_finite_differences_along_two_directions(S, B, FD_STEP):
    """On a segment v + t d of variable space along which no LeakyReLU mask and no hinge mask changes (asserted for the five points
    used: a condition on FD_SEED and the case's step, not a tolerance), d_total_f64 is a polynomial p(t): every variable enters linearly or,
    through gamma beta and the kernels of the layers above, as a product.  The central quotient q(e) = (p(e) - p(-e)) / 2e is then
    p'(0) + c3 e^2 + c5 e^4 + ..., so q(2e) - q(e) = 3 c3 e^2 + O(e^4): the truncation of q(e) is a third of the difference of the two
    quotients up to O(e^4), and |q(2e) - q(e)| bounds it with a factor 3 to spare.  The rounding of the evaluations is kept out of the
    way by numpy's extended precision (u = 2^-64): a loss value is an O(1) number formed by about 5 * 1028 + 262 operations a path on
    magnitudes the gen test measured at M <= 2e5, so its error is below 5402 u M = 6e-11 and the quotient's below that over e.  Both
    are computed from the objective alone, never from disc_grad.  <grad, d> is summed in extended precision from disc_grad's float64
    gradient on inputs rounded to the 1/256 grid (the statement resizes in float32, the objective takes exact means; on the grid the two
    agree, which is asserted); its own rounding, 54 variables of at most 65536 elements, is below 1e-11 of sum |grad d|.  At these sizes B h_k^2 is a power
    of two, so the statement's float32 w_k is the objective's divisor exactly."""
    u = float(np.finfo(LD).eps) / 2
    w = init_discriminator_weights(3)
    gt, con, mask = (np.round(a * f32(256)) / f32(256) for a in host.example_inputs(S, B, FD_SEED))
    for k in (2, 3):          # on the 1/256 grid the statement's float32 resize is exact, so both sides differentiate one objective
        x = host.disc_input(gt, con, mask, k).astype(np.float64)
        ds, lo = host.DOWNSIZE[k - 1], k - 2
        full = host.disc_input(gt, con, mask, 1).astype(np.float64).reshape(2 * B, S // ds, ds, S // ds, ds, 6)
        assert (x == full[:, :, lo:lo + 2, :, lo:lo + 2].mean(axis=(2, 4))).all()
    res = host.disc_grad(w, gt, con, mask)
    rng = np.random.default_rng(FD_SEED)
    names = discriminator_trainable_names()
    for j in range(2):
        d = {n: rng.standard_normal(w[n].shape) * np.abs(w[n]).max() for n in names}          # a step relative to each variable's scale

        def at(t):
            moved = {n: np.asarray(v, LD) + (LD(t) * LD(FD_STEP) * d[n].astype(LD) if n in d else LD(0)) for n, v in w.items()}
            masks = []
            return host.d_total_f64(moved, gt, con, mask, masks=masks, dtype=LD), masks

        values = {t: at(t) for t in (-2, -1, 0, 1, 2)}
        for t in (-2, -1, 1, 2):
            assert len(values[t][1]) == len(values[0][1]) == 3 * (N_LAYER_D + 2)
            for a, b in zip(values[t][1], values[0][1]):
                assert (a == b).all(), "a LeakyReLU or hinge mask differs between the evaluation points"
        q1 = (values[1][0] - values[-1][0]) / (2 * LD(FD_STEP))
        q2 = (values[2][0] - values[-2][0]) / (4 * LD(FD_STEP))
        want = sum((res[n].astype(LD) * d[n].astype(LD)).sum() for n in names)
        mass = float(sum(np.abs(res[n] * d[n]).sum() for n in names))
        bound = abs(float(q2 - q1)) + 5402 * u * 2e5 / FD_STEP + 1e-11 * mass
        print("discriminator wgrad S=%d B=%d direction %d: quotient %.12g, <grad, d> %.12g, |difference| %.3g, bound %.3g (|q(2e) - q(e)| %.3g)"
              % (S, B, j, float(q1), float(want), abs(float(q1 - want)), bound, abs(float(q2 - q1))))
        print("discriminator wgrad S=%d B=%d direction %d: sum |grad d| %.3g" % (S, B, j, mass))
        assert mass > 100 * bound, "the bound must mean something beside the terms of the derivative"
        assert abs(float(q1 - want)) <= bound


def test_pack_wgrad_against_its_unpack():
    w = init_discriminator_weights(4)
    blob = pack.pack_discriminators_wgrad(w)
    layout, per = pack.disc_wgrad_layout()
    assert len(blob) == 3 * per * 4 and per == 16 * (8 * 32 + 32 * 32 + 32 * 64 + 64 * 64) + 4 * (32 + 32 + 64 + 64)
    back = pack.unpack_discriminators_wgrad(blob)
    for k in (1, 2, 3):
        for i in range(N_LAYER_D):
            st = "discriminator_%d/conv_stack/%d/" % (k, i)
            kern = w[st + "conv/kernel"]
            got = back[k - 1]["conv%d/kernel" % i]
            np.testing.assert_array_equal(got[:, :kern.shape[2]], kern.reshape(16, kern.shape[2], kern.shape[3]))
            assert not got[:, kern.shape[2]:].any() and got.shape[1] % 8 == 0
            vecs = back[k - 1]["conv%d/vecs" % i]
            rstd = 1.0 / np.sqrt(w[st + "bnorm/moving_variance"].astype(np.float64) + BN_EPS)
            np.testing.assert_array_equal(vecs[0], w[st + "conv/bias"])
            np.testing.assert_array_equal(vecs[1], (w[st + "bnorm/gamma"].astype(np.float64) * rstd).astype(f32))
            np.testing.assert_array_equal(vecs[2], w[st + "bnorm/moving_mean"])
            np.testing.assert_array_equal(vecs[3], rstd.astype(f32))
            np.testing.assert_array_equal(vecs[1].astype(np.float64), host.bn_inv(w, k, i).astype(f32))
    with pytest.raises(ValueError, match="weight-gradient blob"):
        pack.unpack_discriminators_wgrad(blob[:-4])
    with pytest.raises(ValueError, match="missing discriminator variables"):
        pack.pack_discriminators_wgrad({})


def test_trainable_names_against_the_inventory():
    names = discriminator_trainable_names()
    shapes = discriminator_variable_shapes()
    assert len(names) == 54 and len(set(names)) == 54
    assert names == [n for n in shapes if "moving_" not in n]
    assert sum(int(np.prod(shapes[n])) for n in names) == 3 * (16 * (6 * 32 + 32 * 32 + 32 * 64 + 64 * 64) + 3 * 192 + 16 * 64 + 1)
    with open(os.path.join(GOLDEN, "disc_ckpt_inventory.json")) as f:
        inventory = json.load(f)
    text = json.dumps(inventory)
    for n in names:
        assert n in text, n
