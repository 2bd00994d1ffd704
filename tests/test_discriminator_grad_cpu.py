"""The host statement of d gen / d con_rgb (blindshadowremoval_amd/discriminator.py: gen_grad) against torch autograd in float64,
against central finite differences of the float64 objective, and on the constructed cases of discriminator_grad_cases; and
pack.pack_discriminators_dgrad against its un-pack."""
import os

import numpy as np
import pytest

from blindshadowremoval_amd import discriminator as host
from blindshadowremoval_amd import pack
from blindshadowremoval_amd.weights import BN_EPS, N_LAYER_D, init_discriminator_weights

import discriminator_grad_cases as cases

f32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FD_SEED, FD_STEP = 1, 1e-6


def host_run(weights, gt, con_rgb, mask_sv, upstream=None):
    acts = host.forward(weights, gt, con_rgb, mask_sv)
    return {"grad": host.gen_grad(weights, gt, con_rgb, mask_sv, upstream=upstream, acts=acts)["grad"], "acts": acts, "dtype": np.float64}


@pytest.mark.parametrize("check", cases.CONSTRUCTED, ids=lambda c: c.__name__)
def test_constructed_case(check):
    check(host_run)


def autograd_bound():
    measured = max(float(np.load(os.path.join(GOLDEN, "discriminator_grad_%d.npz" % S))["measured"]) for S, _ in cases.FIXTURES)
    return min(4 * measured, cases.AUTOGRAD_CAP)


@pytest.mark.parametrize("S,B", cases.AUTOGRAD_SIZES)
def test_statement_matches_torch_autograd_in_float64(S, B):
    w = init_discriminator_weights(3)
    arrays = host.example_inputs(S, B, 1)
    res = host.gen_grad(w, *arrays)
    d = cases.scaled_diff(res["grad"], cases.autograd_grad(w, *arrays))
    print("discriminator grad S=%d B=%d: statement against torch autograd, scaled difference %.3g (bound %.3g)" % (S, B, d, autograd_bound()))
    assert res["grad"].shape == (B, S, S, 3) and res["grad"].dtype == np.float64 and d <= autograd_bound()
    for k in (1, 2, 3):
        sides = host.map_sides(S, k)
        assert res["d%d/in" % k].shape == (B, sides[0], sides[0], 3) and res["d%d/out" % k].shape == (B, sides[-1], sides[-1], 1)
        for i in range(N_LAYER_D):
            assert res["d%d/conv%d" % (k, i)].shape == (B, sides[i + 1], sides[i + 1], host.DISC_CH[i])


def test_stages_given_acts_are_those_of_the_own_forward():
    w = init_discriminator_weights(3)
    arrays = host.example_inputs(32, 2, 1)
    own, given = host.gen_grad(w, *arrays), host.gen_grad(w, *arrays, acts=host.forward(w, *arrays))
    assert sorted(own) == sorted(given) and all(own[n].tobytes() == given[n].tobytes() for n in own)


LD = np.longdouble


def conv_ld(x, kernel, bias, stride):
    """discriminator.conv2d_same in extended precision (numpy's longdouble: the x87 format with a 64-bit significand here)."""
    x, kernel = np.asarray(x, LD), np.asarray(kernel, LD)
    n, h, _, c = x.shape
    (pt, pb) = host.same_pad(h, 4, stride)
    ho = -(-h // stride)
    xp = np.zeros((n, h + pt + pb, h + pt + pb, c), LD)
    xp[:, pt:pt + h, pt:pt + h] = x
    out = np.zeros((n, ho, ho, kernel.shape[3]), LD)
    for a in range(4):
        for b in range(4):
            out += xp[:, a:a + (ho - 1) * stride + 1:stride, b:b + (ho - 1) * stride + 1:stride] @ kernel[a, b]
    return out + np.asarray(bias, LD)


def gen_ld(weights, con_rgb, mask_sv, masks=None, magnitudes=False):
    """discriminator.gen_f64's objective evaluated in extended precision; every LeakyReLU mask goes to `masks`.  With `magnitudes` the
    same operations with every operand replaced by its magnitude and every slope by 1: an upper bound M of the sum of the magnitudes
    of the terms of every sum along the evaluation."""
    mag = np.abs if magnitudes else (lambda a: a)
    x = mag(np.concatenate([np.asarray(con_rgb, LD), np.asarray(mask_sv, LD)], axis=3))
    n, S = x.shape[:2]
    gen = LD(0)
    for k in (1, 2, 3):
        ds = host.DOWNSIZE[k - 1]
        lo = 0 if ds < 4 else 1
        h = x if ds == 1 else x.reshape(n, S // ds, ds, S // ds, ds, 6)[:, :, lo:lo + 2, :, lo:lo + 2].mean(axis=(2, 4))
        for i in range(N_LAYER_D):
            st = "discriminator_%d/conv_stack/%d/" % (k, i)
            g, beta, mean, var = (np.asarray(weights[st + "bnorm/" + p], LD) for p in ("gamma", "beta", "moving_mean", "moving_variance"))
            inv = mag(g) / np.sqrt(var + LD(BN_EPS))
            y = conv_ld(h, mag(weights[st + "conv/kernel"]), mag(weights[st + "conv/bias"]), 2) * inv
            y = y + (mag(beta) + mag(mean) * inv if magnitudes else beta - mean * inv)
            if masks is not None:
                masks.append(np.asarray(y > 0))
            h = y if magnitudes else np.where(y >= 0, y, LD(host.LRELU_ALPHA) * y)
        st = "discriminator_%d/conv2/conv/" % k
        out = conv_ld(h, mag(weights[st + "kernel"]), mag(weights[st + "bias"]), 1).mean()
        gen = gen + out if magnitudes else gen - out
    return gen


@pytest.mark.parametrize("S,B", ((32, 2), (64, 1)))
def test_central_finite_differences_along_two_directions(S, B):
    """The gen objective is piecewise linear in con_rgb.  Where no LeakyReLU mask differs between x - e d, x and x + e d (asserted: a
    condition on FD_SEED and FD_STEP, not a tolerance) every pre-activation is linear on the segment, layer after layer, so the central
    quotient IS the directional derivative up to the rounding of the two loss values and of the two points.  That rounding is bounded a
    priori by the standard bound for sums of products: a loss value passes through five convolutions, each a sum of at most 16 * 64
    products plus the bias, then BatchNormalization's two operations and the slope, and at last a mean of at most 256 terms and the
    sum of three; it carries at most n u M with n = 5 * (1024 + 4) + 256 + 6 operations along a path, u the unit round-off and M the
    same evaluation on magnitudes (gen_ld(magnitudes=True)), which bounds the magnitude of everything any sum adds up.  M is about
    2e5 on these inputs, so in float64 (u = 2^-53) the bound n u M / e would be as large as the derivative itself at any step small
    enough for the masks to hold; the objective is therefore evaluated in numpy's extended precision (u = 2^-64 here; the variables
    are still the float32 ones), where the bound is three orders of magnitude below the derivative.  The points x +- e d are rounded
    within u (|x| + e |d|) per element, which moves a loss by at most u sum |grad| (|x| + e |d|); <grad, d> is itself summed in
    extended precision from gen_grad's float64 gradient, which the autograd tests hold to 4e-15 of its scale."""
    u = float(np.finfo(LD).eps) / 2
    w = init_discriminator_weights(3)
    gt, con, mask = host.example_inputs(S, B, FD_SEED)
    res = host.gen_grad(w, gt, con, mask)
    own = [np.asarray(host.forward(w, gt, con, mask)["d%d/conv%d" % (k, i)])[B:] > 0 for k in (1, 2, 3) for i in range(N_LAYER_D)]
    n_ops = 5 * (1024 + 4) + 256 + 6
    rng = np.random.default_rng(FD_SEED)
    grad, x, step = res["grad"].astype(LD), con.astype(LD), LD(FD_STEP)
    for j in range(2):
        d = rng.standard_normal(con.shape).astype(LD)
        masks = [[], [], []]
        lo, mid, hi = (gen_ld(w, x + LD(t) * step * d, mask, masks=m) for t, m in zip((-1, 0, 1), masks))
        for a, b, c, o in zip(*masks, own):
            assert (a == b).all() and (b == c).all() and (b == o).all(), "a LeakyReLU mask differs between the evaluation points"
        quotient, want = float((hi - lo) / (2 * step)), float((grad * d).sum())
        M = float(max(gen_ld(w, x + LD(t) * step * d, mask, magnitudes=True) for t in (-1, 1)))
        point = u * float((np.abs(grad) * (np.abs(x) + step * np.abs(d))).sum())
        bound = (n_ops * u * M + point) / FD_STEP + (3 * S * S * B * u + 4e-15) * float(np.abs(grad * d).sum())
        print("discriminator grad S=%d B=%d direction %d: quotient %.12g, <grad, d> %.12g, |difference| %.3g, a-priori bound %.3g (M %.3g, u %.3g)"
              % (S, B, j, quotient, want, abs(quotient - want), bound, M, u))
        assert abs(want) > 100 * bound, "the bound must mean something beside the derivative"
        assert abs(quotient - want) <= bound
        assert abs(float(mid - (hi + lo) / 2)) <= 2 * n_ops * u * M + 2 * point


def test_gen_f64_is_the_gen_term():
    w = init_discriminator_weights(3)
    gt, con, mask = host.example_inputs(32, 2, 1)
    gen = float(host.gan_losses(w, gt, con, mask)["losses"][0])
    assert abs(host.gen_f64(w, con, mask) - gen) <= 1e-6 * max(1.0, abs(gen))


def test_pack_dgrad_against_its_unpack():
    w = init_discriminator_weights(4)
    blob = pack.pack_discriminators_dgrad(w)
    layout, per = pack.disc_dgrad_layout()
    assert len(blob) == 3 * per * 4 == 1_394_688 and [n for n, _, _ in layout] == ["conv%d/dgrad" % i for i in range(N_LAYER_D)]
    back = pack.unpack_discriminators_dgrad(blob)
    for k in (1, 2, 3):
        folded = pack.disc_folded(w, k)
        np.testing.assert_array_equal(back[k - 1]["conv0"], folded["conv0"][0][:, :3])
        for i in range(1, N_LAYER_D):
            np.testing.assert_array_equal(back[k - 1]["conv%d" % i], folded["conv%d" % i][0])
    # the layout the kernel stages: chunk j of 8 output channels, tap t, channel o of the chunk, input channel c
    rec = np.frombuffer(blob, f32)[:per]
    off = dict((n, o) for n, o, _ in layout)["conv2/dgrad"]
    kern = pack.disc_folded(w, 1)["conv2"][0]                             # [16][32][64]
    for j, t, o, c in ((0, 0, 0, 0), (3, 5, 7, 31), (7, 15, 2, 9)):
        assert rec[off + ((j * 16 + t) * 8 + o) * 32 + c] == kern[t, c, j * 8 + o]
    with pytest.raises(ValueError, match="gradient blob"):
        pack.unpack_discriminators_dgrad(blob[:-4])
