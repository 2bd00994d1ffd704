"""The host statement of the backward of res_stack/5's lower half (blindshadowremoval_amd/generator_grad.py: bottleneck_grad) against
torch autograd in float64, on the closed forms of bottleneck_grad_cases and against central finite differences of the objective
<d_y3, y3> + <d_skip, xin> in extended precision; pack.pack_bottleneck_grad against its un-pack and
weights.generator_bottleneck_trainable_names against the checkpoint inventory."""
import json
import os

import numpy as np
import pytest

from blindshadowremoval_amd import generator_grad as host
from blindshadowremoval_amd import pack
from blindshadowremoval_amd.weights import BN_EPS, generator_bottleneck_trainable_names, generator_variable_shapes, init_weights

import bottleneck_grad_cases as cases

f32 = np.float32
LD = np.longdouble
ST = cases.ST
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def host_run(weights, xin, d_y3, d_skip, acts):
    out = host.bottleneck_grad(weights, xin, d_y3, d_skip, acts=acts)
    out["dtype"] = np.float64
    return out


@pytest.mark.parametrize("check", cases.CONSTRUCTED, ids=lambda c: c.__name__)
def test_constructed_case(check):
    check(host_run)


@pytest.mark.parametrize("h,w,B", cases.AUTOGRAD_SIZES)
def test_statement_matches_torch_autograd_in_float64(h, w, B):
    wt, xin, d_y3, d_skip = cases.case(h, w, B, 1)             # asserts both signs in a1 and in a2
    res = host.bottleneck_grad(wt, xin, d_y3, d_skip)
    d, at = cases.worst_scaled_diff(res, cases.autograd_grads(wt, xin, d_y3, d_skip))
    print("bottleneck grad h=%d w=%d B=%d: statement against torch autograd, worst scaled difference %.3g at %s (bound %.3g)"
          % (h, w, B, d, at, cases.AUTOGRAD_BOUND))
    assert d <= cases.AUTOGRAD_BOUND
    shapes = generator_variable_shapes()
    for name in cases.NAMES:
        assert res[name].shape == shapes[name] and res[name].dtype == np.float64 and np.abs(res[name]).max() > 0, name
    assert res["d_xin"].shape == (B, h, w, 261)
    for name in ("gz2", "gz1", "a1", "a2"):
        assert res[name].shape == (B, h, w, 128), name
    fw = host.bottleneck_forward(wt, xin)
    assert sorted(fw) == ["a1", "a2", "c1", "c2", "c3", "y3"] and fw["y3"].shape == (B, h, w, 257)
    # without d_skip the gradient at xin is the convolutions' share alone
    none = host.bottleneck_grad(wt, xin, d_y3)
    d, at = cases.worst_scaled_diff(none, cases.autograd_grads(wt, xin, d_y3))
    assert d <= cases.AUTOGRAD_BOUND, (d, at)


def test_the_statement_is_width_agnostic():
    """TSM's 877 input channels: the same statement against autograd, C read from xin."""
    wt, xin, d_y3, d_skip = cases.case(1, 4, 1, 2, C=877)
    assert wt["res_stack/5/conv1/kernel"].shape == (1, 1, 877, 128) and xin.shape == (1, 1, 4, 877)
    res = host.bottleneck_grad(wt, xin, d_y3, d_skip)
    d, at = cases.worst_scaled_diff(res, cases.autograd_grads(wt, xin, d_y3, d_skip))
    print("bottleneck grad C=877: statement against torch autograd, worst scaled difference %.3g at %s" % (d, at))
    assert res["d_xin"].shape == (1, 1, 4, 877) and d <= cases.AUTOGRAD_BOUND, (d, at)
    assert generator_bottleneck_trainable_names(variant="tsm") == list(cases.NAMES)
    for fn in (pack.pack_bottleneck_grad, pack.bottleneck_grad_record):
        with pytest.raises(ValueError) as e:
            fn(wt)
        assert str(e.value) == (pack.BOTTLENECK_TSM_TEXT if fn is pack.pack_bottleneck_grad else
                                "res_stack/5/conv1/kernel must be [1, 1, 261, 128], got (1, 1, 877, 128)")


def test_acts_given_are_those_of_the_own_forward():
    wt, xin, d_y3, d_skip = cases.case(2, 4, 2, 2)
    fw = host.bottleneck_forward(wt, xin)
    own = host.bottleneck_grad(wt, xin, d_y3, d_skip)
    given = host.bottleneck_grad(wt, xin, d_y3, d_skip, acts={"a1": fw["a1"], "a2": fw["a2"]})
    assert sorted(own) == sorted(given)
    for n in own:
        np.testing.assert_array_equal(given[n], own[n], err_msg=n)
    low = host.bottleneck_grad(wt, xin, d_y3, d_skip, dtype=f32)
    assert all(low[n].dtype == f32 for n in cases.OUTPUTS)
    assert cases.worst_scaled_diff(low, own)[0] <= 1e-4


@pytest.mark.parametrize("block", (3, 4))
def test_blocks_3_and_4_are_stated_and_packed(block):
    """The colour branch's blocks share their shapes: the statement of block 3 or 4 against autograd on block 5's slots holding that
    block's variables, and the blob of that block against the blob of those slots."""
    wt, xin, d_y3, d_skip = cases.case(2, 4, 2, 3)
    names = generator_bottleneck_trainable_names(block)
    assert names == [n.replace("res_stack/5/", "res_stack/%d/" % block) for n in cases.NAMES]
    res = host.bottleneck_grad(wt, xin, d_y3, d_skip, block=block)
    moved = cases.with_block5(wt, block)
    ref = cases.autograd_grads(moved, xin, d_y3, d_skip)
    as5 = {n5: res[n] for n5, n in zip(cases.NAMES, names)}
    as5["d_xin"] = res["d_xin"]
    d, at = cases.worst_scaled_diff(as5, ref)
    assert d <= cases.AUTOGRAD_BOUND, (d, at)
    assert not np.array_equal(res["d_xin"], host.bottleneck_grad(wt, xin, d_y3, d_skip)["d_xin"])
    assert pack.pack_bottleneck_grad(wt, block) == pack.pack_bottleneck_grad(moved) != pack.pack_bottleneck_grad(wt)
    assert tuple(host.bottleneck_norms(res, block)) == ("d_xin",) + tuple(names)
    for bad in (2, 6):
        with pytest.raises(ValueError) as e:
            pack.pack_bottleneck_grad(wt, bad)
        assert str(e.value) == pack.BOTTLENECK_BLOCK_TEXT % (bad,)


def _mass(wt, xin):
    """The absolute mass of y3: the same forward on |x|, |K|, |b|, a BatchNormalization as |inv| (c + |mean|) + |beta| and the LeakyReLU
    as the identity."""
    m = np.abs(np.asarray(xin, np.float64))
    for j in (1, 2, 3):
        K = np.abs(np.asarray(wt[ST + "conv%d/kernel" % j], np.float64))
        bias, inv, mean, _, _, beta = host.bottleneck_bn_vectors(wt, j)
        c = (host.conv3x3_same(m, K) if j == 2 else m @ K[0, 0]) + np.abs(bias)
        m = np.abs(inv) * (c + np.abs(mean)) + np.abs(beta)
    return m


def test_central_finite_differences(h=2, w=4, B=1, FD_STEP=1e-7):
    """On a segment along which neither LeakyReLU's mask changes (asserted for the five points used: a condition on the seed and the step,
    not a tolerance) the objective <d_y3, y3> + <d_skip, xin> is a smooth function p(t) of the step.  The central quotient
    q(e) = (p(e) - p(-e)) / 2e is p'(0) + c3 e^2 + O(e^4), so |q(2e) - q(e)| = 3 |c3| e^2 + O(e^4) bounds the truncation of q(e) with a
    factor 3 to spare, as the colour tail's test bounds its own.  The evaluations run in numpy's extended precision (u = 2^-64).  A value
    of y3 is formed by fewer than 2 (261 + 9 x 128 + 128) + 40 < 3200 operations a path, so its error is below 3200 u times its absolute
    mass (`_mass`).  The objective's error is below 3200 u A with A = sum |d_y3| mass(y3) + sum |d_skip| |xin|, the quotient's below that
    over e.  <grad, d> is summed in extended precision from bottleneck_grad's float64 gradient; its own rounding is below 1e-11 of
    sum |grad d|.  Two random directions in variable space and one in xin."""
    u = float(np.finfo(LD).eps) / 2
    wt, xin, d_y3, d_skip = cases.case(h, w, B, 4)
    res = host.bottleneck_grad(wt, xin, d_y3, d_skip)
    A = float((np.abs(d_y3.astype(np.float64)) * _mass(wt, xin)).sum() + np.abs(d_skip.astype(np.float64) * xin).sum())
    rng = np.random.default_rng(13)
    directions = [{n: rng.standard_normal(wt[n].shape) * np.abs(wt[n]).max() for n in cases.NAMES} for _ in range(2)]
    directions.append({"xin": rng.standard_normal(xin.shape) * np.abs(xin).max()})
    for j, d in enumerate(directions):
        def at(t):
            moved = {n: np.asarray(v, LD) + (LD(t) * LD(FD_STEP) * d[n].astype(LD) if n in d else LD(0)) for n, v in wt.items()
                     if n.startswith(ST) and "non_local" not in n}
            x2 = np.asarray(xin, LD) + (LD(t) * LD(FD_STEP) * d["xin"].astype(LD) if "xin" in d else LD(0))
            masks = []
            return host.bottleneck_objective_f64(moved, x2, d_y3, d_skip, masks=masks, dtype=LD), masks

        values = {t: at(t) for t in (-2, -1, 0, 1, 2)}
        assert values[0][0].dtype == LD
        for t in (-2, -1, 1, 2):
            assert len(values[t][1]) == 2
            for a, b in zip(values[t][1], values[0][1]):
                assert (a == b).all(), "a LeakyReLU's mask differs between the evaluation points"
        q1 = (values[1][0] - values[-1][0]) / (2 * LD(FD_STEP))
        q2 = (values[2][0] - values[-2][0]) / (4 * LD(FD_STEP))
        key = {"xin": "d_xin"}
        want = sum((res[key.get(n, n)].astype(LD) * d[n].astype(LD)).sum() for n in d)
        mass = float(sum(np.abs(res[key.get(n, n)] * d[n]).sum() for n in d))
        bound = abs(float(q2 - q1)) + 3200 * u * A / FD_STEP + 1e-11 * mass
        print("bottleneck grad direction %d: quotient %.12g, <grad, d> %.12g, |difference| %.3g, bound %.3g (|q(2e) - q(e)| %.3g), sum |grad d| %.3g"
              % (j, float(q1), float(want), abs(float(q1 - want)), bound, abs(float(q2 - q1)), mass))
        assert mass > 100 * bound, "the bound must mean something beside the terms of the derivative"
        assert abs(float(q1 - want)) <= bound


def test_pack_against_its_unpack():
    wt = init_weights(4)
    blob = pack.pack_bottleneck_grad(wt)
    layout, total = pack.bottleneck_grad_layout()
    k2n = 9 * 128 * 128
    assert len(blob) == total * 4 == (272 * 128 + 128 + k2n + 128 + 272 * 128 + k2n + 128 * 384 + 261 * 128 + k2n + 128 * 257 + 8 * 128 + 4 * 257) * 4
    assert all(off % 4 == 0 for name, off, _ in layout if name[0] in "wb")          # every folded image is read with 16-byte loads
    back = pack.unpack_bottleneck_grad(blob)
    assert sorted(back) == sorted(name for name, _, _ in layout) == sorted(pack.bottleneck_grad_record(wt))
    k1, k2, k3 = (wt[ST + "conv%d/kernel" % j].astype(np.float64) for j in (1, 2, 3))
    vec = {}
    for j in (1, 2, 3):
        rstd = 1.0 / np.sqrt(wt[ST + "bnorm%d/moving_variance" % j].astype(np.float64) + BN_EPS)
        inv = wt[ST + "bnorm%d/gamma" % j].astype(np.float64) * rstd
        vec[j] = (inv, rstd)
        np.testing.assert_array_equal(back["vecs%d" % j][0], wt[ST + "conv%d/bias" % j])
        np.testing.assert_array_equal(back["vecs%d" % j][1], inv.astype(f32))
        np.testing.assert_array_equal(back["vecs%d" % j][2], wt[ST + "bnorm%d/moving_mean" % j])
        np.testing.assert_array_equal(back["vecs%d" % j][3], rstd.astype(f32))
        np.testing.assert_array_equal(back["k%d" % j].reshape(-1), wt[ST + "conv%d/kernel" % j].reshape(-1))
    # formed in float64, rounded once
    np.testing.assert_array_equal(back["w1f"][:261], (k1[0, 0] * vec[1][0]).astype(f32))
    np.testing.assert_array_equal(back["w1t"][:, :261], (k1[0, 0] * vec[1][0]).T.astype(f32))
    np.testing.assert_array_equal(back["w3t"][:257], (k3[0, 0] * vec[3][0]).T.astype(f32))
    assert not back["w1f"][261:].any() and not back["w1t"][:, 261:].any() and not back["w3t"][257:].any()
    for a in range(3):
        for b in range(3):
            np.testing.assert_array_equal(back["w2f"][3 * a + b], (k2[a, b] * vec[2][0]).astype(f32))
            # turned by 180 degrees, channel roles swapped, inv2 on the rows
            np.testing.assert_array_equal(back["w2t"][3 * a + b], (k2[2 - a, 2 - b] * vec[2][0]).T.astype(f32))
    for j in (1, 2):
        bias, mean, beta = (wt[ST + n % j].astype(np.float64) for n in ("conv%d/bias", "bnorm%d/moving_mean", "bnorm%d/beta"))
        np.testing.assert_array_equal(back["b%df" % j], ((bias - mean) * vec[j][0] + beta).astype(f32))
    # the folded images reproduce the statement's activations, and the turned image its data gradient
    wt3, xin, d_y3, _ = cases.case(2, 4, 1, 6)
    rec = {k: v.astype(np.float64) for k, v in pack.bottleneck_grad_record(wt3).items()}
    fw = host.bottleneck_forward(wt3, xin)
    x = xin.astype(np.float64)
    lrelu = lambda z: np.where(z >= 0, z, 0.3 * z)                                   # noqa: E731
    a1 = lrelu(x @ rec["w1f"][:261] + rec["b1f"])
    a2 = lrelu(host.conv3x3_same(a1, rec["w2f"].reshape(3, 3, 128, 128)) + rec["b2f"])
    assert np.abs(a1 - fw["a1"]).max() <= 1e-5 * np.abs(fw["a1"]).max() and np.abs(a2 - fw["a2"]).max() <= 1e-5 * np.abs(fw["a2"]).max()
    st = host.bottleneck_grad(wt3, xin, d_y3)
    pre = host.conv3x3_same(st["gz2"], rec["w2t"].reshape(3, 3, 128, 128))
    want = host.conv3x3_same_dgrad(st["gz2"] * host.bottleneck_bn_vectors(wt3, 2)[1], wt3[ST + "conv2/kernel"])
    assert np.abs(pre - want).max() <= 1e-6 * np.abs(want).max()
    with pytest.raises(ValueError, match="bottleneck gradient blob"):
        pack.unpack_bottleneck_grad(blob[:-4])


def test_trainable_names_against_the_inventory():
    names = generator_bottleneck_trainable_names()
    shapes = generator_variable_shapes()
    assert names == [ST + p for p in ("conv1/kernel", "conv1/bias", "conv2/kernel", "conv2/bias", "conv3/kernel", "conv3/bias", "bnorm1/gamma",
                                      "bnorm1/beta", "bnorm2/gamma", "bnorm2/beta", "bnorm3/gamma", "bnorm3/beta")]
    assert tuple(names) == host.BOTTLENECK_NORM_NAMES[1:] and host.BOTTLENECK_NORM_NAMES[0] == "d_xin"
    assert sum(int(np.prod(shapes[n])) for n in names) == 215299
    assert generator_bottleneck_trainable_names(3)[0] == "res_stack/3/conv1/kernel"
    with open(os.path.join(GOLDEN, "gsc_ckpt94_inventory.json")) as fh:
        inventory = json.load(fh)["gsc"]["variables"]
    for n in names:
        assert tuple(inventory[n]) == shapes[n], n
    norms = host.bottleneck_norms({n: np.full(shapes.get(n, (1, 1, 4, 261)), -2.0) for n in host.BOTTLENECK_NORM_NAMES})
    assert tuple(norms) == host.BOTTLENECK_NORM_NAMES and norms[ST + "conv1/bias"] == (256.0, 2.0)
