"""The host statement of the generator's grey decoder backward (blindshadowremoval_amd/generator_grad.py: grey_decoder_grad) against
torch autograd in float64 over F.conv_transpose2d and torch.cat, on the closed forms of grey_decoder_grad_cases and against central
finite differences of the objective <d_y, y> in extended precision; pack.pack_grey_decoder_grad against its un-pack and the statement's
data gradient; weights.generator_grey_decoder_trainable_names against the checkpoint inventory; and decoder_grad, which shares the
per-layer body, against the colour decoder's fixture."""
import json
import os

import numpy as np
import pytest

from blindshadowremoval_amd import generator_grad as host
from blindshadowremoval_amd import pack
from blindshadowremoval_amd.weights import BN_EPS, generator_grey_decoder_trainable_names, generator_variable_shapes, init_weights

import grey_decoder_grad_cases as cases

f32 = np.float32
LD = np.longdouble
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def host_run(weights, x, x3, x2, d_y, acts):
    out = host.grey_decoder_grad(weights, x, x3, x2, d_y, acts=acts)
    out["dtype"] = np.float64
    return out


@pytest.mark.parametrize("check", cases.CONSTRUCTED, ids=lambda c: c.__name__)
def test_constructed_case(check):
    check(host_run)


@pytest.mark.parametrize("h,w,B", cases.AUTOGRAD_SIZES)
def test_statement_matches_torch_autograd_in_float64(h, w, B):
    wt, x, x3, x2, d_y = cases.case(h, w, B, 1)                     # asserts both signs of all three pre-activations
    res = host.grey_decoder_grad(wt, x, x3, x2, d_y)
    ref = cases.autograd_grads(wt, x, x3, x2, d_y)
    for name in cases.OUTPUTS:
        print("grey decoder grad h=%d w=%d B=%d %s: statement against torch autograd, scaled difference %.3g"
              % (h, w, B, name, cases.worst_scaled_diff(res, ref, (name,))[0]))
    d, at = cases.worst_scaled_diff(res, ref)
    print("grey decoder grad h=%d w=%d B=%d: worst scaled difference %.3g at %s (bound %.3g)" % (h, w, B, d, at, cases.AUTOGRAD_BOUND))
    assert d <= cases.AUTOGRAD_BOUND <= cases.AUTOGRAD_CAP
    shapes = generator_variable_shapes()
    for name in cases.NAMES:
        assert res[name].shape == shapes[name] and res[name].dtype == np.float64 and np.abs(res[name]).max() > 0, name
    assert res["d_x"].shape == (B, h, w, 257) and res["d_x3"].shape == (B, 2 * h, 2 * w, 64) and res["d_x2"].shape == (B, 4 * h, 4 * w, 64)
    for name, m, c in (("gz1", 2, 96), ("gz2", 4, 64), ("gz3", 8, 64), ("up1", 2, 96), ("up2", 4, 64), ("y", 8, 64)):
        assert res[name].shape == (B, m * h, m * w, c), name


def test_acts_given_are_those_of_the_own_forward():
    wt, x, x3, x2, d_y = cases.case(2, 4, 2, 2)
    up1, up2, y = host.grey_decoder_forward(wt, x, x3, x2)
    own = host.grey_decoder_grad(wt, x, x3, x2, d_y)
    given = host.grey_decoder_grad(wt, x, x3, x2, d_y, acts={"up1": up1, "up2": up2, "y": y})
    assert sorted(own) == sorted(given)
    for n in own:
        np.testing.assert_array_equal(given[n], own[n], err_msg=n)


def test_central_finite_differences(h=1, w=4, B=1, FD_STEP=1e-7):
    """On a segment along which no LeakyReLU mask changes (asserted for the five points used: a condition on the seed and the step, not a
    tolerance) the objective <d_y, y> is a polynomial p(t) in the step.  The central quotient q(e) = (p(e) - p(-e)) / 2e is p'(0) + c3 e^2
    + ..., so |q(2e) - q(e)| = 3 |c3| e^2 + O(e^4) bounds the truncation of q(e) with a factor 3 to spare, as the colour tail's test bounds
    its own.  The evaluations run in numpy's extended precision (u = 2^-64): a value of y is formed by fewer than 9 (257 + 160 + 128) + 3 x 8
    = 4929 operations a path, so its error is below 5000 u times its absolute mass — the same forward on |x|, |x3|, |x2|, |K|, |bias|,
    with the BatchNormalization as |inv| (c + |mean|) + |beta| and the LeakyReLU as the identity — and the objective's below 5000 u A with
    A = sum |d_y| mass(y), the quotient's below that over e.  <grad, d> is summed in extended precision from grey_decoder_grad's float64
    gradient; its own rounding is below 1e-11 of sum |grad d|.  Two random directions in variable space and one each in x, x3 and x2."""
    u = float(np.finfo(LD).eps) / 2
    wt, x, x3, x2, d_y = cases.case(h, w, B, 4)
    ins = {"x": x, "x3": x3, "x2": x2}
    res = host.grey_decoder_grad(wt, x, x3, x2, d_y)
    mass = np.abs(np.asarray(x, np.float64))
    for stem, skip in zip(host.GREY_DECODER_LAYERS, (None, x3, x2)):
        if skip is not None:
            mass = np.concatenate([mass, np.abs(np.asarray(skip, np.float64))], axis=3)
        bias, inv, mean, _, beta = host.bn_vectors(wt, stem)
        c = host.convt3x3_same(mass, np.abs(np.asarray(wt[stem + "/conv/kernel"], np.float64))) + np.abs(bias)
        mass = np.abs(inv) * (c + np.abs(mean)) + np.abs(beta)
    A = float((np.abs(d_y.astype(np.float64)) * mass).sum())
    rng = np.random.default_rng(11)
    directions = [{n: rng.standard_normal(wt[n].shape) * np.abs(wt[n]).max() for n in cases.NAMES} for _ in range(2)]
    directions += [{k: rng.standard_normal(v.shape) * np.abs(v).max()} for k, v in ins.items()]
    for j, d in enumerate(directions):
        def at(t):
            moved = {n: np.asarray(v, LD) + (LD(t) * LD(FD_STEP) * d[n].astype(LD) if n in d else LD(0)) for n, v in wt.items()
                     if n.split("/", 1)[0] in host.GREY_DECODER_LAYERS}
            xs = [np.asarray(v, LD) + (LD(t) * LD(FD_STEP) * d[k].astype(LD) if k in d else LD(0)) for k, v in ins.items()]
            masks = []
            return host.grey_decoder_objective_f64(moved, *xs, d_y, masks=masks, dtype=LD), masks

        values = {t: at(t) for t in (-2, -1, 0, 1, 2)}
        for t in (-2, -1, 1, 2):
            assert len(values[t][1]) == 3
            for a, b in zip(values[t][1], values[0][1]):
                assert (a == b).all(), "a LeakyReLU mask differs between the evaluation points"
        q1 = (values[1][0] - values[-1][0]) / (2 * LD(FD_STEP))
        q2 = (values[2][0] - values[-2][0]) / (4 * LD(FD_STEP))
        key = {"x": "d_x", "x3": "d_x3", "x2": "d_x2"}
        want = sum((res[key.get(n, n)].astype(LD) * d[n].astype(LD)).sum() for n in d)
        mass_d = float(sum(np.abs(res[key.get(n, n)] * d[n]).sum() for n in d))
        bound = abs(float(q2 - q1)) + 5000 * u * A / FD_STEP + 1e-11 * mass_d
        print("grey decoder grad direction %d: quotient %.12g, <grad, d> %.12g, |difference| %.3g, bound %.3g (|q(2e) - q(e)| %.3g), sum |grad d| %.3g"
              % (j, float(q1), float(want), abs(float(q1 - want)), bound, abs(float(q2 - q1)), mass_d))
        assert mass_d > 100 * bound, "the bound must mean something beside the terms of the derivative"
        assert abs(float(q1 - want)) <= bound


def test_pack_against_its_unpack_and_the_statements_data_gradient():
    wt = init_weights(4)
    blob = pack.pack_grey_decoder_grad(wt)
    layout, total = pack.grey_decoder_grad_layout()
    assert len(blob) == total * 4 == (222048 + 248832 + 384 + 2 * 92160 + 256 + 2 * 73728 + 256) * 4
    assert all(off % 4 == 0 for _, off, _ in layout)                      # every record is read with 16-byte loads
    back = pack.unpack_grey_decoder_grad(blob)
    x, x3, x2, d_y = host.grey_decoder_example_inputs(1, 4, 1, 3)
    st = host.grey_decoder_grad(wt, x, x3, x2, d_y)
    skips = {3: "d_x2", 2: "d_x3"}
    for i, (o, c, cp) in enumerate(pack.GREY_DECODER_SHAPES, 1):
        stem = "up%d" % i
        k = wt[stem + "/conv/kernel"]
        assert k.shape == (3, 3, o, c)
        np.testing.assert_array_equal(back["k%d" % i].reshape(3, 3, o, c), k)
        rstd = 1.0 / np.sqrt(wt[stem + "/bnorm/moving_variance"].astype(np.float64) + BN_EPS)
        inv = wt[stem + "/bnorm/gamma"].astype(np.float64) * rstd
        vecs = back["vecs%d" % i]
        np.testing.assert_array_equal(vecs[0], wt[stem + "/conv/bias"])
        np.testing.assert_array_equal(vecs[1], inv.astype(f32))
        np.testing.assert_array_equal(vecs[2], wt[stem + "/bnorm/moving_mean"])
        np.testing.assert_array_equal(vecs[3], rstd.astype(f32))
        kf = back["kf%d" % i].reshape(3, 3, o, cp)
        np.testing.assert_array_equal(kf[..., :c], (k.astype(np.float64) * inv[:, None]).astype(f32))       # formed in float64, rounded once
        assert not kf[..., c:].any()
        # the folded kernel is the data gradient's: gz through it is the statement's dx within the one float32 rounding of kf
        dx = host.convt3x3_same_dgrad(st["gz%d" % i], kf[..., :c])
        own = {1: 0, 2: 96, 3: 64}[i]
        want = st["d_x"] if i == 1 else st[skips[i]]
        assert np.abs(dx[..., own:] - want).max() <= 1e-6 * np.abs(want).max(), stem
    with pytest.raises(ValueError, match="grey decoder gradient blob"):
        pack.unpack_grey_decoder_grad(blob[:-4])


@pytest.mark.parametrize("variant,stem,shape", (("tsm", "up1", (3, 3, 96, 291)), ("rgb", "up1", (3, 3, 192, 513))))
def test_pack_refuses_other_widths(variant, stem, shape):
    wt = init_weights(3, variant=variant)
    assert wt[stem + "/conv/kernel"].shape == shape
    with pytest.raises(ValueError) as e:
        pack.pack_grey_decoder_grad(wt)
    assert str(e.value) == pack.GREY_DECODER_WIDTH_TEXT % (stem, 96, 257, shape)
    assert "GSC widths only" in str(e.value) and "TSM" in str(e.value) and "RGB" in str(e.value)


def test_trainable_names_against_the_inventory():
    names = generator_grey_decoder_trainable_names()
    shapes = generator_variable_shapes()
    assert names == ["up%d/%s" % (i, p) for i in (1, 2, 3) for p in ("conv/kernel", "conv/bias", "bnorm/gamma", "bnorm/beta")]
    assert host.GREY_DECODER_LAYERS == ("up1", "up2", "up3")
    assert host.GREY_DECODER_NORM_NAMES == ("d_x", "d_x3", "d_x2") + tuple(names)
    assert [shapes[n] for n in names[::4]] == [(3, 3, 96, 257), (3, 3, 64, 160), (3, 3, 64, 128)]
    assert [int(np.prod(shapes[n])) for n in names[::4]] == [222048, 92160, 73728]
    assert sum(int(np.prod(shapes[n])) for n in names) == 388608
    assert generator_variable_shapes("tsm")[generator_grey_decoder_trainable_names("tsm")[0]] == (3, 3, 96, 291)
    with open(os.path.join(GOLDEN, "gsc_ckpt94_inventory.json")) as fh:
        inventory = json.load(fh)["gsc"]["variables"]
    for n in names:
        assert tuple(inventory[n]) == shapes[n], n
    data = {"d_x": (1, 1, 4, 257), "d_x3": (1, 2, 8, 64), "d_x2": (1, 4, 16, 64)}
    norms = host.grey_decoder_norms({n: np.full(data[n] if n in data else shapes[n], -2.0) for n in host.GREY_DECODER_NORM_NAMES})
    assert tuple(norms) == host.GREY_DECODER_NORM_NAMES and norms["up3/conv/bias"] == (128.0, 2.0)


def test_example_inputs():
    x, x3, x2, d_y = host.grey_decoder_example_inputs(2, 4, 2, 1)
    assert [a.shape for a in (x, x3, x2, d_y)] == [(2, 2, 4, 257), (2, 4, 8, 64), (2, 8, 16, 64), (2, 16, 32, 64)]
    assert all(a.dtype == f32 for a in (x, x3, x2, d_y))
    for a in (x, x3, x2):                                    # like LeakyReLU outputs: the negative side is 0.3 of a normal draw's
        assert 0.4 < (a > 0).mean() < 0.6 and a.min() > 0.3 * -6
    again = host.grey_decoder_example_inputs(2, 4, 2, 1)
    assert all(a.tobytes() == b.tobytes() for a, b in zip((x, x3, x2, d_y), again))
    assert host.grey_decoder_example_inputs(2, 4, 2, 2)[3].tobytes() != d_y.tobytes()


def test_decoder_grad_keeps_its_bytes_on_the_shared_layer_body():
    """decoder_grad now runs grey_decoder_grad's per-layer body.  On decoder_example_inputs(2, 4, 2) its thirteen outputs are within the
    colour decoder fixture's own bound of what that fixture holds from before (tests/test_clr_decoder_grad_fixture.py: float32 copies),
    and they are byte for byte those of the loop as it stood before the helper, restated here."""
    import clr_decoder_grad_cases as clr
    h, w, B = clr.FIXTURE
    stem = os.path.join(GOLDEN, "clr_decoder_grad_%dx%d" % (h, w))
    fix = np.load(stem + ".npz")
    want = {n: fix[n] for n in clr.OUTPUTS if n != "clr_up1/conv/kernel"}
    want["clr_up1/conv/kernel"] = np.concatenate([np.load(stem + "_k1a.npz")["k1a"], np.load(stem + "_k1b.npz")["k1b"]])
    wt, x, d_f = clr.case(h, w, B, int(fix["seed"]))
    res = host.decoder_grad(wt, x, d_f)
    assert clr.worst_scaled_diff(res, want)[0] <= min(4 * float(fix["measured"]), clr.AUTOGRAD_CAP) + 2.0 ** -24
    T = np.float64
    f1, f2, f = host.decoder_forward(wt, np.asarray(x, T), T)
    before = {}
    g = np.asarray(d_f, T)
    for i, a_in, a_out in ((3, f2, f), (2, f1, f2), (1, np.asarray(x, T), f1)):
        st = host.DECODER_LAYERS[i - 1]
        K = np.asarray(wt[st + "/conv/kernel"], T)
        bias, inv, mean, rstd, _ = host.bn_vectors(wt, st)
        gz = host.leaky_grad(g, a_out)
        S = gz.sum(axis=(0, 1, 2))
        Wg = host.convt3x3_same_wgrad(a_in, gz)
        before["gz%d" % i] = gz
        before[st + "/conv/kernel"] = Wg * inv[:, None]
        before[st + "/conv/bias"] = inv * S
        before[st + "/bnorm/gamma"] = (((K * Wg).sum(axis=(0, 1, 3)) + bias * S) - mean * S) * rstd
        before[st + "/bnorm/beta"] = S
        g = host.convt3x3_same_dgrad(gz * inv, K)
    before["d_x"] = g
    assert set(before) | {"f1", "f2", "f"} == set(res)
    for n, v in before.items():
        assert res[n].tobytes() == v.tobytes(), n
