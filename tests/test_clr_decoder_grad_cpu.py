"""The host statement of the generator's colour decoder backward (blindshadowremoval_amd/generator_grad.py: decoder_grad) against torch
autograd in float64 over F.conv_transpose2d, on the closed forms of clr_decoder_grad_cases and against central finite differences of
the objective <d_f, f> in extended precision; pack.pack_clr_decoder_grad against its un-pack and
weights.generator_decoder_trainable_names against the checkpoint inventory."""
import json
import os

import numpy as np
import pytest

from blindshadowremoval_amd import generator_grad as host
from blindshadowremoval_amd import pack
from blindshadowremoval_amd.weights import BN_EPS, generator_decoder_trainable_names, generator_variable_shapes, init_weights

import clr_decoder_grad_cases as cases

f32 = np.float32
LD = np.longdouble
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def host_run(weights, x, d_f, acts):
    out = host.decoder_grad(weights, x, d_f, acts=acts)
    out["dtype"] = np.float64
    return out


def autograd_bound():
    """4 x the largest figure tools/make_clr_decoder_grad_fixture.py measured when it wrote the fixture (`measured`), never above 1e-9."""
    measured = float(np.load(os.path.join(GOLDEN, "clr_decoder_grad_%dx%d.npz" % cases.FIXTURE[:2]))["measured"])
    assert abs(measured - cases.AUTOGRAD_MEASURED) <= 0.05e-15
    return min(4 * measured, cases.AUTOGRAD_CAP)


@pytest.mark.parametrize("check", cases.CONSTRUCTED, ids=lambda c: c.__name__)
def test_constructed_case(check):
    check(host_run)


@pytest.mark.parametrize("h,w,B", cases.AUTOGRAD_SIZES)
def test_statement_matches_torch_autograd_in_float64(h, w, B):
    wt, x, d_f = cases.case(h, w, B, 1)                     # asserts both signs of all three pre-activations
    res = host.decoder_grad(wt, x, d_f)
    d, at = cases.worst_scaled_diff(res, cases.autograd_grads(wt, x, d_f))
    print("colour decoder grad h=%d w=%d B=%d: statement against torch autograd, worst scaled difference %.3g at %s (bound %.3g)"
          % (h, w, B, d, at, autograd_bound()))
    assert d <= autograd_bound()
    shapes = generator_variable_shapes()
    for name in cases.NAMES:
        assert res[name].shape == shapes[name] and res[name].dtype == np.float64 and np.abs(res[name]).max() > 0, name
    assert res["d_x"].shape == (B, h, w, 261)
    for name, m, c in (("gz1", 2, 128), ("gz2", 4, 96), ("gz3", 8, 64), ("f1", 2, 128), ("f2", 4, 96), ("f", 8, 64)):
        assert res[name].shape == (B, m * h, m * w, c), name


def test_the_statement_is_width_agnostic():
    """TSM's 877 input channels: the same statement against autograd, C read from the kernel."""
    wt = init_weights(3, variant="tsm")
    assert wt["clr_up1/conv/kernel"].shape == (3, 3, 128, 877)
    x, d_f = host.decoder_example_inputs(1, 4, 1, 2, C=877)
    res = host.decoder_grad(wt, x, d_f)
    d, at = cases.worst_scaled_diff(res, cases.autograd_grads(wt, x, d_f))
    assert res["d_x"].shape == (1, 1, 4, 877) and d <= autograd_bound(), (d, at)
    with pytest.raises(ValueError) as e:
        pack.pack_clr_decoder_grad(wt)
    assert str(e.value) == pack.CLR_DECODER_TSM_TEXT % ((3, 3, 128, 877),)


def test_acts_given_are_those_of_the_own_forward():
    wt, x, d_f = cases.case(2, 4, 2, 2)
    f1, f2, f = host.decoder_forward(wt, x)
    own, given = host.decoder_grad(wt, x, d_f), host.decoder_grad(wt, x, d_f, acts={"f1": f1, "f2": f2, "f": f})
    assert sorted(own) == sorted(given)
    for n in own:
        np.testing.assert_array_equal(given[n], own[n], err_msg=n)


def test_central_finite_differences(h=1, w=4, B=1, FD_STEP=1e-7):
    """On a segment along which no LeakyReLU mask changes (asserted for the five points used: a condition on the seed and the step, not a
    tolerance) the objective <d_f, f> is a polynomial p(t) in the step.  The central quotient q(e) = (p(e) - p(-e)) / 2e is p'(0) + c3 e^2
    + ..., so |q(2e) - q(e)| = 3 |c3| e^2 + O(e^4) bounds the truncation of q(e) with a factor 3 to spare, as the colour tail's test bounds
    its own.  The evaluations run in numpy's extended precision (u = 2^-64): a value of f is formed by fewer than 9 (261 + 128 + 96) + 3 x 8
    = 4389 operations a path, so its error is below 5000 u times its absolute mass — the same forward on |x|, |K|, |bias|, with the
    BatchNormalization as |inv| (c + |mean|) + |beta| and the LeakyReLU as the identity — and the objective's below 5000 u A with A =
    sum |d_f| mass(f), the quotient's below that over e.  <grad, d> is summed in extended precision from decoder_grad's float64 gradient;
    its own rounding is below 1e-11 of sum |grad d|.  Two random directions in variable space and one in x."""
    u = float(np.finfo(LD).eps) / 2
    wt, x, d_f = cases.case(h, w, B, 4)
    res = host.decoder_grad(wt, x, d_f)
    mass_f = np.abs(np.asarray(x, np.float64))
    for stem in host.DECODER_LAYERS:
        bias, inv, mean, _, beta = host.bn_vectors(wt, stem)
        c = host.convt3x3_same(mass_f, np.abs(np.asarray(wt[stem + "/conv/kernel"], np.float64))) + np.abs(bias)
        mass_f = np.abs(inv) * (c + np.abs(mean)) + np.abs(beta)
    A = float((np.abs(d_f.astype(np.float64)) * mass_f).sum())
    rng = np.random.default_rng(11)
    directions = [{n: rng.standard_normal(wt[n].shape) * np.abs(wt[n]).max() for n in cases.NAMES} for _ in range(2)]
    directions.append({"x": rng.standard_normal(x.shape) * np.abs(x).max()})
    for j, d in enumerate(directions):
        def at(t):
            moved = {n: np.asarray(v, LD) + (LD(t) * LD(FD_STEP) * d[n].astype(LD) if n in d else LD(0)) for n, v in wt.items()
                     if n.split("/", 1)[0] in host.DECODER_LAYERS}
            x2 = np.asarray(x, LD) + (LD(t) * LD(FD_STEP) * d["x"].astype(LD) if "x" in d else LD(0))
            masks = []
            return host.decoder_objective_f64(moved, x2, d_f, masks=masks, dtype=LD), masks

        values = {t: at(t) for t in (-2, -1, 0, 1, 2)}
        for t in (-2, -1, 1, 2):
            for a, b in zip(values[t][1], values[0][1]):
                assert (a == b).all(), "a LeakyReLU mask differs between the evaluation points"
        q1 = (values[1][0] - values[-1][0]) / (2 * LD(FD_STEP))
        q2 = (values[2][0] - values[-2][0]) / (4 * LD(FD_STEP))
        key = {"x": "d_x"}
        want = sum((res[key.get(n, n)].astype(LD) * d[n].astype(LD)).sum() for n in d)
        mass = float(sum(np.abs(res[key.get(n, n)] * d[n]).sum() for n in d))
        bound = abs(float(q2 - q1)) + 5000 * u * A / FD_STEP + 1e-11 * mass
        print("colour decoder grad direction %d: quotient %.12g, <grad, d> %.12g, |difference| %.3g, bound %.3g (|q(2e) - q(e)| %.3g), sum |grad d| %.3g"
              % (j, float(q1), float(want), abs(float(q1 - want)), bound, abs(float(q2 - q1)), mass))
        assert mass > 100 * bound, "the bound must mean something beside the terms of the derivative"
        assert abs(float(q1 - want)) <= bound


def test_pack_against_its_unpack():
    wt = init_weights(4)
    blob = pack.pack_clr_decoder_grad(wt)
    layout, total = pack.clr_decoder_grad_layout()
    assert len(blob) == total * 4 == 965376 * 4
    assert all(off % 4 == 0 for _, off, _ in layout)                      # every record is read with 16-byte loads
    back = pack.unpack_clr_decoder_grad(blob)
    for i, (o, c, cp) in enumerate(pack.CLR_DECODER_SHAPES, 1):
        stem = "clr_up%d" % i
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
    with pytest.raises(ValueError, match="colour decoder gradient blob"):
        pack.unpack_clr_decoder_grad(blob[:-4])


def test_trainable_names_against_the_inventory():
    names = generator_decoder_trainable_names()
    shapes = generator_variable_shapes()
    assert names == ["clr_up%d/%s" % (i, p) for i in (1, 2, 3) for p in ("conv/kernel", "conv/bias", "bnorm/gamma", "bnorm/beta")]
    assert tuple(names) == host.DECODER_NORM_NAMES[1:] and host.DECODER_NORM_NAMES[0] == "d_x"
    assert [shapes[n] for n in names[::4]] == [(3, 3, 128, 261), (3, 3, 96, 128), (3, 3, 64, 96)]
    assert sum(int(np.prod(shapes[n])) for n in names) == 467424
    assert generator_variable_shapes("tsm")[generator_decoder_trainable_names("tsm")[0]] == (3, 3, 128, 877)
    with open(os.path.join(GOLDEN, "gsc_ckpt94_inventory.json")) as fh:
        inventory = json.load(fh)["gsc"]["variables"]
    for n in names:
        assert tuple(inventory[n]) == shapes[n], n
    norms = host.decoder_norms({n: np.full(shapes[n] if n != "d_x" else (1, 1, 4, 261), -2.0) for n in host.DECODER_NORM_NAMES})
    assert tuple(norms) == host.DECODER_NORM_NAMES and norms["clr_up3/conv/bias"] == (128.0, 2.0)
