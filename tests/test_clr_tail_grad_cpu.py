"""The host statement of the generator's colour tail backward (blindshadowremoval_amd/generator_grad.py: tail_grad) against torch
autograd in float64, on the closed forms of clr_tail_grad_cases and against central finite differences of the float64 objective
<g_con, con_rgb> in extended precision; pack.pack_clr_tail_grad against its un-pack and weights.generator_tail_trainable_names against
the checkpoint inventory."""
import json
import os

import numpy as np
import pytest

from blindshadowremoval_amd import generator_grad as host
from blindshadowremoval_amd import pack
from blindshadowremoval_amd.weights import BN_EPS, generator_tail_trainable_names, generator_variable_shapes, init_weights

import clr_tail_grad_cases as cases

f32 = np.float32
LD = np.longdouble
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# The largest scaled difference between the statement and torch autograd over AUTOGRAD_SIZES and the fixture's size, as
# tools/make_clr_tail_grad_fixture.py measured it when it wrote the fixture (stored there as `measured`): 2.76e-15.
AUTOGRAD_MEASURED = 2.76e-15


def host_run(weights, gs, f, g_con, g_gs):
    out = host.tail_grad(weights, gs, f, g_con, g_gs)
    out["dtype"] = np.float64
    return out


def autograd_bound():
    measured = float(np.load(os.path.join(GOLDEN, "clr_tail_grad_%d.npz" % cases.FIXTURE[0]))["measured"])
    assert abs(measured - AUTOGRAD_MEASURED) <= 0.005e-15
    return min(4 * measured, cases.AUTOGRAD_CAP)


@pytest.mark.parametrize("check", cases.CONSTRUCTED, ids=lambda c: c.__name__)
def test_constructed_case(check):
    check(host_run)


@pytest.mark.parametrize("H,W,B", cases.AUTOGRAD_SIZES)
def test_statement_matches_torch_autograd_in_float64(H, W, B):
    w, gs, f, g_con, g_gs = cases.case(H, W, B, 1)
    res = host.tail_grad(w, gs, f, g_con, g_gs)
    d, at = cases.worst_scaled_diff(res, cases.autograd_grads(w, gs, f, g_con, g_gs))
    print("colour tail grad H=%d W=%d B=%d: statement against torch autograd, worst scaled difference %.3g at %s (bound %.3g)"
          % (H, W, B, d, at, autograd_bound()))
    assert d <= autograd_bound()
    shapes = generator_variable_shapes()
    for name in cases.NAMES:
        assert res[name].shape == shapes[name] and res[name].dtype == np.float64 and np.abs(res[name]).max() > 0, name
    assert res["d_f"].shape == (B, H, W, 64) and res["d_gs"].shape == (B, H, W, 1)
    for name in ("a1", "a2", "gz1", "gz2"):
        assert res[name].shape == (B, H, W, 16)


def test_acts_given_are_those_of_the_own_forward():
    w, gs, f, g_con, g_gs = cases.case(8, 32, 2, 2)
    fw = host.tail_forward(w, gs, f)
    own, given = host.tail_grad(w, gs, f, g_con, g_gs), host.tail_grad(w, gs, f, g_con, g_gs, acts=fw)
    assert sorted(own) == sorted(given)
    for n in own:
        np.testing.assert_allclose(given[n], own[n], rtol=0, atol=1e-13 * max(1e-300, np.abs(own[n]).max()), err_msg=n)


def test_an_activation_of_exactly_zero_takes_the_slope():
    """TensorFlow's LeakyReluGrad passes the gradient where the feature is > 0: planted zeros in a1 (of either sign) take 0.3."""
    w, gs, f, g_con, g_gs = cases.case(8, 32, 1, 3)
    fw = host.tail_forward(w, gs, f)
    a1 = fw["a1"].copy()
    planted = np.zeros(a1.shape, bool)
    planted[0, ::2, ::3, ::5] = True
    a1[planted] = np.where(np.arange(planted.sum()) % 2 == 0, 0.0, -0.0)
    res = host.tail_grad(w, gs, f, g_con, g_gs, acts={"a1": a1, "a2": fw["a2"]})
    _, inv2, _, _, _ = host.bn_vectors(w, "clr_conv2")
    pre = (res["gz2"] * inv2) @ np.asarray(w["clr_conv2/conv/kernel"], np.float64)[0, 0].T
    assert np.abs(pre[planted]).min() > 0
    np.testing.assert_array_equal(res["gz1"][planted], 0.3 * pre[planted])
    pos = a1 > 0
    np.testing.assert_array_equal(res["gz1"][pos], pre[pos])


@pytest.mark.parametrize("H,W,B,FD_STEP", ((8, 32, 1, 1e-7),))
def test_central_finite_differences(H, W, B, FD_STEP):
    """On a segment along which no LeakyReLU mask changes (asserted for the five points used: a condition on the seed and the step, not a
    tolerance) the objective <G, con_rgb> is a polynomial p(t) in the step: every variable and input enters linearly or as a product
    with those of the layers above.  The central quotient q(e) = (p(e) - p(-e)) / 2e is p'(0) + c3 e^2 + ..., so |q(2e) - q(e)| = 3 |c3|
    e^2 + O(e^4) bounds the truncation of q(e) with a factor 3 to spare, as the discriminators' weight-gradient test bounds its own.  The
    evaluations run in numpy's extended precision (u = 2^-64): a value is formed by fewer than 9 * 65 + 16 + 16 + 3 * 8 = 641 operations a
    path, so its error is below 700 u A with A = sum |G| (|a2| |K3| + |b3|) the value's absolute mass, and the quotient's below that
    over e.  <grad, d> is summed in extended precision from tail_grad's float64 gradient; its own rounding is below 1e-11 of sum |grad d|.
    Two random directions in variable space and one in (gs, f)."""
    u = float(np.finfo(LD).eps) / 2
    w, gs, f, g_con, _ = cases.case(H, W, B, 4)
    res = host.tail_grad(w, gs, f, g_con)
    fw = host.tail_forward(w, gs, f)
    A = float((np.abs(g_con.astype(np.float64)) * (np.abs(fw["a2"]) @ np.abs(w["clr_conv3/conv/kernel"].astype(np.float64))[0, 0]
                                                   + np.abs(w["clr_conv3/conv/bias"].astype(np.float64)))).sum())
    rng = np.random.default_rng(11)
    names = list(cases.NAMES)
    directions = [{n: rng.standard_normal(w[n].shape) * np.abs(w[n]).max() for n in names} for _ in range(2)]
    directions.append({"gs": rng.standard_normal(gs.shape) * np.abs(gs).max(), "f": rng.standard_normal(f.shape) * np.abs(f).max()})
    for j, d in enumerate(directions):
        def at(t):
            moved = {n: np.asarray(v, LD) + (LD(t) * LD(FD_STEP) * d[n].astype(LD) if n in d else LD(0)) for n, v in w.items()}
            g2, f2 = (np.asarray(v, LD) + (LD(t) * LD(FD_STEP) * d[n].astype(LD) if n in d else LD(0)) for n, v in (("gs", gs), ("f", f)))
            masks = []
            return host.objective_f64(moved, g2, f2, g_con, masks=masks, dtype=LD), masks

        values = {t: at(t) for t in (-2, -1, 0, 1, 2)}
        for t in (-2, -1, 1, 2):
            for a, b in zip(values[t][1], values[0][1]):
                assert (a == b).all(), "a LeakyReLU mask differs between the evaluation points"
        q1 = (values[1][0] - values[-1][0]) / (2 * LD(FD_STEP))
        q2 = (values[2][0] - values[-2][0]) / (4 * LD(FD_STEP))
        key = {"gs": "d_gs", "f": "d_f"}
        want = sum((res[key.get(n, n)].astype(LD) * d[n].astype(LD)).sum() for n in d)
        mass = float(sum(np.abs(res[key.get(n, n)] * d[n]).sum() for n in d))
        bound = abs(float(q2 - q1)) + 700 * u * A / FD_STEP + 1e-11 * mass
        print("colour tail grad direction %d: quotient %.12g, <grad, d> %.12g, |difference| %.3g, bound %.3g (|q(2e) - q(e)| %.3g), sum |grad d| %.3g"
              % (j, float(q1), float(want), abs(float(q1 - want)), bound, abs(float(q2 - q1)), mass))
        assert mass > 100 * bound, "the bound must mean something beside the terms of the derivative"
        assert abs(float(q1 - want)) <= bound


def test_pack_against_its_unpack():
    w = init_weights(4)
    blob = pack.pack_clr_tail_grad(w)
    layout, total = pack.clr_tail_grad_layout()
    assert len(blob) == total * 4 == 30080 * 4
    assert all(off % 4 == 0 for _, off, _ in layout)                      # every record is read with 16-byte loads
    back = pack.unpack_clr_tail_grad(blob)
    k1 = w["clr_conv1/conv/kernel"]
    np.testing.assert_array_equal(back["k1"].reshape(3, 3, 65, 16), k1)
    np.testing.assert_array_equal(back["k2"], w["clr_conv2/conv/kernel"][0, 0])
    np.testing.assert_array_equal(back["tail/k3"][:, :3], w["clr_conv3/conv/kernel"][0, 0])
    assert not back["tail/k3"][:, 3].any()
    for i, stem in ((1, "clr_conv1"), (2, "clr_conv2")):
        rstd = 1.0 / np.sqrt(w[stem + "/bnorm/moving_variance"].astype(np.float64) + BN_EPS)
        vecs = back["vecs%d" % i]
        np.testing.assert_array_equal(vecs[0], w[stem + "/conv/bias"])
        np.testing.assert_array_equal(vecs[1], (w[stem + "/bnorm/gamma"].astype(np.float64) * rstd).astype(f32))
        np.testing.assert_array_equal(vecs[2], w[stem + "/bnorm/moving_mean"])
        np.testing.assert_array_equal(vecs[3], rstd.astype(f32))
    _, inv1, mean1, _, beta1 = host.bn_vectors(w, "clr_conv1")
    folded = (k1.astype(np.float64) * inv1)
    np.testing.assert_array_equal(back["dgrad/w"].reshape(3, 3, 64, 16), folded[::-1, ::-1, 1:].astype(f32))
    np.testing.assert_array_equal(back["dgrad/gs"].reshape(3, 3, 16), folded[::-1, ::-1, 0].astype(f32))
    # the forward images are the generator blob's own
    mats = pack.layer_matrices(w)
    fw, fb = pack.pack_taps(*mats["clr_conv1"], 32, 64, 16)
    np.testing.assert_array_equal(back["fwd/w"], fw)
    np.testing.assert_array_equal(back["fwd/bias"], fb)
    np.testing.assert_array_equal(back["fwd/gs"], pack.clr_gs_weights(w))
    np.testing.assert_array_equal(np.concatenate([back["tail/k2f"].reshape(-1), back["tail/b2f"]]), pack.tail_weights(w)[:272])
    with pytest.raises(ValueError, match="colour tail gradient blob"):
        pack.unpack_clr_tail_grad(blob[:-4])


def test_trainable_names_against_the_inventory():
    names = generator_tail_trainable_names()
    shapes = generator_variable_shapes()
    assert names == ["clr_conv1/conv/kernel", "clr_conv1/conv/bias", "clr_conv1/bnorm/gamma", "clr_conv1/bnorm/beta",
                     "clr_conv2/conv/kernel", "clr_conv2/conv/bias", "clr_conv2/bnorm/gamma", "clr_conv2/bnorm/beta",
                     "clr_conv3/conv/kernel", "clr_conv3/conv/bias"]
    assert [shapes[n] for n in names[::4]] == [(3, 3, 65, 16), (1, 1, 16, 16), (1, 1, 16, 3)]
    assert sum(int(np.prod(shapes[n])) for n in names) == 9763
    with open(os.path.join(GOLDEN, "gsc_ckpt94_inventory.json")) as fh:
        inventory = json.load(fh)["gsc"]["variables"]
    for n in names:
        assert tuple(inventory[n]) == shapes[n], n
