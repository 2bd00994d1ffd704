"""The host statement of the backward of res_stack/5's upper half (blindshadowremoval_amd/generator_grad.py: nonlocal_grad) against torch
autograd in float64, on the closed forms of nonlocal_grad_cases, against central finite differences of the objective <d_out, out> in
extended precision and on a hard softmax; pack.pack_nonlocal_grad against its un-pack and weights.generator_nonlocal_trainable_names
against the checkpoint inventory."""
import json
import os

import numpy as np
import pytest

from blindshadowremoval_amd import generator_grad as host
from blindshadowremoval_amd import pack
from blindshadowremoval_amd.weights import BN_EPS, generator_nonlocal_trainable_names, generator_variable_shapes, init_weights

import nonlocal_grad_cases as cases

f32 = np.float32
LD = np.longdouble
ST = cases.ST
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def host_run(weights, y3, xin, d_out, acts):
    out = host.nonlocal_grad(weights, y3, xin, d_out, acts=acts)
    out["dtype"] = np.float64
    out["y3"] = y3
    return out


def autograd_bound():
    """min(4 x the largest figure tools/make_nonlocal_grad_fixture.py measured when it wrote the fixture (`measured`), 1e-9)."""
    measured = float(np.load(os.path.join(GOLDEN, "nonlocal_grad_%dx%d.npz" % cases.FIXTURE[:2]))["measured"])
    assert abs(measured - cases.AUTOGRAD_MEASURED) <= 0.05e-15
    return min(4 * measured, cases.AUTOGRAD_CAP)


@pytest.mark.parametrize("check", cases.CONSTRUCTED, ids=lambda c: c.__name__)
def test_constructed_case(check):
    check(host_run)


@pytest.mark.parametrize("h,w,B", cases.AUTOGRAD_SIZES)
def test_statement_matches_torch_autograd_in_float64(h, w, B):
    wt, y3, xin, d_out = cases.case(h, w, B, 1)             # asserts both signs of pad(z) + xin
    res = host.nonlocal_grad(wt, y3, xin, d_out)
    d, at = cases.worst_scaled_diff(res, cases.autograd_grads(wt, y3, xin, d_out))
    print("non-local grad h=%d w=%d B=%d: statement against torch autograd, worst scaled difference %.3g at %s (bound %.3g)"
          % (h, w, B, d, at, autograd_bound()))
    assert d <= autograd_bound()
    shapes = generator_variable_shapes()
    for name in cases.NAMES:
        assert res[name].shape == shapes[name] and res[name].dtype == np.float64, name
        assert name == cases.PHI_BIAS or np.abs(res[name]).max() > 0, name
    T = h * w
    assert res["d_y3"].shape == (B, h, w, 257) and res["d_skip"].shape == res["gz"].shape == res["out"].shape == (B, h, w, 261)
    for name in ("dA", "d_theta", "d_phi", "d_g", "A"):
        assert res[name].shape == (B, T, 128), name
    assert res["D"].shape == (B, T)
    fw = host.nonlocal_forward(wt, y3, xin)
    assert all(k in fw for k in ("theta", "phi", "g", "A", "c", "z", "out"))


def test_the_statement_is_width_agnostic():
    """TSM's 877 input channels: the same statement against autograd, C read from xin."""
    wt, y3, xin, d_out = cases.case(1, 4, 1, 2, C=877)
    assert wt["res_stack/5/conv1/kernel"].shape == (1, 1, 877, 128) and xin.shape == (1, 1, 4, 877)
    res = host.nonlocal_grad(wt, y3, xin, d_out)
    d, at = cases.worst_scaled_diff(res, cases.autograd_grads(wt, y3, xin, d_out))
    assert res["d_skip"].shape == (1, 1, 4, 877) and d <= autograd_bound(), (d, at)
    with pytest.raises(ValueError) as e:
        pack.pack_nonlocal_grad(wt)
    assert str(e.value) == pack.NONLOCAL_TSM_TEXT


def test_acts_given_are_those_of_the_own_forward():
    wt, y3, xin, d_out = cases.case(2, 4, 2, 2)
    fw = host.nonlocal_forward(wt, y3, xin)
    own = host.nonlocal_grad(wt, y3, xin, d_out)
    for acts in ({"out": fw["out"]}, {"out": fw["out"], "A": fw["A"]}):
        given = host.nonlocal_grad(wt, y3, xin, d_out, acts=acts)
        assert sorted(own) == sorted(given)
        for n in own:
            np.testing.assert_array_equal(given[n], own[n], err_msg=n)


def test_central_finite_differences(h=1, w=4, B=1, FD_STEP=1e-7):
    """On a segment along which relu3's mask does not change (asserted for the five points used: a condition on the seed and the step, not
    a tolerance) the objective <d_out, out> is a smooth function p(t) of the step.  The central quotient q(e) = (p(e) - p(-e)) / 2e is
    p'(0) + c3 e^2 + O(e^4), so |q(2e) - q(e)| = 3 |c3| e^2 + O(e^4) bounds the truncation of q(e) with a factor 3 to spare, as the colour
    tail's test bounds its own.  The evaluations run in numpy's extended precision (u = 2^-64).  A value of out is formed by fewer than
    2 (257 + 128 + T + T + 128) + 40 < 1200 operations a path (T = 4), so its error is below 1200 u times its absolute mass: the same
    forward on |X|, |W|, |b|, where the softmax — whose weights carry the ABSOLUTE error of S as a relative one, at most 2 max(mass S)
    between numerator and denominator — enters as (1 + 2 max mass(S)) P mass(g), the BatchNormalization as |inv| (c + |mean|) + |beta|
    and the LeakyReLU as the identity.  The objective's error is below 1200 u A with A = sum |d_out| mass(out), the quotient's below that
    over e.  <grad, d> is summed in extended precision from nonlocal_grad's float64 gradient; its own rounding is below 1e-11 of
    sum |grad d|.  Two random directions in variable space and one in y3."""
    u = float(np.finfo(LD).eps) / 2
    wt, y3, xin, d_out = cases.case(h, w, B, 4)
    res = host.nonlocal_grad(wt, y3, xin, d_out)
    a64 = lambda n: np.abs(np.asarray(wt[ST + n], np.float64))                          # noqa: E731
    mX = np.abs(y3.astype(np.float64)).reshape(B, h * w, 257)
    m = {n: mX @ a64(n + "/kernel")[0, 0] + a64(n + "/bias") for n in ("theta", "phi", "g")}
    mS = m["theta"] @ np.transpose(m["phi"], (0, 2, 1))
    fw = host.nonlocal_forward(wt, y3, xin)
    mA = (1 + 2 * mS.max()) * (fw["P"] @ m["g"])
    bw, inv, mean, _, _, beta = host.nonlocal_bn_vectors(wt)
    mz = mX + np.abs(inv) * (mA @ a64("w/kernel")[0, 0] + np.abs(bw) + np.abs(mean)) + np.abs(beta)
    m_out = np.abs(xin.astype(np.float64))
    m_out[..., :257] += mz.reshape(B, h, w, 257)
    A = float((np.abs(d_out.astype(np.float64)) * m_out).sum())
    rng = np.random.default_rng(11)
    directions = [{n: rng.standard_normal(wt[n].shape) * np.abs(wt[n]).max() for n in cases.NAMES} for _ in range(2)]
    directions.append({"y3": rng.standard_normal(y3.shape) * np.abs(y3).max()})
    for j, d in enumerate(directions):
        def at(t):
            moved = {n: np.asarray(v, LD) + (LD(t) * LD(FD_STEP) * d[n].astype(LD) if n in d else LD(0)) for n, v in wt.items() if n.startswith(ST)}
            y2 = np.asarray(y3, LD) + (LD(t) * LD(FD_STEP) * d["y3"].astype(LD) if "y3" in d else LD(0))
            masks = []
            return host.nonlocal_objective_f64(moved, y2, xin, d_out, masks=masks, dtype=LD), masks

        values = {t: at(t) for t in (-2, -1, 0, 1, 2)}
        assert values[0][0].dtype == LD
        for t in (-2, -1, 1, 2):
            for a, b in zip(values[t][1], values[0][1]):
                assert (a == b).all(), "relu3's mask differs between the evaluation points"
        q1 = (values[1][0] - values[-1][0]) / (2 * LD(FD_STEP))
        q2 = (values[2][0] - values[-2][0]) / (4 * LD(FD_STEP))
        key = {"y3": "d_y3"}
        want = sum((res[key.get(n, n)].astype(LD) * d[n].astype(LD)).sum() for n in d)
        mass = float(sum(np.abs(res[key.get(n, n)] * d[n]).sum() for n in d))
        bound = abs(float(q2 - q1)) + 1200 * u * A / FD_STEP + 1e-11 * mass
        print("non-local grad direction %d: quotient %.12g, <grad, d> %.12g, |difference| %.3g, bound %.3g (|q(2e) - q(e)| %.3g), sum |grad d| %.3g"
              % (j, float(q1), float(want), abs(float(q1 - want)), bound, abs(float(q2 - q1)), mass))
        assert mass > 100 * bound, "the bound must mean something beside the terms of the derivative"
        assert abs(float(q1 - want)) <= bound


def test_hard_softmax():
    """max |S| > 200 with a near-one-hot and an ordinary row (asserted by hard_case): every output is finite, the statement still agrees
    with autograd, and the statement run in float32 throughout against float64 gives the figure the device's bound is taken from."""
    wt, y3, xin, d_out = cases.hard_case()
    res = host.nonlocal_grad(wt, y3, xin, d_out)
    for name in cases.OUTPUTS + host.NONLOCAL_MAPS:
        assert np.isfinite(res[name]).all(), name
    with np.errstate(over="ignore"):
        assert not np.isfinite(np.exp(np.asarray(host.nonlocal_forward(wt, y3, xin)["S"], f32))).all()     # the row maximum is needed
    d, at = cases.worst_scaled_diff(res, cases.autograd_grads(wt, y3, xin, d_out))
    print("non-local grad, hard softmax: statement against torch autograd, worst scaled difference %.3g at %s" % (d, at))
    assert d <= 1e-9
    low = host.nonlocal_grad(wt, y3, xin, d_out, dtype=f32)
    assert all(low[n].dtype == f32 for n in cases.OUTPUTS)
    e, at = cases.worst_scaled_diff(low, res)
    print("non-local grad, hard softmax: the statement in float32 against float64, worst scaled error %.4g at %s (recorded %.4g)"
          % (e, at, cases.HARD_F32_MEASURED))
    assert abs(e - cases.HARD_F32_MEASURED) <= 0.05 * cases.HARD_F32_MEASURED


def test_pack_against_its_unpack():
    wt = init_weights(4)
    blob = pack.pack_nonlocal_grad(wt)
    layout, total = pack.nonlocal_grad_layout()
    assert len(blob) == total * 4 == (272 * 384 + 384 + 272 * 128 + 384 * 384 + 128 * 257 + 4 * 257) * 4
    assert all(off % 4 == 0 for _, off, _ in layout)                      # every record is read with 16-byte loads
    back = pack.unpack_nonlocal_grad(blob)
    kt, kp, kg, kw = (wt[ST + n + "/kernel"][0, 0] for n in ("theta", "phi", "g", "w"))
    np.testing.assert_array_equal(back["wqkv"][:257], np.concatenate([kt, kp, kg], axis=1))
    assert not back["wqkv"][257:].any()
    np.testing.assert_array_equal(back["bqkv"], np.concatenate([wt[ST + n + "/bias"] for n in ("theta", "phi", "g")]))
    np.testing.assert_array_equal(back["wqkvT"][:, :272], back["wqkv"].T)
    assert not back["wqkvT"][:, 272:].any()
    rstd = 1.0 / np.sqrt(wt[ST + "bnorm/moving_variance"].astype(np.float64) + BN_EPS)
    inv = wt[ST + "bnorm/gamma"].astype(np.float64) * rstd
    np.testing.assert_array_equal(back["wwf"][:257], (kw.astype(np.float64) * inv[None, :]).T.astype(f32))      # formed in float64, rounded once
    assert not back["wwf"][257:].any()
    np.testing.assert_array_equal(back["ww"], kw)
    np.testing.assert_array_equal(back["vecs"][0], wt[ST + "w/bias"])
    np.testing.assert_array_equal(back["vecs"][1], inv.astype(f32))
    np.testing.assert_array_equal(back["vecs"][2], wt[ST + "bnorm/moving_mean"])
    np.testing.assert_array_equal(back["vecs"][3], rstd.astype(f32))
    with pytest.raises(ValueError, match="non-local gradient blob"):
        pack.unpack_nonlocal_grad(blob[:-4])


def test_trainable_names_against_the_inventory():
    names = generator_nonlocal_trainable_names()
    shapes = generator_variable_shapes()
    assert names == [ST + p for p in ("g/kernel", "g/bias", "phi/kernel", "phi/bias", "theta/kernel", "theta/bias", "w/kernel", "w/bias",
                                      "bnorm/gamma", "bnorm/beta")]
    assert tuple(names) == host.NONLOCAL_NORM_NAMES[2:] and host.NONLOCAL_NORM_NAMES[:2] == ("d_y3", "d_skip")
    assert sum(int(np.prod(shapes[n])) for n in names) == 132739
    assert generator_nonlocal_trainable_names(3)[0] == "res_stack/3/non_local/g/kernel"
    with open(os.path.join(GOLDEN, "gsc_ckpt94_inventory.json")) as fh:
        inventory = json.load(fh)["gsc"]["variables"]
    for n in names:
        assert tuple(inventory[n]) == shapes[n], n
    norms = host.nonlocal_norms({n: np.full(shapes.get(n, (1, 1, 4, 257)), -2.0) for n in host.NONLOCAL_NORM_NAMES})
    assert tuple(norms) == host.NONLOCAL_NORM_NAMES and norms[ST + "g/bias"] == (256.0, 2.0)
