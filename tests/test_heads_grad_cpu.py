"""The host statement of the backward of the generator's grey heads (blindshadowremoval_amd/generator_grad.py: heads_grad) against torch
autograd in float64, on the closed forms of heads_grad_cases and against central finite differences of the objective <d_gs, gs> in
extended precision; pack.pack_heads_grad against its un-pack and the statement, and weights.generator_heads_trainable_names against
the checkpoint inventory."""
import json
import os

import numpy as np
import pytest

from blindshadowremoval_amd import generator_grad as host
from blindshadowremoval_amd import pack
from blindshadowremoval_amd.weights import generator_heads_trainable_names, generator_variable_shapes, init_weights

import heads_grad_cases as cases

f32 = np.float32
LD = np.longdouble
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def host_run(weights, inputs, y, d_gs):
    """The float64 statement on the mask as the float32 forward rounds it, which is what the device chain is handed (b2 = 20 saturates
    tanh to exactly 1 in float32; in float64 it stays a few 1e-15 short)."""
    mask = host.heads_forward(weights, inputs, y)["mask"].astype(f32)
    out = host.heads_grad(weights, inputs, y, d_gs, acts={"mask": mask})
    out["dtype"] = np.float64
    return out


@pytest.mark.parametrize("check", cases.CONSTRUCTED, ids=lambda c: c.__name__)
def test_constructed_case(check):
    check(host_run)


def test_constructed_cases_in_float32():
    """dtype=np.float32 runs the same arithmetic in float32: the closed forms hold there as well."""
    def run(weights, inputs, y, d_gs):
        out = host.heads_grad(weights, inputs, y, d_gs, dtype=f32)
        assert all(out[n].dtype == f32 for n in cases.OUTPUTS + ("g_m", "g_con", "mask"))
        out["dtype"] = f32
        return out
    for check in cases.CONSTRUCTED:
        check(run)


@pytest.mark.parametrize("H,W,B", cases.AUTOGRAD_SIZES)
def test_statement_matches_torch_autograd_in_float64(H, W, B):
    wt, inputs, y, d_gs = cases.case(H, W, B, 1)
    res = host.heads_grad(wt, inputs, y, d_gs)
    ref = cases.autograd_grads(wt, inputs, y, d_gs)
    d, at = cases.worst_scaled_diff(res, ref)
    print("heads grad H=%d W=%d B=%d: statement against torch autograd, worst scaled difference %.3g at %s (bound %.3g)"
          % (H, W, B, d, at, cases.AUTOGRAD_BOUND))
    assert d <= cases.AUTOGRAD_BOUND
    assert (ref["m"] > 0).any() and (ref["m"] < 0).any()                  # both signs of the mask head's pre-activation
    shapes = generator_variable_shapes()
    for name in cases.NAMES:
        assert res[name].shape == shapes[name] and res[name].dtype == np.float64 and np.abs(res[name]).max() > 0, name
    assert res["d_y"].shape == (B, H, W, 64)
    for name in ("g_m", "g_con", "mask"):
        assert res[name].shape == (B, H, W, 1), name
    fw = host.heads_forward(wt, inputs, y)
    assert sorted(fw) == ["con", "gray", "gs", "m", "mask"] and all(v.shape == (B, H, W, 1) for v in fw.values())
    np.testing.assert_allclose(fw["m"], ref["m"], rtol=0, atol=1e-13 * np.abs(ref["m"]).max())


def test_acts_given_are_those_of_the_own_forward():
    wt, inputs, y, d_gs = cases.case(5, 3, 2, 2)
    own = host.heads_grad(wt, inputs, y, d_gs)
    given = host.heads_grad(wt, inputs, y, d_gs, acts={"mask": host.heads_forward(wt, inputs, y)["mask"]})
    assert sorted(own) == sorted(given)
    for n in own:
        np.testing.assert_array_equal(given[n], own[n], err_msg=n)
    other = host.heads_grad(wt, inputs, y, d_gs, acts={"mask": np.zeros((2, 5, 3, 1), f32)})
    np.testing.assert_array_equal(other["g_m"], d_gs.astype(np.float64) * host.heads_forward(wt, inputs, y)["gray"])      # the given mask is used
    low = host.heads_grad(wt, inputs, y, d_gs, dtype=f32)
    assert all(low[n].dtype == f32 for n in cases.OUTPUTS)
    assert cases.worst_scaled_diff(low, own)[0] <= 1e-4


def test_the_odd_k_forms_are_the_3x3_ones_at_k_3():
    rng = np.random.default_rng(3)
    x, k, gy = rng.standard_normal((2, 4, 5, 3)), rng.standard_normal((3, 3, 3, 2)), rng.standard_normal((2, 4, 5, 2))
    np.testing.assert_array_equal(host.convk_same(x, k), host.conv3x3_same(x, k))
    np.testing.assert_array_equal(host.convk_same_wgrad(x, gy, 3), host.conv3x3_same_wgrad(x, gy))
    np.testing.assert_array_equal(host.convk_same_dgrad(gy, k), host.conv3x3_same_dgrad(gy, k))


def test_central_finite_differences(H=5, W=6, B=2, FD_STEP=1e-5):
    """The objective <d_gs, gs> is a smooth function p(t) of a step along any direction (tanh; no mask).  The central quotient
    q(e) = (p(e) - p(-e)) / 2e is p'(0) + c3 e^2 + O(e^4), so |q(2e) - q(e)| = 3 |c3| e^2 + O(e^4) bounds the truncation of q(e) with a
    factor 3 to spare, as the colour tail's test bounds its own.  The evaluations run in numpy's extended precision (u = 2^-64).  m and
    con are each formed by fewer than 2 x 49 x 64 + 2 < 6300 operations, so their errors are below 6300 u times their absolute masses
    M_m, M_con (the same sums on |y|, |K|, |b|); tanh has slope at most 1 and is taken to a few u, so gs carries at most
    |gray| (6300 u M_m + 8 u) + 6300 u M_con + 8 u |gs|.  The objective's error is below 6400 u A with
    A = sum |d_gs| (|gray| (2 + M_m) + M_con), the quotient's below that over e.  <grad, d> is summed in extended precision from
    heads_grad's float64 gradient; its own rounding is below 1e-11 of sum |grad d|.  Two random directions in variable space and one
    in y."""
    u = float(np.finfo(LD).eps) / 2
    wt, inputs, y, d_gs = cases.case(H, W, B, 4)
    res = host.heads_grad(wt, inputs, y, d_gs)
    fw = host.heads_forward(wt, inputs, y)
    ay = np.abs(y.astype(np.float64))
    M_m = host.convk_same(ay, np.abs(wt[cases.K2].astype(np.float64))) + np.abs(wt[cases.B2].astype(np.float64))
    M_con = host.convk_same(ay, np.abs(wt[cases.K3].astype(np.float64))) + np.abs(wt[cases.B3].astype(np.float64))
    A = float((np.abs(d_gs.astype(np.float64)) * (np.abs(fw["gray"]) * (2 + M_m) + M_con)).sum())
    rng = np.random.default_rng(13)
    directions = [{n: rng.standard_normal(wt[n].shape) * np.abs(wt[n]).max() for n in cases.NAMES} for _ in range(2)]
    directions.append({"y": rng.standard_normal(y.shape) * np.abs(y).max()})
    for j, d in enumerate(directions):
        def at(t):
            moved = {n: np.asarray(wt[n], LD) + (LD(t) * LD(FD_STEP) * d[n].astype(LD) if n in d else LD(0)) for n in cases.NAMES}
            y2 = np.asarray(y, LD) + (LD(t) * LD(FD_STEP) * d["y"].astype(LD) if "y" in d else LD(0))
            return host.heads_objective_f64(moved, inputs, y2, d_gs, dtype=LD)

        values = {t: at(t) for t in (-2, -1, 1, 2)}
        assert values[1].dtype == LD
        q1 = (values[1] - values[-1]) / (2 * LD(FD_STEP))
        q2 = (values[2] - values[-2]) / (4 * LD(FD_STEP))
        key = {"y": "d_y"}
        want = sum((res[key.get(n, n)].astype(LD) * d[n].astype(LD)).sum() for n in d)
        mass = float(sum(np.abs(res[key.get(n, n)] * d[n]).sum() for n in d))
        bound = abs(float(q2 - q1)) + 6400 * u * A / FD_STEP + 1e-11 * mass
        print("heads grad direction %d: quotient %.12g, <grad, d> %.12g, |difference| %.3g, bound %.3g (|q(2e) - q(e)| %.3g), sum |grad d| %.3g"
              % (j, float(q1), float(want), abs(float(q1 - want)), bound, abs(float(q2 - q1)), mass))
        assert mass > 100 * bound, "the bound must mean something beside the terms of the derivative"
        assert abs(float(q1 - want)) <= bound


def test_pack_against_its_unpack_and_the_statement():
    wt = init_weights(4)
    blob = pack.pack_heads_grad(wt)
    layout, total = pack.heads_grad_layout()
    assert layout == [("kt", 0, (100, 64))] and len(blob) == total * 4 == 100 * 64 * 4
    back = pack.unpack_heads_grad(blob)
    assert sorted(back) == ["conv2/conv/kernel", "conv3/conv/kernel", "kt"]
    np.testing.assert_array_equal(back["kt"], pack.heads_grad_record(wt)["kt"])
    np.testing.assert_array_equal(back[cases.K2], wt[cases.K2])
    np.testing.assert_array_equal(back[cases.K3], wt[cases.K3])
    assert not back["kt"][98:].any()
    for a in range(7):
        for b in range(7):
            np.testing.assert_array_equal(back["kt"][2 * (7 * a + b)], wt[cases.K2][a, b, :, 0])
            np.testing.assert_array_equal(back["kt"][2 * (7 * a + b) + 1], wt[cases.K3][a, b, :, 0])
    # the image reproduces the statement's data gradient: d_y[p] = sum_k g2[p - (a - 3, b - 3)][j] kt[k], zero outside the image
    _, inputs, y, d_gs = cases.case(9, 7, 2, 6)
    st = host.heads_grad(wt, inputs, y, d_gs)
    g2 = np.concatenate([st["g_m"], st["g_con"]], axis=3)
    gp = np.zeros((2, 9 + 6, 7 + 6, 2))
    gp[:, 3:12, 3:10] = g2
    kt = back["kt"].astype(np.float64)
    d_y = np.zeros((2, 9, 7, 64))
    for k in range(98):
        a, b, j = (k // 2) // 7, (k // 2) % 7, k % 2
        d_y += gp[:, 6 - a:6 - a + 9, 6 - b:6 - b + 7, j:j + 1] * kt[k]
    assert np.abs(d_y - st["d_y"]).max() <= 1e-13 * np.abs(st["d_y"]).max()
    with pytest.raises(ValueError, match="heads gradient blob"):
        pack.unpack_heads_grad(blob[:-4])
    assert pack.pack_heads_grad(init_weights(4, variant="tsm")) == pack.pack_heads_grad({n: init_weights(4, variant="tsm")[n] for n in cases.NAMES})
    for fn in (pack.pack_heads_grad, pack.heads_grad_record):
        with pytest.raises(ValueError) as e:
            fn(init_weights(4, variant="rgb"))
        assert str(e.value) == pack.HEADS_RGB_TEXT


def test_trainable_names_against_the_inventory():
    names = generator_heads_trainable_names()
    shapes = generator_variable_shapes()
    assert names == ["conv2/conv/kernel", "conv2/conv/bias", "conv3/conv/kernel", "conv3/conv/bias"]
    assert [n for n in shapes if n in names] == names                      # generator_variable_shapes' order
    assert tuple(names) == host.HEADS_NORM_NAMES[1:] and host.HEADS_NORM_NAMES[0] == "d_y"
    assert sum(int(np.prod(shapes[n])) for n in names) == 6274
    assert generator_heads_trainable_names("tsm") == names
    with open(os.path.join(GOLDEN, "gsc_ckpt94_inventory.json")) as fh:
        inventory = json.load(fh)["gsc"]["variables"]
    for n in names:
        assert tuple(inventory[n]) == shapes[n], n
    norms = host.heads_norms({n: np.full(shapes.get(n, (1, 2, 4, 64)), -2.0) for n in host.HEADS_NORM_NAMES})
    assert tuple(norms) == host.HEADS_NORM_NAMES and norms["conv2/conv/kernel"] == (2.0 * 3136, 2.0) and norms["d_y"] == (1024.0, 2.0)


def test_example_inputs():
    inputs, y, d_gs = host.heads_example_inputs(8, 32, 2, 0)
    assert inputs.shape == (2, 8, 32, 3) and y.shape == (2, 8, 32, 64) and d_gs.shape == (2, 8, 32, 1)
    assert all(a.dtype == f32 for a in (inputs, y, d_gs))
    assert 0 <= inputs.min() and inputs.max() <= 1 and (y < 0).any() and -y.min() < 0.5 * y.max()
    assert 0.1 < np.abs(d_gs).mean() * 2 * 8 * 32 < 10
