"""The host statement of the backward of res_stack/4, res_stack/3 and the hole (blindshadowremoval_amd/generator_grad.py:
colour_trunk_grad, hole_grad) against torch autograd in float64, on the constructed cases of colour_trunk_grad_cases, and against central
differences of colour_trunk_objective_f64 in extended precision."""
import numpy as np
import pytest

from blindshadowremoval_amd import generator_grad as host
from blindshadowremoval_amd.weights import generator_variable_shapes

import colour_trunk_grad_cases as cases

f32 = np.float32
LD = np.longdouble


@pytest.mark.parametrize("check", cases.CONSTRUCTED, ids=lambda c: c.__name__)
def test_constructed_case(check):
    check(cases.host_run)


@pytest.mark.parametrize("h,w,B", cases.AUTOGRAD_SIZES)
def test_statement_matches_torch_autograd_in_float64(h, w, B):
    wt, x, bmask, uv, d_xin, d_x = cases.case(h, w, B, 1)     # asserts both signs in every activation and the hole's share
    res = cases.host_run(wt, x, bmask, uv, d_xin, d_x)
    d, at = cases.worst_scaled_diff(res, cases.autograd_grads(wt, x, bmask, uv, d_xin, d_x))
    print("colour trunk grad h=%d w=%d B=%d: statement against torch autograd, worst scaled difference %.3g at %s (bound %.3g)"
          % (h, w, B, d, at, cases.AUTOGRAD_BOUND))
    assert d <= cases.AUTOGRAD_BOUND, (d, at)
    shapes = generator_variable_shapes()
    assert len(cases.NAMES) == 44 and sum(int(np.prod(shapes[n])) for n in cases.NAMES) == 696076
    for name in cases.NAMES:
        assert res[name].shape == shapes[name] and res[name].dtype == np.float64 and np.abs(res[name]).max() > 0, name
    assert res["d_res2"].shape == (B, h, w, 257)
    for b in (3, 4):
        assert res["d_y3_%d" % b].shape == (B, h, w, 257) and res["d_skip_%d" % b].shape == res["d_xin%d" % b].shape == (B, h, w, 261)
        assert res["a1_%d" % b].shape == res["a2_%d" % b].shape == (B, h, w, 128)
    # without d_x the gradient at res_stack/2's output is the colour branch's share alone
    none = cases.host_run(wt, x, bmask, uv, d_xin, None)
    d, at = cases.worst_scaled_diff(none, cases.autograd_grads(wt, x, bmask, uv, d_xin))
    assert d <= cases.AUTOGRAD_BOUND, (d, at)
    assert tuple(host.colour_trunk_norms(res)) == host.COLOUR_TRUNK_NORM_NAMES == ("d_res2",) + cases.NAMES


def test_trunk_forward_and_the_example_inputs():
    wt = cases.ct_weights()
    x, bmask, uv, d_xin, d_x, xh, y3_3, res3, y3_4, res4 = host.colour_trunk_example_inputs(2, 4, 2, 3, weights=wt)
    again = host.colour_trunk_example_inputs(2, 4, 2, 3)
    for a, b in zip((x, bmask, uv, d_xin, d_x), again):
        assert a.dtype == f32 and a.tobytes() == b.tobytes()
    assert x.shape == d_x.shape == (2, 2, 4, 257) and bmask.shape == (2, 2, 4, 1) and uv.shape == (2, 2, 4, 3) and d_xin.shape == (2, 2, 4, 261)
    assert set(np.unique(bmask)) <= {0.0, 1.0} and (x < 0).any() and (x > 0).any()
    fw = host.trunk_forward(wt, x, bmask, uv)
    assert sorted(fw) == sorted(["xh"] + [k % b for b in (3, 4) for k in ("y3_%d", "res%d", "a1_%d", "a2_%d", "pre_%d")])
    np.testing.assert_array_equal(fw["xh"], np.concatenate([x * (1 - bmask), bmask, uv], axis=3).astype(np.float64))
    for k, t in (("xh", xh), ("y3_3", y3_3), ("res3", res3), ("y3_4", y3_4), ("res4", res4)):
        assert t.dtype == f32 and t.tobytes() == fw[k].astype(f32).tobytes(), k
    # it is the existing statements with block=: block 3 on xh, block 4 on res3
    b3 = host.bottleneck_forward(wt, fw["xh"], block=3)
    np.testing.assert_array_equal(fw["y3_3"], b3["y3"])
    np.testing.assert_array_equal(fw["res3"], host.nonlocal_forward(wt, b3["y3"], fw["xh"], block=3)["out"])
    b4 = host.bottleneck_forward(wt, fw["res3"], block=4)
    np.testing.assert_array_equal(fw["res4"], host.nonlocal_forward(wt, b4["y3"], fw["res3"], block=4)["out"])


def test_acts_given_are_those_of_the_own_forward():
    wt, x, bmask, uv, d_xin, d_x = cases.case(2, 4, 2, 2)
    fw = host.trunk_forward(wt, x, bmask, uv)
    feeds = (fw["xh"], fw["y3_3"], fw["res3"], fw["y3_4"], fw["res4"], d_xin, d_x)
    own = host.colour_trunk_grad(wt, *feeds)
    given = host.colour_trunk_grad(wt, *feeds, acts={k: fw[k] for k in ("a1_3", "a2_3", "a1_4", "a2_4")})
    assert sorted(own) == sorted(given)
    for n in own:
        np.testing.assert_array_equal(given[n], own[n], err_msg=n)


def test_hole_grad_in_float32_is_the_float64_statement_rounded_at_most_once():
    wt, x, bmask, uv, d_xin, d_x = cases.case(3, 4, 3, 3)
    xh = host.trunk_forward(wt, x, bmask, uv)["xh"].astype(f32)
    d_xin3 = d_xin                                             # any float32 [B,h,w,261] serves as the gradient at xh
    low, high = host.hole_grad(xh, d_xin3, dtype=f32), host.hole_grad(xh, d_xin3)
    assert low.dtype == f32 and high.dtype == np.float64 and low.shape == high.shape == (3, 3, 4, 257)
    np.testing.assert_array_equal(low.astype(np.float64), high)           # no d_x: a product with 0 or 1, exact
    inside = bmask[..., 0] == 1
    assert inside.any() and not inside.all() and not low[inside].any()
    assert low[~inside].tobytes() == d_xin3[..., :257][~inside].tobytes()
    low, high = host.hole_grad(xh, d_xin3, d_x, dtype=f32), host.hole_grad(xh, d_xin3, d_x)
    assert low.tobytes() == high.astype(f32).tobytes()                    # with d_x: the one float32 addition, rounded to nearest
    assert low[inside].tobytes() == d_x[inside].tobytes()
    moved = d_xin3.copy()
    moved[..., 257:] += f32(1.0)                                          # bmask's and uv's channels of d_xin3 reach nothing
    assert host.hole_grad(xh, moved, d_x, dtype=f32).tobytes() == low.tobytes()


def test_central_finite_differences(h=2, w=4, B=1, FD_STEP=1e-7):
    """Single entries of x and of variables of both blocks, on segments along which none of the six LeakyReLU masks changes (asserted for
    the five points used: a condition on the seed and the step, not a tolerance).  There the objective <d_xin, res4> + <d_x, x> is a
    smooth function p(t) of the step; the central quotient q(e) = (p(e) - p(-e)) / 2e is p'(0) + c3 e^2 + O(e^4), so |q(2e) - q(e)| = 3
    |c3| e^2 + O(e^4) bounds the truncation of q(e) with a factor 3 to spare, as the bottleneck's test bounds its own.  The evaluations
    run in numpy's extended precision (u = 2^-64); a value of res4 is reached through fewer than 1e4 operations, so p carries an error of
    1e4 u |p| at most as long as no cancellation inside it is worse than p's own, and the quotient that over e: the allowance beside the
    truncation term.  The two together are asserted to lie below a thousandth of the derivative."""
    u = float(np.finfo(LD).eps) / 2
    wt, x, bmask, uv, d_xin, d_x = cases.case(h, w, B, 4)
    res = cases.host_run(wt, x, bmask, uv, d_xin, d_x)
    open_pixel = tuple(int(i) for i in np.argwhere(bmask[..., 0] == 0)[0])
    entries = [("x", open_pixel + (5,)), ("res_stack/3/conv2/kernel", (1, 1, 3, 7)), ("res_stack/3/bnorm1/gamma", (4,)),
               ("res_stack/3/non_local/theta/kernel", (0, 0, 10, 3)), ("res_stack/4/conv1/kernel", (0, 0, 258, 2)),
               ("res_stack/4/non_local/w/bias", (9,)), ("res_stack/4/bnorm3/beta", (100,))]
    trunk = {n: v for n, v in wt.items() if n.startswith(("res_stack/3/", "res_stack/4/"))}
    for name, index in entries:
        base = x if name == "x" else wt[name]
        step = LD(FD_STEP) * LD(float(np.abs(base).max()))

        def at(t):
            moved = {n: np.asarray(v, LD) for n, v in trunk.items()}
            x2 = np.asarray(x, LD).copy()
            target = x2 if name == "x" else moved[name].copy()
            target[index] += LD(t) * step
            if name != "x":
                moved[name] = target
            masks = []
            return host.colour_trunk_objective_f64(moved, x2, bmask, uv, d_xin, d_x, masks=masks, dtype=LD), masks

        values = {t: at(t) for t in (-2, -1, 0, 1, 2)}
        assert values[0][0].dtype == LD
        for t in (-2, -1, 1, 2):
            assert len(values[t][1]) == 6
            for a, b in zip(values[t][1], values[0][1]):
                assert (a == b).all(), "a LeakyReLU's mask differs between the evaluation points"
        q1 = (values[1][0] - values[-1][0]) / (2 * step)
        q2 = (values[2][0] - values[-2][0]) / (4 * step)
        want = LD(res["d_res2" if name == "x" else name][index])
        rounding = 1e4 * u * abs(float(values[0][0])) / float(step)
        bound = abs(float(q2 - q1)) + rounding
        print("colour trunk grad %s%s: quotient %.12g, gradient %.12g, |difference| %.3g, bound %.3g (|q(2e) - q(e)| %.3g, rounding %.3g)"
              % (name, list(index), float(q1), float(want), abs(float(q1 - want)), bound, abs(float(q2 - q1)), rounding))
        assert abs(float(want)) > 1e3 * bound, "the bound must mean something beside the derivative"
        assert abs(float(q1 - want)) <= bound
