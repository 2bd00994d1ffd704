"""The host statement of the backward of res_stack/2, res_stack/1 and res_stack/0 (blindshadowremoval_amd/generator_grad.py:
lower_trunk_grad, and nonlocal_forward / nonlocal_grad with a skip narrower than the block) against torch autograd in float64, on the
constructed cases of lower_trunk_grad_cases, and against central differences of lower_trunk_objective_f64 in extended precision."""
import numpy as np
import pytest

from blindshadowremoval_amd import generator_grad as host
from blindshadowremoval_amd.weights import generator_variable_shapes

import lower_trunk_grad_cases as cases

f32 = np.float32
LD = np.longdouble


@pytest.mark.parametrize("check", cases.CONSTRUCTED, ids=lambda c: c.__name__)
def test_constructed_case(check):
    check(cases.host_run)


@pytest.mark.parametrize("h,w,B", cases.AUTOGRAD_SIZES)
def test_statement_matches_torch_autograd_in_float64(h, w, B):
    wt, x0, d_res2 = cases.case(h, w, B, 1)     # asserts both signs in every activation
    res = cases.host_run(wt, x0, d_res2)
    d, at = cases.worst_scaled_diff(res, cases.autograd_grads(wt, x0, d_res2))
    print("lower trunk grad h=%d w=%d B=%d: statement against torch autograd, worst scaled difference %.3g at %s (bound %.3g)"
          % (h, w, B, d, at, cases.AUTOGRAD_BOUND))
    assert d <= cases.AUTOGRAD_BOUND, (d, at)
    shapes = generator_variable_shapes()
    per_block = [sum(int(np.prod(shapes[n])) for n in cases.NAMES if n.startswith("res_stack/%d/" % b)) for b in (0, 1, 2)]
    assert len(cases.NAMES) == 66 and per_block == [194563 + 132739, 214787 + 132739, 214787 + 132739] and sum(per_block) == 1022354
    for name in cases.NAMES:
        assert res[name].shape == shapes[name] and res[name].dtype == np.float64 and np.abs(res[name]).max() > 0, name
    assert shapes["res_stack/0/conv1/kernel"] == (1, 1, 99, 128) and shapes["res_stack/1/conv1/kernel"] == (1, 1, 257, 128)
    assert res["d_x0"].shape == res["d_skip_0"].shape == (B, h, w, 99) and np.abs(res["d_x0"][..., 96:]).max() > 0
    for b in (0, 1, 2):
        assert res["d_y3_%d" % b].shape == (B, h, w, 257) and res["a1_%d" % b].shape == res["a2_%d" % b].shape == (B, h, w, 128)
    for k in ("d_skip_2", "d_xin2", "d_skip_1", "d_xin1"):
        assert res[k].shape == (B, h, w, 257), k
    assert tuple(host.lower_trunk_norms(res)) == host.LOWER_TRUNK_NORM_NAMES == ("d_x0",) + cases.NAMES
    assert all(k in res for k in host.LOWER_TRUNK_DATA)


def test_lower_trunk_forward_and_the_example_inputs():
    wt = cases.lt_weights()
    x0, d_res2, y3_0, res0, y3_1, res1, y3_2, res2 = host.lower_trunk_example_inputs(2, 4, 2, 3, weights=wt)
    again = host.lower_trunk_example_inputs(2, 4, 2, 3)
    for a, b in zip((x0, d_res2), again):
        assert a.dtype == f32 and a.tobytes() == b.tobytes()
    assert x0.shape == (2, 2, 4, 99) and d_res2.shape == (2, 2, 4, 257)
    assert (x0[..., :96] < 0).any() and (x0[..., :96] > 0).any() and x0[..., 96:].min() >= 0 and x0[..., 96:].max() <= 1
    fw = host.lower_trunk_forward(wt, x0)
    assert sorted(fw) == sorted(k % b for b in (0, 1, 2) for k in ("y3_%d", "res%d", "a1_%d", "a2_%d", "pre_%d"))
    for k, t in zip(cases.FORWARD_KEYS, (y3_0, res0, y3_1, res1, y3_2, res2)):
        assert t.dtype == f32 and t.shape == (2, 2, 4, 257) and t.tobytes() == fw[k].astype(f32).tobytes(), k
    # it is the existing statements with block=: block 0 on x0, block 1 on res0, block 2 on res1
    xin = x0
    for b in (0, 1, 2):
        bf = host.bottleneck_forward(wt, xin, block=b)
        np.testing.assert_array_equal(fw["y3_%d" % b], bf["y3"])
        nf = host.nonlocal_forward(wt, bf["y3"], xin, block=b)
        np.testing.assert_array_equal(fw["res%d" % b], nf["out"])
        np.testing.assert_array_equal(fw["pre_%d" % b], nf["pre"])
        xin = nf["out"]
    # block 0's skip reaches the first 99 channels alone
    z = host.nonlocal_forward(wt, fw["y3_0"], x0, block=0)["z"]
    np.testing.assert_array_equal(fw["pre_0"][..., 99:], z[..., 99:])
    np.testing.assert_array_equal(fw["pre_0"][..., :99], z[..., :99] + x0.astype(np.float64))


def test_acts_given_are_those_of_the_own_forward():
    wt, x0, d_res2 = cases.case(2, 4, 2, 2)
    fw = host.lower_trunk_forward(wt, x0)
    feeds = (x0,) + tuple(fw[k] for k in cases.FORWARD_KEYS) + (d_res2,)
    own = host.lower_trunk_grad(wt, *feeds)
    given = host.lower_trunk_grad(wt, *feeds, acts={k % b: fw[k % b] for b in (0, 1, 2) for k in ("a1_%d", "a2_%d")})
    assert sorted(own) == sorted(given)
    for n in own:
        np.testing.assert_array_equal(given[n], own[n], err_msg=n)


@pytest.mark.parametrize("C", (99, 257))
def test_the_narrow_skip_alone(C):
    """nonlocal_grad with a skip of C <= 257 channels against autograd of out = lrelu(z + pad_257(xin)); d_skip is gz[..., :C]; and
    d_out moved only in the channels the skip does not reach (where the pad's mask is 0) changes no byte of d_skip."""
    wt = cases.lt_weights()
    block = 0 if C == 99 else 1
    rng = np.random.default_rng(40 + C)
    B, h, w = 2, 2, 4
    y3 = (0.25 * rng.standard_normal((B, h, w, 257))).astype(f32)
    xin = rng.standard_normal((B, h, w, C)).astype(f32)
    d_out = (rng.standard_normal((B, h, w, 257)) / (B * h * w * 257)).astype(f32)
    fw = host.nonlocal_forward(wt, y3, xin, block=block)
    assert fw["out"].shape == fw["pre"].shape == (B, h, w, 257) and (fw["pre"] > 0).any() and (fw["pre"] < 0).any()
    res = host.nonlocal_grad(wt, y3, xin, d_out, block=block)
    assert res["gz"].shape == (B, h, w, 257) and res["d_skip"].shape == (B, h, w, C) and res["d_y3"].shape == (B, h, w, 257)
    assert res["d_skip"].tobytes() == np.ascontiguousarray(res["gz"][..., :C]).tobytes()
    d_y3, d_skip = cases.autograd_nonlocal(wt, y3, xin, d_out, block)
    for name, want in (("d_y3", d_y3), ("d_skip", d_skip)):
        e = float(np.abs(res[name] - want).max() / np.abs(want).max())
        print("non-local grad with a %d-wide skip: %s against torch autograd, scaled difference %.3g" % (C, name, e))
        assert e <= cases.AUTOGRAD_CAP, (name, e)
    # the skip's gradient is d_out times relu3's slope, channel for channel: beyond channel C nothing of d_out reaches d_skip
    moved = d_out.copy()
    moved[..., C:] = -3 * moved[..., C:] + f32(1e-3)
    res2 = host.nonlocal_grad(wt, y3, xin, moved, block=block)
    assert res2["d_skip"].tobytes() == res["d_skip"].tobytes()
    if C < 257:
        assert np.abs(res2["d_y3"] - res["d_y3"]).max() > 0
    # the objective agrees with the forward
    assert host.nonlocal_objective_f64(wt, y3, xin, d_out, block=block) == (d_out.astype(np.float64) * fw["out"]).sum()


def test_the_bottleneck_statements_take_the_lower_blocks_widths():
    """bottleneck_forward / bottleneck_grad at C = 257 (block 1) and C = 99 (block 0): shapes, and d_xin against autograd through
    autograd_block's own conv chain is covered by the whole-trunk test; here d_xin = d_skip + the conv path, and the skip adds in."""
    wt = cases.lt_weights()
    for block, C in ((1, 257), (0, 99)):
        xin, d_y3, d_skip = host.bottleneck_example_inputs(2, 4, 2, 6, C=C)
        res = host.bottleneck_grad(wt, xin, d_y3, d_skip, block=block)
        none = host.bottleneck_grad(wt, xin, d_y3, None, block=block)
        assert res["d_xin"].shape == (2, 2, 4, C) and res["res_stack/%d/conv1/kernel" % block].shape == (1, 1, C, 128)
        np.testing.assert_array_equal(res["d_xin"], d_skip.astype(np.float64) + none["d_xin"])


def test_the_statements_of_the_colour_branch_keep_their_bytes():
    """nonlocal_forward, nonlocal_grad, bottleneck_grad and colour_trunk_grad at C = 261 on colour_trunk_grad_cases.case(4, 32, 1): the
    hashes of the commit before the skip could be narrower than the block.  And lower_trunk_forward, lower_trunk_grad and the two
    trunk blobs: the hashes of the commit before the two stages shared one statement of the chain."""
    assert cases.statement_hashes() == cases.PARENT_HASHES


def test_central_finite_differences(h=2, w=4, B=1, FD_STEP=1e-7):
    """Single entries of x0 and of variables of the three blocks, on segments along which none of the nine LeakyReLU masks changes
    (asserted for the five points used: a condition on the seed and the step, not a tolerance).  There the objective <d_res2, res2> is a
    smooth function p(t) of the step; the central quotient q(e) = (p(e) - p(-e)) / 2e is p'(0) + c3 e^2 + O(e^4), so |q(2e) - q(e)| = 3
    |c3| e^2 + O(e^4) bounds the truncation of q(e) with a factor 3 to spare, as the colour trunk's test bounds its own.  The evaluations
    run in numpy's extended precision (u = 2^-64); a value of res2 is reached through fewer than 1e4 operations, so p carries an error of
    1e4 u |p| at most, and the quotient that over e: the allowance beside the truncation term.  The two together are asserted to lie
    below a thousandth of the derivative."""
    u = float(np.finfo(LD).eps) / 2
    wt, x0, d_res2 = cases.case(h, w, B, 4)
    res = cases.host_run(wt, x0, d_res2)
    entries = [("x0", (0, 1, 2, 5)), ("x0", (0, 0, 3, 97)), ("res_stack/0/conv1/kernel", (0, 0, 98, 2)), ("res_stack/0/conv1/kernel", (0, 0, 40, 7)),
               ("res_stack/0/non_local/theta/kernel", (0, 0, 10, 3)), ("res_stack/1/conv2/kernel", (1, 1, 3, 7)), ("res_stack/1/bnorm1/gamma", (4,)),
               ("res_stack/2/conv1/kernel", (0, 0, 256, 2)), ("res_stack/2/non_local/w/bias", (9,)), ("res_stack/2/bnorm3/beta", (100,))]
    trunk = {n: v for n, v in wt.items() if n.startswith(("res_stack/0/", "res_stack/1/", "res_stack/2/"))}
    for name, index in entries:
        base = x0 if name == "x0" else wt[name]
        step = LD(FD_STEP) * LD(float(np.abs(base).max()))

        def at(t):
            moved = {n: np.asarray(v, LD) for n, v in trunk.items()}
            x2 = np.asarray(x0, LD).copy()
            target = x2 if name == "x0" else moved[name].copy()
            target[index] += LD(t) * step
            if name != "x0":
                moved[name] = target
            masks = []
            return host.lower_trunk_objective_f64(moved, x2, d_res2, masks=masks, dtype=LD), masks

        values = {t: at(t) for t in (-2, -1, 0, 1, 2)}
        assert values[0][0].dtype == LD
        for t in (-2, -1, 1, 2):
            assert len(values[t][1]) == 9
            for a, b in zip(values[t][1], values[0][1]):
                assert (a == b).all(), "a LeakyReLU's mask differs between the evaluation points"
        q1 = (values[1][0] - values[-1][0]) / (2 * step)
        q2 = (values[2][0] - values[-2][0]) / (4 * step)
        want = LD(res["d_x0" if name == "x0" else name][index])
        rounding = 1e4 * u * abs(float(values[0][0])) / float(step)
        bound = abs(float(q2 - q1)) + rounding
        print("lower trunk grad %s%s: quotient %.12g, gradient %.12g, |difference| %.3g, bound %.3g (|q(2e) - q(e)| %.3g, rounding %.3g)"
              % (name, list(index), float(q1), float(want), abs(float(q1 - want)), bound, abs(float(q2 - q1)), rounding))
        assert abs(float(want)) > 1e3 * bound, "the bound must mean something beside the derivative"
        assert abs(float(q1 - want)) <= bound
