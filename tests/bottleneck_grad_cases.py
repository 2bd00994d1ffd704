"""What the host tests (test_bottleneck_grad_cpu.py) and the device tests (test_bottleneck_grad_gpu.py) of the backward of res_stack/5's
lower half share: seeded weights and inputs, the torch autograd restatement the statement is held to, the scaled difference over the
thirteen outputs, the bounds, and constructed cases with closed-form answers.  Every `check_*` takes
`run(weights, xin, d_y3, d_skip, acts)` -> dict(the thirteen outputs by name, the stage maps `gz2`, `gz1`, `a1`, `a2` as used, `dtype`:
the arithmetic's type); `acts` is None (the runner's own forward) or dict(a1, a2); `d_skip` may be None."""
import numpy as np

from blindshadowremoval_amd import generator_grad as host
from blindshadowremoval_amd.weights import BN_EPS, LRELU_ALPHA, generator_bottleneck_trainable_names, init_weights

f32 = np.float32
ST = "res_stack/5/"
NAMES = tuple(generator_bottleneck_trainable_names())
OUTPUTS = ("d_xin",) + NAMES
AUTOGRAD_SIZES = ((1, 4, 1), (2, 4, 2), (3, 4, 3), (4, 32, 1))      # coarse (h, w, B)
# the largest scaled difference between the statement and autograd over AUTOGRAD_SIZES and the C = 877 case, measured on the CPU
# (test_bottleneck_grad_cpu.py prints each figure)
AUTOGRAD_MEASURED = 5.07e-15            # bnorm2/gamma at (3, 4, 3); 1.75e-15, 2.52e-15, 4.34e-15 at the other sizes, 1.62e-15 at C = 877
AUTOGRAD_CAP = 1e-9
AUTOGRAD_BOUND = min(4 * AUTOGRAD_MEASURED, AUTOGRAD_CAP)
STAGE_BUDGET = 1e-5                # the project's fp32-class stage budget (tests/stage_parity.py)
GPU_SIZES = ((4, 32, 1), (8, 32, 2), (12, 32, 3), (4, 64, 1), (32, 32, 1))
# the largest scaled error of an output of the device chain against bottleneck_grad(acts = the device's own a1, a2), measured on an
# MI355X over GPU_SIZES (tools/bottleneck_grad_bench.py --parity, profiles/bottleneck_grad_bench.json)
E2E_MEASURED = 1.1e-6         # bnorm1/beta at (12, 32, 3); 9.61e-7, 7.92e-7, 8.1e-7, 7.61e-7 at the other four sizes in GPU_SIZES' order
E2E_BOUND = min(4 * E2E_MEASURED, 1e-3)

_weights = {}


def bn_weights(seed=3, variant="gsc"):
    """init_weights(seed): non-trivial BN statistics.  Cached: treat as read-only."""
    if (seed, variant) not in _weights:
        _weights[(seed, variant)] = init_weights(seed, variant=variant)
    return _weights[(seed, variant)]


def case(h, w, B, seed=0, C=261):
    """(weights, xin, d_y3, d_skip) at a coarse size, with both signs asserted present in a1 and in a2."""
    wt = bn_weights(variant="gsc" if C == 261 else "tsm")
    xin, d_y3, d_skip = host.bottleneck_example_inputs(h, w, B, seed, C)
    fw = host.bottleneck_forward(wt, xin)
    for k in ("a1", "a2"):
        frac = float((fw[k] > 0).mean())
        assert 0.02 < frac < 0.98, (k, frac)
    return wt, xin, d_y3, d_skip


def with_block5(weights, block):
    """A weights dict whose res_stack/5 holds res_stack/<block>'s variables: what a statement of block 5 computes for block `block`."""
    out = dict(weights)
    src = "res_stack/%d/" % block
    for n in weights:
        if n.startswith(src):
            out[ST + n[len(src):]] = weights[n]
    return out


def worst_scaled_diff(got, ref, names=OUTPUTS):
    """The largest of max |got[v] - ref[v]| / max |ref[v]| over `names` (an output whose reference is all 0 must be all 0), and the name
    it occurred at."""
    worst, at = 0.0, ""
    for name in names:
        a, b = np.asarray(got[name], np.float64), np.asarray(ref[name], np.float64)
        assert a.shape == b.shape, (name, a.shape, b.shape)
        scale = np.abs(b).max()
        d = float(np.abs(a - b).max() / scale) if scale > 0 else (0.0 if not a.any() else np.inf)
        if d > worst:
            worst, at = d, name
    return worst, at


# ---- torch autograd in float64, written from the reference's semantics (model.py:81-101): conv2d with padding 1, inference BN,
# leaky_relu 0.3; the twelve variables and xin are leaves
def autograd_grads(weights, xin, d_y3, d_skip=None):
    """d (<d_y3, y3> + <d_skip, xin>) / d each of the twelve variables and xin by torch autograd in float64 from the float32 variables:
    name -> float64 array in the variable's shape, `d_xin` [B,h,w,C]."""
    import torch
    import torch.nn.functional as F
    t64 = lambda a: torch.from_numpy(np.array(a, np.float64))                        # noqa: E731
    leaves = {n: t64(weights[n]).requires_grad_(True) for n in NAMES}
    x = t64(xin).requires_grad_(True)

    def layer(t, j, pad):
        k = leaves[ST + "conv%d/kernel" % j].permute(3, 2, 0, 1)                     # HWIO -> OIHW
        c = F.conv2d(t, k, leaves[ST + "conv%d/bias" % j], padding=pad)
        mean, var = (t64(weights[ST + "bnorm%d/%s" % (j, p)]) for p in ("moving_mean", "moving_variance"))
        shape = (1, -1, 1, 1)
        return ((c - mean.reshape(shape)) / torch.sqrt(var.reshape(shape) + BN_EPS) * leaves[ST + "bnorm%d/gamma" % j].reshape(shape)
                + leaves[ST + "bnorm%d/beta" % j].reshape(shape))

    t = x.permute(0, 3, 1, 2)
    t = F.leaky_relu(layer(t, 1, 0), LRELU_ALPHA)
    t = F.leaky_relu(layer(t, 2, 1), LRELU_ALPHA)
    y3 = layer(t, 3, 0).permute(0, 2, 3, 1)
    obj = (y3 * t64(d_y3)).sum()
    if d_skip is not None:
        obj = obj + (x * t64(d_skip)).sum()
    obj.backward()
    res = {k: v.grad.numpy() for k, v in leaves.items()}
    res["d_xin"] = x.grad.numpy()
    return res


# ---- closed forms
def _tol(r):
    return 1e-12 if r["dtype"] is np.float64 else 1e-5


def _close(r, what, got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, what
    assert np.abs(want).max() > 0 and np.abs(got - want).max() <= _tol(r) * np.abs(want).max(), what


def _same(what, got, want):
    np.testing.assert_array_equal(np.asarray(got, np.float64), np.asarray(want, np.float64), err_msg=what)


def _zero(r, names):
    for name in names:
        assert not np.asarray(r[name]).any(), name


def _vectors(wt, j):
    return host.bottleneck_bn_vectors(wt, j)


def check_zero_d_y3(run, h=4, w=32, B=1):
    """d_y3 = 0: d_xin is d_skip bit for bit and all twelve gradients are exactly 0."""
    wt, xin, d_y3, d_skip = case(h, w, B, 5)
    r = run(wt, xin, np.zeros_like(d_y3), d_skip, None)
    _same("d_xin", r["d_xin"], d_skip)
    for name in NAMES:
        assert np.asarray(r[name]).shape == wt[name].shape, name
    _zero(r, NAMES)


def check_zero_gamma3(run, h=4, w=32, B=1):
    """gamma3 = 0 (inv3 = 0): d_xin = d_skip, everything of conv1, conv2 and conv3's kernel and bias is exactly 0, d beta3 = sum d_y3 and
    d gamma3 is the hand sum sum d_y3 (c3 - mean3) rstd3 with c3 = a2 W3 + b3."""
    wt, xin, d_y3, d_skip = case(h, w, B, 6)
    wt = dict(wt)
    wt[ST + "bnorm3/gamma"] = np.zeros_like(wt[ST + "bnorm3/gamma"])
    r = run(wt, xin, d_y3, d_skip, None)
    _same("d_xin", r["d_xin"], d_skip)
    _zero(r, ("gz2", "gz1") + tuple(n for n in NAMES if n not in (ST + "bnorm3/gamma", ST + "bnorm3/beta")))
    b3, _, mean3, rstd3, _, _ = _vectors(wt, 3)
    g = d_y3.astype(np.float64).reshape(-1, 257)
    c3 = np.asarray(r["a2"], np.float64).reshape(-1, 128) @ np.asarray(wt[ST + "conv3/kernel"], np.float64)[0, 0] + b3
    _close(r, "d beta3", r[ST + "bnorm3/beta"], g.sum(axis=0))
    _close(r, "d gamma3", r[ST + "bnorm3/gamma"], (g * (c3 - mean3) * rstd3).sum(axis=0))


def check_zero_conv2_kernel(run, h=4, w=32, B=1):
    """K2 = 0 passes nothing below conv2: gz1 = 0, everything of layer 1 is exactly 0 and d_xin = d_skip.  d K2 itself is NOT 0 (it is a1
    against gz2 inv2, whatever K2 holds): its centre tap is held to a hand sum."""
    wt, xin, d_y3, d_skip = case(h, w, B, 7)
    wt = dict(wt)
    wt[ST + "conv2/kernel"] = np.zeros_like(wt[ST + "conv2/kernel"])
    r = run(wt, xin, d_y3, d_skip, None)
    _zero(r, ("gz1", ST + "conv1/kernel", ST + "conv1/bias", ST + "bnorm1/gamma", ST + "bnorm1/beta"))
    _same("d_xin", r["d_xin"], d_skip)
    inv2 = _vectors(wt, 2)[1]
    a1, gz2 = (np.asarray(r[k], np.float64).reshape(-1, 128) for k in ("a1", "gz2"))
    _close(r, "d K2 centre tap", np.asarray(r[ST + "conv2/kernel"])[1, 1], (a1.T @ gz2) * inv2)


def check_zero_a1_takes_the_slope(run, h=4, w=32, B=1):
    """W1 = 0, b1 = mean1, beta1 = 0: a1 is exactly +0 everywhere, so gz1 = 0.3 da1 with da1 the 3x3 data gradient of gz2 inv2 (an
    activation of exactly 0 takes the slope), and d_xin = d_skip."""
    wt, xin, d_y3, d_skip = case(h, w, B, 8)
    wt = dict(wt)
    wt[ST + "conv1/kernel"] = np.zeros_like(wt[ST + "conv1/kernel"])
    wt[ST + "conv1/bias"] = wt[ST + "bnorm1/moving_mean"].copy()
    wt[ST + "bnorm1/beta"] = np.zeros_like(wt[ST + "bnorm1/beta"])
    r = run(wt, xin, d_y3, d_skip, None)
    a1 = np.asarray(r["a1"])
    assert not a1.any() and not np.signbit(a1).any()
    inv2 = _vectors(wt, 2)[1]
    da1 = host.conv3x3_same_dgrad(np.asarray(r["gz2"], np.float64) * inv2, wt[ST + "conv2/kernel"])
    if r["dtype"] is np.float64:
        _same("gz1", r["gz1"], LRELU_ALPHA * da1)
    else:
        _close(r, "gz1", r["gz1"], LRELU_ALPHA * da1)
    _same("d_xin", r["d_xin"], d_skip)


def check_single_pixel(run, h=4, w=32, B=2):
    """d_y3 supported at the single pixel (0, 0) of image 1 and d_skip = 0: a tap of d K2 in row 0 or column 0 would read a1 above or left
    of the image (or the end of image 0) and is exactly 0, the other four are not; d_xin of image 0 is exactly 0 and image 1's support is
    the four pixels (0..1, 0..1)."""
    wt, xin, d_y3, _ = case(h, w, B, 9)
    one = np.zeros_like(d_y3)
    one[1, 0, 0] = d_y3[1, 0, 0]
    r = run(wt, xin, one, np.zeros_like(xin), None)
    dk = np.asarray(r[ST + "conv2/kernel"])
    for a in range(3):
        for b in range(3):
            assert dk[a, b].any() == (a > 0 and b > 0), (a, b)
    d_xin = np.asarray(r["d_xin"])
    assert not d_xin[0].any()
    support = np.abs(d_xin[1]).max(axis=2) > 0
    want = np.zeros((h, w), bool)
    want[:2, :2] = True
    np.testing.assert_array_equal(support, want)


def check_the_skips_own_channels_reach_nothing_else(run, h=4, w=32, B=1):
    """d_skip changed in channels 257..260 only changes d_xin in those channels only, and nothing else by a bit."""
    wt, xin, d_y3, d_skip = case(h, w, B, 10)
    r = run(wt, xin, d_y3, d_skip, None)
    moved = d_skip.copy()
    moved[..., 257:] = -2 * moved[..., 257:] + f32(1e-3)
    r2 = run(wt, xin, d_y3, moved, None)
    assert not np.array_equal(np.asarray(r2["d_xin"])[..., 257:], np.asarray(r["d_xin"])[..., 257:])
    np.testing.assert_array_equal(np.asarray(r2["d_xin"])[..., :257], np.asarray(r["d_xin"])[..., :257])
    for name in NAMES + ("gz2", "gz1", "a1", "a2"):
        np.testing.assert_array_equal(np.asarray(r2[name]), np.asarray(r[name]), err_msg=name)


CONSTRUCTED = (check_zero_d_y3, check_zero_gamma3, check_zero_conv2_kernel, check_zero_a1_takes_the_slope, check_single_pixel,
               check_the_skips_own_channels_reach_nothing_else)
