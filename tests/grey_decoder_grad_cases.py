"""What the host tests (test_grey_decoder_grad_cpu.py) and the device tests (test_grey_decoder_grad_gpu.py) of the generator's grey
decoder backward share: seeded weights and inputs, the torch autograd restatement the statement is held to, the scaled difference over
the fifteen outputs, the bounds, and constructed cases with closed-form answers.  Every `check_*` takes `run(weights, x, x3, x2, d_y,
acts)` -> dict(the fifteen outputs by name, `gz3`, `gz2`, `gz1`, `up1`, `up2`, `y` as used, `dtype`: the arithmetic's type); `acts` is
None (the runner's own forward) or dict(up1, up2, y)."""
import numpy as np

from blindshadowremoval_amd import generator_grad as host
from blindshadowremoval_amd.weights import LRELU_ALPHA, BN_EPS, generator_grey_decoder_trainable_names, init_weights

f32 = np.float32
NAMES = tuple(generator_grey_decoder_trainable_names())
DATA = ("d_x", "d_x3", "d_x2")
OUTPUTS = DATA + NAMES
AUTOGRAD_SIZES = ((1, 4, 1), (2, 4, 2), (3, 4, 3), (4, 32, 1))      # coarse (h, w, B)
AUTOGRAD_MEASURED = 3.5e-15        # the largest scaled difference between the statement and autograd over AUTOGRAD_SIZES when this was written: up3/bnorm/beta at (4, 32, 1)
AUTOGRAD_CAP = 1e-9
AUTOGRAD_BOUND = min(4 * AUTOGRAD_MEASURED, AUTOGRAD_CAP)
STAGE_BUDGET = 1e-5                # the project's fp32-class stage budget (tests/stage_parity.py)
# the largest scaled error of an output of the device chain against grey_decoder_grad(acts = the device's own up1, up2, y), measured on an
# MI355X over the GPU test's four shapes (tools/grey_decoder_bench.py --parity, profiles/grey_decoder_grad_bench.json)
E2E_MEASURED = 1.27e-6        # d_x at (96, 256, 3); 1.09e-6, 1.19e-6, 1.06e-6 at the other three shapes, d_x each time
E2E_BOUND = min(4 * E2E_MEASURED, 1e-5)

_weights = {}


def decoder_weights(seed=3):
    """init_weights(seed): non-trivial BN statistics.  Cached: treat as read-only."""
    if seed not in _weights:
        _weights[seed] = init_weights(seed)
    return _weights[seed]


def case(h, w, B, seed=0):
    """(weights, x, x3, x2, d_y) at a coarse size, with both signs of the three pre-activations asserted present."""
    wt = decoder_weights()
    x, x3, x2, d_y = host.grey_decoder_example_inputs(h, w, B, seed)
    for a in host.grey_decoder_forward(wt, x, x3, x2):
        frac = float((a > 0).mean())
        assert 0.02 < frac < 0.98, frac
    return wt, x, x3, x2, d_y


def forward32(wt, x, x3, x2):
    """(up1, up2, y) float32: grey_decoder_forward in float32."""
    return tuple(np.ascontiguousarray(a, f32) for a in host.grey_decoder_forward(wt, x, x3, x2, f32))


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


# ---- torch autograd in float64: F.conv_transpose2d, torch.cat, F.leaky_relu; the twelve variables, x, x3 and x2 are leaves
def autograd_grads(weights, x, x3, x2, d_y):
    """d <d_y, y> / d each of the twelve variables, x, x3 and x2 by torch autograd in float64 from the float32 variables (the reference's
    model.py:243-245: y = up1(x); y = up2(cat[y, x3]); y = up3(cat[y, x2])): name -> float64 array in the variable's shape (kernels
    [3,3,O,C]), `d_x`, `d_x3`, `d_x2` NHWC."""
    import torch
    import torch.nn.functional as F
    t64 = lambda a: torch.from_numpy(np.array(a, np.float64))                        # noqa: E731
    is_k = lambda n: n.endswith("/kernel")                                            # noqa: E731
    # conv_transpose2d takes [C_in, C_out, kh, kw]; the variable is [kh, kw, C_out, C_in]
    leaves = {n: t64(np.ascontiguousarray(np.transpose(weights[n], (3, 2, 0, 1))) if is_k(n) else weights[n]).requires_grad_(True) for n in NAMES}
    ins = [t64(a).requires_grad_(True) for a in (x, x3, x2)]
    h = ins[0].permute(0, 3, 1, 2)
    for stem, skip in zip(host.GREY_DECODER_LAYERS, (None, ins[1], ins[2])):
        if skip is not None:
            h = torch.cat([h, skip.permute(0, 3, 1, 2)], dim=1)
        y = F.conv_transpose2d(h, leaves[stem + "/conv/kernel"], leaves[stem + "/conv/bias"], stride=2, padding=0)
        y = y[:, :, :2 * h.shape[2], :2 * h.shape[3]]
        g, beta = (leaves[stem + "/bnorm/" + p].reshape(1, -1, 1, 1) for p in ("gamma", "beta"))
        mean, var = (t64(weights[stem + "/bnorm/" + p]).reshape(1, -1, 1, 1) for p in ("moving_mean", "moving_variance"))
        h = F.leaky_relu((y - mean) / torch.sqrt(var + BN_EPS) * g + beta, LRELU_ALPHA)
    (h.permute(0, 2, 3, 1) * t64(d_y)).sum().backward()
    out = {n: np.ascontiguousarray(np.transpose(leaves[n].grad.numpy(), (2, 3, 1, 0))) if is_k(n) else leaves[n].grad.numpy() for n in NAMES}
    out.update(zip(DATA, (t.grad.numpy() for t in ins)))
    return out


# ---- closed forms
def _tol(r):
    return 1e-12 if r["dtype"] is np.float64 else 1e-5


def _close(r, got, want, what):
    want = np.asarray(want, np.float64)
    assert np.abs(want).max() > 0 and np.abs(np.asarray(got, np.float64) - want).max() <= _tol(r) * np.abs(want).max(), what


def _same(a, b, name):
    assert np.asarray(a).tobytes() == np.asarray(b).tobytes(), name


def check_zero_d_y(run, h=4, w=32, B=1):
    """(a) d_y = 0 gives all fifteen outputs exactly 0."""
    wt, x, x3, x2, d_y = case(h, w, B, 5)
    r = run(wt, x, x3, x2, np.zeros_like(d_y), None)
    shapes = dict(d_x=x.shape, d_x3=x3.shape, d_x2=x2.shape)
    for name in OUTPUTS:
        assert np.asarray(r[name]).shape == (shapes[name] if name in shapes else wt[name].shape), name
        assert not np.asarray(r[name]).any(), name


def check_zero_k3_own_half(run, h=4, w=32, B=1):
    """(b) up3's kernel columns 0..63 (the up2 half of its input) set to 0 pass nothing down the decoder: gz2 is exactly 0, so are the
    eight gradients of up2 and up1, d_x3 and d_x.  d_x2 is not 0, and up3's d kernel columns 0..63 are not 0: they are gz3 against up2's
    output whatever the kernel holds — their centre tap is held to the hand sum."""
    wt, x, x3, x2, d_y = case(h, w, B, 6)
    wt = dict(wt)
    k = wt["up3/conv/kernel"].copy()
    k[..., :64] = 0
    wt["up3/conv/kernel"] = k
    r = run(wt, x, x3, x2, d_y, None)
    for name in NAMES[:8] + ("d_x", "d_x3", "gz2", "gz1"):
        assert not np.asarray(r[name]).any(), name
    assert np.asarray(r["d_x2"]).any()
    _, inv, _, _, _ = host.bn_vectors(wt, "up3")
    gz3 = np.asarray(r["gz3"], np.float64)
    want = np.einsum("nijo,nijc->oc", gz3[:, 1::2, 1::2], np.asarray(r["up2"], np.float64)) * inv[:, None]
    _close(r, np.asarray(r["up3/conv/kernel"])[1, 1, :, :64], want, "up3's kernel gradient, centre tap, own half")


def check_zero_k3_skip_half(run, h=4, w=32, B=1):
    """(c) up3's kernel columns 64..127 (the x2 half) set to 0: d_x2 is exactly 0 and the decoder below still gets its gradient."""
    wt, x, x3, x2, d_y = case(h, w, B, 6)
    wt = dict(wt)
    k = wt["up3/conv/kernel"].copy()
    k[..., 64:] = 0
    wt["up3/conv/kernel"] = k
    r = run(wt, x, x3, x2, d_y, None)
    assert not np.asarray(r["d_x2"]).any()
    for name in ("d_x", "d_x3", "gz2"):
        assert np.asarray(r[name]).any(), name


def check_the_skips_feed_their_own_columns_alone(run, h=4, w=32, B=1):
    """(d) On fixed activations up1, up2, y, other draws of x2 and x3 move no bit of d_x, d_x3, d_x2 and the three gz, nor of up3's d kernel
    columns 0..63 and up2's columns 0..95, nor of any d bias or d beta: the skip halves get no mask and feed only their own kernel
    columns and, through sum K Wg, d gamma — which do move."""
    wt, x, x3, x2, d_y = case(h, w, B, 7)
    acts = dict(zip(("up1", "up2", "y"), forward32(wt, x, x3, x2)))
    _, x3b, x2b, _ = host.grey_decoder_example_inputs(h, w, B, 70)
    r, rb = run(wt, x, x3, x2, d_y, acts), run(wt, x, x3b, x2b, d_y, acts)
    for name in DATA + ("gz3", "gz2", "gz1") + tuple(n for n in NAMES if n.endswith("bias") or n.endswith("beta")) + ("up1/conv/kernel", "up1/bnorm/gamma"):
        _same(r[name], rb[name], name)
    for stem, own in (("up3", 64), ("up2", 96)):
        k, kb = np.asarray(r[stem + "/conv/kernel"]), np.asarray(rb[stem + "/conv/kernel"])
        _same(np.ascontiguousarray(k[..., :own]), np.ascontiguousarray(kb[..., :own]), stem + " own columns")
        assert (k[..., own:] != kb[..., own:]).any(), stem
        assert (np.asarray(r[stem + "/bnorm/gamma"]) != np.asarray(rb[stem + "/bnorm/gamma"])).any(), stem


def check_masks_on_the_own_halves_alone(run, h=4, w=32, B=1):
    """(e) x2 and x3 negative throughout, with +0 and -0 planted: d_x2 and d_x3 are the plain data gradients of gz3 and gz2 (a mask read
    from the skip would scale them by 0.3).  Activations of exactly +0 and -0 planted in y, up2's and up1's output take the slope
    (TensorFlow's LeakyReluGrad): gz there is 0.3 g."""
    wt, x, x3, x2, d_y = case(h, w, B, 8)
    x3, x2 = -np.abs(x3) - f32(1), -np.abs(x2) - f32(1)
    x3[0, 0, 0, :2] = np.array([0.0, -0.0], f32)
    x2[0, 1, 2, :2] = np.array([0.0, -0.0], f32)
    up1, up2, y = (a.copy() for a in forward32(wt, x, x3, x2))
    planted = ((0, 0, 0, 0), (0, 0, 0, 1), (0, 3, 5, 9))
    for a in (up1, up2, y):
        for at, z in zip(planted, (0.0, -0.0, -0.0)):
            a[at] = f32(z)
    r = run(wt, x, x3, x2, d_y, {"up1": up1, "up2": up2, "y": y})
    K3, K2 = (np.asarray(wt[s + "/conv/kernel"], np.float64) for s in ("up3", "up2"))
    inv3, inv2 = host.bn_vectors(wt, "up3")[1], host.bn_vectors(wt, "up2")[1]
    dx3 = host.convt3x3_same_dgrad(np.asarray(r["gz3"], np.float64) * inv3, K3)
    dx2 = host.convt3x3_same_dgrad(np.asarray(r["gz2"], np.float64) * inv2, K2)
    _close(r, r["d_x2"], dx3[..., 64:], "d_x2 is unmasked")
    _close(r, r["d_x3"], dx2[..., 96:], "d_x3 is unmasked")
    for at in planted:
        for got, g in ((r["gz3"], d_y), (r["gz2"], dx3[..., :64]), (r["gz1"], dx2[..., :96])):
            want, scale = 0.3 * float(g[at]), float(np.abs(g).max())
            assert abs(want) > 100 * _tol(r) * scale, at                     # the slope 1 would miss the bound below by far
            assert abs(float(np.asarray(got)[at]) - want) <= _tol(r) * scale, at
    st = host.grey_decoder_grad(wt, x, x3, x2, d_y, acts={"up1": up1, "up2": up2, "y": y})
    assert worst_scaled_diff(r, st)[0] <= (1e-12 if r["dtype"] is np.float64 else E2E_BOUND)


def check_no_contribution_from_the_cropped_row(run, h=4, w=32, B=1):
    """(f) One unit of gradient at a pixel of the LAST fine row and column of y, channel o, everything else 0, slopes all 1 (y > 0
    planted): up3's kernel gradient is a hand sum over c3 = cat[up2, x2] — the last fine row 8h - 1 = 2 (4h - 1) + 1 is reached by tap
    a = 1 from coarse row 4h - 1 alone, likewise the last column; fine row 8h and fine column 8w, which taps a = 2 and b = 2 of that coarse
    pixel would reach, do not exist.  The same unit one row up reaches taps a = 0 from coarse row 4h - 1 and a = 2 from 4h - 2."""
    wt, x, x3, x2, _ = case(h, w, B, 9)
    up1, up2, y = forward32(wt, x, x3, x2)
    y = np.abs(y) + f32(1)
    acts = {"up1": up1, "up2": up2, "y": y}
    c3 = np.concatenate([up2, x2], axis=3).astype(np.float64)
    o = 5
    Y, X = y.shape[1] - 1, y.shape[2] - 1
    _, inv, _, _, _ = host.bn_vectors(wt, "up3")
    d_y = np.zeros(y.shape, f32)
    d_y[0, Y, X, o] = 1
    r = run(wt, x, x3, x2, d_y, acts)
    want = np.zeros(wt["up3/conv/kernel"].shape, np.float64)
    want[1, 1, o, :] = inv[o] * c3[0, Y // 2, X // 2, :]                       # 2i + 1 = Y, 2j + 1 = X: the only in-range pair
    got = np.asarray(r["up3/conv/kernel"], np.float64)
    assert np.abs(got - want).max() <= _tol(r) * np.abs(want).max()
    assert not got[2].any() and not got[:, 2].any() and not got[0].any() and not got[:, 0].any()
    d_y2 = np.zeros(y.shape, f32)
    d_y2[0, Y - 1, X, o] = 1
    got2 = np.asarray(run(wt, x, x3, x2, d_y2, acts)["up3/conv/kernel"], np.float64)
    want2 = np.zeros_like(want)
    want2[0, 1, o, :] = inv[o] * c3[0, Y // 2, X // 2, :]
    want2[2, 1, o, :] = inv[o] * c3[0, Y // 2 - 1, X // 2, :]
    assert np.abs(got2 - want2).max() <= _tol(r) * np.abs(want2).max()


def check_images_do_not_mix(run, h=4, w=32, B=2):
    """(g) B = 2 with d_y non-zero on image 1 only: d_x, d_x3 and d_x2 of image 0 are exactly 0, those of image 1 are not."""
    wt, x, x3, x2, d_y = case(h, w, B, 10)
    d_y = d_y.copy()
    d_y[0] = 0
    r = run(wt, x, x3, x2, d_y, None)
    for name in DATA:
        a = np.asarray(r[name])
        assert not a[0].any() and a[1].any(), name


CONSTRUCTED = (check_zero_d_y, check_zero_k3_own_half, check_zero_k3_skip_half, check_the_skips_feed_their_own_columns_alone,
               check_masks_on_the_own_halves_alone, check_no_contribution_from_the_cropped_row, check_images_do_not_mix)
