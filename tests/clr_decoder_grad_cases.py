"""What the host tests (test_clr_decoder_grad_cpu.py, test_clr_decoder_grad_fixture.py) and the device tests
(test_clr_decoder_grad_gpu.py) of the generator's colour decoder backward share: seeded weights and inputs, the torch autograd
restatement the statement is held to, the scaled difference over the thirteen outputs, the bounds, and constructed cases with
closed-form answers.  Every `check_*` takes `run(weights, x, d_f, acts)` -> dict(the thirteen outputs by name, `gz3`, `gz2`, `gz1`,
`f1`, `f2`, `f` as used, `dtype`: the arithmetic's type); `acts` is None (the runner's own forward) or dict(f1, f2, f)."""
import numpy as np

from blindshadowremoval_amd import generator_grad as host
from blindshadowremoval_amd.weights import LRELU_ALPHA, BN_EPS, generator_decoder_trainable_names, init_weights

f32 = np.float32
NAMES = tuple(generator_decoder_trainable_names())
OUTPUTS = ("d_x",) + NAMES
AUTOGRAD_SIZES = ((1, 4, 1), (2, 4, 2), (3, 4, 3), (4, 32, 1))      # coarse (h, w, B)
FIXTURE = (2, 4, 2)                                                  # tests/golden/clr_decoder_grad_2x4*.npz
AUTOGRAD_MEASURED = 3.0e-15        # the largest scaled difference between the statement and autograd when the fixture was made (its `measured`)
AUTOGRAD_CAP = 1e-9
AUTOGRAD_BOUND = min(4 * AUTOGRAD_MEASURED, AUTOGRAD_CAP)
STAGE_BUDGET = 1e-5                # the project's fp32-class stage budget (tests/stage_parity.py)
# the largest scaled error of an output of the device chain against decoder_grad(acts = the device's own f1, f2, f), measured on an
# MI355X over the GPU test's four shapes (tools/clr_decoder_bench.py --parity, profiles/clr_decoder_grad_bench.json)
E2E_MEASURED = 1.72e-6        # d_x at (96, 256, 3); 1.22e-6, 1.40e-6, 1.34e-6 at the other three shapes, d_x each time
E2E_BOUND = min(4 * E2E_MEASURED, 1e-3)

_weights = {}


def decoder_weights(seed=3):
    """init_weights(seed): non-trivial BN statistics.  Cached: treat as read-only."""
    if seed not in _weights:
        _weights[seed] = init_weights(seed)
    return _weights[seed]


def case(h, w, B, seed=0):
    """(weights, x, d_f) at a coarse size, with both signs of the three pre-activations asserted present."""
    wt = decoder_weights()
    x, d_f = host.decoder_example_inputs(h, w, B, seed)
    for a in host.decoder_forward(wt, x):
        frac = float((a > 0).mean())
        assert 0.02 < frac < 0.98, frac
    return wt, x, d_f


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


# ---- torch autograd in float64: F.conv_transpose2d, F.leaky_relu; the twelve variables and x are leaves
def autograd_grads(weights, x, d_f):
    """d <d_f, f> / d each of the twelve variables and x by torch autograd in float64 from the float32 variables: name -> float64 array in
    the variable's shape (kernels [3,3,O,C]), `d_x` [B,h,w,C]."""
    import torch
    import torch.nn.functional as F
    t64 = lambda a: torch.from_numpy(np.array(a, np.float64))                        # noqa: E731
    is_k = lambda n: n.endswith("/kernel")                                            # noqa: E731
    # conv_transpose2d takes [C_in, C_out, kh, kw]; the variable is [kh, kw, C_out, C_in]
    leaves = {n: t64(np.ascontiguousarray(np.transpose(weights[n], (3, 2, 0, 1))) if is_k(n) else weights[n]).requires_grad_(True) for n in NAMES}
    x_t = t64(x).requires_grad_(True)
    h = x_t.permute(0, 3, 1, 2)
    for stem in host.DECODER_LAYERS:
        y = F.conv_transpose2d(h, leaves[stem + "/conv/kernel"], leaves[stem + "/conv/bias"], stride=2, padding=0)
        y = y[:, :, :2 * h.shape[2], :2 * h.shape[3]]
        g, beta = (leaves[stem + "/bnorm/" + p].reshape(1, -1, 1, 1) for p in ("gamma", "beta"))
        mean, var = (t64(weights[stem + "/bnorm/" + p]).reshape(1, -1, 1, 1) for p in ("moving_mean", "moving_variance"))
        h = F.leaky_relu((y - mean) / torch.sqrt(var + BN_EPS) * g + beta, LRELU_ALPHA)
    (h.permute(0, 2, 3, 1) * t64(d_f)).sum().backward()
    out = {n: np.ascontiguousarray(np.transpose(leaves[n].grad.numpy(), (2, 3, 1, 0))) if is_k(n) else leaves[n].grad.numpy() for n in NAMES}
    out["d_x"] = x_t.grad.numpy()
    return out


# ---- closed forms
def _tol(r):
    return 1e-12 if r["dtype"] is np.float64 else 1e-5


def check_zero_d_f(run, h=4, w=32, B=1):
    """d_f = 0 gives all thirteen outputs exactly 0."""
    wt, x, d_f = case(h, w, B, 5)
    r = run(wt, x, np.zeros_like(d_f), None)
    for name in OUTPUTS:
        assert np.asarray(r[name]).shape == (x.shape if name == "d_x" else wt[name].shape), name
        assert not np.asarray(r[name]).any(), name


def check_zero_k3(run, h=4, w=32, B=1):
    """clr_up3's kernel 0 passes nothing down: everything below — clr_up1's and clr_up2's eight gradients and d_x — is exactly 0, and
    d bias3, d beta3, d gamma3 are their sums over gz3 (the pre-activation is the bias alone).  d K3 itself is NOT 0 (it is gz3 against
    f2, whatever K3 holds): its centre tap is held to a hand sum, Wg[1, 1, o, c] = sum gz3[n, 2i + 1, 2j + 1, o] f2[n, i, j, c]."""
    wt, x, d_f = case(h, w, B, 6)
    wt = dict(wt)
    wt["clr_up3/conv/kernel"] = np.zeros_like(wt["clr_up3/conv/kernel"])
    r = run(wt, x, d_f, None)
    for name in NAMES[:8] + ("d_x",):
        assert not np.asarray(r[name]).any(), name
    bias, inv, mean, rstd, _ = host.bn_vectors(wt, "clr_up3")
    gz3 = np.asarray(r["gz3"], np.float64)
    S = gz3.sum(axis=(0, 1, 2))
    assert np.abs(S).max() > 0
    want_k = np.einsum("nijo,nijc->oc", gz3[:, 1::2, 1::2], np.asarray(r["f2"], np.float64)) * inv[:, None]
    for name, got, want in (("clr_up3/bnorm/beta", r["clr_up3/bnorm/beta"], S), ("clr_up3/conv/bias", r["clr_up3/conv/bias"], inv * S),
                            ("clr_up3/bnorm/gamma", r["clr_up3/bnorm/gamma"], (bias - mean) * rstd * S),
                            ("clr_up3/conv/kernel centre tap", np.asarray(r["clr_up3/conv/kernel"])[1, 1], want_k)):
        assert np.abs(want).max() > 0 and np.abs(np.asarray(got, np.float64) - want).max() <= _tol(r) * np.abs(want).max(), name


def check_planted_zeros_take_the_slope(run, h=4, w=32, B=1):
    """Activations of exactly +0 and -0 planted in f take the slope 0.3 (TensorFlow's LeakyReluGrad): gz3 there is 0.3 d_f."""
    wt, x, d_f = case(h, w, B, 7)
    f1, f2, f = (a.astype(f32) for a in host.decoder_forward(wt, x, f32))
    f = f.copy()
    f[0, 0, 0, :4] = np.array([0.0, -0.0, 0.0, -0.0], f32)
    f[0, 5, 7, 9] = f32(-0.0)
    r = run(wt, x, d_f, {"f1": f1, "f2": f2, "f": f})
    gz3 = np.asarray(r["gz3"], np.float64)
    for at in ((0, 0, 0, 0), (0, 0, 0, 1), (0, 0, 0, 2), (0, 0, 0, 3), (0, 5, 7, 9)):
        want = 0.3 * float(d_f[at])
        assert want != 0 and abs(gz3[at] - want) <= 1e-6 * abs(want), at
    st = host.decoder_grad(wt, x, d_f, acts={"f1": f1, "f2": f2, "f": f})
    assert worst_scaled_diff(r, st)[0] <= (1e-12 if r["dtype"] is np.float64 else E2E_BOUND)


def check_no_contribution_from_the_cropped_row(run, h=4, w=32, B=1):
    """One unit of gradient at a pixel of the LAST fine row and column of f, channel o, everything else 0, slopes all 1 (f > 0 planted):
    gz3 is that unit, and clr_up3's kernel gradient is a hand sum — the coarse pixels (i, j) with 2i + a = last row, 2j + b = last column
    contribute f2[i, j, :] to tap (a, b): the last fine row 8h - 1 = 2 (4h - 1) + 1 is reached by tap a = 1 from coarse row 4h - 1 alone,
    and likewise the last column; fine row 8h, which tap a = 2 of that coarse row would reach, does not exist."""
    wt, x, _ = case(h, w, B, 8)
    f1, f2, f = (a.astype(f32) for a in host.decoder_forward(wt, x, f32))
    f = np.abs(f) + f32(1)
    o = 5
    d_f = np.zeros(f.shape, f32)
    Y, X = f.shape[1] - 1, f.shape[2] - 1
    d_f[0, Y, X, o] = 1
    r = run(wt, x, d_f, {"f1": f1, "f2": f2, "f": f})
    _, inv, _, _, _ = host.bn_vectors(wt, "clr_up3")
    want = np.zeros(wt["clr_up3/conv/kernel"].shape, np.float64)
    want[1, 1, o, :] = inv[o] * f2[0, Y // 2, X // 2, :].astype(np.float64)          # 2i + 1 = Y, 2j + 1 = X: the only in-range pair
    got = np.asarray(r["clr_up3/conv/kernel"], np.float64)
    assert np.abs(got - want).max() <= _tol(r) * np.abs(want).max()
    assert not got[2].any() and not got[:, 2].any() and not got[0].any() and not got[:, 0].any()
    # the same unit one row up, at an even fine row Y - 1 = 2 (4h - 1): taps a = 0 from coarse row 4h - 1 and a = 2 from 4h - 2
    d_f2 = np.zeros(f.shape, f32)
    d_f2[0, Y - 1, X, o] = 1
    got2 = np.asarray(run(wt, x, d_f2, {"f1": f1, "f2": f2, "f": f})["clr_up3/conv/kernel"], np.float64)
    want2 = np.zeros_like(want)
    want2[0, 1, o, :] = inv[o] * f2[0, Y // 2, X // 2, :].astype(np.float64)
    want2[2, 1, o, :] = inv[o] * f2[0, Y // 2 - 1, X // 2, :].astype(np.float64)
    assert np.abs(got2 - want2).max() <= _tol(r) * np.abs(want2).max()


CONSTRUCTED = (check_zero_d_f, check_zero_k3, check_planted_zeros_take_the_slope, check_no_contribution_from_the_cropped_row)
