"""Constructed inputs with closed-form answers, and the torch autograd form, for d per_loss / d con_rgb, shared by the host tests
(test_perceptual_grad_cpu.py, test_perceptual_grad_fixture.py), the device tests (test_perceptual_grad_gpu.py) and the fixture tool
(tools/make_perceptual_grad_fixture.py).  Every `check_*` takes `run(weights, gt, con_rgb, upstream=None)` -> dict(loss, sums, acts,
grad) and asserts on what it returns.

The constructed cases run at B = 1, where every seed weight w_k = 1 / (h_k^2 C_k) is a power of two, with kernels that hold ones and zeros:
every gradient value is a short sum of such powers, exact in float32 (the device) and in float64 (the host statement) alike, so both
routes are held to the same closed forms bit for bit."""
import numpy as np

from blindshadowremoval_amd import perceptual as host
from blindshadowremoval_amd.weights import VGG_BLOCKS, VGG_LAYERS, VGG_TAPS

import perceptual_cases as cases

f32 = np.float32
GRAD_SIZES = ((32, 1), (32, 3), (64, 2))
FIXTURE_CASES = {32: 2, 64: 1}          # S: B of tests/golden/perceptual_{S}.npz, whose seeds (400 + S) the gradient fixtures share
E2E_MEASURED = 8.8e-7          # the largest scaled error of grad measured on GRAD_SIZES: S = 32, B = 1 (tools/perceptual_bench.py --grad --parity)
E2E_BOUND = min(4 * E2E_MEASURED, 1e-3)


def inputs(S, B):
    return cases.inputs(S, B, seed=500 + S + B)


def torch_grad(weights, gt, con_rgb):
    """d per / d con_rgb by torch autograd in float64 -> (float64 [B,S,S,3], per).  An independent form of the backward: torch's conv2d,
    relu, max_pool2d and abs and their registered gradients.  The network starts from the statement's float32 preprocessed input, so
    both sides see the same pre-activations up to float64 rounding and take the same masks; the chain through the preprocessing is the
    factor 255 and the channel reversal.  Each tap's mean is its sum times the statement's w_k, the float32 constant 1 / (B h_k^2 C_k)
    (perceptual.tap_weights): where B is no power of two that constant is not the exact quotient, and the two forms must differentiate
    one objective."""
    import torch
    import torch.nn.functional as F
    B = gt.shape[0]
    x = torch.from_numpy(host.preprocess(gt, con_rgb).astype(np.float64)).permute(0, 3, 1, 2).contiguous().requires_grad_()
    h, per = x, 0.0
    w = host.tap_weights(B, gt.shape[1])
    for b, (_, n) in enumerate(VGG_BLOCKS):
        for i in range(n):
            name = "block%d_conv%d" % (b + 1, i + 1)
            k = torch.from_numpy(np.asarray(weights[name + "/kernel"], np.float64)).permute(3, 2, 0, 1).contiguous()
            h = F.relu(F.conv2d(h, k, torch.from_numpy(np.asarray(weights[name + "/bias"], np.float64)), padding=1))
            if i == 0:
                per = per + (h[:B] - h[B:]).abs().sum() * float(w[b])
        if b < len(VGG_BLOCKS) - 1:
            h = F.max_pool2d(h, 2)
    per.backward()
    g_bgr = x.grad[B:].permute(0, 2, 3, 1).numpy()
    return 255.0 * g_bgr[..., ::-1], float(per.detach())


def statement_grad64(res):
    """The statement's gradient before its float32 roundings, as d / d con_rgb."""
    return 255.0 * np.asarray(res["grad_input"], np.float64)[..., ::-1]


def autograd_difference(weights, gt, con_rgb):
    """max |statement - autograd| / max |autograd| in float64, and the autograd gradient."""
    want, _ = torch_grad(weights, gt, con_rgb)
    got = statement_grad64(host.per_loss_grad(weights, gt, con_rgb))
    return float(np.abs(got - want).max() / np.abs(want).max()), want


# ---- closed forms, written apart from the statement's own routines
def first_max_unpool(g, x):
    """g [N,h,h,C] through the 2 x 2 pool of x [N,2h,2h,C]: the window's positions in row-major order, the first largest takes it."""
    n, h, _, c = g.shape
    out = np.zeros(x.shape, g.dtype)
    best = np.full(g.shape, -np.inf)
    where = np.zeros(g.shape, np.int64)
    for j, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        v = x[:, dy::2, dx::2]
        better = v > best
        best, where = np.where(better, v, best), np.where(better, j, where)
    for j, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        out[:, dy::2, dx::2] = np.where(where == j, g, 0)
    return out


def one_tap_expected(acts, srcs, a, b, B, S):
    """The gradient at the network's input for cases.one_tap_weights(a, b): each layer sends its output's gradient back along the one
    tap, shifted the other way, and adds the output channels that read one input channel."""
    w = host.tap_weights(B, S)
    g = None
    for i in reversed(range(len(VGG_LAYERS))):
        name = VGG_LAYERS[i]
        y = np.asarray(acts[name], np.float64)
        if name in VGG_TAPS:
            yf = np.asarray(acts[name]).astype(f32)
            seed = np.sign(yf[B:] - yf[:B]).astype(np.float64) * float(w[VGG_TAPS.index(name)])
            g = seed if g is None else g + seed
        g = g * (y[B:] > 0)
        back = cases.shifted(g, 2 - a, 2 - b)                      # back[n, iy, ix] = g[n, iy - (a - 1), ix - (b - 1)]
        cin = 3 if i == 0 else VGG_BLOCKS[int(VGG_LAYERS[i - 1][5]) - 1][0]
        gx = np.zeros(back.shape[:3] + (cin,), np.float64)
        np.add.at(gx, (Ellipsis, srcs[name]), back)
        g = gx
        if i > 0 and name.endswith("conv1"):
            g = first_max_unpool(g, np.asarray(acts[VGG_LAYERS[i - 1]], np.float64)[B:])
    return (f32(255) * g.astype(f32)[..., ::-1])


def check_one_tap_layers(run, tap, S=32):
    a, b = cases.TAPS[tap]
    gt, con = cases.inputs(S, 1, 11 + tap)
    w, srcs = cases.one_tap_weights(a, b, 100 + tap)
    r = run(w, gt, con)
    want = one_tap_expected(r["acts"], srcs, a, b, 1, S)
    assert r["grad"].dtype == np.float32 and r["grad"].shape == (1, S, S, 3)
    assert np.abs(want).max() > 0, "the gradient must travel"
    np.testing.assert_array_equal(r["grad"], want, err_msg="tap (%d, %d)" % (a, b))
    return (w, gt, con), r


def check_tie_map(run, S=32):
    """Constant images under centre_weights: every feature is constant over the map, so every pooling window holds four equal positive
    values and its gradient must go to element (0, 0).  With fake > real everywhere the gradient at pixel (y, x) is
    255 (w_1 + [y, x even] (w_2 + [y, x multiples of 4] (w_3 + ...))) in each channel."""
    gt = np.full((1, S, S, 3), 0.6, f32)
    con = np.full((1, S, S, 3), 0.9, f32)
    r = run(cases.centre_weights(), gt, con)
    pre = host.preprocess(gt, con)
    assert (pre > 0).all() and (pre[1] > pre[0]).all()
    w = [float(v) for v in host.tap_weights(1, S)]
    yy, xx = np.meshgrid(np.arange(S), np.arange(S), indexing="ij")
    want = np.zeros((S, S))
    for k in reversed(range(host.K)):
        want = (want + w[k]) * ((yy % (1 << k) == 0) & (xx % (1 << k) == 0))
    want = np.repeat((255.0 * want)[None, :, :, None], 3, axis=3).astype(f32)
    assert len(np.unique(want)) == host.K
    np.testing.assert_array_equal(r["grad"], want)
    return (cases.centre_weights(), gt, con), r


def check_equal_images(run, S=32, B=2):
    """gt == con_rgb: every sign is 0 and the gradient is exactly 0."""
    gt, _ = cases.inputs(S, B, 23)
    for w in (cases.centre_weights(), cases.one_tap_weights(0, 2, 7)[0]):
        r = run(w, gt, gt.copy())
        assert r["grad"].shape == (B, S, S, 3) and not r["grad"].any() and r["loss"].tobytes() == f32(0).tobytes()


def check_item_order(run, weights, S=32, B=3):
    """The items in the other order give the gradient rows in the other order, bit for bit."""
    gt, con = inputs(S, B)
    r = run(weights, gt, con)
    rev = run(weights, np.ascontiguousarray(gt[::-1]), np.ascontiguousarray(con[::-1]))
    assert r["grad"][::-1].tobytes() == rev["grad"].tobytes() and r["grad"][0].tobytes() != r["grad"][1].tobytes()


def check_upstream(run, weights, S=32, B=3):
    """upstream = 0.005 (per_loss' weight in g_total_loss) is one float32 multiply of the gradient."""
    gt, con = inputs(S, B)
    plain = run(weights, gt, con)["grad"]
    scaled = run(weights, gt, con, upstream=np.array([0.005], f32))["grad"]
    assert np.abs(plain).max() > 0 and scaled.dtype == np.float32
    assert scaled.tobytes() == (plain * f32(0.005)).tobytes()
