"""Constructed inputs with closed-form answers for d gen / d con_rgb through the three discriminators, shared by the host tests
(test_discriminator_grad_cpu.py) and the device tests (test_discriminator_grad_gpu.py), and the torch autograd restatement the
statement is held to.  Every `check_*` takes `run(weights, gt, con_rgb, mask_sv, upstream=None)` -> dict(grad [B,S,S,3], acts:
{`d{k}/conv{i}`: the forward's kept activations [2B,.,.,C]}, dtype: the arithmetic's type) and asserts on what it returns, bit for
bit: the host statement works in float64, the device in float32, and each closed form is evaluated in `dtype` in the route's own
order of operations (every sum in these cases has at most one term that is not 0)."""
import numpy as np

from blindshadowremoval_amd import discriminator as host
from blindshadowremoval_amd.weights import N_LAYER_D, init_discriminator_weights

from discriminator_cases import TAPS, identity_stack, inputs

f32 = np.float32
AUTOGRAD_SIZES = ((32, 1), (32, 3), (64, 2))
GPU_SIZES = ((32, 1), (32, 3), (64, 2), (128, 1))
FIXTURES = ((32, 2), (64, 1))                 # tests/golden/discriminator_grad_<S>.npz
AUTOGRAD_CAP = 1e-9
E2E_MEASURED = 6.6e-7          # the largest scaled error of grad measured on GPU_SIZES: S = 32, B = 1 (tools/discriminator_bench.py --grad --parity)
E2E_BOUND = min(4 * E2E_MEASURED, 1e-3)


def scaled_diff(a, b) -> float:
    """max |a - b| / max |b|."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


# ---- torch autograd in float64: F.conv2d on explicitly padded input, F.leaky_relu, F.interpolate(bilinear, align_corners=False)
def autograd_grad(weights, gt, con_rgb, mask_sv):
    """d gen / d con_rgb by torch autograd in float64 from the float32 variables, with the statement's float32 w_k: float64 [B,S,S,3]."""
    import torch
    import torch.nn.functional as F
    t64 = lambda a: torch.from_numpy(np.asarray(a, np.float64))                      # noqa: E731
    con = t64(con_rgb).requires_grad_(True)
    B, S = con.shape[:2]
    x = torch.cat([con, t64(mask_sv)], dim=3).permute(0, 3, 1, 2)                    # the fake rows, NCHW
    gen = torch.zeros((), dtype=torch.float64)
    for k, w_k in zip((1, 2, 3), host.seed_weights(B, S)):
        ds = host.DOWNSIZE[k - 1]
        h = x if ds == 1 else F.interpolate(x, size=(S // ds, S // ds), mode="bilinear", align_corners=False)
        for i in range(N_LAYER_D):
            st = "discriminator_%d/conv_stack/%d/" % (k, i)
            before, after = host.same_pad(h.shape[2], 4, 2)
            h = F.conv2d(F.pad(h, (before, after, before, after)), t64(weights[st + "conv/kernel"]).permute(3, 2, 0, 1), t64(weights[st + "conv/bias"]), stride=2)
            g, beta, mean, var = (t64(weights[st + "bnorm/" + p]).reshape(1, -1, 1, 1) for p in ("gamma", "beta", "moving_mean", "moving_variance"))
            inv = g / torch.sqrt(var + host.BN_EPS)
            h = F.leaky_relu(h * inv + (beta - mean * inv), host.LRELU_ALPHA)
        st = "discriminator_%d/conv2/conv/" % k
        before, after = host.same_pad(h.shape[2], 4, 1)
        out = F.conv2d(F.pad(h, (before, after, before, after)), t64(weights[st + "kernel"]).permute(3, 2, 0, 1), t64(weights[st + "bias"]))
        gen = gen - out.sum() * float(w_k)
    gen.backward()
    return con.grad.numpy()


# ---- a scatter-add written apart from the statement
def scatter_stride(g, a, b, stride, side):
    """g [N,ho,ho] at a convolution's output -> [N,side,side] at its input through the one tap (a, b), pad 1 before: out[stride oy + a - 1,
    stride ox + b - 1] = g[oy, ox] where that lies inside the map."""
    g = np.asarray(g)
    out = np.zeros((g.shape[0], side, side), g.dtype)
    for oy in range(g.shape[1]):
        for ox in range(g.shape[2]):
            iy, ix = stride * oy + a - 1, stride * ox + b - 1
            if 0 <= iy < side and 0 <= ix < side:
                out[:, iy, ix] = g[:, oy, ox]
    return out


def slope(y, dtype):
    return np.where(np.asarray(y) > 0, dtype(1), dtype(0.3))


def upsample(g, ds):
    """resize's transpose, written with loops: [N,s,s] -> [N,s ds,s ds]."""
    g = np.asarray(g)
    n, s = g.shape[:2]
    out = np.zeros((n, s * ds, s * ds), g.dtype)
    if ds == 1:
        return g.copy()
    for y in range(s * ds):
        for x in range(s * ds):
            if ds == 2 or (y % 4 in (1, 2) and x % 4 in (1, 2)):
                out[:, y, x] = g.dtype.type(0.25) * g[:, y // ds, x // ds]
    return out


def one_tap_weights(base, a, b, t, head_tap):
    """Every stride-2 layer's kernel 1 at tap (a, b), one input and one output channel per layer (discriminator_cases' choice), the
    head's kernel 1 at `head_tap` on the last layer's output channel.  -> (weights, [(cin, cout)] per layer)."""
    w = {k: v.copy() for k, v in base.items()}
    chans, cin = [], t % 3
    for i in range(N_LAYER_D):
        cout = (3 * t + i) % 32
        for k in (1, 2, 3):
            kern = w["discriminator_%d/conv_stack/%d/conv/kernel" % (k, i)]
            kern[:] = 0
            kern[a, b, cin, cout] = 1
        chans.append((cin, cout))
        cin = cout
    for k in (1, 2, 3):
        kern = w["discriminator_%d/conv2/conv/kernel" % k]
        kern[:] = 0
        kern[head_tap[0], head_tap[1], cin, 0] = 1
    return w, chans


def one_tap_want(r, chans, a, b, head_tap, B, S):
    """The closed form of the one-tap case from the route's own kept activations, in the route's dtype and order."""
    dt = r["dtype"]
    want = np.zeros((B, S, S, 3), dt)
    total = None
    for k, w_k in zip((1, 2, 3), host.seed_weights(B, S)):
        sides = host.map_sides(S, k)
        g = np.full((B, sides[-1], sides[-1]), -dt(w_k), dt)
        g = scatter_stride(g, head_tap[0], head_tap[1], 1, sides[N_LAYER_D])
        for i in reversed(range(N_LAYER_D)):
            y = np.asarray(r["acts"]["d%d/conv%d" % (k, i)])[B:, :, :, chans[i][1]]
            g = scatter_stride(g * slope(y, dt), a, b, 2, sides[i])
        up = upsample(g, host.DOWNSIZE[k - 1])
        total = up if total is None else total + up
    want[..., chans[0][0]] = total
    return want


def check_one_tap(run, S=32):
    """All four layers and the head are one-tap kernels with the exact BatchNormalization identity, for each of the 16 taps (the
    head's tap runs through the 16 as well): the gradient is -w_k carried back through the taps' index maps, the kept outputs' slopes
    and the resizes.  At S = 32 discriminator 3's last maps are 1 x 1."""
    gt, con, mask = inputs(S, 1, 11)
    base = identity_stack(init_discriminator_weights(5))
    travelled = 0
    for t, (a, b) in enumerate(TAPS):
        head_tap = TAPS[(5 * t + 5) % 16]
        w, chans = one_tap_weights(base, a, b, t, head_tap)
        r = run(w, gt, con, mask)
        want = one_tap_want(r, chans, a, b, head_tap, 1, S)
        np.testing.assert_array_equal(np.asarray(r["grad"]), want, err_msg="tap (%d, %d), head tap %s" % (a, b, head_tap))
        travelled += int(np.abs(want).max() > 0)
    assert travelled >= 8, "the signal must travel"


def check_zero_heads(run, S=32, B=2):
    """Head kernels 0: the gradient is exactly 0."""
    gt, con, mask = inputs(S, B, 13)
    w = init_discriminator_weights(7)
    for k in (1, 2, 3):
        w["discriminator_%d/conv2/conv/kernel" % k][:] = 0
    g = np.asarray(run(w, gt, con, mask)["grad"])
    assert g.shape == (B, S, S, 3) and not g.any()


def check_gt_ignored(run, S=32, B=2):
    """Changing gt leaves every bit of grad."""
    gt, con, mask = inputs(S, B, 14)
    w = init_discriminator_weights(8)
    g = np.asarray(run(w, gt, con, mask)["grad"])
    other = np.asarray(run(w, np.ascontiguousarray(gt[::-1] * f32(0.5)), con, mask)["grad"])
    assert g.tobytes() == other.tobytes() and np.abs(g).max() > 0


def check_items_reversed(run, S=32, B=3):
    """Items reversed give rows reversed."""
    gt, con, mask = inputs(S, B, 15)
    w = init_discriminator_weights(9)
    g = np.asarray(run(w, gt, con, mask)["grad"])
    rev = np.asarray(run(w, *(np.ascontiguousarray(v[::-1]) for v in (gt, con, mask)))["grad"])
    assert g[::-1].tobytes() == rev.tobytes() and g[0].tobytes() != g[1].tobytes()


def only_discriminator(weights, k):
    """The head kernels of the other two discriminators 0."""
    w = {n: v.copy() for n, v in weights.items()}
    for j in (1, 2, 3):
        if j != k:
            w["discriminator_%d/conv2/conv/kernel" % j][:] = 0
    return w


def check_downsize_patterns(run, S=32, B=1):
    """One discriminator at a time: downsize 1 is some dense g; downsize 2 puts one value 0.25 g on all four pixels of each 2 x 2 block;
    downsize 4 on the middle four of each 4 x 4 block, with exact zeros on the other twelve."""
    gt, con, mask = inputs(S, B, 16)
    base = init_discriminator_weights(10)
    for k, ds in zip((1, 2, 3), host.DOWNSIZE):
        g = np.asarray(run(only_discriminator(base, k), gt, con, mask)["grad"])
        assert np.abs(g).max() > 0
        if ds == 1:
            continue
        blocks = g.reshape(B, S // ds, ds, S // ds, ds, 3)
        lo = 0 if ds == 2 else 1
        mid = blocks[:, :, lo:lo + 2, :, lo:lo + 2]
        first = mid[:, :, :1, :, :1]
        np.testing.assert_array_equal(mid, np.broadcast_to(first, mid.shape))
        rest = blocks.copy()
        rest[:, :, lo:lo + 2, :, lo:lo + 2] = 0
        assert not rest.any()
        assert len(np.unique(first)) > 8, "the blocks differ from one another"


def check_upstream(run, S=32, B=2):
    """upstream = 0.005 equals the float32 product of the float32 gradient with float32(0.005)."""
    gt, con, mask = inputs(S, B, 17)
    w = init_discriminator_weights(11)
    g = np.asarray(run(w, gt, con, mask)["grad"])
    up = np.asarray(run(w, gt, con, mask, upstream=f32(0.005))["grad"])
    np.testing.assert_array_equal(up.astype(f32), g.astype(f32) * f32(0.005))
    assert up.astype(f32).astype(up.dtype).tobytes() == up.tobytes()


CONSTRUCTED = (check_one_tap, check_zero_heads, check_gt_ignored, check_items_reversed, check_downsize_patterns, check_upstream)
