"""What the host tests (test_heads_grad_cpu.py) and the device tests (test_heads_grad_gpu.py) of the backward of the generator's grey
heads share: seeded weights and inputs, the torch autograd restatement the statement is held to, the scaled difference over the five
outputs, the bounds, and constructed cases with closed-form answers.  Every `check_*` takes
`run(weights, inputs, y, d_gs)` -> dict(the five outputs by name, the stage maps `g_m`, `g_con`, `mask` as used, `dtype`: the
arithmetic's type).  A `run` differentiates the forward as float32 rounds its mask: the device's hands the chain the mask22 of the
statement's own forward (`mask22_of`), the host's float64 one the same mask through `acts`."""
import numpy as np

from blindshadowremoval_amd import generator_grad as host
from blindshadowremoval_amd.weights import generator_heads_trainable_names, init_weights

f32 = np.float32
NAMES = tuple(generator_heads_trainable_names())
K2, B2, K3, B3 = NAMES
OUTPUTS = ("d_y",) + NAMES
AUTOGRAD_SIZES = ((1, 4, 1), (5, 3, 2), (8, 32, 1), (9, 7, 3))      # (H, W, B): images narrower and wider than the 7-tap window
# the largest scaled difference between the statement and autograd over AUTOGRAD_SIZES, measured on the CPU
# (test_heads_grad_cpu.py prints each figure)
AUTOGRAD_MEASURED = 1.38e-15           # conv2/conv/kernel at (8, 32, 1); 2.65e-16, 3.08e-16, 1.12e-15 at (1, 4, 1), (5, 3, 2), (9, 7, 3)
AUTOGRAD_CAP = 1e-9
AUTOGRAD_BOUND = min(4 * AUTOGRAD_MEASURED, AUTOGRAD_CAP)
STAGE_BUDGET = 1e-5                # the project's fp32-class stage budget (tests/stage_parity.py)
# (8, 32, 1): one tile, the 3-pixel halo meets both borders at once; (16, 32, 2): an image seam inside one slice's tiles; (8, 64, 1) and
# (24, 96, 3): more than one tile each way; (24, 96, 3) has 27 tiles in 14 slices and (40, 32, 1) 5 tiles in 3: more than one slice and
# a tile count that is no multiple of the slice count (test_heads_bindings_cpu.py holds bsr_heads_grad_partials to these figures)
GPU_SIZES = ((8, 32, 1), (16, 32, 2), (8, 64, 1), (24, 96, 3), (40, 32, 1))
SLICES = {(8, 32, 1): (1, 1), (16, 32, 2): (4, 2), (8, 64, 1): (2, 1), (24, 96, 3): (27, 14), (40, 32, 1): (5, 3)}      # (tiles, slices)
# the largest scaled error of an output of the device chain against heads_grad(acts = the device's own mask), measured on an MI355X
# over GPU_SIZES (tools/heads_grad_bench.py --parity, profiles/heads_grad_bench.json)
E2E_MEASURED = 4.21e-7        # d_y at (24, 96, 3); 3.07e-7, 2.94e-7, 3.09e-7, 3.69e-7 at the other four sizes in GPU_SIZES' order, all at d_y
E2E_BOUND = min(4 * E2E_MEASURED, 1e-3)

_weights = {}


def heads_weights(seed=3, variant="gsc"):
    """init_weights(seed).  Cached: treat as read-only."""
    if (seed, variant) not in _weights:
        _weights[(seed, variant)] = init_weights(seed, variant=variant)
    return _weights[(seed, variant)]


def case(H, W, B, seed=0):
    """(weights, inputs, y, d_gs) at a size."""
    inputs, y, d_gs = host.heads_example_inputs(H, W, B, seed)
    return heads_weights(), inputs, y, d_gs


def mask22_of(weights, inputs, y):
    """The forward's mask22 [B,H,W,3] = [relu(mask), 0, relu(-mask)] float32 of the statement's own forward, mask = tanh(m) rounded to
    float32: what the device chain reads its mask from."""
    mask = host.heads_forward(weights, inputs, y)["mask"].astype(f32)
    return np.concatenate([np.maximum(mask, f32(0)), np.zeros_like(mask), np.maximum(-mask, f32(0))], axis=3)


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


# ---- torch autograd in float64, written from the reference's semantics (model.py:246-250): conv2d with padding 3, tanh, the grey
# weights of tf.image.rgb_to_grayscale; the four variables and y are leaves
def autograd_grads(weights, inputs, y, d_gs):
    """d <d_gs, gs> / d each of the four variables and y by torch autograd in float64 from the float32 variables: name -> float64 array
    in the variable's shape, `d_y` [B,H,W,64], and `m` [B,H,W,1] the mask head's pre-activation."""
    import torch
    import torch.nn.functional as F
    t64 = lambda a: torch.from_numpy(np.array(a, np.float64))                        # noqa: E731
    # the kernels are leaves in torch's own OIHW order (conv2d's backward wants them contiguous), turned back below
    leaves = {n: (t64(weights[n]).permute(3, 2, 0, 1).contiguous() if n.endswith("kernel") else t64(weights[n])).requires_grad_(True)
              for n in NAMES}
    yt = t64(y).requires_grad_(True)
    t = yt.permute(0, 3, 1, 2)
    m = F.conv2d(t, leaves[K2], leaves[B2], padding=3)
    con = F.conv2d(t, leaves[K3], leaves[B3], padding=3)
    x = np.asarray(inputs, f32)
    w = [f32(v) for v in (0.2989, 0.5870, 0.1140)]              # tf.image.rgb_to_grayscale in float32, as the forward computes it
    gray = t64((x[..., 0] * w[0] + x[..., 1] * w[1]) + x[..., 2] * w[2])[:, None]
    gs = gray * (1 + torch.tanh(m)) + con
    (gs.permute(0, 2, 3, 1) * t64(d_gs)).sum().backward()
    res = {n: (v.grad.permute(2, 3, 1, 0).numpy() if n.endswith("kernel") else v.grad.numpy()) for n, v in leaves.items()}
    res["d_y"] = yt.grad.numpy()
    res["m"] = m.detach().permute(0, 2, 3, 1).numpy()
    return res


# ---- closed forms
def _same(what, got, want):
    np.testing.assert_array_equal(np.asarray(got, np.float64), np.asarray(want, np.float64), err_msg=what)


def _zero(r, names):
    for name in names:
        assert not np.asarray(r[name]).any(), name


def _with(wt, **changes):
    out = dict(wt)
    for name, value in changes.items():
        full = {"K2": K2, "b2": B2, "K3": K3, "b3": B3}[name]
        out[full] = np.full_like(wt[full], value)
    return out


def check_zero_d_gs(run, H=8, W=32, B=1):
    """(a) d_gs = 0: everything is exactly 0."""
    wt, inputs, y, d_gs = case(H, W, B, 5)
    r = run(wt, inputs, y, np.zeros_like(d_gs))
    for name in NAMES:
        assert np.asarray(r[name]).shape == wt[name].shape, name
    _zero(r, OUTPUTS + ("g_m", "g_con"))


def check_saturated_mask(run, H=8, W=32, B=1):
    """(b) b2 = 20: mask is exactly 1, so g_m, d K2 and d b2 are exactly 0, and d_y and d K3 equal those of K2 = 0."""
    wt, inputs, y, d_gs = case(H, W, B, 6)
    r = run(_with(wt, b2=20.0), inputs, y, d_gs)
    _same("mask", r["mask"], np.ones_like(np.asarray(r["mask"])))
    _zero(r, ("g_m", K2, B2))
    r0 = run(_with(wt, K2=0.0), inputs, y, d_gs)
    assert np.asarray(r0["g_m"]).any() and np.asarray(r["d_y"]).any()
    for name in ("d_y", K3, B3):
        _same(name, r[name], r0[name])


def check_zero_inputs(run, H=8, W=32, B=1):
    """(c) inputs = 0: gray = 0 and the same zeros as (b)."""
    wt, inputs, y, d_gs = case(H, W, B, 7)
    r = run(wt, np.zeros_like(inputs), y, d_gs)
    assert (np.abs(np.asarray(r["mask"])) < 1).all()
    _zero(r, ("g_m", K2, B2))
    r0 = run(_with(wt, K2=0.0), np.zeros_like(inputs), y, d_gs)
    assert np.asarray(r["d_y"]).any()
    for name in ("d_y", K3, B3):
        _same(name, r[name], r0[name])


def check_zero_kernels(run, H=8, W=32, B=1):
    """(d) K2 = K3 = 0 (and b2 = 0): d_y is exactly 0, mask = 0 and g_m = d_gs gray."""
    from blindshadowremoval_amd.train_losses import gray
    wt, inputs, y, d_gs = case(H, W, B, 8)
    r = run(_with(wt, K2=0.0, K3=0.0, b2=0.0), inputs, y, d_gs)
    _zero(r, ("d_y", "mask"))
    T = r["dtype"]
    _same("g_m", r["g_m"], d_gs.astype(T) * gray(inputs)[..., None].astype(T))
    assert np.asarray(r[K2]).any() and np.asarray(r[K3]).any()


def _single_pixel(run, H, W, corner):
    wt, inputs, y, d_gs = case(H, W, 2, 9)
    img, i, j = (1, 0, 0) if corner == 0 else (0, H - 1, W - 1)
    one = np.zeros_like(d_gs)
    one[img, i, j] = d_gs[img, i, j]
    r = run(wt, inputs, y, one)
    d_y = np.asarray(r["d_y"])
    assert not d_y[1 - img].any()
    support = np.abs(d_y[img]).max(axis=2) > 0
    want = np.zeros((H, W), bool)
    if corner == 0:
        want[:4, :4] = True
    else:
        want[H - 4:, W - 4:] = True
    np.testing.assert_array_equal(support, want)
    dead = 0
    for name in (K2, K3):
        dk = np.asarray(r[name])
        for a in range(7):
            for b in range(7):
                outside = (a < 3 or b < 3) if corner == 0 else (a > 3 or b > 3)
                assert dk[a, b].any() == (not outside), (name, a, b)
                dead += outside
    assert dead == 2 * 33


def check_single_pixel_top_left(run, H=8, W=32):
    """(e) d_gs is the single pixel (0, 0) of image 1 of 2: d_y of image 0 is exactly 0, image 1's support is rows 0..3 by columns 0..3,
    and the 33 taps of d K2 and of d K3 with a < 3 or b < 3 (which would read y above or left of the image, or the end of image 0) are
    exactly 0; the other 16 are not."""
    _single_pixel(run, H, W, 0)


def check_single_pixel_bottom_right(run, H=8, W=32):
    """(f) the mirror: the pixel (H - 1, W - 1) of image 0; taps with a > 3 or b > 3 are 0 and image 1 is 0."""
    _single_pixel(run, H, W, 1)


def check_ones(run, H=8, W=32, B=2):
    """(g) y = 1, d_gs = 1: d K3[a, b, c] = B (H - |a - 3|) (W - |b - 3|) exactly (the pixels whose tap lies inside the image; integers far
    below 2^24), d b3 = B H W."""
    wt, inputs, y, d_gs = case(H, W, B, 10)
    r = run(wt, inputs, np.ones_like(y), np.ones_like(d_gs))
    a = np.arange(7)
    want = B * np.maximum(H - np.abs(a - 3), 0)[:, None] * np.maximum(W - np.abs(a - 3), 0)[None, :]
    _same("d K3", r[K3], np.broadcast_to(want[:, :, None, None], (7, 7, 64, 1)))
    _same("d b3", r[B3], [B * H * W])


def check_the_con_head_knows_nothing_of_the_mask(run, H=8, W=32, B=1):
    """(h) d K3, d b3 and the con head's share of d_y (d_y at K2 = 0) do not depend on inputs or mask22, by a bit."""
    wt, inputs, y, d_gs = case(H, W, B, 11)
    r = run(_with(wt, K2=0.0), inputs, y, d_gs)
    r2 = run(_with(wt, K2=0.0, b2=-0.7), (1 - inputs).astype(f32), y, d_gs)
    assert not np.array_equal(np.asarray(r2["g_m"]), np.asarray(r["g_m"])) and not np.array_equal(np.asarray(r2["mask"]), np.asarray(r["mask"]))
    assert np.asarray(r["d_y"]).any()
    for name in ("d_y", K3, B3, "g_con"):
        _same(name, r2[name], r[name])


CONSTRUCTED = (check_zero_d_gs, check_saturated_mask, check_zero_inputs, check_zero_kernels, check_single_pixel_top_left,
               check_single_pixel_bottom_right, check_ones, check_the_con_head_knows_nothing_of_the_mask)
