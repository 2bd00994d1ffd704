"""Constructed inputs with closed-form answers for train_step's VGG19 perceptual term, shared by the host tests (test_perceptual_cpu.py)
and the device tests (test_perceptual_gpu.py).  Every `check_*` takes `run(weights, gt, con_rgb)` -> dict(loss [1], sums [B,5], acts:
{`input`, `block<b>_conv<i>`, `block<b>_pool`}) and asserts on what it returns.

The constructed kernels hold one 1.0 per output channel and zeros, the biases are 0: every product is x * 1 or x * 0 and every sum adds
zeros to one term, so a layer's output is exact in float32 (the device) and in float64 (the host statement) alike, and the two routes are
held to the same closed forms.  Values are compared as numbers: the device's ReLU, a median of {x, 0 x, FLT_MAX}, leaves a negative x as
-0, which equals the statement's 0."""
import numpy as np

from blindshadowremoval_amd import perceptual as host
from blindshadowremoval_amd.weights import VGG_BLOCKS, VGG_LAYERS, VGG_TAPS, vgg_variable_shapes

f32 = np.float32
TAPS = [(a, b) for a in range(3) for b in range(3)]
GPU_SIZES = ((32, 1), (32, 3), (64, 2), (128, 1))
SUM_REL = 1e-9            # float64 sums of at most 2^22 non-negative float32 terms taken in another order: 2^22 * 2^-53 = 5e-10
E2E_MEASURED = 3.6e-6          # the largest scaled error of a tapped feature measured on GPU_SIZES: block5_conv1 at S = 128 (tools/perceptual_bench.py --parity)
E2E_BOUND = min(4 * E2E_MEASURED, 1e-3)


def one_ulp_apart(a, b) -> bool:
    """float32 arrays: equal, or neighbours (of one sign)."""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    return bool(np.isfinite(a).all() and np.isfinite(b).all() and (np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)) <= 1).all())


def inputs(S, B, seed=0):
    return host.example_inputs(S, B, seed)


def layer_input_name(name):
    """The activation layer `name` reads."""
    i = VGG_LAYERS.index(name)
    if i == 0:
        return "input"
    b = int(name[5])
    return "block%d_pool" % (b - 1) if name.endswith("conv1") else VGG_LAYERS[i - 1]


def zero_weights():
    return {k: np.zeros(s, f32) for k, s in vgg_variable_shapes().items()}


def one_tap_weights(a, b, seed):
    """Every layer's kernel is 1 at tap (a, b) from input channel src[o] to output channel o, src a permutation of the output channels
    folded onto the input channels; biases 0.  -> (weights, {layer: src})."""
    rng = np.random.default_rng(seed)
    w, srcs = zero_weights(), {}
    for name in VGG_LAYERS:
        kern = w[name + "/kernel"]
        src = rng.permutation(kern.shape[3]) % kern.shape[2]
        kern[a, b, src, np.arange(kern.shape[3])] = 1
        srcs[name] = src
    return w, srcs


def shifted(prev, a, b):
    """prev [N,H,H,C] -> prev[n, oy + a - 1, ox + b - 1, c], 0 outside the map."""
    prev = np.asarray(prev)
    n, h, _, c = prev.shape
    pad = np.zeros((n, h + 2, h + 2, c), prev.dtype)
    pad[:, 1:1 + h, 1:1 + h] = prev
    return pad[:, a:a + h, b:b + h]


def check_one_tap_layers(run, tap, S=32):
    """Every layer's output is the ReLU of its own input, shifted by tap (a, b) with zeros in the padding and its channels rearranged;
    every pooled map is the 2 x 2 maximum of its input.  At S = 32 block 5 sees the 2 x 2 map."""
    a, b = TAPS[tap]
    gt, con = inputs(S, 1, 11 + tap)
    w, srcs = one_tap_weights(a, b, 100 + tap)
    acts = run(w, gt, con)["acts"]
    assert np.array_equal(acts["input"], host.preprocess(gt, con))
    for i, name in enumerate(VGG_LAYERS):
        prev = np.asarray(acts[layer_input_name(name)])
        got = np.asarray(acts[name])
        side = S >> (int(name[5]) - 1)
        assert got.shape == (2, side, side, VGG_BLOCKS[int(name[5]) - 1][0]), name
        want = np.maximum(shifted(prev, a, b)[..., srcs[name]], 0)
        np.testing.assert_array_equal(got, want.astype(got.dtype), err_msg="tap (%d, %d) %s" % (a, b, name))
    for blk in range(1, 5):
        np.testing.assert_array_equal(np.asarray(acts["block%d_pool" % blk]), host.max_pool(np.asarray(acts["block%d_conv%d" % (blk, VGG_BLOCKS[blk - 1][1])])))
    assert np.abs(acts["block2_conv1"]).max() > 0, "the signal must travel"
    assert acts["block5_conv1"].shape[1] == S // 16


def centre_weights():
    """Every layer passes its first three channels through the centre tap: kernel[1, 1, c, c] = 1 for c < 3."""
    w = zero_weights()
    for name in VGG_LAYERS:
        for c in range(3):
            w[name + "/kernel"][1, 1, c, c] = 1
    return w


def centre_expected(gt, con_rgb):
    """The five features' first three channels, the sums [B,5] and the loss of centre_weights, from numpy pooling alone."""
    B, S = gt.shape[:2]
    f = np.maximum(host.preprocess(gt, con_rgb), f32(0))
    feats = []
    for k in range(host.K):
        feats.append(f)
        f = host.max_pool(f)
    sums = np.stack([np.abs(x[:B] - x[B:]).reshape(B, -1).sum(axis=1, dtype=np.float64) for x in feats], axis=1)
    t = np.zeros(host.K)
    for row in sums:
        t = t + row
    m = [t[k] / (B * (S >> k) ** 2 * host.TAP_CH[k]) for k in range(host.K)]
    return feats, sums, np.array([(((m[0] + m[1]) + m[2]) + m[3]) + m[4]]).astype(f32)


def _check_centre(run, gt, con, label):
    feats, sums, loss = centre_expected(gt, con)
    r = run(centre_weights(), gt, con)
    for k, name in enumerate(VGG_TAPS):
        got = np.asarray(r["acts"][name])
        assert got.shape[-1] == host.TAP_CH[k] and got.dtype in (np.float32, np.float64)
        np.testing.assert_array_equal(got[..., :3], feats[k].astype(got.dtype), err_msg="%s %s" % (label, name))
        assert not got[..., 3:].any(), (label, name)
    assert r["sums"].shape == sums.shape and (np.abs(r["sums"] - sums) <= SUM_REL * sums).all() and (sums > 0).all(), (label, r["sums"], sums)
    assert one_ulp_apart(r["loss"], loss) and loss[0] > 0, (label, r["loss"], loss)
    return r


def check_centre_pass_through(run, S=32, B=2):
    """The five features are repeated 2 x 2 maxima of the ReLU of the preprocessed input in channels 0..2 and zero elsewhere: the
    routing of the taps and the divisors B h_k^2 C_k."""
    gt, con = inputs(S, B, 21)
    _check_centre(run, gt, con, "centre")


def check_out_of_range_con_rgb(run, S=32, B=2):
    """con_rgb below 0 and above 1 (a generator's output is not clipped): the preprocessing neither clips nor scales."""
    gt, con = inputs(S, B, 22)
    con = (con * f32(2) - f32(0.5)).astype(f32)
    assert con.min() < -0.25 and con.max() > 1.25
    _check_centre(run, gt, con, "out of range")


def check_equal_images(run, S=32, B=2):
    """gt == con_rgb: every sum and the loss are exactly 0."""
    gt, _ = inputs(S, B, 23)
    for w in (centre_weights(), one_tap_weights(0, 2, 7)[0]):
        r = run(w, gt, gt.copy())
        assert r["sums"].shape == (B, host.K) and not r["sums"].any() and r["loss"].tobytes() == f32(0).tobytes()
        assert np.abs(r["acts"]["block1_conv1"]).max() > 0


def check_item_order(run, S=32, B=3):
    """The items in the other order give the sum rows in the other order, bit for bit."""
    gt, con = inputs(S, B, 24)
    w = centre_weights()
    r = run(w, gt, con)
    rev = run(w, np.ascontiguousarray(gt[::-1]), np.ascontiguousarray(con[::-1]))
    assert r["sums"][::-1].tobytes() == rev["sums"].tobytes() and r["sums"][0].tobytes() != r["sums"][1].tobytes()
    assert one_ulp_apart(r["loss"], rev["loss"])


CONSTRUCTED = (check_centre_pass_through, check_out_of_range_con_rgb, check_equal_images, check_item_order)
