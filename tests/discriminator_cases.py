"""Constructed inputs with closed-form answers for train_step's three discriminators and GAN losses, shared by the host tests
(test_discriminator_cpu.py) and the device tests (test_discriminator_gpu.py).  Every `check_*` takes `run(weights, gt, con_rgb, mask_sv)`
-> dict(losses [3], sums [B,9], logits: three maps [2B,h_k,h_k], acts: {`d{k}/in`, `d{k}/conv{i}`, `d{k}/out`}) and asserts on what it
returns.

The one-tap cases need BatchNormalization to be the identity bit for bit, on the host statement (unfolded, float64) and on the device
(folded into float32 weights) alike.  `identity_stack` sets gamma = 2^22 and moving_variance = 2^44 with beta, moving_mean and the bias
0: in float64 var + 1e-3 rounds back to 2^44 (1e-3 is below half a step there, 2^-9), its root is exactly 2^22, so the scale gamma /
sqrt(var + eps) is exactly 1.0 and fold_bn hands the device 1.0f.  A one-tap kernel then multiplies by 1 and adds 0, and the closed
form holds exactly on both routes."""
import numpy as np

from blindshadowremoval_amd import discriminator as host
from blindshadowremoval_amd.weights import N_LAYER_D, init_discriminator_weights

f32 = np.float32
TAPS = [(a, b) for a in range(4) for b in range(4)]
HINGE_SEED = 5            # the first seed from 1 on at which `hinge_condition` holds (S = 128, B = 2); the CPU suite re-checks it
HINGE_GAIN = 8.0
GPU_SIZES = ((32, 1), (32, 3), (64, 2), (128, 2), (256, 1))


def one_ulp_apart(a, b) -> bool:
    """float32 arrays: equal, or neighbours (of one sign)."""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    return bool(np.isfinite(a).all() and np.isfinite(b).all() and (np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)) <= 1).all())


def inputs(S, B, seed=0):
    return host.example_inputs(S, B, seed)


def identity_stack(weights):
    """The conv_stack layers' biases 0 and their BatchNormalization exactly the identity (the module docstring)."""
    w = {k: v.copy() for k, v in weights.items()}
    for name in w:
        if "/conv_stack/" not in name:
            continue
        leaf = name.rsplit("/", 1)[1]
        if leaf == "gamma":
            w[name][:] = f32(2.0 ** 22)
        elif leaf == "moving_variance":
            w[name][:] = f32(2.0 ** 44)
        elif leaf in ("bias", "beta", "moving_mean"):
            w[name][:] = 0
    return w


def shifted(prev, a, b, c, stride, out_side):
    """prev [N,H,H,C] -> [N,out_side,out_side]: prev[n, stride oy + a - 1, stride ox + b - 1, c], 0 outside the map (pad 1 before)."""
    prev = np.asarray(prev)
    n, h = prev.shape[0], prev.shape[1]
    pad = np.zeros((n, h + 5, h + 5), prev.dtype)
    pad[:, 1:1 + h, 1:1 + h] = prev[..., c]
    span = (out_side - 1) * stride + 1
    return pad[:, a:a + span:stride, b:b + span:stride]


def leaky(x):
    x = np.asarray(x)
    return np.where(x >= 0, x, x.dtype.type(0.3) * x)


def check_one_tap_layers(run, S=32):
    """Every stride-2 layer's kernel is 1 at one tap (a, b), one input channel and one output channel, for all 16 taps: its output is
    the preceding activation shifted and strided, zeros where the tap falls in the padding.  At S = 32 the third discriminator's
    layers see 8, 4, 2 and 1 pixels a side: even maps (pad 1, 1) and the 1 x 1 map (pad 1, 2)."""
    gt, con, mask = inputs(S, 1, 11)
    base = identity_stack(init_discriminator_weights(5))
    for t, (a, b) in enumerate(TAPS):
        w = {k: v.copy() for k, v in base.items()}
        chans = []
        cin = t % 6
        for i in range(N_LAYER_D):
            cout = (3 * t + i) % 32
            for k in (1, 2, 3):
                kern = w["discriminator_%d/conv_stack/%d/conv/kernel" % (k, i)]
                kern[:] = 0
                kern[a, b, cin, cout] = 1
            chans.append((cin, cout))
            cin = cout
        acts = run(w, gt, con, mask)["acts"]
        for k in (1, 2, 3):
            sides = host.map_sides(S, k)
            assert acts["d%d/in" % k].shape == (2, sides[0], sides[0], 6)
            for i, (cin, cout) in enumerate(chans):
                prev = acts["d%d/in" % k] if i == 0 else acts["d%d/conv%d" % (k, i - 1)]
                got = np.asarray(acts["d%d/conv%d" % (k, i)])
                want = np.zeros(got.shape, got.dtype)
                want[..., cout] = leaky(shifted(prev, a, b, cin, 2, sides[i + 1]).astype(got.dtype))
                label = "tap (%d, %d) d%d/conv%d" % (a, b, k, i)
                np.testing.assert_array_equal(got, want, err_msg=label)
        assert np.abs(acts["d1/conv1"]).max() > 0, "the signal must travel"


def check_one_tap_head(run, S=32):
    """The head's kernel is 1 at one tap and one input channel, its bias 0: the logits are the last activation shifted by (a - 1, b - 1),
    zeros in the padding (1 before, 2 after) — exactly, products with 1 and sums with 0 being exact."""
    gt, con, mask = inputs(S, 1, 12)
    base = init_discriminator_weights(6)
    for t, (a, b) in enumerate(TAPS):
        w = {k: v.copy() for k, v in base.items()}
        c = (5 * t + 3) % 64
        for k in (1, 2, 3):
            w["discriminator_%d/conv2/conv/kernel" % k][:] = 0
            w["discriminator_%d/conv2/conv/kernel" % k][a, b, c, 0] = 1
            w["discriminator_%d/conv2/conv/bias" % k][:] = 0
        r = run(w, gt, con, mask)
        for k in (1, 2, 3):
            prev = np.asarray(r["acts"]["d%d/conv3" % k])
            h = host.final_side(S, k)
            want = shifted(prev, a, b, c, 1, h)
            np.testing.assert_array_equal(np.asarray(r["logits"][k - 1]), want, err_msg="tap (%d, %d) d%d" % (a, b, k))
            np.testing.assert_array_equal(np.asarray(r["acts"]["d%d/out" % k])[..., 0], want)
            if h == 1:
                assert (want != 0).any() == ((a, b) == (1, 1))


def check_constant_heads(run, S=32, B=2):
    """Head kernels 0 and biases c_k that differ per discriminator: the logits equal c_k exactly and the losses follow in closed form —
    the weight sets reach their own scales and the divisors are B h_k^2."""
    gt, con, mask = inputs(S, B, 13)
    w = init_discriminator_weights(7)
    c = (0.5, -0.25, 2.0)
    for k in (1, 2, 3):
        w["discriminator_%d/conv2/conv/kernel" % k][:] = 0
        w["discriminator_%d/conv2/conv/bias" % k][:] = c[k - 1]
    r = run(w, gt, con, mask)
    want_sums = np.zeros((B, host.K))
    for k in (1, 2, 3):
        h = host.final_side(S, k)
        assert np.asarray(r["logits"][k - 1]).shape == (2 * B, h, h)
        np.testing.assert_array_equal(np.asarray(r["logits"][k - 1]), np.full((2 * B, h, h), c[k - 1]))
        want_sums[:, 3 * (k - 1):3 * k] = [h * h * max(0.0, 1 - c[k - 1]), h * h * max(0.0, 1 + c[k - 1]), h * h * c[k - 1]]
    np.testing.assert_array_equal(r["sums"], want_sums)
    want = np.array([(-c[0] - c[1]) - c[2], sum(max(0.0, 1 - v) for v in c), sum(max(0.0, 1 + v) for v in c)], np.float64).astype(f32)
    np.testing.assert_array_equal(r["losses"], want)


def check_equal_images(run, S=32, B=2):
    """gt == con_rgb: the real and the fake logits are the same bits (the batch order, and mask_sv under both halves); and the items
    in the other order give the rows in the other order."""
    gt, _, mask = inputs(S, B, 14)
    w = init_discriminator_weights(8)
    r = run(w, gt, gt.copy(), mask)
    rev = run(w, np.ascontiguousarray(gt[::-1]), np.ascontiguousarray(gt[::-1]), np.ascontiguousarray(mask[::-1]))
    for k in range(3):
        y, z = np.asarray(r["logits"][k]), np.asarray(rev["logits"][k])
        assert y[:B].tobytes() == y[B:].tobytes() and np.abs(y).max() > 0
        assert y[:B][::-1].tobytes() == z[:B].tobytes() and y[0].tobytes() != y[1].tobytes()
    assert (r["sums"][:, [2, 5, 8]] != 0).all()


def hinge_weights(seed):
    w = init_discriminator_weights(seed)
    for k in (1, 2, 3):
        w["discriminator_%d/conv2/conv/kernel" % k] *= f32(HINGE_GAIN)
    return w


def hinge_condition(logits, B) -> bool:
    """By the float64 statement: each of the six hinge terms has an active and an inactive logit, and no logit lies within 1e-3 of +-1."""
    for y in logits:
        y = np.asarray(y, np.float64)
        if np.abs(np.abs(y) - 1).min() <= 1e-3:
            return False
        real, fake = 1 - y[:B] > 0, 1 + y[B:] > 0
        if real.all() or not real.any() or fake.all() or not fake.any():
            return False
    return True


def hinge_case(seed=HINGE_SEED, S=128, B=2):
    """(weights, gt, con_rgb, mask_sv) of the hinge case."""
    return (hinge_weights(seed),) + tuple(inputs(S, B, seed))


def find_hinge_seed(S=128, B=2, first=1, tries=64):
    for seed in range(first, first + tries):
        args = hinge_case(seed, S, B)
        if hinge_condition(host.logits_of(host.forward(*args)), B):
            return seed
    raise AssertionError("no seed in %d..%d gives the hinge condition" % (first, first + tries - 1))


CONSTRUCTED = (check_one_tap_head, check_constant_heads, check_equal_images)
