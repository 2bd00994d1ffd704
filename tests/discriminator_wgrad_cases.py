"""What the host tests (test_discriminator_wgrad_cpu.py, test_discriminator_wgrad_fixture.py) and the device tests
(test_discriminator_wgrad_gpu.py) of d d_total_loss / d the discriminators' variables share: the torch autograd restatement the
statement is held to, the scaled difference over all 54 variables, and constructed cases with closed-form answers.  Every `check_*`
takes `run(weights, gt, con_rgb, mask_sv)` -> dict(grads: name -> array in the variable's shape, acts: the forward's kept activations,
dtype: the arithmetic's type) and asserts on what it returns."""
import numpy as np

from blindshadowremoval_amd import discriminator as host
from blindshadowremoval_amd.weights import N_LAYER_D, discriminator_trainable_names, init_discriminator_weights

from discriminator_cases import inputs

f32 = np.float32
AUTOGRAD_SIZES = ((32, 1), (32, 3), (64, 2))
FIXTURE = (32, 2)                              # tests/golden/discriminator_wgrad_32.npz
AUTOGRAD_CAP = 1e-9
NAMES = discriminator_trainable_names()


def worst_scaled_diff(got, ref):
    """The largest of max |got[v] - ref[v]| / max |ref[v]| over the 54 variables (a variable whose reference is all 0 must be all 0),
    and the name it occurred at."""
    worst, at = 0.0, ""
    for name in NAMES:
        a, b = np.asarray(got[name], np.float64), np.asarray(ref[name], np.float64)
        assert a.shape == b.shape, name
        scale = np.abs(b).max()
        d = float(np.abs(a - b).max() / scale) if scale > 0 else (0.0 if not a.any() else np.inf)
        if d > worst:
            worst, at = d, name
    return worst, at


# ---- torch autograd in float64: F.conv2d on explicitly padded input, F.leaky_relu, the hinge as relu; parameters are leaves
def autograd_grads(weights, gt, con_rgb, mask_sv):
    """d (disc_real + disc_fake) / d every trainable variable by torch autograd in float64 from the float32 variables and the
    statement's float32 inputs of each discriminator (disc_input) and float32 w_k: name -> float64 array in the variable's shape."""
    import torch
    import torch.nn.functional as F
    t64 = lambda a: torch.from_numpy(np.asarray(a, np.float64))                      # noqa: E731
    B, S = np.asarray(gt).shape[:2]
    oihw = lambda n: n.endswith("/kernel")                                            # noqa: E731 (kernel leaves in torch's own layout, dense)
    leaves = {n: t64(np.ascontiguousarray(np.transpose(weights[n], (3, 2, 0, 1))) if oihw(n) else weights[n]).requires_grad_(True) for n in NAMES}
    total = torch.zeros((), dtype=torch.float64)
    for k, w_k in zip((1, 2, 3), host.seed_weights(B, S)):
        h = t64(host.disc_input(gt, con_rgb, mask_sv, k)).permute(0, 3, 1, 2)
        for i in range(N_LAYER_D):
            st = "discriminator_%d/conv_stack/%d/" % (k, i)
            before, after = host.same_pad(h.shape[2], 4, 2)
            h = F.conv2d(F.pad(h, (before, after, before, after)), leaves[st + "conv/kernel"], leaves[st + "conv/bias"], stride=2)
            g, beta = (leaves[st + "bnorm/" + p].reshape(1, -1, 1, 1) for p in ("gamma", "beta"))
            mean, var = (t64(weights[st + "bnorm/" + p]).reshape(1, -1, 1, 1) for p in ("moving_mean", "moving_variance"))
            inv = g / torch.sqrt(var + host.BN_EPS)
            h = F.leaky_relu(h * inv + (beta - mean * inv), host.LRELU_ALPHA)
        st = "discriminator_%d/conv2/conv/" % k
        before, after = host.same_pad(h.shape[2], 4, 1)
        out = F.conv2d(F.pad(h, (before, after, before, after)), leaves[st + "kernel"], leaves[st + "bias"])
        total = total + (F.relu(1 - out[:B]).sum() + F.relu(1 + out[B:]).sum()) * float(w_k)
    total.backward()
    return {n: np.ascontiguousarray(np.transpose(leaves[n].grad.numpy(), (2, 3, 1, 0))) if oihw(n) else leaves[n].grad.numpy() for n in NAMES}


# ---- closed forms
HEAD_BIASES = (2.0, -2.0, 0.5)


def constant_head_weights(seed=7):
    """Head kernels 0 and head biases 2, -2, 0.5: the logits are the biases.  Discriminator 1 (y = 2): the real term 1 - y = -1 is
    inactive, the fake term 3 active.  Discriminator 2 (y = -2): the real term alone.  Discriminator 3 (y = 0.5): both, and they cancel."""
    w = init_discriminator_weights(seed)
    for k in (1, 2, 3):
        w["discriminator_%d/conv2/conv/kernel" % k][:] = 0
        w["discriminator_%d/conv2/conv/bias" % k][:] = HEAD_BIASES[k - 1]
    return w


def padded_head_einsum(conv3, seed):
    """sum_{n, oy, ox} seed[n, oy, ox] x[n, oy + a - 1, ox + b - 1, c] over an explicitly padded x (1 before, 2 after): [4, 4, 64, 1]."""
    conv3, seed = np.asarray(conv3, np.float64), np.asarray(seed, np.float64)
    n, h, _, c = conv3.shape
    xp = np.pad(conv3, ((0, 0), (1, 2), (1, 2), (0, 0)))
    out = np.zeros((4, 4, c, 1))
    for a in range(4):
        for b in range(4):
            out[a, b, :, 0] = np.einsum("nyx,nyxc->c", seed, xp[:, a:a + h, b:b + h])
    return out


def check_constant_heads(run, S=32, B=2):
    """Head kernels 0 pass nothing down: all 48 non-head gradients are exactly 0.  The head-bias gradients are sums of 2 B h_k^2 seeds of
    one magnitude w_k: B h_k^2 w_k = +1 (the fake side alone; the product of a power of two count with float32(1 / count) is exact
    here), -1 (the real side alone) and 0 (both sides, a full cancel).  The head-kernel gradient is the einsum of the seed with the
    explicitly padded conv3 activation."""
    gt, con, mask = inputs(S, B, 13)
    w = constant_head_weights()
    r = run(w, gt, con, mask)
    grads = r["grads"]
    zeros = 0
    for name in NAMES:
        if "/conv2/" not in name:
            assert not np.asarray(grads[name]).any(), name
            assert np.asarray(grads[name]).shape == w[name].shape
            zeros += 1
    assert zeros == 48
    for k, w_k, want in zip((1, 2, 3), host.seed_weights(B, S), (1.0, -1.0, 0.0)):
        h = host.final_side(S, k)
        n = B * h * h
        assert float(w_k) * n == 1.0
        np.testing.assert_array_equal(np.asarray(grads["discriminator_%d/conv2/conv/bias" % k], np.float64), [want])
        seed = np.zeros((2 * B, h, h))
        if HEAD_BIASES[k - 1] < 1:
            seed[:B] = -float(w_k)
        if HEAD_BIASES[k - 1] > -1:
            seed[B:] = float(w_k)
        ref = padded_head_einsum(r["acts"]["d%d/conv3" % k], seed)
        got = np.asarray(grads["discriminator_%d/conv2/conv/kernel" % k], np.float64)
        assert got.shape == (4, 4, 64, 1) and np.abs(ref).max() > 0
        tol = 1e-12 if r["dtype"] is np.float64 else 1e-5
        assert np.abs(got - ref).max() <= tol * np.abs(ref).max(), k


CONSTRUCTED = (check_constant_heads,)
