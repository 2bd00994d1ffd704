"""The three multi-scale patch discriminators of the reference's `train_step` and its three GAN losses as a host statement: `gen`,
`disc_real` and `disc_fake` (train_test_GSC.py:121-123, 264-268, 302, 334-336, 353-355; model.py:115-147, 292-312; utils.py:100-102),
restated in numpy for training=False.  It plays the role for csrc/disc_kernels.h (bsr_disc_losses, discriminator_gpu.Discriminators)
that train_losses.py plays for its chain.  The VGG perceptual term, g_total_loss (objective.py), training=True (batch statistics, dropout), the
generator's backward and the optimisers are not here.

INPUTS.  gt, con_rgb (deshadow_img_c), mask_sv [B,S,S,3] float32; S in SIZES, B in 1..32767.  The variables are float32
(weights.discriminator_variable_shapes).

THE INPUT.  x = concat([concat([gt, con_rgb], axis 0), concat([mask_sv, mask_sv], axis 0)], axis 3): [2B,S,S,6], rows [0, B) real,
rows [B, 2B) fake, channels [image 3 | mask_sv 3].  Discriminator k = 1, 2, 3 (downsize 1, 2, 4) first resizes x to S // downsize:
tf.image.resize, bilinear, half-pixel centres, no antialiasing, in ucb_post.resize_bilinear's float32 arithmetic.  At these ratios an
output pixel is one lerp of 0.5 per axis: top = tl + (tr - tl) * .5, bottom = bl + (br - bl) * .5, out = top + (bottom - top) * .5 of
the pixels (2y, 2x) .. (2y + 1, 2x + 1) for downsize 2 and (4y + 1, 4x + 1) .. (4y + 2, 4x + 2) for downsize 4.

THE LAYERS (float64 arithmetic from the float32 input and variables).  Four Conv(n_ch[i], ksize 4, stride 2, norm 'batch'), n_ch = 32,
32, 64, 64, then conv2 = Conv(1, ksize 4, stride 1, no norm, no activation):
  Conv2D SAME    out = ceil(in / s) per axis; total = max((out - 1) s + 4 - in, 0), before = total // 2, the rest after (same_pad):
                 stride 2 on an even size pads 1, 1; on a 1 x 1 map 1, 2; the stride-1 head always 1, 2.  Cross-correlation with the HWIO
                 kernel, y[n, oy, ox, o] = sum_{a, b, c} x[n, s oy + a - before, s ox + b - before, c] k[a, b, c, o] + bias[o], positions
                 outside the map reading 0.
  BatchNormalization (moving statistics, eps 1e-3)    inv = gamma / sqrt(moving_variance + eps);  y * inv + (beta - moving_mean * inv)
  LeakyReLU(0.3)                                        y if y >= 0 else 0.3 y
At S = 32 the third discriminator's maps are 8, 4, 2, 1, 1 on a side; the final map of discriminator k has side h_k = max(S / (16
downsize), 1).  `forward` returns every activation: `d{k}/in` float32 [2B,s,s,6], `d{k}/conv{i}` float64 [2B,.,.,n_ch[i]], `d{k}/out`
float64 [2B,h_k,h_k,1].

THE LOSSES.  The output is split in two along the batch: real = out[:B], fake = out[B:].  With y the float32 logits:
  hinge(y, +1) terms   max(0, 1 - y), `1 - y` rounded once to float32;   hinge(y, -1) terms   max(0, 1 + y), likewise
Every sum is a float64 sum of float32 terms, kept per item as a row of DISC_SUM_NAMES: per discriminator hinge_real (over the real
row of the item), hinge_fake and fake (the plain sum of the fake logits): [B, 9].  The losses are formed from the batch totals t (the
items' rows added in order) in float64 and rounded once to float32; the divisor of discriminator k is n_k = B h_k^2:
  m_k = t[fake_k] / n_k;  gen = (-m_1 - m_2) - m_3
  disc_real = (t[hinge_real_1] / n_1 + t[hinge_real_2] / n_2) + t[hinge_real_3] / n_3;  disc_fake the same over hinge_fake.

WHAT IS NOT PINNED.  TensorFlow convolves and reduces in float32 in orders of its own; tests/golden/discriminator_*.npz holds the
reference's Discriminator, Conv and hinge_loss and train_step's statements executed over a numpy stand-in
(tools/make_discriminator_fixture.py), and tests/test_discriminator_fixture.py holds this statement to it.

THE BACKWARD: d gen / d con_rgb (`gen_grad`, csrc/disc_grad_kernels.h, Discriminators.gen_grad).  For the generator's update the
discriminators are constants and gt and mask_sv are data, so the data gradient with respect to con_rgb is the whole backward of the
term; only the rows [B, 2B) are differentiated.  `gen_grad`'s docstring writes every operation out; it is pinned to this restatement
of TensorFlow's gradient definitions (Conv2DBackpropInput, the moving-statistics BatchNormalization, LeakyReluGrad, the transpose of
the bilinear resize) and tests/golden/discriminator_grad_*.npz holds torch autograd's float64 gradient of the same objective
(tools/make_discriminator_grad_fixture.py).

`python -m blindshadowremoval_amd.discriminator FOLDER [--ckpt DIR] [--batch N] [--host] [--grad] [--wgrad]` scores the three terms on a folder written
by `python -m blindshadowremoval_amd.shadow_synth`, with the folder handling and the loop all three commands share (objective.folder_steps, objective.score_steps): the
generator runs on row 0 of each element and its con_rgb is the fake image.  The weights of the generator and of the discriminators
come from the latest checkpoint under --ckpt, from init_weights / init_discriminator_weights without it.  The step-weighted means
are printed as Logging.display prints them.  --host computes the three terms with this statement from the same generator outputs.
With --grad each batch's line also carries gen_grad_l1 and gen_grad_linf, the L1 and L-infinity norms of d gen / d con_rgb
(Discriminators.gen_grad; --host: gen_grad).  With --wgrad it carries d_grad_l1 and d_grad_linf, the norms over all 54 gradients of
d_total_loss with respect to the discriminators' variables (Discriminators.disc_grad; --host: disc_grad).

THE BACKWARD: d d_total_loss / d the discriminators' variables (`disc_grad`, csrc/disc_wgrad_kernels.h, Discriminators.disc_grad).  For
the discriminators' update the images are data and d_total_loss = disc_real + disc_fake is differentiated with respect to the 54
trainable variables (weights.discriminator_trainable_names) over all 2B rows, in the mode everything here runs in (training=False,
moving statistics).  `disc_grad`'s docstring writes every operation out; tests/golden/discriminator_wgrad_32.npz holds torch autograd's
float64 gradients as float32 (tools/make_discriminator_wgrad_fixture.py), and `d_total_f64` is the objective without float32 rounding
for the finite-difference test.
"""
from __future__ import annotations

import sys
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from .shadow_synth import SIZES
from .ucb_post import resize_bilinear
from .weights import BN_EPS, DISC_CH, LRELU_ALPHA, N_LAYER_D  # noqa: F401 (DISC_CH: the binding reads it here)

f32 = np.float32
DOWNSIZE = (1, 2, 4)
MAX_B = 32767
LOSS_NAMES = ("gen", "disc_real", "disc_fake")
DISC_SUM_NAMES = tuple("%s_%d" % (n, k) for k in (1, 2, 3) for n in ("hinge_real", "hinge_fake", "fake"))
K = len(DISC_SUM_NAMES)
IDX = {n: i for i, n in enumerate(DISC_SUM_NAMES)}
SIZE_TEXT = "discriminators take 1..32767 items of side 32, 64, 128 or 256, got B=%d S=%d"


def same_pad(size: int, k: int, s: int) -> Tuple[int, int]:
    """TF 'SAME' padding of one axis (oracle.gsc_oracle.same_pad): (before, after)."""
    out = -(-size // s)
    total = max((out - 1) * s + k - size, 0)
    return total // 2, total - total // 2


def map_sides(S: int, k: int) -> List[int]:
    """The sides of discriminator k's maps: its input, the four stride-2 outputs, the head's output."""
    sides = [S // DOWNSIZE[k - 1]]
    for _ in range(N_LAYER_D):
        sides.append(-(-sides[-1] // 2))
    return sides + [sides[-1]]


def final_side(S: int, k: int) -> int:
    return map_sides(S, k)[-1]


def conv2d_same(x: np.ndarray, kernel: np.ndarray, bias: np.ndarray, stride: int) -> np.ndarray:
    """[N,H,W,C] x HWIO kernel -> float64 [N,ceil(H/s),ceil(W/s),O]: Conv2D(padding='same') + bias."""
    x, kernel = np.asarray(x, np.float64), np.asarray(kernel, np.float64)
    n, h, w, c = x.shape
    kh, kw = kernel.shape[:2]
    (pt, pb), (pl, pr) = same_pad(h, kh, stride), same_pad(w, kw, stride)
    ho, wo = -(-h // stride), -(-w // stride)
    xp = np.zeros((n, h + pt + pb, w + pl + pr, c), np.float64)
    xp[:, pt:pt + h, pl:pl + w] = x
    out = np.zeros((n, ho, wo, kernel.shape[3]), np.float64)
    for a in range(kh):
        for b in range(kw):
            out += xp[:, a:a + (ho - 1) * stride + 1:stride, b:b + (wo - 1) * stride + 1:stride] @ kernel[a, b]
    return out + np.asarray(bias, np.float64)


def layer(weights: Dict[str, np.ndarray], k: int, i: int, x: np.ndarray) -> np.ndarray:
    """conv_stack[i] of discriminator k on [N,H,W,C]: Conv2D stride 2 + bias, BatchNormalization (moving statistics), LeakyReLU."""
    st = "discriminator_%d/conv_stack/%d/" % (k, i)
    y = conv2d_same(x, weights[st + "conv/kernel"], weights[st + "conv/bias"], 2)
    g, beta, mean, var = (np.asarray(weights[st + "bnorm/" + p], np.float64) for p in ("gamma", "beta", "moving_mean", "moving_variance"))
    inv = g / np.sqrt(var + BN_EPS)
    y = y * inv + (beta - mean * inv)
    return np.where(y >= 0, y, LRELU_ALPHA * y)


def head(weights: Dict[str, np.ndarray], k: int, x: np.ndarray) -> np.ndarray:
    """conv2 of discriminator k on [N,h,h,64] -> float64 [N,h,h,1]."""
    st = "discriminator_%d/conv2/conv/" % k
    return conv2d_same(x, weights[st + "kernel"], weights[st + "bias"], 1)


def check_inputs(gt, con_rgb, mask_sv) -> Tuple[int, int]:
    arrays = [np.asarray(a) for a in (gt, con_rgb, mask_sv)]
    if arrays[0].ndim != 4:
        raise ValueError("discriminators: gt must be [B,S,S,3], got %s" % (arrays[0].shape,))
    B, S = arrays[0].shape[:2]
    if S not in SIZES or not 1 <= B <= MAX_B:
        raise ValueError(SIZE_TEXT % (B, S))
    for name, a in zip(("gt", "con_rgb", "mask_sv"), arrays):
        if a.shape != (B, S, S, 3):
            raise ValueError("discriminators: %s must be [%d,%d,%d,3] like gt, got %s" % (name, B, S, S, a.shape))
    return B, S


def disc_input(gt, con_rgb, mask_sv, k: int) -> np.ndarray:
    """The input of discriminator k: float32 [2B, S // downsize, S // downsize, 6]."""
    gt, con_rgb, mask_sv = (np.asarray(a, f32) for a in (gt, con_rgb, mask_sv))
    x = np.concatenate([np.concatenate([gt, con_rgb], axis=0), np.concatenate([mask_sv, mask_sv], axis=0)], axis=3)
    ds = DOWNSIZE[k - 1]
    return x if ds == 1 else np.stack([resize_bilinear(item, x.shape[1] // ds) for item in x])


def forward(weights: Dict[str, np.ndarray], gt, con_rgb, mask_sv) -> Dict[str, np.ndarray]:
    """Every activation of the three discriminators: `d{k}/in`, `d{k}/conv{i}`, `d{k}/out`."""
    check_inputs(gt, con_rgb, mask_sv)
    acts: Dict[str, np.ndarray] = {}
    for k in (1, 2, 3):
        x = disc_input(gt, con_rgb, mask_sv, k)
        acts["d%d/in" % k] = x
        h = x.astype(np.float64)
        for i in range(N_LAYER_D):
            h = layer(weights, k, i, h)
            acts["d%d/conv%d" % (k, i)] = h
        acts["d%d/out" % k] = head(weights, k, h)
    return acts


def logits_of(acts: Dict[str, np.ndarray]) -> List[np.ndarray]:
    """The three logit maps [2B,h_k,h_k] of `forward`'s result."""
    return [np.asarray(acts["d%d/out" % k])[..., 0] for k in (1, 2, 3)]


def losses_from_logits(logits: Sequence[np.ndarray]) -> Dict[str, np.ndarray]:
    """Three logit maps [2B,h_k,h_k] -> dict(losses float32 [3] (LOSS_NAMES), sums float64 [B,9] (DISC_SUM_NAMES))."""
    maps = [np.asarray(y).astype(f32) for y in logits]
    B = maps[0].shape[0] // 2
    sums = np.zeros((B, K), np.float64)
    for j, y in enumerate(maps):
        assert y.ndim == 3 and y.shape[0] == 2 * B and y.shape[1] == y.shape[2]
        real, fake = y[:B].reshape(B, -1), y[B:].reshape(B, -1)
        sums[:, 3 * j + 0] = np.maximum(f32(0), f32(1) - real).sum(axis=1, dtype=np.float64)
        sums[:, 3 * j + 1] = np.maximum(f32(0), f32(1) + fake).sum(axis=1, dtype=np.float64)
        sums[:, 3 * j + 2] = fake.sum(axis=1, dtype=np.float64)
    return {"losses": losses_from_sums(sums, [y.shape[1] for y in maps]), "sums": sums}


def losses_from_sums(sums: np.ndarray, sides: Sequence[int]) -> np.ndarray:
    """float64 [B,9] and the three final sides h_k -> float32 [3]: gen, disc_real, disc_fake over the whole batch."""
    sums = np.asarray(sums, np.float64)
    t = np.zeros(K, np.float64)
    for row in sums:
        t = t + row
    n = [float(sums.shape[0] * h * h) for h in sides]
    m = [t[3 * j + 2] / n[j] for j in range(3)]
    gen = (-m[0] - m[1]) - m[2]
    real = (t[0] / n[0] + t[3] / n[1]) + t[6] / n[2]
    fake = (t[1] / n[0] + t[4] / n[1]) + t[7] / n[2]
    return np.array([gen, real, fake], np.float64).astype(f32)


def gan_losses(weights: Dict[str, np.ndarray], gt, con_rgb, mask_sv) -> Dict[str, np.ndarray]:
    """Batches -> dict(losses float32 [3], sums float64 [B,9], logits: three float64 maps [2B,h_k,h_k], acts: `forward`'s dict)."""
    acts = forward(weights, gt, con_rgb, mask_sv)
    logits = logits_of(acts)
    out = losses_from_logits(logits)
    out.update(logits=logits, acts=acts)
    return out


def example_inputs(S: int, B: int, seed: int = 0):
    """gt, con_rgb, mask_sv of train_losses.example_inputs(S, B, seed)."""
    from .train_losses import example_inputs as ex
    _, gt, mask_sv, _, con = ex(S, B, seed)
    return gt, con, mask_sv


# ---- the backward: d gen / d con_rgb
GRAD_NAMES = ("gen_grad_l1", "gen_grad_linf")


def seed_weights(B: int, S: int) -> List[np.float32]:
    """w_k = float32(1 / (B h_k^2)), k = 1, 2, 3."""
    return [f32(1.0 / (float(B) * float(final_side(S, k) ** 2))) for k in (1, 2, 3)]


def conv2d_same_dgrad(gy: np.ndarray, kernel: np.ndarray, stride: int, side: int) -> np.ndarray:
    """The gradient [N,Ho,Wo,O] at a Conv2D(padding='same') output -> float64 [N,side,side,C] at its input of side `side`:
    gx[n, s oy + a - before, s ox + b - before, c] += sum_o gy[n, oy, ox, o] k[a, b, c, o], positions outside the map dropped."""
    gy, kernel = np.asarray(gy, np.float64), np.asarray(kernel, np.float64)
    n, ho, wo, _ = gy.shape
    kh, kw = kernel.shape[:2]
    (pt, pb), (pl, pr) = same_pad(side, kh, stride), same_pad(side, kw, stride)
    assert ho == -(-side // stride) and wo == ho
    gp = np.zeros((n, side + pt + pb, side + pl + pr, kernel.shape[2]), np.float64)
    for a in range(kh):
        for b in range(kw):
            gp[:, a:a + (ho - 1) * stride + 1:stride, b:b + (wo - 1) * stride + 1:stride] += gy @ kernel[a, b].T
    return gp[:, pt:pt + side, pl:pl + side].copy()


def leaky_grad(g: np.ndarray, y: np.ndarray) -> np.ndarray:
    """TensorFlow's LeakyReluGrad on the layer's kept output y: g where y > 0, 0.3 g otherwise (0 takes 0.3)."""
    g = np.asarray(g)
    return np.where(np.asarray(y) > 0, g, g.dtype.type(LRELU_ALPHA) * g)


def resize_grad(g: np.ndarray, ds: int) -> np.ndarray:
    """The gradient [N,s,s,C] at disc_input's resize output -> [N,s ds,s ds,C] at its input: the identity for 1; 0.25 g[y // 2, x // 2]
    on all four pixels of the 2 x 2 block for 2; 0.25 g[y // 4, x // 4] on the middle 2 x 2 of each 4 x 4 block and 0 on the other
    twelve for 4."""
    g = np.asarray(g)
    if ds == 1:
        return g.copy()
    n, s, _, c = g.shape
    q = g.dtype.type(0.25) * g
    out = np.zeros((n, s, ds, s, ds, c), g.dtype)
    lo = 0 if ds == 2 else 1
    out[:, :, lo:lo + 2, :, lo:lo + 2, :] = q[:, :, None, :, None, :]
    return out.reshape(n, s * ds, s * ds, c)


def bn_inv(weights: Dict[str, np.ndarray], k: int, i: int) -> np.ndarray:
    """inv = gamma / sqrt(moving_variance + eps) of conv_stack[i] of discriminator k, float64 [n_ch[i]]."""
    st = "discriminator_%d/conv_stack/%d/bnorm/" % (k, i)
    return np.asarray(weights[st + "gamma"], np.float64) / np.sqrt(np.asarray(weights[st + "moving_variance"], np.float64) + BN_EPS)


def gen_grad(weights: Dict[str, np.ndarray], gt, con_rgb, mask_sv, upstream=None, acts=None) -> Dict[str, np.ndarray]:
    """d gen / d con_rgb for a batch, training=False -> dict(`grad` float64 [B,S,S,3], and each stage's gradient under `forward`'s
    names: `d{k}/out` [B,h_k,h_k,1] the seed, `d{k}/conv{i}` [B,.,.,n_ch[i]] the gradient at conv_stack[i]'s BatchNormalization output
    (LeakyReLU's input), `d{k}/in` [B,s,s,3] the gradient at the image channels of discriminator k's input).  float64 arithmetic from the
    float32 variables, for discriminator k = 1, 2, 3 from the top down:
      seed             gen = (-m_1 - m_2) - m_3 is linear in the fake logits, with no hinge: d gen / d out_k[B + b, y, x] = -w_k, w_k =
                       float32(1 / (B h_k^2)).  The real rows [0, B) get nothing and are never computed.
      conv dgrad       the input gradient of the cross-correlation, with `before` of same_pad:
                         gx[n, s oy + a - before, s ox + b - before, c] += sum_o gy[n, oy, ox, o] k[a, b, c, o]
                       for the head conv2 (s = 1, pad 1 before and 2 after) and the four stride-2 layers, the 1 x 1 -> 1 x 1 map (pad 1, 2)
                       of discriminator 3 at S = 32 included.  The bias has no part.
      BatchNormalization (moving statistics)   gy * inv per output channel, inv = gamma / sqrt(moving_variance + eps), before the
                       convolution's gradient.
      LeakyReLU(0.3)   TensorFlow's LeakyReluGrad on the layer's kept post-activation output y, whose sign is the pre-activation's:
                       g where y > 0, 0.3 g otherwise, so 0 takes 0.3.
      resize           the gradient is read on channels 0..2 of the discriminator's input (the mask channels are dropped) and goes back
                       through the resize (`resize_grad`): downsize 1 the identity; 2 sends 0.25 g[y // 2, x // 2] to all four pixels of
                       the 2 x 2 block; 4 sends 0.25 g[y // 4, x // 4] to the middle 2 x 2 of each 4 x 4 block and 0 to the other twelve.
    The three contributions are added in the order 1, 2, 3: t = (r_1 + r_2) + r_3.  Without `upstream`, grad = t; with it (a float32),
    grad = float32(t) * float32(upstream) as one float32 product, as the device forms it.  With `acts` given (a dict like `forward`'s,
    for example the device's kept activations) the LeakyReLU masks are read from it instead of from the statement's own float64
    forward: pre-activations within 3e-7 of 0 occur on the example inputs, so masks flip between float32 and float64."""
    B, S = check_inputs(gt, con_rgb, mask_sv)
    A = forward(weights, gt, con_rgb, mask_sv) if acts is None else acts
    out: Dict[str, np.ndarray] = {}
    total = None
    for k, w_k in zip((1, 2, 3), seed_weights(B, S)):
        sides = map_sides(S, k)
        g = np.full((B, sides[-1], sides[-1], 1), -float(w_k), np.float64)
        out["d%d/out" % k] = g
        g = conv2d_same_dgrad(g, weights["discriminator_%d/conv2/conv/kernel" % k], 1, sides[N_LAYER_D])
        for i in reversed(range(N_LAYER_D)):
            g = leaky_grad(g, np.asarray(A["d%d/conv%d" % (k, i)])[B:])
            out["d%d/conv%d" % (k, i)] = g
            g = conv2d_same_dgrad(g * bn_inv(weights, k, i), weights["discriminator_%d/conv_stack/%d/conv/kernel" % (k, i)], 2, sides[i])
        g = np.ascontiguousarray(g[..., :3])
        out["d%d/in" % k] = g
        r = resize_grad(g, DOWNSIZE[k - 1])
        total = r if total is None else total + r
    out["grad"] = total if upstream is None else (total.astype(f32) * f32(np.asarray(upstream).reshape(-1)[0])).astype(np.float64)
    return out


def gen_f64(weights: Dict[str, np.ndarray], con_rgb, mask_sv, masks: Optional[List[np.ndarray]] = None) -> float:
    """gen as a function of a float64 con_rgb with no float32 rounding anywhere (the variables are still the float32 ones, the
    resizes the exact means of their four pixels): the objective gen_grad differentiates.  A list given as `masks` receives every
    LeakyReLU mask (y > 0) in order.  tests/test_discriminator_grad_cpu.py takes its finite differences of the same operations in
    extended precision, where the rounding of a loss value can be bounded usefully."""
    x = np.concatenate([np.asarray(con_rgb, np.float64), np.asarray(mask_sv, np.float64)], axis=3)
    n, S = x.shape[:2]
    gen = 0.0
    for k in (1, 2, 3):
        ds = DOWNSIZE[k - 1]
        lo = 0 if ds < 4 else 1
        h = x if ds == 1 else x.reshape(n, S // ds, ds, S // ds, ds, 6)[:, :, lo:lo + 2, :, lo:lo + 2].mean(axis=(2, 4))
        for i in range(N_LAYER_D):
            h = layer(weights, k, i, h)
            if masks is not None:
                masks.append(h > 0)
        gen = gen - float(head(weights, k, h).mean())
    return gen


def grad_norms(grad) -> Tuple[float, float]:
    g = np.abs(np.asarray(grad, np.float64))
    return float(g.sum()), float(g.max())


# ---- the backward: d d_total_loss / d the discriminators' variables
WGRAD_NAMES = ("d_grad_l1", "d_grad_linf")


def hinge_seed(logits: np.ndarray, B: int, w_k) -> np.ndarray:
    """The float32 logits [2B,h,h] of one discriminator -> float64 [2B,h,h,1], d d_total_loss / d out: -w_k on a real row where the
    float32 term 1 - y is > 0, +w_k on a fake row where the float32 term 1 + y is > 0, 0 elsewhere (a term of exactly 0 passes
    nothing: TensorFlow's Maximum hands a tie to its first argument, the constant 0.)."""
    y = np.asarray(logits).astype(f32)
    seed = np.zeros(y.shape, np.float64)
    seed[:B] = np.where(f32(1) - y[:B] > 0, -float(w_k), 0.0)
    seed[B:] = np.where(f32(1) + y[B:] > 0, float(w_k), 0.0)
    return seed[..., None]


def conv2d_same_wgrad(x: np.ndarray, gy: np.ndarray, stride: int, ksize: int = 4) -> np.ndarray:
    """The input [N,H,H,C] of a Conv2D(padding='same') and the gradient [N,Ho,Ho,O] at its output -> float64 [ksize,ksize,C,O], the
    gradient at its HWIO kernel: gk[a, b, c, o] = sum_{n, oy, ox} x[n, s oy + a - before, s ox + b - before, c] gy[n, oy, ox, o],
    positions outside the map reading 0."""
    x, gy = np.asarray(x, np.float64), np.asarray(gy, np.float64)
    n, h, _, c = x.shape
    ho = gy.shape[1]
    pt, pb = same_pad(h, ksize, stride)
    assert ho == -(-h // stride) and gy.shape[2] == ho
    xp = np.zeros((n, h + pt + pb, h + pt + pb, c), np.float64)
    xp[:, pt:pt + h, pt:pt + h] = x
    out = np.zeros((ksize, ksize, c, gy.shape[3]), np.float64)
    span = (ho - 1) * stride + 1
    for a in range(ksize):
        for b in range(ksize):
            out[a, b] = np.tensordot(xp[:, a:a + span:stride, b:b + span:stride], gy, axes=([0, 1, 2], [0, 1, 2]))
    return out


def disc_grad(weights: Dict[str, np.ndarray], gt, con_rgb, mask_sv, acts=None, logits=None) -> Dict[str, np.ndarray]:
    """d d_total_loss / d v for each of the 54 trainable variables v of the three discriminators
    (weights.discriminator_trainable_names), training=False, with d_total_loss = disc_real + disc_fake -> dict(name -> float64 array in
    the variable's own shape (HWIO kernels), and each stage's gradient for all 2B rows under `forward`'s names: `d{k}/out` [2B,h_k,h_k,1]
    the seed, `d{k}/conv{i}` [2B,.,.,n_ch[i]] the gradient at conv_stack[i]'s BatchNormalization output).  float64 arithmetic from the
    float32 variables, for discriminator k = 1, 2, 3 from the top down:
      seed             with w_k = float32(1 / (B h_k^2)) and y the float32 logit (`hinge_seed`): a real row gets -w_k where the float32
                       term 1 - y is > 0, a fake row +w_k where the float32 term 1 + y is > 0, everything else 0.  This is TensorFlow's
                       Maximum gradient with the constant 0. as first argument: a tie goes to the constant, so a term of exactly 0
                       passes nothing.
      head             d kernel[a, b, c, 0] = sum_{n, oy, ox} seed[n, oy, ox] x[n, oy + a - 1, ox + b - 1, c] over conv3's kept output x,
                       positions outside the map reading 0 (`conv2d_same_wgrad`, stride 1); d bias = sum seed; the gradient handed
                       down is conv2d_same_dgrad(seed, kernel, 1, side).
      each stride-2 layer i, from 3 down to 0, with gz the incoming gradient after LeakyReluGrad on the layer's kept output
      (`leaky_grad`: g where y > 0, 0.3 g otherwise), inv = gamma / sqrt(moving_variance + eps) (`bn_inv`), x the layer's input
      (`d{k}/in`, 6 channels, for layer 0 and `d{k}/conv{i-1}` otherwise) and c = conv2d_same(x, kernel, bias, 2):
                       d beta[o] = sum gz[..., o]
                       d gamma[o] = sum gz[..., o] (c[..., o] - moving_mean[o]) / sqrt(moving_variance[o] + eps)
                       d bias[o] = inv[o] sum gz[..., o]
                       d kernel[a, b, c, o] = inv[o] sum_{n, oy, ox} x[n, 2 oy + a - before, 2 ox + b - before, c] gz[n, oy, ox, o],
                       `before` of same_pad and positions outside the map reading 0, the 1 x 1 -> 1 x 1 layer (pad 1, 2) of
                       discriminator 3 at S = 32 included.
                       The gradient handed down is conv2d_same_dgrad(gz inv, kernel, 2, side); it is not formed below conv0.
    With `logits` given (three maps [2B,h_k,h_k], for example the device's) the hinge masks are read from them instead of from the
    statement's own float64 forward rounded to float32; with `acts` given (a dict like `forward`'s) the LeakyReLU masks, the layers'
    inputs x and the convolution outputs c are read or formed from it, as gen_grad reads its masks."""
    B, S = check_inputs(gt, con_rgb, mask_sv)
    A = forward(weights, gt, con_rgb, mask_sv) if acts is None else acts
    Y = logits_of(A) if logits is None else logits
    out: Dict[str, np.ndarray] = {}
    for k, w_k in zip((1, 2, 3), seed_weights(B, S)):
        sides = map_sides(S, k)
        head_st = "discriminator_%d/conv2/conv/" % k
        g = hinge_seed(np.asarray(Y[k - 1]).reshape(2 * B, sides[-1], sides[-1]), B, w_k)
        out["d%d/out" % k] = g
        out[head_st + "kernel"] = conv2d_same_wgrad(A["d%d/conv%d" % (k, N_LAYER_D - 1)], g, 1)
        out[head_st + "bias"] = g.sum(axis=(0, 1, 2))
        g = conv2d_same_dgrad(g, weights[head_st + "kernel"], 1, sides[N_LAYER_D])
        for i in reversed(range(N_LAYER_D)):
            st = "discriminator_%d/conv_stack/%d/" % (k, i)
            gz = leaky_grad(g, np.asarray(A["d%d/conv%d" % (k, i)]))
            out["d%d/conv%d" % (k, i)] = gz
            inv = bn_inv(weights, k, i)
            x = np.asarray(A["d%d/in" % k] if i == 0 else A["d%d/conv%d" % (k, i - 1)], np.float64)
            c = conv2d_same(x, weights[st + "conv/kernel"], weights[st + "conv/bias"], 2)
            mean, var = (np.asarray(weights[st + "bnorm/" + p], np.float64) for p in ("moving_mean", "moving_variance"))
            total = gz.sum(axis=(0, 1, 2))
            out[st + "bnorm/beta"] = total
            out[st + "bnorm/gamma"] = (gz * ((c - mean) / np.sqrt(var + BN_EPS))).sum(axis=(0, 1, 2))
            out[st + "conv/bias"] = inv * total
            out[st + "conv/kernel"] = conv2d_same_wgrad(x, gz, 2) * inv
            if i > 0:
                g = conv2d_same_dgrad(gz * inv, weights[st + "conv/kernel"], 2, sides[i])
    return out


def d_total_f64(weights: Dict[str, np.ndarray], gt, con_rgb, mask_sv, masks: Optional[List[np.ndarray]] = None, dtype=np.float64):
    """d_total_loss = disc_real + disc_fake as a function of the variables with no float32 rounding anywhere (the resizes are the
    exact means of their four pixels, the hinge terms and the divisors B h_k^2 are formed in `dtype`): the objective disc_grad
    differentiates, up to w_k's rounding to float32.  `weights` may hold arrays of any float type; they are used in `dtype`
    (float64, or numpy's extended precision for tests/test_discriminator_wgrad_cpu.py's finite differences).  A list given as `masks`
    receives every LeakyReLU mask (y > 0) and then the two hinge masks of each discriminator, in order."""
    T = dtype
    gt, con_rgb, mask_sv = (np.asarray(a, T) for a in (gt, con_rgb, mask_sv))
    x = np.concatenate([np.concatenate([gt, con_rgb], axis=0), np.concatenate([mask_sv, mask_sv], axis=0)], axis=3)
    n, S = x.shape[:2]
    B = n // 2
    total = T(0)
    for k in (1, 2, 3):
        ds = DOWNSIZE[k - 1]
        lo = 0 if ds < 4 else 1
        h = x if ds == 1 else x.reshape(n, S // ds, ds, S // ds, ds, 6)[:, :, lo:lo + 2, :, lo:lo + 2].mean(axis=(2, 4))
        for i in range(N_LAYER_D):
            st = "discriminator_%d/conv_stack/%d/" % (k, i)
            g, beta, mean, var = (np.asarray(weights[st + "bnorm/" + p], T) for p in ("gamma", "beta", "moving_mean", "moving_variance"))
            inv = g / np.sqrt(var + T(BN_EPS))
            y = _conv_same_any(h, weights[st + "conv/kernel"], weights[st + "conv/bias"], 2, T) * inv + (beta - mean * inv)
            if masks is not None:
                masks.append(np.asarray(y > 0))
            h = np.where(y >= 0, y, T(LRELU_ALPHA) * y)
        st = "discriminator_%d/conv2/conv/" % k
        out = _conv_same_any(h, weights[st + "kernel"], weights[st + "bias"], 1, T)[..., 0]
        real, fake = T(1) - out[:B], T(1) + out[B:]
        if masks is not None:
            masks += [np.asarray(real > 0), np.asarray(fake > 0)]
        total = total + (np.maximum(T(0), real).sum() + np.maximum(T(0), fake).sum()) / T(B * out.shape[1] * out.shape[2])
    return total


def _conv_same_any(x, kernel, bias, stride: int, T) -> np.ndarray:
    """conv2d_same in the float type T."""
    x, kernel = np.asarray(x, T), np.asarray(kernel, T)
    n, h, _, c = x.shape
    pt, pb = same_pad(h, kernel.shape[0], stride)
    ho = -(-h // stride)
    xp = np.zeros((n, h + pt + pb, h + pt + pb, c), T)
    xp[:, pt:pt + h, pt:pt + h] = x
    out = np.zeros((n, ho, ho, kernel.shape[3]), T)
    span = (ho - 1) * stride + 1
    for a in range(kernel.shape[0]):
        for b in range(kernel.shape[1]):
            out += xp[:, a:a + span:stride, b:b + span:stride] @ kernel[a, b]
    return out + np.asarray(bias, T)


def wgrad_norms(grads: Dict[str, np.ndarray]) -> Tuple[float, float]:
    """The L1 and L-infinity norms over all 54 gradients of a dict that holds them under the trainable variables' names."""
    from .weights import discriminator_trainable_names
    mags = [np.abs(np.asarray(grads[n], np.float64)) for n in discriminator_trainable_names()]
    return float(sum(m.sum() for m in mags)), float(max(m.max() for m in mags))


# ---- the command-line entry
def score_folder(folder: str, ckpt: Optional[str] = None, batch: int = 8, host: bool = False, device: int = 0, quiet: bool = False,
                 stats: Optional[Dict[str, float]] = None, grad: bool = False, wgrad: bool = False) -> Dict[str, float]:
    """Every item folder `<folder>/<name>/` the shadow_synth command wrote -> the step-weighted means of gen, disc_real and disc_fake.
    With `host`, a `stats` dict receives `max_abs_logit`, the largest magnitude of the statement's logits over all steps.  With `grad`
    each batch's line and the means also carry GRAD_NAMES, the norms of d gen / d con_rgb; with `wgrad`, WGRAD_NAMES, the norms over the
    54 gradients of d_total_loss with respect to the discriminators' variables."""
    import torch
    from .objective import discriminator_weights, score_steps
    weights = discriminator_weights(ckpt, "discriminator")
    dev = torch.device("cuda", device)
    if host:
        def step(gt_a, mask_a, con_rgb):
            torch.cuda.synchronize(dev)
            con_a = con_rgb.cpu().numpy()
            r = gan_losses(weights, gt_a, con_a, mask_a)
            if stats is not None:
                stats["max_abs_logit"] = max([stats.get("max_abs_logit", 0.0)] + [float(np.abs(y).max()) for y in r["logits"]])
            return (r["losses"], grad_norms(gen_grad(weights, gt_a, con_a, mask_a, acts=r["acts"])["grad"]) if grad else (),
                    wgrad_norms(disc_grad(weights, gt_a, con_a, mask_a, acts=r["acts"], logits=r["logits"])) if wgrad else ())
    else:
        from .discriminator_gpu import Discriminators
        runner = Discriminators(device)
        runner.load_weights(weights)

        def step(gt_a, mask_a, con_rgb):
            gt_d, mask_d = torch.from_numpy(gt_a).to(dev), torch.from_numpy(mask_a).to(dev)
            if grad:
                res = runner.gen_grad(gt_d, con_rgb.contiguous(), mask_d)
                loss, norms = res[0].cpu().numpy(), grad_norms(res[2].cpu().numpy())
            else:
                loss, norms = runner.gan_losses(gt_d, con_rgb, mask_d)[0].cpu().numpy(), ()
            if not wgrad:
                return loss, norms, ()
            return loss, norms, wgrad_norms({k: v.cpu().numpy() for k, v in runner.disc_grad(gt_d, con_rgb.contiguous(), mask_d)[2].items()})

    def record(_, gt_a, mask_a, __, con_rgb):
        loss, norms, wnorms = step(gt_a, mask_a, con_rgb)
        return dict(list(zip(LOSS_NAMES, (float(v) for v in loss))) + list(zip(GRAD_NAMES, norms)) + list(zip(WGRAD_NAMES, wnorms))), ()

    return score_steps(folder, ckpt, batch, device, "discriminator", record, quiet)


def main(argv=None) -> int:
    import argparse
    ap = argparse.ArgumentParser(prog="python -m blindshadowremoval_amd.discriminator",
                                 description="Score a generator on synthesised pairs with train_step's three GAN terms.")
    ap.add_argument("folder")
    ap.add_argument("--ckpt", default=None, help="checkpoint directory; without it the weights come from init_weights / init_discriminator_weights")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--host", action="store_true", help="compute the three terms with the host statement instead of the device chain")
    ap.add_argument("--grad", action="store_true", help="per batch also the L1 and L-infinity norms of d gen / d con_rgb")
    ap.add_argument("--wgrad", action="store_true", help="per batch also the L1 and L-infinity norms over the 54 gradients of d_total_loss")
    a = ap.parse_args(argv)
    means = score_folder(a.folder, ckpt=a.ckpt, batch=a.batch, host=a.host, grad=a.grad, wgrad=a.wgrad)
    print(", ".join("%s:%.9g" % (k, means[k]) for k in LOSS_NAMES + (GRAD_NAMES if a.grad else ()) + (WGRAD_NAMES if a.wgrad else ())))
    return 0


if __name__ == "__main__":
    sys.exit(main())
