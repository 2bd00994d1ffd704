"""The host statement of the generator's backward pass, from the output down, training=False (moving statistics).  So far the colour
tail (model.py:217-219, 267-269): clr_conv1 (3x3, cat[gs, f] 65 -> 16, BN, LeakyReLU), clr_conv2 (1x1, 16 -> 16, BN, LeakyReLU) and
clr_conv3 (1x1, 16 -> 3).  `tail_grad` writes the arithmetic out in float64 from the float32 variables; csrc/clr_tail_grad_kernels.h
is held to it (clr_tail_gpu.ColourTail).  Below it the colour decoder (model.py:214-216, 264-266): clr_up1, clr_up2, clr_up3, each
Conv2DTranspose(3, stride 2, SAME), BN, LeakyReLU; `decoder_grad` is its statement, any input width (261 for GSC, 877 for TSM), and
csrc/clr_up_grad_kernels.h is held to it (clr_decoder_gpu.ColourDecoder).  Below that the upper half of res_stack/5 (model.py:6-61, 102-113): the
NonLocalBlock — theta, phi, g (1x1, 257 -> 128), softmax(theta phi^T) g, w (1x1, 128 -> 257), BN, z = y3 + w_y — then the block's zero-padded
skip and relu3; `nonlocal_grad` is its statement, from the gradient at the block's output to the gradient at bnorm3's output y3, the gradient
the skip carries to the block's input and the ten variables of the non-local block, any input width; csrc/nonlocal_grad_kernels.h is held to
it (nonlocal_grad_gpu.NonLocalGrad).  Below that the lower half of the same block (model.py:84-101): conv1 (1x1, C -> 128), conv2 (3x3, 128 -> 128),
conv3 (1x1, 128 -> 257), each with its BatchNormalization and the first two with a LeakyReLU; `bottleneck_grad` is its statement, from d_y3
and d_skip to the gradient at the block's input and the twelve variables; csrc/bottleneck_grad_kernels.h is held to it
(bottleneck_grad_gpu.BottleneckGrad).  On the grey branch the heads (model.py:246-250): conv2 (7x7, 64 -> 1, tanh) gives mask, conv3
(7x7, 64 -> 1) gives con, gs = gray(inputs) (1 + mask) + con; `heads_grad` is its statement, from the complete d_gs to the gradient at up3's
output y and the four variables; csrc/heads_grad_kernels.h is held to it (heads_grad_gpu.HeadsGrad).  Below the heads the grey decoder
(model.py:243-245): up1, up2 on cat[up1, x3], up3 on cat[up2, x2], the colour decoder's layer type; `grey_decoder_grad` is its statement,
from d_y to the gradient at res_stack/2's output, the two skip gradients and the twelve variables; csrc/grey_up_grad_kernels.h is held
to it (grey_decoder_gpu.GreyDecoder).  Where the two branches meet (model.py:256-262): res_stack/4, res_stack/3 and the hole xh =
cat[x (1 - bmask), bmask, uv]; `colour_trunk_grad` chains the two block statements for blocks 4 and 3 and ends in `hole_grad`, from the
gradient at res_stack/5's input and the grey decoder's d_x to the complete gradient at res_stack/2's output and the 44 variables;
csrc/colour_trunk_grad_kernels.h is held to it (colour_trunk_gpu.ColourTrunk)."""
from __future__ import annotations

import functools
from typing import Dict, Optional, Tuple

import numpy as np

from .discriminator import conv2d_same_dgrad, leaky_grad
from .weights import (BN_EPS, LRELU_ALPHA, RES_CH, generator_bottleneck_trainable_names, generator_colour_trunk_trainable_names, generator_decoder_trainable_names,
                      generator_grey_decoder_trainable_names, generator_heads_trainable_names, generator_lower_trunk_trainable_names,
                      generator_nonlocal_trainable_names, generator_tail_trainable_names)

TAIL_LAYERS = ("clr_conv1", "clr_conv2", "clr_conv3")
TAIL_NORM_NAMES = ("d_f", "d_gs") + tuple(generator_tail_trainable_names())
DECODER_LAYERS = ("clr_up1", "clr_up2", "clr_up3")
DECODER_NORM_NAMES = ("d_x",) + tuple(generator_decoder_trainable_names())
NONLOCAL_NORM_NAMES = ("d_y3", "d_skip") + tuple(generator_nonlocal_trainable_names())
NONLOCAL_MAPS = ("gz", "dA", "D", "d_theta", "d_phi", "d_g")


def bn_vectors(weights: Dict[str, np.ndarray], stem: str, dtype=np.float64):
    """(bias, inv, moving_mean, rstd, beta) of `stem`'s convolution and BatchNormalization in `dtype`: rstd = 1 / sqrt(moving_variance +
    eps), inv = gamma rstd."""
    T = dtype
    gamma, beta, mean, var = (np.asarray(weights["%s/bnorm/%s" % (stem, p)], T) for p in ("gamma", "beta", "moving_mean", "moving_variance"))
    rstd = T(1) / np.sqrt(var + T(BN_EPS))
    return np.asarray(weights[stem + "/conv/bias"], T), gamma * rstd, mean, rstd, beta


def conv3x3_same(x: np.ndarray, kernel: np.ndarray) -> np.ndarray:
    """[N,H,W,C] x HWIO [3,3,C,O] -> [N,H,W,O] in x's type: stride 1, zero outside the image, no bias; taps in index order."""
    n, h, w, c = x.shape
    xp = np.zeros((n, h + 2, w + 2, c), x.dtype)
    xp[:, 1:h + 1, 1:w + 1] = x
    out = np.zeros((n, h, w, kernel.shape[3]), x.dtype)
    for a in range(3):
        for b in range(3):
            out += xp[:, a:a + h, b:b + w] @ kernel[a, b].astype(x.dtype)
    return out


def conv3x3_same_wgrad(x: np.ndarray, gy: np.ndarray) -> np.ndarray:
    """The input [N,H,W,C] of a 3x3 stride-1 SAME convolution and the gradient [N,H,W,O] at its output -> float64 [3,3,C,O]:
    gk[a, b, c, o] = sum x[n, y + a - 1, x + b - 1, c] gy[n, y, x, o], zero outside the image."""
    x, gy = np.asarray(x, np.float64), np.asarray(gy, np.float64)
    n, h, w, c = x.shape
    xp = np.zeros((n, h + 2, w + 2, c), np.float64)
    xp[:, 1:h + 1, 1:w + 1] = x
    out = np.zeros((3, 3, c, gy.shape[3]), np.float64)
    for a in range(3):
        for b in range(3):
            out[a, b] = np.tensordot(xp[:, a:a + h, b:b + w], gy, axes=([0, 1, 2], [0, 1, 2]))
    return out


def conv3x3_same_dgrad(gy: np.ndarray, kernel: np.ndarray) -> np.ndarray:
    """The gradient [N,H,W,O] at a 3x3 stride-1 SAME convolution's output -> float64 [N,H,W,C] at its input.  A square image goes through
    discriminator.conv2d_same_dgrad; any other through the same sum written for two sides."""
    gy, kernel = np.asarray(gy, np.float64), np.asarray(kernel, np.float64)
    n, h, w, _ = gy.shape
    if h == w:
        return conv2d_same_dgrad(gy, kernel, 1, h)
    gp = np.zeros((n, h + 2, w + 2, kernel.shape[2]), np.float64)
    for a in range(3):
        for b in range(3):
            gp[:, a:a + h, b:b + w] += gy @ kernel[a, b].T
    return gp[:, 1:h + 1, 1:w + 1].copy()


def _lrelu(z: np.ndarray) -> np.ndarray:
    return np.where(z >= 0, z, z.dtype.type(LRELU_ALPHA) * z)


def tail_forward(weights: Dict[str, np.ndarray], gs, f, dtype=np.float64) -> Dict[str, np.ndarray]:
    """gs [B,H,W,1], f [B,H,W,64] -> dict(x = cat[gs, f], c1, a1, c2, a2 [B,H,W,16], con_rgb [B,H,W,3]) in `dtype`:
    c1 = conv3x3_SAME(x, K1) + b1, z1 = (c1 - mean1) rstd1 gamma1 + beta1, a1 = lrelu_0.3(z1); c2 = a1 K2 + b2, z2 likewise,
    a2 = lrelu(z2); con_rgb = a2 K3 + b3."""
    T = dtype
    x = np.concatenate([np.asarray(gs, T), np.asarray(f, T)], axis=3)
    out = {"x": x}
    h = x
    for i, stem in enumerate(TAIL_LAYERS[:2], 1):
        k = np.asarray(weights[stem + "/conv/kernel"], T)
        bias, inv, mean, rstd, beta = bn_vectors(weights, stem, T)
        c = (conv3x3_same(h, k) if i == 1 else h @ k[0, 0]) + bias
        h = _lrelu((c - mean) * rstd * np.asarray(weights[stem + "/bnorm/gamma"], T) + beta)
        out["c%d" % i], out["a%d" % i] = c, h
    out["con_rgb"] = h @ np.asarray(weights["clr_conv3/conv/kernel"], T)[0, 0] + np.asarray(weights["clr_conv3/conv/bias"], T)
    return out


def tail_grad(weights: Dict[str, np.ndarray], gs, f, g_con, g_gs=None, acts: Optional[Dict[str, np.ndarray]] = None) -> Dict[str, np.ndarray]:
    """The gradient G = g_con [B,H,W,3] at con_rgb (and g_gs [B,H,W,1], the gradient that reaches gs directly, or None for none) ->
    dict(the ten variables of weights.generator_tail_trainable_names() in their own shapes, `d_f` [B,H,W,64] at clr_up3's output, `d_gs`
    [B,H,W,1] the complete gradient at gs, and the stage maps `gz2`, `gz1` [B,H,W,16] and `a1`, `a2` as used), all float64, from the
    float32 variables, in this order:
      clr_conv3        d K3[k, n] = sum a2[k] G[n];  d b3 = sum G
      clr_conv2        gz2 = leaky_grad(G K3^T, a2);  d beta2 = sum gz2;  d gamma2 = sum gz2 (c2 - mean2) rstd2;  d b2 = inv2 sum gz2;
                       d K2[k, n] = inv2[n] sum a1[k] gz2[n]
      clr_conv1        gz1 = leaky_grad((gz2 inv2) K2^T, a1);  d beta1, d gamma1, d b1 likewise;
                       d K1[a, b, c, o] = inv1[o] sum x[n, y + a - 1, x + b - 1, c] gz1[n, y, x, o], zero outside the image
      inputs           dx = the 3x3 data gradient of gz1 inv1 through K1;  d_gs = dx[..., 0] + g_gs;  d_f = dx[..., 1:]
    with rstd = 1 / sqrt(moving_variance + eps), inv = gamma rstd and the sums over every pixel of the batch.  The LeakyReLU masks are
    read from the activations (slope 0.3: a > 0 <=> z > 0; an activation of exactly +-0 takes the slope, TensorFlow's LeakyReluGrad).
    With `acts` given (a dict with `a1` and `a2`, for example the device's), those are the activations: the masks, clr_conv2's input and
    clr_conv3's input are read from them, and c2 is formed from that a1; c1 is always formed from x."""
    T = np.float64
    G = np.asarray(g_con, T)
    fw = tail_forward(weights, gs, f, T)
    x, c1 = fw["x"], fw["c1"]
    a1 = np.asarray(acts["a1"], T) if acts is not None else fw["a1"]
    a2 = np.asarray(acts["a2"], T) if acts is not None else fw["a2"]
    K1, K2, K3 = (np.asarray(weights[s + "/conv/kernel"], T) for s in TAIL_LAYERS)
    b1, inv1, mean1, rstd1, _ = bn_vectors(weights, "clr_conv1")
    b2, inv2, mean2, rstd2, _ = bn_vectors(weights, "clr_conv2")
    c2 = a1 @ K2[0, 0] + b2 if acts is not None else fw["c2"]
    ax = (0, 1, 2)
    out: Dict[str, np.ndarray] = {"a1": a1, "a2": a2}
    out["clr_conv3/conv/kernel"] = np.tensordot(a2, G, axes=(ax, ax)).reshape(K3.shape)
    out["clr_conv3/conv/bias"] = G.sum(axis=ax)
    gz2 = leaky_grad(G @ K3[0, 0].T, a2)
    out["gz2"] = gz2
    out["clr_conv2/bnorm/beta"] = gz2.sum(axis=ax)
    out["clr_conv2/bnorm/gamma"] = (gz2 * ((c2 - mean2) * rstd2)).sum(axis=ax)
    out["clr_conv2/conv/bias"] = inv2 * gz2.sum(axis=ax)
    out["clr_conv2/conv/kernel"] = (np.tensordot(a1, gz2, axes=(ax, ax)) * inv2).reshape(K2.shape)
    gz1 = leaky_grad((gz2 * inv2) @ K2[0, 0].T, a1)
    out["gz1"] = gz1
    out["clr_conv1/bnorm/beta"] = gz1.sum(axis=ax)
    out["clr_conv1/bnorm/gamma"] = (gz1 * ((c1 - mean1) * rstd1)).sum(axis=ax)
    out["clr_conv1/conv/bias"] = inv1 * gz1.sum(axis=ax)
    out["clr_conv1/conv/kernel"] = conv3x3_same_wgrad(x, gz1) * inv1
    dx = conv3x3_same_dgrad(gz1 * inv1, K1)
    out["d_gs"] = dx[..., :1] + (0.0 if g_gs is None else np.asarray(g_gs, T))
    out["d_f"] = dx[..., 1:].copy()
    return out


def objective_f64(weights: Dict[str, np.ndarray], gs, f, g_con, masks: Optional[list] = None, dtype=np.float64):
    """<g_con, con_rgb> in `dtype` with no float32 rounding anywhere: the scalar whose gradient tail_grad(g_gs=None) states.  A list
    given as `masks` receives the two LeakyReLU masks (z > 0)."""
    fw = tail_forward(weights, gs, f, dtype)
    if masks is not None:
        masks += [fw["a1"] > 0, fw["a2"] > 0]
    return (np.asarray(g_con, dtype) * fw["con_rgb"]).sum()


def grad_norms(grads: Dict[str, np.ndarray], names) -> Dict[str, Tuple[float, float]]:
    """name -> (L1, L-infinity) of grads[name] for every name of `names`: the sum and the largest of its magnitudes, in float64.
    <stage>_norms(grads) is this over the stage's <STAGE>_NORM_NAMES."""
    out = {}
    for name in names:
        m = np.abs(np.asarray(grads[name], np.float64))
        out[name] = (float(m.sum()), float(m.max()))
    return out


tail_norms = functools.partial(grad_norms, names=TAIL_NORM_NAMES)          # of `d_f`, the complete `d_gs` and each of the ten variable gradients


def example_inputs(H: int, W: int, B: int, seed: int = 0):
    """Seeded (gs [B,H,W,1], f [B,H,W,64], g_con [B,H,W,3], g_gs [B,H,W,1]) float32: gs like a grey image, f like a LeakyReLU output."""
    rng = np.random.default_rng(1000 + seed)
    gs = rng.uniform(0.0, 1.0, (B, H, W, 1)).astype(np.float32)
    f = rng.standard_normal((B, H, W, 64)).astype(np.float32)
    f = np.where(f >= 0, f, np.float32(LRELU_ALPHA) * f).astype(np.float32)
    g_con = (rng.standard_normal((B, H, W, 3)) / (B * H * W)).astype(np.float32)
    g_gs = (rng.standard_normal((B, H, W, 1)) / (B * H * W)).astype(np.float32)
    return gs, f, g_con, g_gs


# ---- the colour decoder: clr_up1, clr_up2, clr_up3
def convt3x3_same(x: np.ndarray, kernel: np.ndarray) -> np.ndarray:
    """[N,h,w,C] x [3,3,O,C] -> [N,2h,2w,O] in x's type: Conv2DTranspose(3, stride 2, SAME) without bias,
    y[n, 2i + a, 2j + b, o] += x[n, i, j, c] K[a, b, o, c], the (2h + 1, 2w + 1) scatter cropped at the end; taps in index order."""
    n, h, w, _ = x.shape
    full = np.zeros((n, 2 * h + 1, 2 * w + 1, kernel.shape[2]), x.dtype)
    for a in range(3):
        for b in range(3):
            full[:, a:a + 2 * h:2, b:b + 2 * w:2] += x @ kernel[a, b].astype(x.dtype).T
    return full[:, :2 * h, :2 * w].copy()


def _fine_padded(gz: np.ndarray) -> np.ndarray:
    """[N,2h,2w,O] -> float64 [N,2h+1,2w+1,O] with fine row 2h and column 2w zero."""
    n, h2, w2, o = gz.shape
    gp = np.zeros((n, h2 + 1, w2 + 1, o), np.float64)
    gp[:, :h2, :w2] = gz
    return gp


def convt3x3_same_wgrad(x: np.ndarray, gz: np.ndarray) -> np.ndarray:
    """A ConvT's input [N,h,w,C] and the gradient [N,2h,2w,O] at its output -> float64 [3,3,O,C]:
    Wg[a, b, o, c] = sum gz[n, 2i + a, 2j + b, o] x[n, i, j, c], fine rows 2h and columns 2w counting as 0."""
    x = np.asarray(x, np.float64)
    n, h, w, c = x.shape
    gp = _fine_padded(gz)
    out = np.zeros((3, 3, gz.shape[3], c), np.float64)
    for a in range(3):
        for b in range(3):
            out[a, b] = np.tensordot(gp[:, a:a + 2 * h:2, b:b + 2 * w:2], x, axes=([0, 1, 2], [0, 1, 2]))
    return out


def convt3x3_same_dgrad(gz: np.ndarray, kernel: np.ndarray) -> np.ndarray:
    """The gradient [N,2h,2w,O] at a ConvT's output -> float64 [N,h,w,C] at its input: dx[n, i, j, c] = sum gz[n, 2i + a, 2j + b, o]
    K[a, b, o, c], a 3x3 stride-2 correlation over the fine grid with padding 0 before and 1 after."""
    kernel = np.asarray(kernel, np.float64)
    n, h2, w2, _ = gz.shape
    h, w = h2 // 2, w2 // 2
    gp = _fine_padded(gz)
    out = np.zeros((n, h, w, kernel.shape[3]), np.float64)
    for a in range(3):
        for b in range(3):
            out += gp[:, a:a + 2 * h:2, b:b + 2 * w:2] @ kernel[a, b]
    return out


def decoder_forward(weights: Dict[str, np.ndarray], x, dtype=np.float64) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """x [B,h,w,C] (C = clr_up1's kernel's width) -> (f1 [B,2h,2w,128], f2 [B,4h,4w,96], f [B,8h,8w,64]) in `dtype`: per layer
    c = ConvT(a_in, K) + bias, z = (c - mean) rstd gamma + beta, a_out = lrelu_0.3(z)."""
    T = dtype
    h = np.asarray(x, T)
    outs = []
    for stem in DECODER_LAYERS:
        bias, _, mean, rstd, beta = bn_vectors(weights, stem, T)
        c = convt3x3_same(h, np.asarray(weights[stem + "/conv/kernel"], T)) + bias
        h = _lrelu((c - mean) * rstd * np.asarray(weights[stem + "/bnorm/gamma"], T) + beta)
        outs.append(h)
    return tuple(outs)


def _convt_layer_grad(weights: Dict[str, np.ndarray], stem: str, a_in: np.ndarray, a_out: np.ndarray, g: np.ndarray, out: Dict[str, np.ndarray]):
    """One Conv2DTranspose + BN + LeakyReLU layer of decoder_grad and grey_decoder_grad, in float64: its four variable gradients go into
    `out` under `stem`'s names -> (gz, dx), the gradient at its BatchNormalization output and at its input a_in (no mask applied)."""
    K = np.asarray(weights[stem + "/conv/kernel"], np.float64)
    bias, inv, mean, rstd, _ = bn_vectors(weights, stem)
    gz = leaky_grad(g, a_out)
    S = gz.sum(axis=(0, 1, 2))
    Wg = convt3x3_same_wgrad(a_in, gz)
    KW = (K * Wg).sum(axis=(0, 1, 3))
    out[stem + "/conv/kernel"] = Wg * inv[:, None]
    out[stem + "/conv/bias"] = inv * S
    out[stem + "/bnorm/gamma"] = ((KW + bias * S) - mean * S) * rstd
    out[stem + "/bnorm/beta"] = S
    return gz, convt3x3_same_dgrad(gz * inv, K)


def decoder_grad(weights: Dict[str, np.ndarray], x, d_f, acts: Optional[Dict[str, np.ndarray]] = None) -> Dict[str, np.ndarray]:
    """The gradient d_f [B,8h,8w,64] at f -> dict(the twelve variables of weights.generator_decoder_trainable_names() in their own shapes,
    `d_x` [B,h,w,C] at clr_up1's input x, the stage maps `gz3` [B,8h,8w,64], `gz2` [B,4h,4w,96], `gz1` [B,2h,2w,128] — the gradients at
    each BatchNormalization output — and `f1`, `f2`, `f` as used), all float64 from the float32 variables.  Per layer from the top down,
    a_in its input, a_out its output, g the gradient at a_out, K [3,3,O,C]:
      gz = leaky_grad(g, a_out);  S = sum gz;  Wg = convt3x3_same_wgrad(a_in, gz)
      d kernel = Wg inv;  d beta = S;  d bias = inv S;  d gamma = ((KW + bias S) - moving_mean S) rstd with KW[o] = sum_{a,b,c} K Wg
      (the pre-activation is sum K a_in + bias, so no second pass over the activations is needed)
      dx = convt3x3_same_dgrad(gz inv, K), the g of the layer below; clr_up1's is d_x and gets no mask (res_stack/5's LeakyReLU belongs
      to that block's own backward).
    With `acts` given (a dict with `f1`, `f2`, `f`, for example the device's), the masks and the layer inputs are read from it."""
    T = np.float64
    x = np.asarray(x, T)
    if acts is not None:
        f1, f2, f = (np.asarray(acts[k], T) for k in ("f1", "f2", "f"))
    else:
        f1, f2, f = decoder_forward(weights, x, T)
    out: Dict[str, np.ndarray] = {"f1": f1, "f2": f2, "f": f}
    g = np.asarray(d_f, T)
    for i, a_in, a_out in ((3, f2, f), (2, f1, f2), (1, x, f1)):
        out["gz%d" % i], g = _convt_layer_grad(weights, DECODER_LAYERS[i - 1], a_in, a_out, g, out)
    out["d_x"] = g
    return out


def decoder_objective_f64(weights: Dict[str, np.ndarray], x, d_f, masks: Optional[list] = None, dtype=np.float64):
    """<d_f, f> in `dtype` with no float32 rounding anywhere: the scalar whose gradient decoder_grad states.  A list given as `masks`
    receives the three LeakyReLU masks (z > 0) of f1, f2, f."""
    fs = decoder_forward(weights, x, dtype)
    if masks is not None:
        masks += [a > 0 for a in fs]
    return (np.asarray(d_f, dtype) * fs[2]).sum()


decoder_norms = functools.partial(grad_norms, names=DECODER_NORM_NAMES)    # of `d_x` and each of the twelve variable gradients


def decoder_example_inputs(h: int, w: int, B: int, seed: int = 0, C: int = 261):
    """Seeded (x [B,h,w,C], d_f [B,8h,8w,64]) float32 at a coarse grid: x like a LeakyReLU output."""
    rng = np.random.default_rng(2000 + seed)
    x = rng.standard_normal((B, h, w, C)).astype(np.float32)
    x = np.where(x >= 0, x, np.float32(LRELU_ALPHA) * x).astype(np.float32)
    d_f = (rng.standard_normal((B, 8 * h, 8 * w, 64)) / (B * h * w * 64)).astype(np.float32)
    return x, d_f


# ---- the grey decoder: up1, up2 (on cat[up1, x3]), up3 (on cat[up2, x2])
GREY_DECODER_LAYERS = ("up1", "up2", "up3")
GREY_DECODER_NORM_NAMES = ("d_x", "d_x3", "d_x2") + tuple(generator_grey_decoder_trainable_names())


def grey_decoder_forward(weights: Dict[str, np.ndarray], x, x3, x2, dtype=np.float64) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """x [B,h,w,257] (res_stack/2's output), x3 [B,2h,2w,64], x2 [B,4h,4w,64] (the encoder's skips) -> (up1 [B,2h,2w,96], up2
    [B,4h,4w,64], y [B,8h,8w,64]) in `dtype` (model.py:243-245): up1 = layer(x), up2 = layer(cat[up1, x3]), y = layer(cat[up2, x2]) with
    decoder_forward's layer, c = ConvT(a_in, K) + bias, z = (c - mean) rstd gamma + beta, a_out = lrelu_0.3(z)."""
    T = dtype
    h = np.asarray(x, T)
    outs = []
    for stem, skip in zip(GREY_DECODER_LAYERS, (None, x3, x2)):
        if skip is not None:
            h = np.concatenate([h, np.asarray(skip, T)], axis=3)
        bias, _, mean, rstd, beta = bn_vectors(weights, stem, T)
        c = convt3x3_same(h, np.asarray(weights[stem + "/conv/kernel"], T)) + bias
        h = _lrelu((c - mean) * rstd * np.asarray(weights[stem + "/bnorm/gamma"], T) + beta)
        outs.append(h)
    return tuple(outs)


def grey_decoder_grad(weights: Dict[str, np.ndarray], x, x3, x2, d_y, acts: Optional[Dict[str, np.ndarray]] = None) -> Dict[str, np.ndarray]:
    """The gradient d_y [B,8h,8w,64] at y, up3's output -> dict(the twelve variables of weights.generator_grey_decoder_trainable_names()
    in their own shapes, `d_x` [B,h,w,257] at up1's input, the skip gradients `d_x3` [B,2h,2w,64] and `d_x2` [B,4h,4w,64], the stage maps
    `gz3` [B,8h,8w,64], `gz2` [B,4h,4w,64], `gz1` [B,2h,2w,96] and `up1`, `up2`, `y` as used), all float64 from the float32 variables.
    Per layer from the top down the arithmetic is decoder_grad's; the layer inputs are cat[up2, x2], cat[up1, x3] and x, the kernels' C
    index in that order.  up3's dx has 128 channels: 0..63 are the g of up2 and take up2's LeakyReLU slope there, 64..127 are d_x2 and
    get no mask (down1's LeakyReLU belongs to the encoder's backward); up2's dx has 160: 0..95 the g of up1, 96..159 d_x3; up1's dx is d_x,
    no mask (res_stack/2's relu belongs to that block's backward).  With `acts` given (a dict with `up1`, `up2`, `y`, for example the
    device's), the masks and the layer inputs are read from it."""
    T = np.float64
    x, x3, x2 = (np.asarray(a, T) for a in (x, x3, x2))
    if acts is not None:
        up1, up2, y = (np.asarray(acts[k], T) for k in ("up1", "up2", "y"))
    else:
        up1, up2, y = grey_decoder_forward(weights, x, x3, x2, T)
    out: Dict[str, np.ndarray] = {"up1": up1, "up2": up2, "y": y}
    out["gz3"], dx = _convt_layer_grad(weights, "up3", np.concatenate([up2, x2], axis=3), y, np.asarray(d_y, T), out)
    out["d_x2"] = dx[..., 64:].copy()
    out["gz2"], dx = _convt_layer_grad(weights, "up2", np.concatenate([up1, x3], axis=3), up2, dx[..., :64], out)
    out["d_x3"] = dx[..., 96:].copy()
    out["gz1"], out["d_x"] = _convt_layer_grad(weights, "up1", x, up1, dx[..., :96], out)
    return out


def grey_decoder_objective_f64(weights: Dict[str, np.ndarray], x, x3, x2, d_y, masks: Optional[list] = None, dtype=np.float64):
    """<d_y, y> in `dtype` with no float32 rounding anywhere: the scalar whose gradient grey_decoder_grad states.  A list given as
    `masks` receives the three LeakyReLU masks (z > 0) of up1, up2, y."""
    outs = grey_decoder_forward(weights, x, x3, x2, dtype)
    if masks is not None:
        masks += [a > 0 for a in outs]
    return (np.asarray(d_y, dtype) * outs[2]).sum()


grey_decoder_norms = functools.partial(grad_norms, names=GREY_DECODER_NORM_NAMES)    # of `d_x`, `d_x3`, `d_x2` and each of the twelve variable gradients


def grey_decoder_example_inputs(h: int, w: int, B: int, seed: int = 0):
    """Seeded (x [B,h,w,257], x3 [B,2h,2w,64], x2 [B,4h,4w,64], d_y [B,8h,8w,64]) float32 at a coarse grid: x, x3, x2 like LeakyReLU
    outputs, d_y scaled as decoder_example_inputs scales d_f."""
    rng = np.random.default_rng(3000 + seed)
    acts = []
    for m, c in ((1, 257), (2, 64), (4, 64)):
        a = rng.standard_normal((B, m * h, m * w, c)).astype(np.float32)
        acts.append(np.where(a >= 0, a, np.float32(LRELU_ALPHA) * a).astype(np.float32))
    d_y = (rng.standard_normal((B, 8 * h, 8 * w, 64)) / (B * h * w * 64)).astype(np.float32)
    return acts[0], acts[1], acts[2], d_y


# ---- the upper half of res_stack/<block>: the non-local block, the skip and relu3
def _nl_stem(block: int) -> str:
    return "res_stack/%d/non_local/" % block


def nonlocal_bn_vectors(weights: Dict[str, np.ndarray], block: int = 5, dtype=np.float64):
    """(w's bias, inv, moving_mean, rstd, gamma, beta) of res_stack/<block>/non_local in `dtype`."""
    T = dtype
    st = _nl_stem(block)
    gamma, beta, mean, var = (np.asarray(weights[st + "bnorm/" + p], T) for p in ("gamma", "beta", "moving_mean", "moving_variance"))
    rstd = T(1) / np.sqrt(var + T(BN_EPS))
    return np.asarray(weights[st + "w/bias"], T), gamma * rstd, mean, rstd, gamma, beta


def nonlocal_forward(weights: Dict[str, np.ndarray], y3, xin, block: int = 5, dtype=np.float64) -> Dict[str, np.ndarray]:
    """y3 [B,h,w,257] (bnorm3's output), xin [B,h,w,C] (the block's input) -> dict(theta, phi, g, A [B,T,128], c [B,T,257],
    z [B,h,w,257], out [B,h,w,max(C, 257)]) in `dtype`, T = h w tokens per image, X = y3 as [B,T,257].  A skip narrower than the block
    (res_stack/0: C = 99) reaches the first C channels: out = lrelu_0.3(z + pad_257(xin)).
      theta = X Wt + bt, phi = X Wp + bp, g = X Wg + bg;  S = theta phi^T, P = softmax_rows(S) per image with the row maximum subtracted;
      A = P g;  c = A Ww + bw;  z = X + ((c - mean) rstd gamma + beta);  out = lrelu_0.3(pad_C(z) + xin)."""
    T = dtype
    st = _nl_stem(block)
    y3 = np.asarray(y3, T)
    xin = np.asarray(xin, T)
    B, h, w, n = y3.shape
    C = xin.shape[3]
    X = y3.reshape(B, h * w, n)
    proj = {}
    for name in ("theta", "phi", "g"):
        proj[name] = X @ np.asarray(weights[st + name + "/kernel"], T)[0, 0] + np.asarray(weights[st + name + "/bias"], T)
    S = proj["theta"] @ np.transpose(proj["phi"], (0, 2, 1))
    E = np.exp(S - S.max(axis=2, keepdims=True))
    P = E / E.sum(axis=2, keepdims=True)
    A = P @ proj["g"]
    bw, _, mean, rstd, gamma, beta = nonlocal_bn_vectors(weights, block, T)
    c = A @ np.asarray(weights[st + "w/kernel"], T)[0, 0] + bw
    z = (X + ((c - mean) * rstd * gamma + beta)).reshape(B, h, w, n)
    if C >= n:
        s = xin.copy()
        s[..., :n] += z
    else:
        s = z.copy()
        s[..., :C] += xin
    out = dict(proj)
    out.update({"S": S, "P": P, "A": A, "c": c, "z": z, "pre": s, "out": _lrelu(s)})
    return out


def nonlocal_grad(weights: Dict[str, np.ndarray], y3, xin, d_out, block: int = 5, acts: Optional[Dict[str, np.ndarray]] = None,
                  dtype=np.float64) -> Dict[str, np.ndarray]:
    """The gradient d_out [B,h,w,max(C, 257)] at res_stack/<block>'s output -> dict(the ten variables of
    weights.generator_nonlocal_trainable_names(block) in their own shapes, `d_y3` [B,h,w,257] at bnorm3's output, `d_skip` [B,h,w,C] the
    gradient the skip carries to the block's input (gz[..., :C]: all of gz for C >= 257), the stage maps `gz` [B,h,w,max(C, 257)], `dA`, `d_theta`, `d_phi`, `d_g` [B,T,128], `D` [B,T],
    and `out`, `A` as used), float64 from the float32 variables (`dtype` float32 runs the same arithmetic in float32: the error model of
    the device's hard-softmax bound).  In this order:
      gz = leaky_grad(d_out, out) (an activation of exactly +-0 takes the slope);  d_skip = gz;  dz = gz[..., :257];  Sz = sum dz
      d beta = Sz;  dc = dz inv;  d bw = inv Sz;  Wgd[k, n] = sum A[k] dz[n];  d Ww = Wgd inv[n]
      d gamma = ((KW + bw Sz) - mean Sz) rstd with KW[n] = sum_k Ww[k, n] Wgd[k, n]      (no second pass over c)
      dA = dc Ww^T;  D[i] = dA_i . A_i;  dP = dA g^T;  dS = P o (dP - D[:, None])
      d_g = P^T dA;  d_theta = dS phi;  d_phi = dS^T theta
      for each of theta, phi, g:  d W = X^T d_proj, d b = sum d_proj
      d_y3 = dz + d_theta Wt^T + d_phi Wp^T + d_g Wg^T
    With `acts` given (a dict with `out`, and optionally `A`, for example the device's), the mask and w's input are read from it."""
    T = dtype
    st = _nl_stem(block)
    fw = nonlocal_forward(weights, y3, xin, block, T)
    out_a = np.asarray(acts["out"], T) if acts is not None else fw["out"]
    A = np.asarray(acts["A"], T).reshape(fw["A"].shape) if acts is not None and "A" in acts else fw["A"]
    X = np.asarray(y3, T)
    B, h, w, n = X.shape
    X = X.reshape(B, h * w, n)
    Wt, Wp, Wg, Ww = (np.asarray(weights[st + k + "/kernel"], T)[0, 0] for k in ("theta", "phi", "g", "w"))
    bw, inv, mean, rstd, _, _ = nonlocal_bn_vectors(weights, block, T)
    gz = leaky_grad(np.asarray(d_out, T), out_a).astype(T)
    res: Dict[str, np.ndarray] = {"out": out_a, "A": A, "gz": gz, "d_skip": gz[..., :np.shape(xin)[3]].copy()}
    dz = gz[..., :n].reshape(B, h * w, n)
    Sz = dz.sum(axis=(0, 1))
    Wgd = np.tensordot(A, dz, axes=([0, 1], [0, 1]))
    KW = (Ww * Wgd).sum(axis=0)
    res[st + "bnorm/beta"] = Sz
    res[st + "w/bias"] = inv * Sz
    res[st + "w/kernel"] = (Wgd * inv).reshape(1, 1, *Ww.shape)
    res[st + "bnorm/gamma"] = ((KW + bw * Sz) - mean * Sz) * rstd
    dA = (dz * inv) @ Ww.T
    D = (dA * A).sum(axis=2)
    P = fw["P"]
    dS = P * (dA @ np.transpose(fw["g"], (0, 2, 1)) - D[:, :, None])
    d = {"g": np.transpose(P, (0, 2, 1)) @ dA, "theta": dS @ fw["phi"], "phi": np.transpose(dS, (0, 2, 1)) @ fw["theta"]}
    res.update({"dA": dA, "D": D, "d_theta": d["theta"], "d_phi": d["phi"], "d_g": d["g"]})
    d_y3 = dz.copy()
    for name, Wk in (("theta", Wt), ("phi", Wp), ("g", Wg)):
        res[st + name + "/kernel"] = np.tensordot(X, d[name], axes=([0, 1], [0, 1])).reshape(1, 1, *Wk.shape)
        res[st + name + "/bias"] = d[name].sum(axis=(0, 1))
        d_y3 = d_y3 + d[name] @ Wk.T
    res["d_y3"] = d_y3.reshape(B, h, w, n)
    return res


def nonlocal_objective_f64(weights: Dict[str, np.ndarray], y3, xin, d_out, block: int = 5, masks: Optional[list] = None, dtype=np.float64):
    """<d_out, out> in `dtype` with no float32 rounding anywhere: the scalar whose gradient nonlocal_grad states.  A list given as `masks`
    receives relu3's mask (pad(z) + xin > 0)."""
    fw = nonlocal_forward(weights, y3, xin, block, dtype)
    if masks is not None:
        masks.append(fw["pre"] > 0)
    return (np.asarray(d_out, dtype) * fw["out"]).sum()


nonlocal_norms = functools.partial(grad_norms, names=NONLOCAL_NORM_NAMES)  # of `d_y3`, `d_skip` and each of the ten variable gradients


def nonlocal_example_inputs(h: int, w: int, B: int, seed: int = 0, C: int = 261):
    """Seeded (y3 [B,h,w,257], xin [B,h,w,C], d_out [B,h,w,C]) float32 at a coarse grid: y3 like a BatchNormalization output, xin like a
    LeakyReLU output."""
    rng = np.random.default_rng(3000 + seed)
    y3 = (0.25 * rng.standard_normal((B, h, w, RES_CH))).astype(np.float32)
    xin = rng.standard_normal((B, h, w, C)).astype(np.float32)
    xin = np.where(xin >= 0, xin, np.float32(LRELU_ALPHA) * xin).astype(np.float32)
    d_out = (rng.standard_normal((B, h, w, C)) / (B * h * w * C)).astype(np.float32)
    return y3, xin, d_out


# ---- the lower half of res_stack/<block>: conv1/bnorm1/relu1, conv2/bnorm2/relu2, conv3/bnorm3
BOTTLENECK_NORM_NAMES = ("d_xin",) + tuple(generator_bottleneck_trainable_names())


def bottleneck_bn_vectors(weights: Dict[str, np.ndarray], j: int, block: int = 5, dtype=np.float64):
    """(conv<j>'s bias, inv, moving_mean, rstd, gamma, beta) of res_stack/<block>'s layer j = 1, 2, 3 in `dtype`."""
    T = dtype
    st = "res_stack/%d/" % block
    gamma, beta, mean, var = (np.asarray(weights[st + "bnorm%d/%s" % (j, p)], T) for p in ("gamma", "beta", "moving_mean", "moving_variance"))
    rstd = T(1) / np.sqrt(var + T(BN_EPS))
    return np.asarray(weights[st + "conv%d/bias" % j], T), gamma * rstd, mean, rstd, gamma, beta


def bottleneck_forward(weights: Dict[str, np.ndarray], xin, block: int = 5, dtype=np.float64) -> Dict[str, np.ndarray]:
    """xin [B,h,w,C] (the block's input; C is conv1's width, 261 for GSC, 877 for TSM) -> dict(c1, a1, c2, a2 [B,h,w,128], c3, y3
    [B,h,w,257]) in `dtype`:
      c1 = xin W1 + b1,  a1 = lrelu_0.3((c1 - mean1) rstd1 gamma1 + beta1)
      c2 = conv3x3_same(a1, K2) + b2,  a2 = lrelu_0.3(bn2(c2))
      c3 = a2 W3 + b3,  y3 = bn3(c3)
    with rstd = 1 / sqrt(moving_variance + eps)."""
    T = dtype
    st = "res_stack/%d/" % block
    x = np.asarray(xin, T)
    K1, K2, K3 = (np.asarray(weights[st + "conv%d/kernel" % j], T) for j in (1, 2, 3))
    out: Dict[str, np.ndarray] = {}
    h = x
    for j, K in ((1, K1), (2, K2), (3, K3)):
        bias, _, mean, rstd, gamma, beta = bottleneck_bn_vectors(weights, j, block, T)
        c = (conv3x3_same(h, K) if j == 2 else h @ K[0, 0]) + bias
        z = (c - mean) * rstd * gamma + beta
        out["c%d" % j] = c
        if j < 3:
            h = _lrelu(z)
            out["a%d" % j] = h
        else:
            out["y3"] = z
    return out


def bottleneck_grad(weights: Dict[str, np.ndarray], xin, d_y3, d_skip=None, block: int = 5, acts: Optional[Dict[str, np.ndarray]] = None,
                    dtype=np.float64) -> Dict[str, np.ndarray]:
    """The gradient d_y3 [B,h,w,257] at bnorm3's output and d_skip [B,h,w,C] (what the block's skip carries to its input; None: zero) ->
    dict(the twelve variables of weights.generator_bottleneck_trainable_names(block) in their own shapes, `d_xin` [B,h,w,C] the gradient at
    the block's input, and the stage maps `gz2`, `gz1` [B,h,w,128] and `a1`, `a2` as used), float64 from the float32 variables (`dtype`
    float32 runs the same arithmetic in float32).  Per layer j, gz the gradient at that BN's output and Wg the unscaled kernel gradient:
      S = sum gz;  d beta = S;  d bias = inv S;  d kernel = Wg inv[o];  d gamma = ((KW + bias S) - mean S) rstd, KW[o] = sum K[..., o] Wg[..., o]
    in this order:
      layer 3   gz = d_y3;  Wg3 = a2^T d_y3
      layer 2   gz2 = leaky_grad((d_y3 inv3) W3^T, a2);  Wg2 = conv3x3_same_wgrad(a1, gz2)
      layer 1   gz1 = leaky_grad(conv3x3_same_dgrad(gz2 inv2, K2), a1);  Wg1 = xin^T gz1;  d_xin = d_skip + (gz1 inv1) W1^T
    An activation of exactly +-0 takes the slope.  With `acts` given (a dict with `a1` and `a2`, for example the device's), the masks and
    the inputs of Wg2 and Wg3 are read from them."""
    T = dtype
    st = "res_stack/%d/" % block
    x = np.asarray(xin, T)
    if acts is not None:
        a1, a2 = np.asarray(acts["a1"], T), np.asarray(acts["a2"], T)
    else:
        fw = bottleneck_forward(weights, x, block, T)
        a1, a2 = fw["a1"], fw["a2"]
    K1, K2, K3 = (np.asarray(weights[st + "conv%d/kernel" % j], T) for j in (1, 2, 3))
    ax = (0, 1, 2)
    out: Dict[str, np.ndarray] = {"a1": a1, "a2": a2}

    def layer(j, K, gz, Wg):
        bias, inv, mean, rstd, _, _ = bottleneck_bn_vectors(weights, j, block, T)
        S = gz.sum(axis=ax)
        KW = (K * Wg).sum(axis=(0, 1, 2))
        out[st + "conv%d/kernel" % j] = (Wg * inv).astype(T)
        out[st + "conv%d/bias" % j] = inv * S
        out[st + "bnorm%d/gamma" % j] = ((KW + bias * S) - mean * S) * rstd
        out[st + "bnorm%d/beta" % j] = S
        return inv

    gz3 = np.asarray(d_y3, T)
    inv3 = layer(3, K3, gz3, np.tensordot(a2, gz3, axes=(ax, ax)).reshape(K3.shape).astype(T))
    gz2 = leaky_grad(((gz3 * inv3) @ K3[0, 0].T).astype(T), a2)
    out["gz2"] = gz2
    inv2 = layer(2, K2, gz2, conv3x3_same_wgrad(a1, gz2).astype(T))
    gz1 = leaky_grad(conv3x3_same_dgrad(gz2 * inv2, K2).astype(T), a1)
    out["gz1"] = gz1
    inv1 = layer(1, K1, gz1, np.tensordot(x, gz1, axes=(ax, ax)).reshape(K1.shape).astype(T))
    dx = ((gz1 * inv1) @ K1[0, 0].T).astype(T)
    out["d_xin"] = dx if d_skip is None else np.asarray(d_skip, T) + dx
    return out


def bottleneck_objective_f64(weights: Dict[str, np.ndarray], xin, d_y3, d_skip=None, block: int = 5, masks: Optional[list] = None,
                             dtype=np.float64):
    """<d_y3, y3> + <d_skip, xin> in `dtype` with no float32 rounding anywhere: the scalar whose gradient bottleneck_grad states.  A list
    given as `masks` receives the two LeakyReLU masks (z > 0) of a1 and a2."""
    fw = bottleneck_forward(weights, xin, block, dtype)
    if masks is not None:
        masks += [fw["a1"] > 0, fw["a2"] > 0]
    s = (np.asarray(d_y3, dtype) * fw["y3"]).sum()
    if d_skip is not None:
        s = s + (np.asarray(d_skip, dtype) * np.asarray(xin, dtype)).sum()
    return s


def bottleneck_norms(grads: Dict[str, np.ndarray], block: int = 5) -> Dict[str, Tuple[float, float]]:
    """name -> (L1, L-infinity) of `d_xin` and each of the twelve variable gradients (BOTTLENECK_NORM_NAMES for block 5)."""
    return grad_norms(grads, ("d_xin",) + tuple(generator_bottleneck_trainable_names(block)))


def bottleneck_example_inputs(h: int, w: int, B: int, seed: int = 0, C: int = 261):
    """Seeded (xin [B,h,w,C], d_y3 [B,h,w,257], d_skip [B,h,w,C]) float32 at a coarse grid: xin like a LeakyReLU output."""
    rng = np.random.default_rng(4000 + seed)
    xin = rng.standard_normal((B, h, w, C)).astype(np.float32)
    xin = np.where(xin >= 0, xin, np.float32(LRELU_ALPHA) * xin).astype(np.float32)
    d_y3 = (rng.standard_normal((B, h, w, RES_CH)) / (B * h * w * RES_CH)).astype(np.float32)
    d_skip = (rng.standard_normal((B, h, w, C)) / (B * h * w * C)).astype(np.float32)
    return xin, d_y3, d_skip


# ---- the grey heads: conv2 (mask), conv3 (con), gs
HEADS_NORM_NAMES = ("d_y",) + tuple(generator_heads_trainable_names())


def convk_same(x: np.ndarray, kernel: np.ndarray) -> np.ndarray:
    """conv3x3_same for any odd k: [N,H,W,C] x HWIO [k,k,C,O] -> [N,H,W,O] in x's type: stride 1, zero outside the image, no bias; taps in
    index order.  The image may be narrower than the window."""
    n, h, w, c = x.shape
    k = kernel.shape[0]
    r = k // 2
    xp = np.zeros((n, h + 2 * r, w + 2 * r, c), x.dtype)
    xp[:, r:r + h, r:r + w] = x
    out = np.zeros((n, h, w, kernel.shape[3]), x.dtype)
    for a in range(k):
        for b in range(k):
            out += xp[:, a:a + h, b:b + w] @ kernel[a, b].astype(x.dtype)
    return out


def convk_same_wgrad(x: np.ndarray, gy: np.ndarray, k: int = 7, dtype=np.float64) -> np.ndarray:
    """conv3x3_same_wgrad for any odd k: the input [N,H,W,C] of a k x k stride-1 SAME convolution and the gradient [N,H,W,O] at its output
    -> `dtype` [k,k,C,O]: gk[a, b, c, o] = sum x[n, i + a - r, j + b - r, c] gy[n, i, j, o], r = k // 2, zero outside the image."""
    x, gy = np.asarray(x, dtype), np.asarray(gy, dtype)
    n, h, w, c = x.shape
    r = k // 2
    xp = np.zeros((n, h + 2 * r, w + 2 * r, c), dtype)
    xp[:, r:r + h, r:r + w] = x
    out = np.zeros((k, k, c, gy.shape[3]), dtype)
    for a in range(k):
        for b in range(k):
            out[a, b] = np.tensordot(xp[:, a:a + h, b:b + w], gy, axes=([0, 1, 2], [0, 1, 2]))
    return out


def convk_same_dgrad(gy: np.ndarray, kernel: np.ndarray, dtype=np.float64) -> np.ndarray:
    """conv3x3_same_dgrad for any odd k: the gradient [N,H,W,O] at a k x k stride-1 SAME convolution's output -> `dtype` [N,H,W,C] at its
    input: dx[n, i, j, c] = sum_{a, b, o} gy[n, i - a + r, j - b + r, o] kernel[a, b, c, o], zero outside the image; taps in index order."""
    gy, kernel = np.asarray(gy, dtype), np.asarray(kernel, dtype)
    n, h, w, _ = gy.shape
    k = kernel.shape[0]
    r = k // 2
    gp = np.zeros((n, h + 2 * r, w + 2 * r, kernel.shape[2]), dtype)
    for a in range(k):
        for b in range(k):
            gp[:, a:a + h, b:b + w] += gy @ kernel[a, b].T
    return gp[:, r:r + h, r:r + w].copy()


def _heads_vars(weights: Dict[str, np.ndarray], dtype):
    K2, b2, K3, b3 = (np.asarray(weights[n], dtype) for n in ("conv2/conv/kernel", "conv2/conv/bias", "conv3/conv/kernel", "conv3/conv/bias"))
    if K2.shape != (7, 7, 64, 1) or K3.shape != (7, 7, 64, 1):
        raise ValueError("the grey heads are 7x7, 64 -> 1 (GSC or TSM weights), got %s and %s" % (K2.shape, K3.shape))
    return K2, b2, K3, b3


def heads_forward(weights: Dict[str, np.ndarray], inputs, y, dtype=np.float64) -> Dict[str, np.ndarray]:
    """inputs [B,H,W,3], y [B,H,W,64] (up3's output) -> dict(m, mask, con, gray, gs), each [B,H,W,1] in `dtype`:
    m = conv7x7_SAME(y, K2) + b2, mask = tanh(m), con = conv7x7_SAME(y, K3) + b3, gray = train_losses.gray(inputs) (float32, the float32
    weights, (r 0.2989 + g 0.587) + b 0.114: glue_kernels.h's gray3 bit for bit; a constant of the backward), gs = gray (1 + mask) + con."""
    from .train_losses import gray as gray_f32
    T = dtype
    K2, b2, K3, b3 = _heads_vars(weights, T)
    y = np.asarray(y, T)
    m = convk_same(y, K2) + b2
    mask = np.tanh(m)
    con = convk_same(y, K3) + b3
    gray = np.asarray(gray_f32(inputs), T)[..., None]          # float32 arithmetic, as the forward and the device chain form it
    return {"m": m, "mask": mask, "con": con, "gray": gray, "gs": gray * (T(1) + mask) + con}


def heads_grad(weights: Dict[str, np.ndarray], inputs, y, d_gs, acts: Optional[Dict[str, np.ndarray]] = None,
               dtype=np.float64) -> Dict[str, np.ndarray]:
    """The complete gradient d_gs [B,H,W,1] at gs -> dict(the four variables of weights.generator_heads_trainable_names() in their own
    shapes, `d_y` [B,H,W,64] at up3's output, and the stage maps `g_m`, `g_con` [B,H,W,1] and `mask` as used), in `dtype` from the float32
    variables, in this order:
      g_con = d_gs;  g_m = (d_gs gray) (1 - mask^2)
      d b3 = sum g_con;  d b2 = sum g_m
      d K3[a, b, c, 0] = sum y[n, i + a - 3, j + b - 3, c] g_con[n, i, j], zero outside the image;  d K2 the same with g_m
      d_y[n, i, j, c] = sum_{a, b} g_m[n, i - a + 3, j - b + 3] K2[a, b, c] + g_con[n, i - a + 3, j - b + 3] K3[a, b, c]
    With `acts` given (a dict with `mask`, for example the device's), that mask is used in place of tanh(m)."""
    T = dtype
    K2, _, K3, _ = _heads_vars(weights, T)
    y = np.asarray(y, T)
    if acts is not None:
        from .train_losses import gray as gray_f32
        gray = np.asarray(gray_f32(inputs), T)[..., None]
        mask = np.asarray(acts["mask"], T).reshape(gray.shape)
    else:
        fw = heads_forward(weights, inputs, y, T)
        gray, mask = fw["gray"], fw["mask"]
    g_con = np.asarray(d_gs, T).reshape(gray.shape)
    g_m = (g_con * gray) * (T(1) - mask * mask)
    ax = (0, 1, 2)
    out: Dict[str, np.ndarray] = {"g_m": g_m, "g_con": g_con, "mask": mask}
    out["conv3/conv/bias"] = g_con.sum(axis=ax)
    out["conv2/conv/bias"] = g_m.sum(axis=ax)
    out["conv3/conv/kernel"] = convk_same_wgrad(y, g_con, 7, T)
    out["conv2/conv/kernel"] = convk_same_wgrad(y, g_m, 7, T)
    out["d_y"] = convk_same_dgrad(g_m, K2, T) + convk_same_dgrad(g_con, K3, T)
    return out


def heads_objective_f64(weights: Dict[str, np.ndarray], inputs, y, d_gs, dtype=np.float64):
    """<d_gs, gs> in `dtype` with no float32 rounding anywhere: the scalar whose gradient heads_grad states."""
    fw = heads_forward(weights, inputs, y, dtype)
    return (np.asarray(d_gs, dtype).reshape(fw["gs"].shape) * fw["gs"]).sum()


heads_norms = functools.partial(grad_norms, names=HEADS_NORM_NAMES)        # of `d_y` and each of the four variable gradients


def heads_example_inputs(H: int, W: int, B: int, seed: int = 0):
    """Seeded (inputs [B,H,W,3] in [0, 1], y [B,H,W,64] like a LeakyReLU output, d_gs [B,H,W,1] of the order 1 / (B H W)) float32."""
    rng = np.random.default_rng(5000 + seed)
    inputs = rng.uniform(0.0, 1.0, (B, H, W, 3)).astype(np.float32)
    y = rng.standard_normal((B, H, W, 64)).astype(np.float32)
    y = np.where(y >= 0, y, np.float32(LRELU_ALPHA) * y).astype(np.float32)
    d_gs = (rng.standard_normal((B, H, W, 1)) / (B * H * W)).astype(np.float32)
    return inputs, y, d_gs


# ---- a chain of residual blocks: what the two trunk stages below share
def blocks_forward(weights: Dict[str, np.ndarray], xin, blocks, dtype=np.float64) -> Dict[str, np.ndarray]:
    """bottleneck_forward and nonlocal_forward of each of `blocks` in the forward's order, the first on `xin`, each next one on the
    output before -> dict(per block b `y3_<b>`, `res<b>`, `a1_<b>`, `a2_<b>`, `pre_<b>`) in `dtype`."""
    out: Dict[str, np.ndarray] = {}
    for b in blocks:
        bf = bottleneck_forward(weights, xin, b, dtype)
        nf = nonlocal_forward(weights, bf["y3"], xin, b, dtype)
        out.update({"y3_%d" % b: bf["y3"], "res%d" % b: nf["out"], "a1_%d" % b: bf["a1"], "a2_%d" % b: bf["a2"], "pre_%d" % b: nf["pre"]})
        xin = nf["out"]
    return out


def blocks_grad(weights: Dict[str, np.ndarray], rows, d_out, acts: Optional[Dict[str, np.ndarray]] = None) -> Dict[str, np.ndarray]:
    """`rows` of (block, y3, xin, out) in the backward's order, d_out the gradient at the first row's output -> dict(per block b its 22
    variables, `d_y3_<b>`, `d_skip_<b>`, `d_xin<b>` and `a1_<b>`, `a2_<b>` as used): nonlocal_grad, then bottleneck_grad, each block's
    d_xin the next row's d_out.  `acts` carries `a1_<b>`, `a2_<b>`."""
    res: Dict[str, np.ndarray] = {}
    for b, y3, xin, out in rows:
        n = nonlocal_grad(weights, y3, xin, d_out, block=b, acts={"out": out})
        a = None if acts is None else {"a1": acts["a1_%d" % b], "a2": acts["a2_%d" % b]}
        t = bottleneck_grad(weights, xin, n["d_y3"], n["d_skip"], block=b, acts=a)
        res.update((name, n[name]) for name in generator_nonlocal_trainable_names(b))
        res.update((name, t[name]) for name in generator_bottleneck_trainable_names(b))
        res.update({"d_y3_%d" % b: n["d_y3"], "d_skip_%d" % b: n["d_skip"], "d_xin%d" % b: t["d_xin"], "a1_%d" % b: t["a1"], "a2_%d" % b: t["a2"]})
        d_out = t["d_xin"]
    return res


# ---- res_stack/4, res_stack/3 and the hole: from the gradient at res_stack/5's input to the complete gradient at res_stack/2's output
COLOUR_TRUNK_BLOCKS = (4, 3)             # in the backward's order
COLOUR_TRUNK_NORM_NAMES = ("d_res2",) + tuple(generator_colour_trunk_trainable_names())
COLOUR_TRUNK_DATA = ("d_y3_4", "d_skip_4", "d_xin4", "d_y3_3", "d_skip_3", "d_xin3")


def hole_grad(xh, d_xin3, d_x=None, dtype=np.float64):
    """The backward of the hole (model.py:256-259: x_hole = x (1 - bmask), xh = cat[x_hole 257 | bmask | uv 3], bmask under
    stop_gradient): xh [B,h,w,261] (its channel 257 is bmask, in {0, 1}), d_xin3 [B,h,w,261] the gradient at xh, d_x [B,h,w,257] the grey
    branch's gradient at res_stack/2's output (None: no such term) ->
      d_res2 = d_xin3[..., :257] (1 - bmask) + d_x
    the complete gradient at res_stack/2's output, in `dtype`.  Channel 257 of d_xin3 reaches nothing (bmask is a constant), nor do
    channels 258..260 (uv is an input).  With `dtype` float32 this is the device's arithmetic exactly: the factor is 0 or 1, so the product
    is exact, and there is one float32 addition."""
    T = dtype
    keep = T(1) - np.asarray(xh, T)[..., RES_CH:RES_CH + 1]
    d = np.asarray(d_xin3, T)[..., :RES_CH] * keep
    return d if d_x is None else d + np.asarray(d_x, T)


def trunk_forward(weights: Dict[str, np.ndarray], x, bmask, uv, dtype=np.float64) -> Dict[str, np.ndarray]:
    """x [B,h,w,257] (res_stack/2's output), bmask [B,h,w,1] in {0, 1}, uv [B,h,w,3] -> dict(`xh` [B,h,w,261] and, per block b = 3, 4,
    `y3_<b>` [B,h,w,257] (bnorm3's output), `res<b>` [B,h,w,261] (the block's output), the bottleneck's `a1_<b>`, `a2_<b>` [B,h,w,128] and
    `pre_<b>` (relu3's input)) in `dtype`: xh = cat[x (1 - bmask), bmask, uv], then bottleneck_forward and nonlocal_forward of block 3 on
    xh and of block 4 on res3 (model.py:256-262)."""
    T = dtype
    x, bmask, uv = np.asarray(x, T), np.asarray(bmask, T), np.asarray(uv, T)
    out = {"xh": np.concatenate([x * (T(1) - bmask), bmask, uv], axis=3)}
    out.update(blocks_forward(weights, out["xh"], (3, 4), T))
    return out


def colour_trunk_grad(weights: Dict[str, np.ndarray], xh, y3_3, res3, y3_4, res4, d_xin5, d_x=None,
                      acts: Optional[Dict[str, np.ndarray]] = None) -> Dict[str, np.ndarray]:
    """The gradient d_xin5 [B,h,w,261] at res_stack/5's input (bottleneck_grad's d_xin) and, optionally, the grey branch's d_x [B,h,w,257]
    at res_stack/2's output (grey_decoder_grad's d_x) -> dict(`d_res2` [B,h,w,257] the complete gradient at res_stack/2's output, the 44
    variables of weights.generator_colour_trunk_trainable_names() under their own blocks' names, the intermediate data gradients `d_xin4`,
    `d_xin3` [B,h,w,261] and `d_y3_<b>`, `d_skip_<b>` per block, and `a1_<b>`, `a2_<b>` as used), float64 from the float32 variables.  The
    statements above chained, for block 4 on (y3_4, res3, res4) and then block 3 on (y3_3, xh, res3):
      nonlocal_grad(y3, xin, d_out, block=b, acts={"out": out_b}) -> d_y3, d_skip;  bottleneck_grad(xin, d_y3, d_skip, block=b) -> d_xin
    with block 4's d_xin as block 3's d_out, and hole_grad(xh, d_xin3, d_x) at the end.  `acts` carries `a1_<b>`, `a2_<b>` (for example the
    device's): the bottlenecks' masks and kernel-gradient inputs are read from them."""
    res = blocks_grad(weights, ((4, y3_4, res3, res4), (3, y3_3, xh, res3)), d_xin5, acts)
    res["d_res2"] = hole_grad(xh, res["d_xin3"], d_x)
    return res


def colour_trunk_objective_f64(weights: Dict[str, np.ndarray], x, bmask, uv, d_xin5, d_x=None, masks: Optional[list] = None, dtype=np.float64):
    """<d_xin5, res4> + <d_x, x> in `dtype` with no float32 rounding anywhere, bmask and uv constants: the scalar whose gradient with
    respect to x and the 44 variables colour_trunk_grad states.  A list given as `masks` receives the six LeakyReLU masks (z > 0) of
    blocks 3 and 4: a1, a2 and relu3's."""
    fw = trunk_forward(weights, x, bmask, uv, dtype)
    if masks is not None:
        masks += [fw[k % b] > 0 for b in (3, 4) for k in ("a1_%d", "a2_%d", "pre_%d")]
    s = (np.asarray(d_xin5, dtype) * fw["res4"]).sum()
    if d_x is not None:
        s = s + (np.asarray(d_x, dtype) * np.asarray(x, dtype)).sum()
    return s


colour_trunk_norms = functools.partial(grad_norms, names=COLOUR_TRUNK_NORM_NAMES)   # of `d_res2` and each of the 44 variable gradients


def colour_trunk_example_inputs(h: int, w: int, B: int, seed: int = 0, weights: Optional[Dict[str, np.ndarray]] = None):
    """Seeded (x [B,h,w,257] like a LeakyReLU output, bmask [B,h,w,1] Bernoulli(1/2) per pixel, uv [B,h,w,3] uniform, d_xin5 [B,h,w,261],
    d_x [B,h,w,257]) float32 at a coarse grid; with `weights`, followed by (xh, y3_3, res3, y3_4, res4): trunk_forward's on these inputs
    in float64, rounded to float32."""
    rng = np.random.default_rng(6000 + seed)
    x = rng.standard_normal((B, h, w, RES_CH)).astype(np.float32)
    x = np.where(x >= 0, x, np.float32(LRELU_ALPHA) * x).astype(np.float32)
    bmask = (rng.uniform(0.0, 1.0, (B, h, w, 1)) < 0.5).astype(np.float32)
    uv = rng.uniform(0.0, 1.0, (B, h, w, 3)).astype(np.float32)
    d_xin5 = (rng.standard_normal((B, h, w, RES_CH + 4)) / (B * h * w * (RES_CH + 4))).astype(np.float32)
    d_x = (rng.standard_normal((B, h, w, RES_CH)) / (B * h * w * RES_CH)).astype(np.float32)
    if weights is None:
        return x, bmask, uv, d_xin5, d_x
    fw = trunk_forward(weights, x, bmask, uv)
    return (x, bmask, uv, d_xin5, d_x) + tuple(fw[k].astype(np.float32) for k in ("xh", "y3_3", "res3", "y3_4", "res4"))


# ---- res_stack/2, res_stack/1 and res_stack/0: from the complete gradient at res_stack/2's output to the gradient at the trunk's input
LOWER_TRUNK_BLOCKS = (2, 1, 0)           # in the backward's order
LOWER_TRUNK_NORM_NAMES = ("d_x0",) + tuple(generator_lower_trunk_trainable_names())
LOWER_TRUNK_DATA = ("d_y3_2", "d_skip_2", "d_xin2", "d_y3_1", "d_skip_1", "d_xin1", "d_y3_0", "d_skip_0")
X0_CH = 99                               # x0 = cat[down3's output 96 | the resized uv 3]


def lower_trunk_forward(weights: Dict[str, np.ndarray], x0, dtype=np.float64) -> Dict[str, np.ndarray]:
    """x0 [B,h,w,99] = cat[down3's output 96 | the resized uv 3] -> dict(per block b = 0, 1, 2 `y3_<b>` [B,h,w,257] (bnorm3's output),
    `res<b>` [B,h,w,257] (the block's output), the bottleneck's `a1_<b>`, `a2_<b>` [B,h,w,128] and `pre_<b>` (relu3's input)) in `dtype`:
    bottleneck_forward and nonlocal_forward of block 0 on x0, whose skip reaches the first 99 output channels, of block 1 on res0 and of
    block 2 on res1 (model.py Generator.call: for i in range(n_res // 2))."""
    return blocks_forward(weights, np.asarray(x0, dtype), (0, 1, 2), dtype)


def lower_trunk_grad(weights: Dict[str, np.ndarray], x0, y3_0, res0, y3_1, res1, y3_2, res2, d_res2,
                     acts: Optional[Dict[str, np.ndarray]] = None) -> Dict[str, np.ndarray]:
    """The complete gradient d_res2 [B,h,w,257] at res_stack/2's output (colour_trunk_grad's d_res2) -> dict(`d_x0` [B,h,w,99] the
    gradient at x0 — channels 0..95 at down3's output; 96..98 belong to the resized uv, an input, and reach nothing — the 66 variables of
    weights.generator_lower_trunk_trainable_names() under their own blocks' names, the intermediate data gradients `d_xin2`, `d_xin1`
    [B,h,w,257], `d_y3_<b>` [B,h,w,257] and `d_skip_<b>` ([B,h,w,257]; block 0's [B,h,w,99]) per block, and `a1_<b>`, `a2_<b>` as used),
    float64 from the float32 variables.  The statements above chained, for block 2 on (y3_2, res1, res2), block 1 on (y3_1, res0, res1)
    and block 0 on (y3_0, x0, res0):
      nonlocal_grad(y3, xin, d_out, block=b, acts={"out": out_b}) -> d_y3, d_skip;  bottleneck_grad(xin, d_y3, d_skip, block=b) -> d_xin
    with each block's d_xin as the next block's d_out.  `acts` carries `a1_<b>`, `a2_<b>` (for example the device's): the bottlenecks'
    masks and kernel-gradient inputs are read from them."""
    res = blocks_grad(weights, ((2, y3_2, res1, res2), (1, y3_1, res0, res1), (0, y3_0, x0, res0)), d_res2, acts)
    res["d_x0"] = res.pop("d_xin0")              # the last block's d_xin is the stage's output
    return res


def lower_trunk_objective_f64(weights: Dict[str, np.ndarray], x0, d_res2, masks: Optional[list] = None, dtype=np.float64):
    """<d_res2, res2> in `dtype` with no float32 rounding anywhere: the scalar whose gradient with respect to x0 and the 66 variables
    lower_trunk_grad states.  A list given as `masks` receives the nine LeakyReLU masks (z > 0) of blocks 0, 1 and 2: a1, a2 and relu3's."""
    fw = lower_trunk_forward(weights, x0, dtype)
    if masks is not None:
        masks += [fw[k % b] > 0 for b in (0, 1, 2) for k in ("a1_%d", "a2_%d", "pre_%d")]
    return (np.asarray(d_res2, dtype) * fw["res2"]).sum()


lower_trunk_norms = functools.partial(grad_norms, names=LOWER_TRUNK_NORM_NAMES)   # of `d_x0` and each of the 66 variable gradients


def lower_trunk_example_inputs(h: int, w: int, B: int, seed: int = 0, weights: Optional[Dict[str, np.ndarray]] = None):
    """Seeded (x0 [B,h,w,99]: 96 channels like a LeakyReLU output and 3 uniform like uv; d_res2 [B,h,w,257]) float32 at a coarse grid;
    with `weights`, followed by (y3_0, res0, y3_1, res1, y3_2, res2): lower_trunk_forward's on x0 in float64, rounded to float32."""
    rng = np.random.default_rng(7000 + seed)
    x = rng.standard_normal((B, h, w, X0_CH - 3)).astype(np.float32)
    x = np.where(x >= 0, x, np.float32(LRELU_ALPHA) * x).astype(np.float32)
    x0 = np.concatenate([x, rng.uniform(0.0, 1.0, (B, h, w, 3)).astype(np.float32)], axis=3)
    d_res2 = (rng.standard_normal((B, h, w, RES_CH)) / (B * h * w * RES_CH)).astype(np.float32)
    if weights is None:
        return x0, d_res2
    fw = lower_trunk_forward(weights, x0)
    return (x0, d_res2) + tuple(fw[k].astype(np.float32) for k in ("y3_0", "res0", "y3_1", "res1", "y3_2", "res2"))
