"""The VGG19 perceptual term of the reference's `train_step` as a host statement: `per_loss = style_content_loss(self.feat_extractor,
d_img)` (train_test_GSC.py:128-139, 153-160, 264, 303; utils.py:104-114), restated in numpy.  It plays the role for
csrc/vgg_kernels.h (bsr_vgg_per_loss, perceptual_gpu.Perceptual) that discriminator.py plays for its chain, and the term's data gradient d per / d con_rgb (THE BACKWARD below; bsr_vgg_per_loss_grad,
csrc/vgg_grad_kernels.h).  training=True, every other backward pass, weight gradients, the optimisers and a training loader are not here.

INPUTS.  gt, con_rgb (deshadow_img_c) [B,S,S,3] float32; S in SIZES, B in 1..MAX_B.  The 26 variables are float32
(weights.vgg_variable_shapes).

THE INPUT ROWS.  d_img = concat([gt, con_rgb], axis 0): [2B,S,S,3], rows [0, B) real, rows [B, 2B) fake.

PREPROCESSING.  tf.keras.applications.vgg19.preprocess_input(d_img * 255), which is "caffe" mode, in float32 with one rounding per
operation and no fused multiply-add:  x = d_img * 255;  the channels reversed, RGB -> BGR;  the means [103.939, 116.779, 123.68]
subtracted from B, G, R.  No scaling.  `preprocess` returns float32 [2B,S,S,3].

THE ARCHITECTURE.  Keras' VGG19(include_top=False) up to block5_conv1 (weights.VGG_BLOCKS): blocks of 2, 2, 4, 4 and 1 layers with
64, 128, 256, 512 and 512 channels, and a 2 x 2 stride-2 max pool ('valid'; every size here is even) after each of blocks 1 to 4.
A layer is Conv2D(3 x 3, stride 1, padding 'same' = one row and column of zeros on every side) + bias + ReLU:
  y[n, oy, ox, o] = max(0, sum_{a, b, c} x[n, oy + a - 1, ox + b - 1, c] k[a, b, c, o] + bias[o]),    positions outside the map reading 0,
a cross-correlation with the HWIO kernel, in float64 arithmetic from the float32 input and variables.  At S = 32 the maps of the five
blocks are 32, 16, 8, 4 and 2 on a side.  The five tapped features are the post-ReLU outputs of block{1..5}_conv1 (weights.VGG_TAPS);
block5's other layers and pool are never computed.  `forward` returns every activation by name: `input` float32 [2B,S,S,3],
`block<b>_conv<i>` and `block<b>_pool` float64.

THE LOSS.  Each feature is split in two along the batch: real = feat[:B], fake = feat[B:].  With the features rounded to float32,
every term |real - fake| is a float32; every sum is a float64 sum of those terms, kept per item as a row of PER_SUM_NAMES: [B, 5].  With
t_k the batch total of tap k (the items' rows added in order), h_k = S / 2^(k-1) and C_k the tap's channels, in float64:
  m_k = t_k / (B h_k^2 C_k)        (tf.reduce_mean(tf.abs(real - fake)), style_weight 1)
  per = (((m_1 + m_2) + m_3) + m_4) + m_5,  rounded once to float32.

WHAT IS NOT PINNED.  The ImageNet weights are in no checkpoint of the reference and are not shipped: `weights.load_vgg_weights(path)`
reads an `.npz` keyed `block<b>_conv<i>/kernel` (HWIO) and `block<b>_conv<i>/bias` (INTEGRATION.md shows how Keras' own weight file
becomes one on a machine that has Keras), and `weights.init_vgg_weights(seed)` draws He-normal kernels for tests and benchmarks.  The
architecture and the preprocessing are pinned to this restatement of Keras, not to Keras itself: tests/golden/perceptual_*.npz holds the
reference's style_content_loss, vgg_feat_extractor and train_step's statements executed over a numpy stand-in whose VGG19 and
preprocess_input are written from Keras' documentation (tools/make_perceptual_fixture.py).  TensorFlow convolves and reduces in float32
in orders of its own.

THE BACKWARD: d per / d con_rgb (`per_loss_grad`).  VGG19 is frozen (`vgg.trainable = False`, train_test_GSC.py:156) and gt is a constant, so
the data gradient with respect to con_rgb is the whole backward of the term; only the network's rows [B, 2B) are differentiated.  It is
pinned to this restatement of TensorFlow's gradient definitions, as the forward is pinned to a restatement of Keras: there is no
GradientTape stand-in to execute the reference's text over.  In float64 from the float32 variables, from the top down:
  seeds            d per / d fake_k = sign(fake_k - real_k) w_k,  w_k = float32(1 / (B h_k^2 C_k)),  sign(0) = 0 (TensorFlow's gradient of
                   tf.abs), the sign taken from the float32 features as the forward's |real - fake| terms are.
  relu_mask        g [y > 0] (ReluGrad): nothing passes at y == 0, so the device's -0 counts as 0.
  conv_dgrad       the data gradient of the layer's cross-correlation:
                     gx[n, iy, ix, c] = sum_{a, b, o} gy[n, iy - a + 1, ix - b + 1, o] k[a, b, c, o],    positions outside the map reading 0,
                   itself a 3 x 3 stride-1 SAME cross-correlation with the taps turned by 180 degrees and the channel roles swapped.
  max_pool_grad    each window's gradient goes to its first maximum in row-major order of the window (TensorFlow's kernels and torch
                   agree), zeros elsewhere.
At each block{k}_conv1 output the seed is added to the gradient arriving from deeper layers before the mask; block5_conv1 gets the seed
alone.  Through the preprocessing, with g_bgr the gradient at the network's input rounded to float32:
  grad[..., c] = (float32(255) g_bgr[..., 2 - c]) upstream,    float32 multiplies in that order, upstream 1 by default.
With `acts` given (a dict like `forward`'s, for example the device's kept activations) the masks, the pooling winners and the signs are
read from it instead of from the statement's own float64 forward, so that a comparison with the device is free of mask flips at values
that round across 0.  `per_loss_f64` is the same objective with no float32 rounding anywhere, for finite differences.

The objective this term is one of (g_total_loss, d_total_loss, PER_WEIGHT, the total gradient) and the command that evaluates it on a folder
are in objective.py: `python -m blindshadowremoval_amd.objective`; `python -m blindshadowremoval_amd.perceptual` delegates to it.
"""
from __future__ import annotations

import sys
from typing import Dict, List, Tuple

import numpy as np

from .discriminator import conv2d_same
from .shadow_synth import SIZES
from .weights import VGG_BLOCKS, VGG_LAYERS, VGG_TAPS, init_vgg_weights, load_vgg_weights, vgg_variable_shapes  # noqa: F401

f32 = np.float32
MAX_B = 4096
MEANS_BGR = (f32(103.939), f32(116.779), f32(123.68))
PER_SUM_NAMES = tuple("l1_block%d" % b for b in range(1, 6))
K = len(PER_SUM_NAMES)
TAP_CH = tuple(ch for ch, _ in VGG_BLOCKS)
SIZE_TEXT = "the perceptual term takes 1..4096 items of side 32, 64, 128 or 256, got B=%d S=%d"


def tap_sides(S: int) -> List[int]:
    """The sides h_k of the five tapped features."""
    return [S >> k for k in range(K)]


def check_inputs(gt, con_rgb) -> Tuple[int, int]:
    g, c = np.asarray(gt), np.asarray(con_rgb)
    if g.ndim != 4:
        raise ValueError("perceptual: gt must be [B,S,S,3], got %s" % (g.shape,))
    B, S = g.shape[:2]
    if S not in SIZES or not 1 <= B <= MAX_B:
        raise ValueError(SIZE_TEXT % (B, S))
    for name, a in (("gt", g), ("con_rgb", c)):
        if a.shape != (B, S, S, 3):
            raise ValueError("perceptual: %s must be [%d,%d,%d,3] like gt, got %s" % (name, B, S, S, a.shape))
    return B, S


def preprocess(gt, con_rgb) -> np.ndarray:
    """vgg19.preprocess_input(concat([gt, con_rgb]) * 255): float32 [2B,S,S,3], BGR, the means subtracted."""
    x = np.concatenate([np.asarray(gt, f32), np.asarray(con_rgb, f32)], axis=0) * f32(255)
    x = x[..., ::-1]
    out = np.empty(x.shape, f32)
    for c in range(3):
        out[..., c] = x[..., c] - MEANS_BGR[c]
    return out


def conv_relu(weights: Dict[str, np.ndarray], name: str, x: np.ndarray) -> np.ndarray:
    """Layer `name` (`block<b>_conv<i>`) on [N,H,W,C] -> float64 [N,H,W,O]."""
    return np.maximum(conv2d_same(x, weights[name + "/kernel"], weights[name + "/bias"], 1), 0.0)


def max_pool(x: np.ndarray) -> np.ndarray:
    """2 x 2 stride-2 max pool of [N,H,W,C], H and W even."""
    n, h, w, c = x.shape
    return x.reshape(n, h // 2, 2, w // 2, 2, c).max(axis=(2, 4))


def forward(weights: Dict[str, np.ndarray], gt, con_rgb) -> Dict[str, np.ndarray]:
    """Every activation up to block5_conv1: `input`, `block<b>_conv<i>`, `block<b>_pool` (b = 1..4)."""
    check_inputs(gt, con_rgb)
    acts: Dict[str, np.ndarray] = {"input": preprocess(gt, con_rgb)}
    h = acts["input"].astype(np.float64)
    for b, (_, n) in enumerate(VGG_BLOCKS):
        for i in range(n):
            name = "block%d_conv%d" % (b + 1, i + 1)
            h = conv_relu(weights, name, h)
            acts[name] = h
        if b < len(VGG_BLOCKS) - 1:
            h = max_pool(h)
            acts["block%d_pool" % (b + 1)] = h
    return acts


def features_of(acts: Dict[str, np.ndarray]) -> List[np.ndarray]:
    """The five tapped features of `forward`'s result."""
    return [np.asarray(acts[n]) for n in VGG_TAPS]


def sums_from_features(feats) -> np.ndarray:
    """Five features [2B,h_k,h_k,C_k] -> float64 [B,5] (PER_SUM_NAMES): per item the float64 sums of the float32 terms |real - fake|."""
    B = np.asarray(feats[0]).shape[0] // 2
    sums = np.zeros((B, K), np.float64)
    for k, feat in enumerate(feats):
        y = np.asarray(feat).astype(f32)
        assert y.ndim == 4 and y.shape[0] == 2 * B
        sums[:, k] = np.abs(y[:B] - y[B:]).reshape(B, -1).sum(axis=1, dtype=np.float64)
    return sums


def loss_from_sums(sums: np.ndarray, S: int) -> np.ndarray:
    """float64 [B,5] and the input side -> float32 [1]: per over the whole batch."""
    sums = np.asarray(sums, np.float64)
    t = np.zeros(K, np.float64)
    for row in sums:
        t = t + row
    m = [t[k] / (float(sums.shape[0]) * float(h * h * TAP_CH[k])) for k, h in enumerate(tap_sides(S))]
    return np.array([(((m[0] + m[1]) + m[2]) + m[3]) + m[4]], np.float64).astype(f32)


def per_loss(weights: Dict[str, np.ndarray], gt, con_rgb) -> Dict[str, np.ndarray]:
    """Batches -> dict(loss float32 [1], sums float64 [B,5], acts: `forward`'s dict)."""
    _, S = check_inputs(gt, con_rgb)
    acts = forward(weights, gt, con_rgb)
    sums = sums_from_features(features_of(acts))
    return {"loss": loss_from_sums(sums, S), "sums": sums, "acts": acts}


# ---- the backward: d per / d con_rgb
GRAD_NAMES = ("per_grad_l1", "per_grad_linf")


def tap_weights(B: int, S: int) -> List[np.float32]:
    """w_k = float32(1 / (B h_k^2 C_k)), k = 1..5."""
    return [f32(1.0 / (float(B) * float(h * h * TAP_CH[k]))) for k, h in enumerate(tap_sides(S))]


def seeds(feats, B: int) -> List[np.ndarray]:
    """Five features [2B,h_k,h_k,C_k] -> five float32 [B,h_k,h_k,C_k]: d per / d fake_k = sign(fake_k - real_k) w_k, sign(0) = 0."""
    S = np.asarray(feats[0]).shape[1]
    out = []
    for k, (feat, w) in enumerate(zip(feats, tap_weights(B, S))):
        y = np.asarray(feat).astype(f32)
        assert y.ndim == 4 and y.shape[0] == 2 * B
        out.append(np.sign(y[B:] - y[:B]).astype(f32) * w)
    return out


def conv_dgrad(weights: Dict[str, np.ndarray], name: str, g: np.ndarray) -> np.ndarray:
    """The gradient [N,H,W,O] at layer `name`'s convolution output -> float64 [N,H,W,C] at its input."""
    kernel = np.asarray(weights[name + "/kernel"], np.float64)
    g = np.asarray(g, np.float64)
    n, h, w, _ = g.shape
    gp = np.zeros((n, h + 2, w + 2, g.shape[3]), np.float64)
    gp[:, 1:1 + h, 1:1 + w] = g
    out = np.zeros((n, h, w, kernel.shape[2]), np.float64)
    for a in range(3):
        for b in range(3):
            out += gp[:, 2 - a:2 - a + h, 2 - b:2 - b + w] @ kernel[a, b].T
    return out


def relu_mask(g: np.ndarray, y: np.ndarray) -> np.ndarray:
    """g [y > 0]: ReluGrad on the layer's post-ReLU output y."""
    return np.where(np.asarray(y) > 0, g, np.zeros((), np.asarray(g).dtype))


def max_pool_grad(g: np.ndarray, x: np.ndarray) -> np.ndarray:
    """The gradient [N,h,w,C] at max_pool(x)'s output -> [N,2h,2w,C] at x: each window's value at its first maximum in row-major order."""
    g, x = np.asarray(g), np.asarray(x)
    n, h, w, c = g.shape
    assert x.shape == (n, 2 * h, 2 * w, c)
    win = x.reshape(n, h, 2, w, 2, c).transpose(0, 1, 3, 5, 2, 4).reshape(n, h, w, c, 4)
    first = np.argmax(win, axis=-1)                      # numpy's argmax is the first maximum; -0 and 0 compare equal
    out = np.zeros((n, h, w, c, 4), g.dtype)
    np.put_along_axis(out, first[..., None], g[..., None], axis=-1)
    return out.reshape(n, h, w, c, 2, 2).transpose(0, 1, 4, 2, 5, 3).reshape(n, 2 * h, 2 * w, c)


def input_grad(g_bgr: np.ndarray, upstream=None) -> np.ndarray:
    """The gradient at the network's input [B,S,S,3] (BGR) -> float32 d / d con_rgb: (255 g_bgr[2 - c]) upstream in float32."""
    up = f32(1) if upstream is None else f32(np.asarray(upstream).reshape(-1)[0])
    return (f32(255) * np.asarray(g_bgr).astype(f32)[..., ::-1]) * up


def per_loss_grad(weights: Dict[str, np.ndarray], gt, con_rgb, upstream=None, acts=None) -> Dict[str, np.ndarray]:
    """`per_loss`'s dict plus `grad`: float32 [B,S,S,3] = d per / d con_rgb * upstream (a float32, 1 without it), and `grad_input`:
    float64 [B,S,S,3], the gradient at the network's input (BGR) before any float32 rounding.  Without `acts` the
    masks, pooling winners and signs come from the statement's own float64 forward; with `acts` from it, and `loss` and `sums` are
    then those of its features."""
    B, S = check_inputs(gt, con_rgb)
    if acts is None:
        res = per_loss(weights, gt, con_rgb)
    else:
        sums = sums_from_features(features_of(acts))
        res = {"loss": loss_from_sums(sums, S), "sums": sums, "acts": acts}
    A = res["acts"]
    seed = dict(zip(VGG_TAPS, seeds(features_of(A), B)))
    g = None
    for i in reversed(range(len(VGG_LAYERS))):
        name = VGG_LAYERS[i]
        if name in seed:
            g = seed[name].astype(np.float64) if g is None else g + seed[name]
        g = conv_dgrad(weights, name, relu_mask(g, np.asarray(A[name])[B:]))
        if i > 0 and name.endswith("conv1"):
            g = max_pool_grad(g, np.asarray(A[VGG_LAYERS[i - 1]])[B:])
    res = dict(res)
    res["grad_input"] = g
    res["grad"] = input_grad(g, upstream)
    return res


def per_loss_f64(weights: Dict[str, np.ndarray], gt, con_rgb) -> float:
    """per as a function of float64 images with no float32 rounding anywhere (the variables are still the float32 ones): what
    per_loss_grad differentiates, for finite differences."""
    x = np.concatenate([np.asarray(gt, np.float64), np.asarray(con_rgb, np.float64)], axis=0) * 255.0
    h = x[..., ::-1] - np.array([float(m) for m in MEANS_BGR])
    B, per = x.shape[0] // 2, 0.0
    for b, (_, n) in enumerate(VGG_BLOCKS):
        for i in range(n):
            h = conv_relu(weights, "block%d_conv%d" % (b + 1, i + 1), h)
            if i == 0:
                per = per + float(np.abs(h[:B] - h[B:]).mean())
        if b < len(VGG_BLOCKS) - 1:
            h = max_pool(h)
    return per


def example_inputs(S: int, B: int, seed: int = 0):
    """gt, con_rgb of train_losses.example_inputs(S, B, seed)."""
    from .train_losses import example_inputs as ex
    _, gt, _, _, con = ex(S, B, seed)
    return gt, con


def main(argv=None) -> int:
    """The objective command under its earlier name."""
    from .objective import main as objective_main
    return objective_main(argv)


if __name__ == "__main__":
    sys.exit(main())
