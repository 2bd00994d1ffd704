"""The host statement of the generator's backward pass, from the output down, training=False (moving statistics).  So far the colour
tail (model.py:217-219, 267-269): clr_conv1 (3x3, cat[gs, f] 65 -> 16, BN, LeakyReLU), clr_conv2 (1x1, 16 -> 16, BN, LeakyReLU) and
clr_conv3 (1x1, 16 -> 3).  `tail_grad` writes the arithmetic out in float64 from the float32 variables; csrc/clr_tail_grad_kernels.h
is held to it (clr_tail_gpu.ColourTail)."""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np

from .discriminator import conv2d_same_dgrad, leaky_grad
from .weights import BN_EPS, LRELU_ALPHA, generator_tail_trainable_names

TAIL_LAYERS = ("clr_conv1", "clr_conv2", "clr_conv3")
TAIL_NORM_NAMES = ("d_f", "d_gs") + tuple(generator_tail_trainable_names())


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


def tail_norms(grads: Dict[str, np.ndarray]) -> Dict[str, Tuple[float, float]]:
    """name -> (L1, L-infinity) of `d_f`, the complete `d_gs` and each of the ten variable gradients (TAIL_NORM_NAMES)."""
    out = {}
    for name in TAIL_NORM_NAMES:
        m = np.abs(np.asarray(grads[name], np.float64))
        out[name] = (float(m.sum()), float(m.max()))
    return out


def example_inputs(H: int, W: int, B: int, seed: int = 0):
    """Seeded (gs [B,H,W,1], f [B,H,W,64], g_con [B,H,W,3], g_gs [B,H,W,1]) float32: gs like a grey image, f like a LeakyReLU output."""
    rng = np.random.default_rng(1000 + seed)
    gs = rng.uniform(0.0, 1.0, (B, H, W, 1)).astype(np.float32)
    f = rng.standard_normal((B, H, W, 64)).astype(np.float32)
    f = np.where(f >= 0, f, np.float32(LRELU_ALPHA) * f).astype(np.float32)
    g_con = (rng.standard_normal((B, H, W, 3)) / (B * H * W)).astype(np.float32)
    g_gs = (rng.standard_normal((B, H, W, 1)) / (B * H * W)).astype(np.float32)
    return gs, f, g_con, g_gs
