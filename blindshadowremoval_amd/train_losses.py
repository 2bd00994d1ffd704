"""The reconstruction and gradient losses of the reference's `train_step` as a host statement: `recon_gs`, `recon_c` and `grad`
(train_test_GSC.py:107-115, 253-258, 287-301, 307-328, 357; utils.py:22-52, 116-125), restated in numpy.  It plays the role for
csrc/train_losses_kernels.h (bsr_train_losses, train_losses_gpu.TrainLosses) that shadow_synth.py plays for its chain.  The three
discriminators, the VGG perceptual term, `mask_loss` (computed by the reference and never used), the generator's backward pass and the
optimisers are not here; the three losses' own gradient with respect to gs and con_rgb is (THE BACKWARD, below).

INPUTS.  img, gt, mask_sv [B,S,S,3], gs (deshadow_img_gs) [B,S,S,1], con_rgb (deshadow_img_c) [B,S,S,3], float32; S in
shadow_synth.SIZES, B in 1..65535.

THE PER-PIXEL ARITHMETIC (float32; every product, sum and quotient rounded on its own, no fused multiply-add).
  gray(x)        (x0 * 0.2989 + x1 * 0.587) + x2 * 0.114                      tf.image.rgb_to_grayscale, left to right
  yuv(x)         Y = (x0 * .299 + x1 * .587) + x2 * .114;  U = (x0 * -.168736 + x1 * -.331264) + x2 * .5;
                 V = (x0 * .5 + x1 * -.418688) + x2 * -.081312                l1_loss_yuv, left to right
  mask_bi        mask_sv > .01, per channel (three channels)
  find_edge      mean_c = ((m0 + m1) + m2) / 3;  min_c = min(m0, m1, m2);  edge0 = (mean_c > .01) - (min_c > .3), which is 0 or 1;
                 then twice: tf.nn.dilation2d with a 5 x 5 filter of ones and SAME padding, minus 1 — a 5 x 5 maximum in which positions
                 outside the image do not take part; mask_edge = result > 0, one channel.  Two such maxima are one 9 x 9 window
                 clipped to the image: mask_edge is 1 where any edge0 pixel within 4 rows and 4 columns is 1.
  bmaskgt        (gray(gt) - gray(img)) > 0.04, one channel
  a_gs           |gs - gray(gt)|;   a_c = |con_rgb - gt| per channel;   a_y, a_u, a_v = |yuv(con_rgb) - yuv(gt)|
  get_img_grad(x, scale), scale = 1, 2, 4, 8, 16:  r = x for scale 1, else tf.image.resize(x, S / scale) (bilinear, half-pixel centres,
                 no antialiasing: ucb_post.resize_bilinear's arithmetic); tf.image.image_gradients: dy[i, j] = r[i + 1, j] - r[i, j],
                 dx[i, j] = r[i, j + 1] - r[i, j], the last row of dy and the last column of dx zero; g = (dy + dx) * 5; for scale > 1
                 the same resize back to S.
  dif_grad_k     a = |grad_k(con_rgb) - grad_k(gt)|;  ((a + (30 * a) * mask_bi) + (10 * a) * mask_edge) / 41, three channels
  dif_grad       (((dif_grad_1 + dif_grad_2) + dif_grad_3) + dif_grad_4) + dif_grad_5;  the figure is dif_grad / 1.2

THE REDUCTIONS.  Every sum is a float64 sum of those float32 terms, kept per item as a row of `SUM_NAMES` (K = 18 partial sums):
the unmasked, mask_bi and mask_edge sums of a_gs, a_c, a_y, a_u, a_v; sum(mask_bi); sum(mask_edge); sum(dif_grad).  The reference's
broadcasting is kept as written: a one-channel |x - y| times the three-channel mask_bi sums three times (once per channel of
mask_bi that is lit), a three-channel |x - y| times the one-channel mask_edge sums its three channels.

THE LOSSES are formed from the batch totals t (the items' rows added in order) in float64, in this order, and rounded once to
float32.  The reductions run over the whole batch, not per item.  n = B S S; d_bi = t[n_bi] + 1e-6; d_edge = t[n_edge] + 1e-6.
  recon_gs = ((t[gs] / n + (t[gs_bi] / d_bi) * 30) + (t[gs_edge] / d_edge) * 10) / 41
  l1 = t[c] / (n * 3);  l1_bi = t[c_bi] / d_bi / 3;  l1_edge = t[c_edge] / d_edge / 3        (l1_loss divides by x.shape[3] under a mask)
  yuv = ((t[y] / n + t[u] / n) + t[v] / n) / 2;  yuv_bi, yuv_edge: the same with the masked sums over d_bi, d_edge
  recon_c = (((((l1 + l1_bi * 30) + l1_edge * 10) + yuv) + yuv_bi * 30) + yuv_edge * 10) / 82
  grad = t[dif_grad] / d_edge

ONE RULE OF OUR OWN.  `min_c > .3` is stated as "every channel > .3", so that a comparison with a NaN is false here and on the device
alike (the reference's result for a NaN is whatever its reduce_min returns).

WHAT IS NOT PINNED.  TensorFlow reduces in float32 in an order of its own, and adds 1e-6 in float32; tests/golden/train_losses_*.npz
holds the reference's functions and statements executed over a numpy stand-in (tools/make_train_losses_fixture.py), and
tests/test_train_losses_fixture.py holds this statement to it.

THE BACKWARD (step_losses_grad; csrc/train_losses_kernels.h: bsr_train_losses_grad).  The gradient of u_gs recon_gs + u_c recon_c +
u_g grad with respect to gs and con_rgb, `upstream` = (u_gs, u_c, u_g) float32, ones by default; G_TOTAL_WEIGHTS = (200, 200, 2) are
the terms' weights in g_total_loss.  img, gt, the masks and the denominators n, d_bi, d_edge are constants of the tape.  Per pixel: nb =
the number of lit mask_bi channels, bi_c = mask_bi's channel c, e = mask_edge.  Everything below is float64 in the written order and
rounded once to float32; sign(0) = 0 (TensorFlow's gradient of tf.abs); every sign is the sign of the float32 difference the forward
forms.
  W1             (1 / n + (30 * nb) / d_bi) + (10 * e) / d_edge
  grad_gs        ((u_gs * sign(gs - gray(gt))) * W1) / 41
  A_c            (1 / (3 n) + (30 * bi_c) / (3 d_bi)) + (10 * e) / (3 d_edge)
  d_recon_c[c]   (u_c * (sign(con_c - gt_c) * A_c + ((((sY * YUV_W[0][c] + sU * YUV_W[1][c]) + sV * YUV_W[2][c]) * W1) / 2))) / 82,
                 sK = sign(K(con_rgb) - K(gt))
  d_grad, per level l = 0..4 (scale 2^l, s = S >> l), U_l the resize s -> S and R_l the resize S -> s as float64 matrices of
  resize_weights (row i holds 1 - lerp at `lower` and lerp at `upper`; U_0 = R_0 = identity):
    D_l[p, c]    (sign(v_con - v_gt) * (((1 + 30 * bi_c) + 10 * e) / 41)) / d_edge, v the forward's float32 samples at S
    g_l          U_l^T D_l along both axes: the maps g0..g4, [s, s, 3]
    rbar_l[i,j]  5 * (((g[i-1, j] [i >= 1] - g[i, j] [i + 1 < s]) + g[i, j-1] [j >= 1]) - g[i, j] [j + 1 < s]): the transpose of (dy + dx) * 5
                 with its zero last row and last column
    R_l^T rbar_l for these power-of-two scales each coarse pixel reads the 2 x 2 fine pixels at rows and columns scale c + scale / 2 - 1
                 and scale c + scale / 2 with weight 1/4 each (resize_quarter_taps; asserted against resize_bilinear in the tests), so
                 a fine pixel receives at most one contribution per level
  d_grad         u_g * ((((t_0 + t_1) + t_2) + t_3) + t_4), t_l = R_l^T rbar_l;   grad_con = d_recon_c + d_grad, added in float64
With f64=True the same objective is evaluated with no float32 rounding anywhere: gray, yuv, both resizes, the differences and so the
signs are float64 (the float32 constants GRAY_W, YUV_W and the resize weights keep their values).  That form is what is compared with
autograd; the float32-sign form equals it wherever the signs agree.

`python -m blindshadowremoval_amd.train_losses FOLDER [--ckpt DIR] [--batch N] [--host] [--grad]` scores a generator on a folder written by
`python -m blindshadowremoval_amd.shadow_synth` (<name>.png, <name>-gt.png, <name>-mask.png, <name>.npy per item): the network inputs
come from Dataset(config, 'test'), the generator runs on row 0 of each element (weights from the latest checkpoint under --ckpt, from
init_weights without it), and the step-weighted means of the three losses are printed as Logging.display prints them.  --host
computes the losses with this statement from the same generator outputs.  --grad adds, per batch, the L1 and L-infinity norms of the
gradients with respect to gs and con_rgb under G_TOTAL_WEIGHTS (GRAD_NAMES), on either route.
The folder handling and the loop are objective.py's (folder_steps, score_steps), as is the objective these losses are terms of.
"""
from __future__ import annotations

import sys
from typing import Dict, Optional, Tuple

import numpy as np

from .shadow_synth import SIZES
from .ucb_post import resize_bilinear, resize_weights

f32 = np.float32
SCALES = (1, 2, 4, 8, 16)
SUM_NAMES = ("gs", "gs_bi", "gs_edge", "c", "c_bi", "c_edge", "y", "y_bi", "y_edge", "u", "u_bi", "u_edge", "v", "v_bi", "v_edge",
             "n_bi", "n_edge", "dif_grad")
K = len(SUM_NAMES)
IDX = {n: i for i, n in enumerate(SUM_NAMES)}
LOSS_NAMES = ("recon_gs", "recon_c", "grad")
GRAY_W = (f32(0.2989), f32(0.587), f32(0.114))
YUV_W = ((f32(.299), f32(.587), f32(.114)), (f32(-.168736), f32(-.331264), f32(.5)), (f32(.5), f32(-.418688), f32(-.081312)))


def _weighted(x: np.ndarray, w) -> np.ndarray:
    return (x[..., 0] * w[0] + x[..., 1] * w[1]) + x[..., 2] * w[2]


def gray(x: np.ndarray) -> np.ndarray:
    """[...,3] float32 -> [...] float32."""
    return _weighted(np.asarray(x, f32), GRAY_W)


def yuv(x: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    x = np.asarray(x, f32)
    return tuple(_weighted(x, w) for w in YUV_W)


def edge0(mask_sv: np.ndarray) -> np.ndarray:
    """[...,S,S,3] -> float32 [...,S,S]: (mean_c > .01) - (min_c > .3)."""
    m = np.asarray(mask_sv, f32)
    mean_c = ((m[..., 0] + m[..., 1]) + m[..., 2]) / f32(3.0)
    with np.errstate(invalid="ignore"):
        above = (m[..., 0] > f32(.3)) & (m[..., 1] > f32(.3)) & (m[..., 2] > f32(.3))          # min_c > .3
        return (mean_c > f32(.01)).astype(f32) - above.astype(f32)


def dilate5(e: np.ndarray) -> np.ndarray:
    """The reference's `dilation2d(e, ones(5,5,1), SAME) - 1` on [...,S,S]: a 5 x 5 maximum over the positions inside the image."""
    S0, S1 = e.shape[-2], e.shape[-1]
    pad = np.full(e.shape[:-2] + (S0 + 4, S1 + 4), -np.inf, f32)
    pad[..., 2:-2, 2:-2] = e
    out = np.full(e.shape, -np.inf, f32)
    for dy in range(5):
        for dx in range(5):
            out = np.maximum(out, pad[..., dy:dy + S0, dx:dx + S1])
    return out


def find_edge(mask_sv: np.ndarray) -> np.ndarray:
    """[...,S,S,3] -> mask_edge float32 [...,S,S]."""
    return (dilate5(dilate5(edge0(mask_sv))) > 0).astype(f32)


def coarse_grad(x: np.ndarray, scale: int) -> np.ndarray:
    """One item [S,S,C] -> (dy + dx) * 5 of the image resized to S / scale: float32 [S/scale, S/scale, C]."""
    x = np.asarray(x, f32)
    r = x if scale == 1 else resize_bilinear(x, x.shape[0] // scale)
    dy, dx = np.zeros_like(r), np.zeros_like(r)
    dy[:-1] = r[1:] - r[:-1]
    dx[:, :-1] = r[:, 1:] - r[:, :-1]
    return (dy + dx) * f32(5.0)


def img_grad(x: np.ndarray, scale: int) -> np.ndarray:
    """get_img_grad for one item [S,S,C]."""
    g = coarse_grad(x, scale)
    return g if scale == 1 else resize_bilinear(g, np.asarray(x).shape[0])


def check_inputs(img, gt, mask_sv, gs, con_rgb) -> Tuple[int, int]:
    arrays = [np.asarray(a) for a in (img, gt, mask_sv, gs, con_rgb)]
    if arrays[1].ndim != 4:
        raise ValueError("train_losses: gt must be [B,S,S,3], got %s" % (arrays[1].shape,))
    B, S = arrays[1].shape[:2]
    if S not in SIZES or not 1 <= B <= 65535:
        raise ValueError("train_losses takes 1..65535 items of side 32, 64, 128 or 256, got B=%d S=%d" % (B, S))
    for name, a, c in (("img", arrays[0], 3), ("gt", arrays[1], 3), ("mask_sv", arrays[2], 3), ("gs", arrays[3], 1), ("con_rgb", arrays[4], 3)):
        if a.shape != (B, S, S, c):
            raise ValueError("train_losses: %s must be [%d,%d,%d,%d] like gt, got %s" % (name, B, S, S, c, a.shape))
    return B, S


def item_terms(img, gt, mask_sv, gs, con_rgb) -> Dict[str, np.ndarray]:
    """One item -> dict(mask_edge, bmaskgt [S,S], dif_grad [S,S,3] (the figure: / 1.2), sums float64 [K])."""
    img, gt, mask_sv, gs, con_rgb = (np.asarray(a, f32) for a in (img, gt, mask_sv, gs, con_rgb))
    with np.errstate(invalid="ignore"):
        mask_bi = (mask_sv > f32(.01)).astype(f32)
        mask_edge = find_edge(mask_sv)
        g_gt = gray(gt)
        bmaskgt = ((g_gt - gray(img)) > f32(0.04)).astype(f32)
    planes = {"gs": np.abs(gs[..., 0] - g_gt)[..., None], "c": np.abs(con_rgb - gt)}
    for name, a, b in zip("yuv", yuv(con_rgb), yuv(gt)):
        planes[name] = np.abs(a - b)[..., None]
    me = mask_edge[..., None]
    total = None
    for scale in SCALES:
        a = np.abs(img_grad(con_rgb, scale) - img_grad(gt, scale))
        d = ((a + (f32(30.0) * a) * mask_bi) + (f32(10.0) * a) * me) / f32(41.0)
        total = d if total is None else total + d
    assert total.dtype == f32
    sums = np.zeros(K, np.float64)
    for name, a in planes.items():
        sums[IDX[name]] = a.sum(dtype=np.float64)
        sums[IDX[name + "_bi"]] = (a * mask_bi).sum(dtype=np.float64)          # a one-channel a broadcasts over mask_bi's three channels
        sums[IDX[name + "_edge"]] = (a * me).sum(dtype=np.float64)
    sums[IDX["n_bi"]] = mask_bi.sum(dtype=np.float64)
    sums[IDX["n_edge"]] = mask_edge.sum(dtype=np.float64)
    sums[IDX["dif_grad"]] = total.sum(dtype=np.float64)
    return {"mask_edge": mask_edge, "bmaskgt": bmaskgt, "dif_grad": total / f32(1.2), "sums": sums}


def batch_totals(sums: np.ndarray) -> np.ndarray:
    """float64 [B,K] -> float64 [K]: the items' rows added in order."""
    t = np.zeros(K, np.float64)
    for row in np.asarray(sums, np.float64):
        t = t + row
    return t


def losses_from_sums(sums: np.ndarray, S: int) -> np.ndarray:
    """float64 [B,K] -> float32 [3]: recon_gs, recon_c, grad over the whole batch."""
    sums = np.asarray(sums, np.float64)
    t = batch_totals(sums)
    n = float(sums.shape[0] * S * S)
    d_bi, d_edge = t[IDX["n_bi"]] + 1e-6, t[IDX["n_edge"]] + 1e-6
    g = lambda name: t[IDX[name]]
    recon_gs = ((g("gs") / n + (g("gs_bi") / d_bi) * 30.0) + (g("gs_edge") / d_edge) * 10.0) / 41.0
    l1, l1_bi, l1_edge = g("c") / (n * 3.0), g("c_bi") / d_bi / 3.0, g("c_edge") / d_edge / 3.0
    yuv_all = ((g("y") / n + g("u") / n) + g("v") / n) / 2.0
    yuv_bi = ((g("y_bi") / d_bi + g("u_bi") / d_bi) + g("v_bi") / d_bi) / 2.0
    yuv_edge = ((g("y_edge") / d_edge + g("u_edge") / d_edge) + g("v_edge") / d_edge) / 2.0
    recon_c = (((((l1 + l1_bi * 30.0) + l1_edge * 10.0) + yuv_all) + yuv_bi * 30.0) + yuv_edge * 10.0) / 82.0
    grad = g("dif_grad") / d_edge
    return np.array([recon_gs, recon_c, grad], np.float64).astype(f32)


def step_losses(img, gt, mask_sv, gs, con_rgb) -> Dict[str, np.ndarray]:
    """Batches -> dict(losses float32 [3] (LOSS_NAMES), sums float64 [B,K], mask_edge, bmaskgt [B,S,S,1], dif_grad [B,S,S,3])."""
    B, S = check_inputs(img, gt, mask_sv, gs, con_rgb)
    items = [item_terms(img[i], gt[i], mask_sv[i], gs[i], con_rgb[i]) for i in range(B)]
    sums = np.stack([it["sums"] for it in items])
    return {"losses": losses_from_sums(sums, S), "sums": sums, "mask_edge": np.stack([it["mask_edge"] for it in items])[..., None],
            "bmaskgt": np.stack([it["bmaskgt"] for it in items])[..., None], "dif_grad": np.stack([it["dif_grad"] for it in items])}


# ---- the backward
G_TOTAL_WEIGHTS = (200.0, 200.0, 2.0)          # recon_gs, recon_c and grad in g_total_loss = recon * 400 + gan + per * .005 + grad * 2, recon = (gs + c) / 2
GRAD_NAMES = ("grad_gs_l1", "grad_gs_linf", "grad_con_l1", "grad_con_linf")
UPSTREAM_TEXT = "upstream must be three float32 values (the weights of recon_gs, recon_c and grad), or None"


def resize_matrix(out_size: int, in_size: int) -> np.ndarray:
    """The bilinear resize in_size -> out_size along one axis as a float64 matrix [out_size, in_size] of resize_weights."""
    lower, upper, lerp = resize_weights(out_size, in_size)
    m = np.zeros((out_size, in_size), np.float64)
    rows = np.arange(out_size)
    np.add.at(m, (rows, lower), 1.0 - lerp.astype(np.float64))
    np.add.at(m, (rows, upper), lerp.astype(np.float64))
    return m


def apply_axes(m: np.ndarray, x: np.ndarray) -> np.ndarray:
    """m [o, i] along both axes of x [i, i, C] -> float64 [o, o, C]; with m.T the transpose of that map."""
    rows = np.tensordot(m, np.asarray(x, np.float64), axes=(1, 0))                  # [o, i, C]
    return np.tensordot(m, rows, axes=(1, 1)).transpose(1, 0, 2)


def diff5(r: np.ndarray) -> np.ndarray:
    """(dy + dx) * 5 of [s, s, C] in r's own precision, the last row of dy and the last column of dx zero."""
    dy, dx = np.zeros_like(r), np.zeros_like(r)
    dy[:-1] = r[1:] - r[:-1]
    dx[:, :-1] = r[:, 1:] - r[:, :-1]
    return (dy + dx) * r.dtype.type(5.0)


def diff5_t(g: np.ndarray) -> np.ndarray:
    """The transpose of diff5 on float64 [s, s, C]."""
    g = np.asarray(g, np.float64)
    up, left, own_y, own_x = np.zeros_like(g), np.zeros_like(g), g.copy(), g.copy()
    up[1:] = g[:-1]
    left[:, 1:] = g[:, :-1]
    own_y[-1] = 0.0
    own_x[:, -1] = 0.0
    return 5.0 * (((up - own_y) + left) - own_x)


def resize_quarter_taps(scale: int) -> Tuple[int, int]:
    """The two fine rows (columns) past scale * c that coarse pixel c of the resize S -> S / scale reads, each with weight 1/2 per axis."""
    return scale // 2 - 1, scale // 2


def resize_quarter_t(rbar: np.ndarray, scale: int) -> np.ndarray:
    """R^T of the resize S -> S / scale in its 2 x 2 quarter-weight form: float64 [s, s, C] -> [S, S, C]."""
    rbar = np.asarray(rbar, np.float64)
    if scale == 1:
        return rbar.copy()
    s = rbar.shape[0]
    out = np.zeros((s * scale, s * scale, rbar.shape[2]), np.float64)
    for dy in resize_quarter_taps(scale):
        for dx in resize_quarter_taps(scale):
            out[dy::scale, dx::scale] = 0.25 * rbar
    return out


def grad_upstream(upstream) -> np.ndarray:
    """None or three float32 values -> float64 [3] holding them."""
    if upstream is None:
        return np.ones(3, np.float64)
    u = np.asarray(upstream)
    if u.dtype != f32 or u.shape != (3,):
        raise TypeError(UPSTREAM_TEXT)
    return u.astype(np.float64)


def d_grad_from_maps(maps, u_g=1.0) -> np.ndarray:
    """The last two steps of d_grad alone: the five maps g_l [B, S >> l, S >> l, 3] -> float64 [B,S,S,3] = u_g * sum_l R_l^T rbar_l."""
    out = []
    for b in range(np.asarray(maps[0]).shape[0]):
        acc = None
        for l, scale in enumerate(SCALES):
            t = resize_quarter_t(diff5_t(maps[l][b]), scale)
            acc = t if acc is None else acc + t
        out.append(float(u_g) * acc)
    return np.stack(out)


def item_grads(gt, mask_sv, gs, con_rgb, mask_edge, n: float, d_bi: float, d_edge: float, up: np.ndarray, f64: bool = False) -> Dict[str, np.ndarray]:
    """One item and the batch's denominators -> float64 grad_gs [S,S,1], d_recon_c, d_grad [S,S,3] and the maps g [5][s,s,3]."""
    wide = np.float64 if f64 else f32
    gt, mask_sv, gs, con_rgb = (np.asarray(a, f32) for a in (gt, mask_sv, gs, con_rgb))
    S = gt.shape[0]
    with np.errstate(invalid="ignore"):
        bi = (mask_sv > f32(.01)).astype(np.float64)
    nb = (bi[..., 0] + bi[..., 1]) + bi[..., 2]
    e = np.asarray(mask_edge, np.float64).reshape(S, S)
    g_w, c_w = gt.astype(wide), con_rgb.astype(wide)
    weighted = lambda x, w: (x[..., 0] * wide(w[0]) + x[..., 1] * wide(w[1])) + x[..., 2] * wide(w[2])
    sign = lambda d: np.sign(d).astype(np.float64)
    w1 = (1.0 / n + (30.0 * nb) / d_bi) + (10.0 * e) / d_edge
    grad_gs = ((up[0] * sign(gs[..., 0].astype(wide) - weighted(g_w, GRAY_W))) * w1) / 41.0
    s_k = [sign(weighted(c_w, w) - weighted(g_w, w)) for w in YUV_W]
    d_recon_c = np.zeros((S, S, 3), np.float64)
    for c in range(3):
        a_c = (1.0 / (3.0 * n) + (30.0 * bi[..., c]) / (3.0 * d_bi)) + (10.0 * e) / (3.0 * d_edge)
        yuv_c = (s_k[0] * float(YUV_W[0][c]) + s_k[1] * float(YUV_W[1][c])) + s_k[2] * float(YUV_W[2][c])
        d_recon_c[..., c] = (up[1] * (sign(c_w[..., c] - g_w[..., c]) * a_c + (yuv_c * w1) / 2.0)) / 82.0
    wgt = ((1.0 + 30.0 * bi) + 10.0 * e[..., None]) / 41.0
    maps = []
    for l, scale in enumerate(SCALES):
        s = S // scale
        if f64:
            r_m, u_m = resize_matrix(s, S), resize_matrix(S, s)
            v = [g if scale == 1 else apply_axes(u_m, g) for g in (diff5(x if scale == 1 else apply_axes(r_m, x)) for x in (c_w, g_w))]
        else:
            v = [img_grad(con_rgb, scale), img_grad(gt, scale)]
        d_l = (sign(v[0] - v[1]) * wgt) / d_edge
        maps.append(d_l if scale == 1 else apply_axes(resize_matrix(S, s).T, d_l))
    return {"grad_gs": grad_gs[..., None], "d_recon_c": d_recon_c, "d_grad": d_grad_from_maps([m[None] for m in maps], up[2])[0], "maps": maps}


def step_losses_grad(img, gt, mask_sv, gs, con_rgb, upstream=None, f64: bool = False) -> Dict[str, np.ndarray]:
    """Batches -> dict(losses, sums as step_losses; grad_gs [B,S,S,1], grad_con = d_recon_c + d_grad, d_recon_c, d_grad [B,S,S,3]: the
    gradient of upstream . (recon_gs, recon_c, grad) with respect to gs and con_rgb; g0..g4 float64 [B, S >> l, S >> l, 3]).  The
    gradients are float32, rounded once; with `f64` they are float64 of the objective evaluated with no float32 rounding."""
    up = grad_upstream(upstream)
    B, S = check_inputs(img, gt, mask_sv, gs, con_rgb)
    fwd = step_losses(img, gt, mask_sv, gs, con_rgb)
    t = batch_totals(fwd["sums"])
    n, d_bi, d_edge = float(B * S * S), t[IDX["n_bi"]] + 1e-6, t[IDX["n_edge"]] + 1e-6
    items = [item_grads(gt[i], mask_sv[i], gs[i], con_rgb[i], fwd["mask_edge"][i], n, d_bi, d_edge, up, f64) for i in range(B)]
    out = {k: np.stack([it[k] for it in items]) for k in ("grad_gs", "d_recon_c", "d_grad")}
    out["grad_con"] = out["d_recon_c"] + out["d_grad"]
    if not f64:
        out = {k: v.astype(f32) for k, v in out.items()}
    out.update({"g%d" % l: np.stack([it["maps"][l] for it in items]) for l in range(len(SCALES))})
    out.update(losses=fwd["losses"], sums=fwd["sums"])
    return out


def grad_norms(grad_gs: np.ndarray, grad_con: np.ndarray) -> Dict[str, float]:
    """GRAD_NAMES of a batch's gradients: the L1 and L-infinity norms, float64 sums of the float32 magnitudes."""
    a, b = np.abs(np.asarray(grad_gs, np.float64)), np.abs(np.asarray(grad_con, np.float64))
    return dict(zip(GRAD_NAMES, (float(a.sum()), float(a.max()), float(b.sum()), float(b.max()))))


def example_inputs(S: int, B: int, seed: int = 0):
    """img, gt, mask_sv, gs, con_rgb for B items of side S from a seed.  Every item's mask_sv holds: an empty area; a block between .01
    and .3 (edge0 = 1); a block above .3 in all channels (edge0 = 0, mask_bi = 1); one isolated lit pixel; lit pixels in the top-left
    and the bottom-right corner and along the bottom border.  gt, img, gs and con_rgb are smooth with added noise; img is gt darkened
    under the mask.  What the tests, the fixture tool and the bench tool feed the losses with."""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.linspace(0, 1, S), np.linspace(0, 1, S), indexing="ij")
    q = S // 8
    img, gt, mask_sv, gs, con = [], [], [], [], []
    for b in range(B):
        ph = rng.uniform(0, 2 * np.pi, 6)
        smooth = np.stack([0.5 + 0.3 * np.sin(2 * np.pi * (yy * (c + 1) + xx) + ph[c]) for c in range(3)], axis=2)
        g = np.clip(smooth + rng.normal(0, 0.03, (S, S, 3)), 0, 1).astype(f32)
        m = np.zeros((S, S, 3), f32)
        m[2 * q:4 * q, 2 * q:6 * q] = rng.uniform(0.05, 0.25, (2 * q, 4 * q, 3))
        m[4 * q:6 * q, 2 * q:6 * q] = rng.uniform(0.4, 0.9, (2 * q, 4 * q, 3))
        m[q // 2 + b % 3, 7 * q - b % 2] = rng.uniform(0.05, 0.25, 3)             # the isolated pixel
        m[0, 0] = m[S - 1, S - 1] = f32(0.2)
        m[S - 1, 2 * q:4 * q] = rng.uniform(0.05, 0.25, (2 * q, 3))
        i = np.clip(g * (1 - f32(0.6) * m) + rng.normal(0, 0.01, (S, S, 3)), 0, 1).astype(f32)
        wob = np.stack([0.08 * np.cos(2 * np.pi * (xx * (c + 1) - yy) + ph[3 + c]) for c in range(3)], axis=2)
        c_ = np.clip(g + wob + rng.normal(0, 0.02, (S, S, 3)), 0, 1).astype(f32)
        s_ = (gray(g) + rng.normal(0, 0.04, (S, S)).astype(f32)).astype(f32)[..., None]
        img.append(i); gt.append(g); mask_sv.append(m); gs.append(s_); con.append(c_)
    return tuple(np.ascontiguousarray(np.stack(a)).astype(f32) for a in (img, gt, mask_sv, gs, con))


# ---- the command-line entry
def score_folder(folder: str, ckpt: Optional[str] = None, batch: int = 8, host: bool = False, device: int = 0, quiet: bool = False,
                 grad: bool = False) -> Dict[str, float]:
    """Every item folder `<folder>/<name>/` the shadow_synth command wrote -> the step-weighted means of recon_gs, recon_c and grad, a
    step being `batch` items (the last one may hold fewer).  With `grad` also those of GRAD_NAMES: the norms of each batch's gradients
    with respect to gs and con_rgb under G_TOTAL_WEIGHTS."""
    import torch
    from .objective import score_steps
    dev = torch.device("cuda", device)
    if host:
        def step(im_d, gt_a, mask_a, gs, con_rgb):
            torch.cuda.synchronize(dev)
            arrays = (im_d.cpu().numpy(), gt_a, mask_a, gs.cpu().numpy(), con_rgb.cpu().numpy())
            if not grad:
                return step_losses(*arrays)["losses"], {}
            res = step_losses_grad(*arrays, upstream=np.array(G_TOTAL_WEIGHTS, f32))
            return res["losses"], grad_norms(res["grad_gs"], res["grad_con"])
    else:
        from .train_losses_gpu import TrainLosses
        runner, weights_d = TrainLosses(device), torch.tensor(G_TOTAL_WEIGHTS, dtype=torch.float32).to(dev)

        def step(im_d, gt_a, mask_a, gs, con_rgb):
            tensors = (im_d, torch.from_numpy(gt_a).to(dev), torch.from_numpy(mask_a).to(dev), gs, con_rgb)
            if not grad:
                return runner.step_losses(*tensors)[0].cpu().numpy(), {}
            res = runner.step_losses_grad(*tensors, upstream=weights_d)
            return res[0].cpu().numpy(), grad_norms(res[2].cpu().numpy(), res[3].cpu().numpy())

    def record(*tensors):
        loss, norms = step(*tensors)
        return dict({k: float(v) for k, v in zip(LOSS_NAMES, loss)}, **norms), ()

    return score_steps(folder, ckpt, batch, device, "train_losses", record, quiet)


def main(argv=None) -> int:
    import argparse
    ap = argparse.ArgumentParser(prog="python -m blindshadowremoval_amd.train_losses",
                                 description="Score a generator on synthesised pairs with train_step's reconstruction and gradient losses.")
    ap.add_argument("folder")
    ap.add_argument("--ckpt", default=None, help="checkpoint directory; without it the weights come from init_weights")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--host", action="store_true", help="compute the losses with the host statement instead of the device chain")
    ap.add_argument("--grad", action="store_true", help="also the L1 and L-infinity norms of the gradients with respect to gs and con_rgb under G_TOTAL_WEIGHTS")
    a = ap.parse_args(argv)
    means = score_folder(a.folder, ckpt=a.ckpt, batch=a.batch, host=a.host, grad=a.grad)
    print(", ".join("%s:%.9g" % (k, means[k]) for k in LOSS_NAMES + (GRAD_NAMES if a.grad else ())))
    return 0


if __name__ == "__main__":
    sys.exit(main())
