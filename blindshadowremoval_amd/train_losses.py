"""The reconstruction and gradient losses of the reference's `train_step` as a host statement: `recon_gs`, `recon_c` and `grad`
(train_test_GSC.py:107-115, 253-258, 287-301, 307-328, 357; utils.py:22-52, 116-125), restated in numpy.  It plays the role for
csrc/train_losses_kernels.h (bsr_train_losses, train_losses_gpu.TrainLosses) that shadow_synth.py plays for its chain.  The three
discriminators, the VGG perceptual term, `mask_loss` (computed by the reference and never used), every backward pass and the
optimisers are not here.

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

`python -m blindshadowremoval_amd.train_losses FOLDER [--ckpt DIR] [--batch N] [--host]` scores a generator on a folder written by
`python -m blindshadowremoval_amd.shadow_synth` (<name>.png, <name>-gt.png, <name>-mask.png, <name>.npy per item): the network inputs
come from Dataset(config, 'test'), the generator runs on row 0 of each element (weights from the latest checkpoint under --ckpt, from
init_weights without it), and the step-weighted means of the three losses are printed as Logging.display prints them.  --host
computes the losses with this statement from the same generator outputs.
"""
from __future__ import annotations

import contextlib
import os
import sys
from typing import Dict, List, Optional, Tuple

import numpy as np

from .shadow_synth import SIZES
from .ucb_post import resize_bilinear

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


def losses_from_sums(sums: np.ndarray, S: int) -> np.ndarray:
    """float64 [B,K] -> float32 [3]: recon_gs, recon_c, grad over the whole batch."""
    sums = np.asarray(sums, np.float64)
    t = np.zeros(K, np.float64)
    for row in sums:
        t = t + row
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
def folder_steps(folder: str, ckpt: Optional[str] = None, batch: int = 8, device: int = 0, who: str = "train_losses"):
    """The folder handling of the commands that score a generator on synthesised pairs: for every step of `batch` item folders
    `<folder>/<name>/` (the last one may hold fewer) yields (step, steps, img on the device, gt [b,S,S,3], mask_sv [b,S,S,3] (numpy), gs,
    con_rgb (the generator's outputs on the device)).  The generator's weights come from the latest checkpoint under `ckpt`, from
    init_weights without it."""
    import torch
    from . import Generator, init_weights
    from .dataset import Dataset
    from .fsrnet import SPLIT_FFHQ, Config
    from .pngio import read_rgb_u8
    cfg = Config(device)
    cfg.DATA_DIR_TEST = [os.path.join(folder, "*")]
    ds = Dataset(cfg, "test")
    if not ds.name_list:
        raise ValueError("%s: no item folder with a .npy under %s" % (who, folder))
    S = cfg.IMG_SIZE
    dev = torch.device("cuda", device)
    gen = Generator(device=device)
    if ckpt is not None:
        gen.restore(ckpt)
        gen._require_weights()
    else:
        gen.load_weights(init_weights(1))
    batch = max(1, int(batch))
    steps = (len(ds.name_list) + batch - 1) // batch
    try:
        for step in range(steps):
            names = ds.name_list[step * batch:(step + 1) * batch]
            rows, gts, masks = [], [], []
            for lm_path in names:
                element = next(ds.feed)[0]
                rows.append(torch.as_tensor(np.asarray(element)).reshape(-1, S, S, sum(SPLIT_FFHQ))[:1])
                stem = os.path.splitext(lm_path)[0]
                for path, dst in ((stem + "-gt.png", gts), (stem + "-mask.png", masks)):
                    a = read_rgb_u8(path)
                    if a.shape != (S, S, 3):
                        raise ValueError("%s: %s is %s, not %d x %d x 3" % (who, path, a.shape, S, S))
                    dst.append(a.astype(f32) / f32(255))
            im, _, uv, _, _ = torch.split(torch.cat(rows, 0).float(), list(SPLIT_FFHQ), dim=3)
            im_d = im.contiguous().to(dev)
            gs, con_rgb, _, _ = gen(im_d, uv.contiguous().to(dev), None, chuck=2, training=False)
            yield step, steps, im_d, np.stack(gts), np.stack(masks), gs, con_rgb
    finally:                    # also when the consumer stops early or raises: the handle is closed with the generator
        gen.close()


def score_folder(folder: str, ckpt: Optional[str] = None, batch: int = 8, host: bool = False, device: int = 0, quiet: bool = False) -> Dict[str, float]:
    """Every item folder `<folder>/<name>/` the shadow_synth command wrote -> the step-weighted means of recon_gs, recon_c and grad, a
    step being `batch` items (the last one may hold fewer)."""
    import torch
    from .fsrnet import Logging
    dev = torch.device("cuda", device)
    runner = None
    acc: Dict[str, List[float]] = {}
    with contextlib.closing(folder_steps(folder, ckpt, batch, device)) as batches:          # closes the generator handle on any way out
        for step, steps, im_d, gt_a, mask_a, gs, con_rgb in batches:
            if host:
                torch.cuda.synchronize(dev)
                loss = step_losses(im_d.cpu().numpy(), gt_a, mask_a, gs.cpu().numpy(), con_rgb.cpu().numpy())["losses"]
            else:
                from .train_losses_gpu import TrainLosses
                runner = runner or TrainLosses(device)
                loss = runner.step_losses(im_d, torch.from_numpy(gt_a).to(dev), torch.from_numpy(mask_a).to(dev), gs, con_rgb)[0].cpu().numpy()
            Logging.accumulate(acc, {k: float(v) for k, v in zip(LOSS_NAMES, loss)})
            if not quiet:
                print(Logging.format_line(acc, step, steps), end="", flush=True)
    if not quiet:
        print("")
    return {k: s / max(c, 1) for k, (s, c) in acc.items()}


def main(argv=None) -> int:
    import argparse
    ap = argparse.ArgumentParser(prog="python -m blindshadowremoval_amd.train_losses",
                                 description="Score a generator on synthesised pairs with train_step's reconstruction and gradient losses.")
    ap.add_argument("folder")
    ap.add_argument("--ckpt", default=None, help="checkpoint directory; without it the weights come from init_weights")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--host", action="store_true", help="compute the losses with the host statement instead of the device chain")
    a = ap.parse_args(argv)
    means = score_folder(a.folder, ckpt=a.ckpt, batch=a.batch, host=a.host)
    print(", ".join("%s:%.9g" % (k, means[k]) for k in LOSS_NAMES))
    return 0


if __name__ == "__main__":
    sys.exit(main())
