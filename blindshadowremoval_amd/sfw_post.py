"""The GSC model's SFW steps after the generator call, host statement: `FSRNet.test_step_sfw` / `test_step_sfw_video` of
/root/reference/train_test_GSC.py:799-838, 893-932.

All arithmetic is on row 0 of the element:
* ``mask_pred = dif * face`` (float32), ``con = clip(con_rgb, 0, 1)``;
* SSIM / PSNR = tf.image.ssim / tf.image.psnr(mask, mask_pred, max_val=1.0) on ONE channel, where ``mask`` is the label plane's raw grey
  level after the crop resize (0..255, not divided by 255: label values 0 / 1 / 2 and their interpolations) — ``metrics.ssim`` / ``psnr``;
* ``label = (mask == 2)``; AUC = sklearn.metrics.roc_auc_score over ``[1, 0] ++ labels`` against ``[1, 0] ++ mask_pred`` (one forced
  sample of each class) — ``fsrnet.roc_auc_score``, the exact Mann-Whitney form with average ranks (sklearn integrates the ROC curve by
  trapezoids and may differ from it in the last bits); a non-finite score raises, as sklearn does;
* the figures: ``[img, con, mask_pred * 2, label]`` (video step: ``[img, con, mask_pred * 2]``), of which ``Logging.get_imgs`` shows row 0.

The reference stores the AUC as ``tf.constant(auc, tf.float32)``; the float64 value is returned here (the progress line prints 3 digits).
Pinned by tests/golden/sfw_post_gsc.npz, produced by executing the reference's own ``test_step_sfw`` source with sklearn
(tools/make_sfw_post_fixture.py); csrc/sfw_kernels.h computes the same on the device (sfw_post_gpu.py).
"""
from typing import Dict, List, Tuple

import numpy as np
import torch

from .metrics import psnr as _psnr, ssim as _ssim

SPLIT_SFW = (3, 3, 1, 3, 6, 1)        # img, cmap, mask, uv, reg, face   (train_test_GSC.py:806)
SPLIT_VIDEO = (3, 3, 6, 1)            # img, uv, reg, face               (train_test_GSC.py:900)


def sfw_score(mask0: np.ndarray, dif0: np.ndarray, face0: np.ndarray) -> Tuple[Dict[str, float], np.ndarray, np.ndarray]:
    """mask0 / dif0 / face0: [S,S,1] (row 0's mask grey level, the generator's dif, the face region).  -> ({'ssim','psnr','auc'},
    mask_pred [S,S,1] float32, label [S,S,1] float32).  Raises ValueError on a non-finite mask_pred value."""
    from .fsrnet import roc_auc_score
    mask = np.asarray(mask0, np.float32)
    pred = (np.asarray(dif0, np.float32) * np.asarray(face0, np.float32)).astype(np.float32)             # :808
    m, p = torch.from_numpy(np.ascontiguousarray(mask))[None], torch.from_numpy(pred)[None]
    losses = {"ssim": float(_ssim(m, p).sum()), "psnr": float(_psnr(m, p).sum())}                       # :817-818 (one channel)
    label = (mask == np.float32(2)).astype(np.float32)                                                   # :820
    if not np.isfinite(pred).all():
        raise ValueError("Input contains NaN or infinity: mask_pred has non-finite values (roc_auc_score raises here)")
    extr = np.array([1, 0])
    losses["auc"] = roc_auc_score(np.concatenate([extr, label.reshape(-1)]), np.concatenate([extr, pred.reshape(-1)]))      # :821-832
    return losses, pred, label


def sfw_postprocess(img0: np.ndarray, con0: np.ndarray, mask0: np.ndarray, dif0: np.ndarray,
                    face0: np.ndarray) -> Tuple[Dict[str, float], List[np.ndarray]]:
    """test_step_sfw after the generator call, for row 0: -> (losses, [img, con, mask_pred * 2, label]) as [1,S,S,C] float32."""
    losses, pred, label = sfw_score(mask0, dif0, face0)
    figs = [np.asarray(img0, np.float32), np.clip(np.asarray(con0, np.float32), 0, 1), pred * np.float32(2), label]      # :837
    return losses, [f.reshape(1, *f.shape) for f in figs]


def sfw_video_figs(img0: np.ndarray, con0: np.ndarray, dif0: np.ndarray, face0: np.ndarray) -> List[np.ndarray]:
    """test_step_sfw_video after the generator call (no losses), for row 0: -> [img, con, mask_pred * 2] as [1,S,S,C] float32."""
    pred = (np.asarray(dif0, np.float32) * np.asarray(face0, np.float32)).astype(np.float32)
    figs = [np.asarray(img0, np.float32), np.clip(np.asarray(con0, np.float32), 0, 1), pred * np.float32(2)]                 # :931
    return [f.reshape(1, *f.shape) for f in figs]


def strip_of(figs: List[np.ndarray]) -> np.ndarray:
    """Logging.get_imgs of the figures: clip, * 255, round half to even, grey -> 3 channels, side by side -> uint8 [S, len * S, 3]."""
    cols = []
    for f in figs:
        a = np.clip(np.asarray(f, np.float32)[0], 0.0, 1.0) * np.float32(255)
        cols.append(np.repeat(a, 3, axis=2) if a.shape[2] == 1 else a[:, :, :3])
    return np.rint(np.concatenate(cols, axis=1)).astype(np.uint8)
