"""UCB post-processing of the temporal-sharing model's `FSRNet.test_step` (/root/reference/train_with_TSM.py:418-618), host statement.

The TSM step runs the generator on the image and its mirror as one group of two frames and post-processes at FULL size: unlike the GSC
step (ucb_post.py) nothing is resized before the decisions, and the masks are read unrounded, as cv2.imread(...)/255.0 gives them.
Steps, with their lines:
  * mask_pred = dif0 * face_hair (:493), a flat threshold 0.01 (:497-519);
  * 4-connected components; a component is kept if its size is >= 0.6 * the largest and its hair fraction (hair = face_hair - face,
    unrounded, :495) is < 0.8 (:527-546);
  * the nose rule with this script's four windows and the mean_intensity < 0.15 split (:548-565);
  * composites of both generator rows: orig = con0 * D + img0 * (1 - D), flipped = con1 * flip(D) + flip(img0) * flip(1 - D)
    (:579-580), con NOT clipped before;
  * output = pad(resize(clip(orig))), gt_sc = pad(resize(gt0)), SSIM / PSNR on those two (:588-600);
  * figures [tmp, out, mask_pred * 2, gt_sc, D, flipped, flip(flipped), max(orig, flip(flipped))] (:614).
The reference also reads the mouth, eyebrow, eye and glasses masks and never uses them: they are not inputs here.

Where the reference raises or produces NaN, this statement does what ucb_post.py does in the same situation:
  * no component at all (the reference's np.max of an empty size list raises): nothing is kept;
  * an empty kept set (the reference's 0/0): mean_intensity is NaN, so `mean_intensity < 0.15` is False and a nose hit clears the
    65-row window;
  * no nose pixel equal to 1 (the reference's np.max of an empty row list raises): ValueError, as ucb_post's nose bounding box; the
    device chain reports it as status 1 (UCB_EMPTY_MASK).
Hair fractions are float64 sums of float32 values that are all multiples of 2**-31 and at most 1 in magnitude, so every partial sum
is exact and the per-component sums (np.bincount) equal the reference's per-component np.sum bit for bit.  The nose denominator and
the mean intensity keep numpy's own sums.  Pinned by tests/golden/ucb_post_tsm_9156.npz, produced by executing the reference's own
`test_step` source (tools/make_ucb_post_tsm_fixture.py); csrc/ucb_tsm_kernels.h runs the same steps on the device.
"""
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from .metrics import psnr as _psnr, ssim as _ssim
from .ucb_post import _pad, resize_bilinear, strip_of  # noqa: F401  (re-exported: the figures' strip, as the GSC and RGB steps lay it out)

FIGS = 8                  # train_with_TSM.py:614
MASKS = ("face_hair", "face", "nose")     # the masks the step reads (MASK_DIRS keys)
NOSE_WINDOWS = ((0.423, 0.425), (0.53, 0.56), (0.35, 0.38), (0.58, 0.605))     # :556


def _flip(a: np.ndarray) -> np.ndarray:
    return a[:, ::-1]                                                  # tf.image.flip_left_right of an [H,W,C] image


def ucb_postprocess_tsm(img0: np.ndarray, gt0: np.ndarray, con0: np.ndarray, con1: np.ndarray, dif0: np.ndarray, box: np.ndarray,
                        masks: Dict[str, np.ndarray], trace: Optional[dict] = None
                        ) -> Tuple[Dict[str, float], List[np.ndarray], float, float]:
    """img0 / gt0: [S,S,3] row 0's input and ground truth; con0 / con1: [S,S,3] the generator's `con` of the image and of its mirror;
    dif0: [S,S,1] row 0's `dif`; box: [4]; masks: 'face_hair', 'face', 'nose' as [S,S,3] (cv2.imread(...)/255.0) or [S,S,1]
    (read_masks(grey=True)); other keys are ignored.  Returns ({'ssim','psnr'}, figs[8] as [1,S,S,3] float32, frac_nose_in_shadow,
    mean_intensity), the last two float64.  trace: optional dict that receives the decisions (for tests)."""
    full = img0.shape[0]
    tr = trace if trace is not None else {}
    box = np.asarray(box).reshape(4)
    size = int(box[3] - box[1])                                                            # :424
    tmp = np.asarray(img0, np.float32)                                                     # :461
    fh, face, nose = (np.asarray(masks[k], np.float64) for k in MASKS)
    gt_sc = _pad(resize_bilinear(gt0, size), size, full)                                   # :441,454
    mp = np.asarray(dif0, np.float32) * fh.astype(np.float32)                              # :493, [S,S,C] float32
    hair = (fh - face).astype(np.float32)                                                  # :495
    detected = (mp > np.float32(0.01)).astype(np.uint8)                                    # :497-519: float32 compare

    from scipy import ndimage
    labels, ncomp = ndimage.label(detected[:, :, 0], structure=[[0, 1, 0], [1, 1, 1], [0, 1, 0]])       # :524, connectivity 4
    sizes = np.bincount(labels.reshape(-1), minlength=ncomp + 1)[1:]
    keep = np.zeros((full, full, 1))
    tr.update(ncomp=int(ncomp), largest=0, n_kept=0, n_hair=0)
    if ncomp:
        min_size = 0.6 * np.max(sizes)                                                     # :533
        hair_sum = np.bincount(labels.reshape(-1), weights=hair[:, :, 0].reshape(-1).astype(np.float64), minlength=ncomp + 1)[1:]
        ok = (sizes >= min_size) & (hair_sum / sizes < 0.8)                                # :541-546
        keep[ok[labels - 1] & (labels > 0), 0] = 1
        tr.update(largest=int(np.max(sizes)), n_kept=int(ok.sum()), n_hair=int(((sizes >= min_size) & ~(hair_sum / sizes < 0.8)).sum()))

    shadow_image = keep * np.mean(tmp, 2).reshape(full, full, 1)                           # :549
    with np.errstate(invalid="ignore", divide="ignore"):
        mean_intensity = np.sum(shadow_image) / np.sum(keep)                               # :550
        frac = np.sum((nose[:, :, 0:1] * shadow_image) > 0) / np.sum(nose[:, :, 0])       # :552
    rows, cols = np.where(nose[:, :, 0] == 1)                                              # :557
    if rows.size == 0:
        raise ValueError("the nose mask has no pixel equal to 1 (the reference's np.max of an empty array)")
    mid_nose_height = (np.max(rows) + np.min(rows)) / 2.0
    lower_nose = np.max(rows)
    mid_nose_width = (np.max(cols) + np.min(cols)) / 2.0
    hit = any(lo < frac < hi for lo, hi in NOSE_WINDOWS)
    tr.update(frac=float(frac), mean_intensity=float(mean_intensity), nose_hit=hit, window=[lo < frac < hi for lo, hi in NOSE_WINDOWS],
              reach=None)
    if hit:                                                                                # :561-565
        reach = 5 if mean_intensity < 0.15 else 65
        keep[int(mid_nose_height):int(lower_nose + reach), int(mid_nose_width - 35):int(mid_nose_width + 35)] = 0
        tr["reach"] = reach

    d = np.concatenate((keep, keep, keep), axis=2).astype(np.float32)                      # :567-571
    one = np.float32(1)
    orig = np.asarray(con0, np.float32) * d + tmp * (one - d)                              # :579
    flipped = np.asarray(con1, np.float32) * _flip(d) + _flip(tmp) * _flip(one - d)        # :580
    out = _pad(resize_bilinear(np.clip(orig, 0, 1), size), size, full)                     # :588-590
    g, o = torch.from_numpy(np.ascontiguousarray(gt_sc))[None], torch.from_numpy(np.ascontiguousarray(out))[None]
    losses = {"ssim": float(_ssim(g, o).sum()), "psnr": float(_psnr(g, o).sum())}          # :594-598
    mp3 = np.broadcast_to(mp, (full, full, 3))
    figs = [tmp, out, mp3 * np.float32(2), gt_sc, d, flipped, _flip(flipped), np.maximum(orig, _flip(flipped))]      # :614
    return losses, [np.ascontiguousarray(f, np.float32).reshape(1, full, full, 3) for f in figs], float(frac), float(mean_intensity)
