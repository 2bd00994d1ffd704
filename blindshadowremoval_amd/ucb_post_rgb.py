"""UCB post-processing of the RGB baseline's `FSRNet.test_step` (/root/reference/train_RGB_test.py:403-505), host statement.

Much simpler than the GSC step (ucb_post.py): row 0's ground truth, prediction and input are resized to the crop-box size and
zero-padded back to the image size, the prediction is composited over the input inside the rounded with-hair face mask, clipped,
and scored with SSIM / PSNR against the ground truth; the figures are [input, composite, ground truth].

The reference also resizes and rounds the six other masks (face, mouth, nose, eyebrow, eye, glasses: :434-445, :458-463) but never
reads them afterwards, so this statement takes the with-hair mask only.  Conventions are those ucb_post.py fixed and are reused
from there: TensorFlow's CPU bilinear arithmetic (`resize_bilinear`), round-half-even, masks as k/255 grey levels of which one
channel stands for three, and `metrics.ssim` / `metrics.psnr`.  Pinned by tests/golden/ucb_post_rgb_9156.npz, produced by executing
the reference's own `test_step` source (tools/make_ucb_post_rgb_fixture.py); csrc/ucb_rgb_kernels.h runs the same steps on the device.
"""
from typing import Dict, List, Tuple

import numpy as np
import torch

from .metrics import psnr as _psnr, ssim as _ssim
from .ucb_post import _pad, read_masks, resize_bilinear, strip_of

FIGS = 3          # tmp, out, gt_sc (train_RGB_test.py:502)


def ucb_postprocess_rgb(img0: np.ndarray, gt0: np.ndarray, con0: np.ndarray, box: np.ndarray,
                        face_hair: np.ndarray) -> Tuple[Dict[str, float], List[np.ndarray]]:
    """img0 / gt0 / con0: [S,S,3] (input, ground truth and the generator's `con` of row 0); box: [4]; face_hair: the with-hair face
    mask, [S,S,3] as cv2.imread(...)/255.0 gives it or [S,S,1] (read_masks(grey=True)).  Returns ({'ssim','psnr'}, figs) with figs
    as in train_RGB_test.py:502: input, composite, ground truth — each [1,S,S,3] float32."""
    full = img0.shape[0]
    box = np.asarray(box).reshape(4)
    size = int(box[3] - box[1])                                                            # :409
    rs = lambda a: resize_bilinear(a, size)
    gt_sc = _pad(rs(gt0), size, full)                                                      # :427,430,447
    pred = rs(con0)                                                                        # :428,431
    # :432-433: tf.round(tf.image.resize(curr_mask)); cv2.imread of a grey PNG gives three IDENTICAL channels, so one is resized and repeated
    fh = np.asarray(face_hair)
    if fh.shape[2] == 1 or (np.array_equal(fh[..., 0], fh[..., 1]) and np.array_equal(fh[..., 0], fh[..., 2])):
        m = np.repeat(np.round(rs(fh[:, :, 0:1].astype(np.float32))), 3, axis=2)
    else:
        m = np.round(rs(fh))
    m = _pad(m, size, full).astype(np.float32)                                             # :457
    tmp = _pad(rs(img0), size, full)                                                       # :449-451
    full_pred = _pad(pred, size, full)                                                     # :465
    # :468,475: composite inside the mask in float32 — the prediction is NOT clipped before, only the composite after
    out = np.clip(full_pred * m + tmp * (np.float32(1) - m), 0, 1).astype(np.float32)
    g, o = torch.from_numpy(gt_sc)[None], torch.from_numpy(out)[None]
    losses = {"ssim": float(_ssim(g, o).sum()), "psnr": float(_psnr(g, o).sum())}          # :481-482
    figs = [tmp, out, gt_sc]                                                               # :502
    return losses, [np.asarray(f, np.float32).reshape(1, full, full, 3) for f in figs]


def run_post_job_rgb(job: dict):
    """One item of FSRNetRGB.test's host post-processing (the counterpart of ucb_post.run_post_job): reads the item's with-hair mask,
    runs ucb_postprocess_rgb, optionally writes the PNG strip itself.  -> (losses, figs | None)."""
    if "shm" in job:           # the batch's [B,S,S,9] float32 block (im3 | gt3 | con3) parked in shared memory by the parent
        shape, idx = job["shape"], job["index"]
        n = int(np.prod(shape[1:]))
        a = np.fromfile(job["shm"], np.float32, count=n, offset=idx * n * 4).reshape(shape[1:])
        job = dict(job, im=a[..., 0:3], gt=a[..., 3:6], con=a[..., 6:9])
    masks = job["masks"]
    face_hair = read_masks({"face_hair": masks["face_hair"]}, grey=True)["face_hair"]
    losses, figs = ucb_postprocess_rgb(job["im"], job["gt"], job["con"], job["box"], face_hair)
    if job.get("png"):
        from .pngio import write_png
        write_png(job["png"], strip_of(figs))
    return losses, (figs if job.get("return_figs", True) else None)
