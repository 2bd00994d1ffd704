"""The TSM model's `FSRNet.test_step` post-processing (/root/reference/train_with_TSM.py:441-614) for a whole batch ON THE DEVICE: binding
of bsr_ucb_post_tsm (csrc/ucb_tsm_kernels.h).  blindshadowremoval_amd/ucb_post_tsm.py is the host statement of the same steps — every
decision and figure of the two is bit-identical (tests/test_ucb_post_tsm_gpu.py); this module has no CPU fallback."""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from . import post_gpu

STATUS_TEXT = {1: "the nose mask has no pixel of level 255 (the reference takes the bounding box of its pixels equal to 1)",
               2: "the crop box is larger than the image or empty"}

ROW_CHANNELS = 13         # input 3 | gt 3 | con of the image 3 | con of the mirror 3 | dif of the image 1


class UcbPostTsmDevice(post_gpu.PostDevice):
    """Reusable runner for one device: keeps its scratch buffer between calls."""
    SYMBOL = "bsr_ucb_post_tsm"
    SIZE_TEXT = "bsr_ucb_post_tsm supports S in {32, 64, 128, 256} (reference: 256), got %(s)d"

    def run(self, rows: torch.Tensor, masks: torch.Tensor, boxes: torch.Tensor, want_figs: bool = False):
        """rows: [B,S,S,13] float32, masks: [B,3,S,S] uint8 grey levels of the with-hair face, face and nose masks, boxes: [B,4] float32
        — all on this device.  -> (losses [B,2] float32 = ssim | psnr, nose_stats [B,2] float64 = frac_nose_in_shadow | mean_intensity,
        strips [B,S,8S,3] uint8, figs [B,8,S,S,3] float32 | None, status [B] int32), on the device, asynchronous on the current stream.
        Check `status` (raise_for_status) once it is on the host."""
        rows, masks, boxes = self.inputs(("rows", rows, torch.float32, 4), ("masks", masks, torch.uint8, 4), ("boxes", boxes, torch.float32, 2))
        b, s = rows.shape[0], rows.shape[1]
        if rows.shape != (b, s, s, ROW_CHANNELS) or masks.shape != (b, 3, s, s) or boxes.shape != (b, 4):
            raise ValueError("shapes: rows [B,S,S,13], masks [B,3,S,S], boxes [B,4]; got %s %s %s" % (tuple(rows.shape), tuple(masks.shape), tuple(boxes.shape)))
        scratch = self.scratch(b, s)
        losses, nose_stats, status = self.empty((b, 2), torch.float32), self.empty((b, 2), torch.float64), self.empty((b,), torch.int32)
        strips = self.empty((b, s, 8 * s, 3), torch.uint8)
        figs = self.empty((b, 8, s, s, 3), torch.float32) if want_figs else None
        self.call(rows, masks, boxes, b, s, losses, nose_stats, strips, figs, status, scratch)
        return losses, nose_stats, strips, figs, status


def raise_for_status(status: Sequence[int], names: Optional[Sequence[str]] = None) -> None:
    """The reference raises (numpy's max of an empty array) where the nose mask is empty: so does the device path, by item."""
    post_gpu.raise_for_status(status, names, STATUS_TEXT, "TSM UCB post-processing of item")
