"""`FSRNet.test_step`'s per-item post-processing (/root/reference/train_test_GSC.py:424-748) for a whole batch ON THE DEVICE:
binding of bsr_ucb_post (csrc/ucb_kernels.h).  blindshadowremoval_amd/ucb_post.py is the host statement of the same steps — every
threshold / mask / component decision of the two is bit-identical (tests/test_ucb_post_gpu.py); this module has no CPU fallback."""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from . import post_gpu
from .ucb_post import MASK_DIRS

from .prep import MASK_ORDER, read_masks_u8      # noqa: F401  (re-exported: the mask order of bsr_ucb_post and the reader the loaders use)

assert MASK_ORDER == tuple(MASK_DIRS)
STATUS_TEXT = {1: "a segmentation mask the reference takes a bounding box of (nose / mouth / forehead / face) is empty after the resize",
               2: "the crop box is larger than the image or empty"}


class UcbPostDevice(post_gpu.PostDevice):
    """Reusable runner for one device: keeps its scratch buffer between calls."""
    SYMBOL = "bsr_ucb_post"
    SIZE_TEXT = "bsr_ucb_post supports S in {32, 64, 128, 256} (reference: 256), got %(s)d"

    def run(self, rows10: torch.Tensor, masks: torch.Tensor, boxes: torch.Tensor, want_figs: bool = False):
        """rows10: [B,S,S,10] float32 (input 3 | gt 3 | con_rgb 3 | dif 1), masks: [B,7,S,S] uint8, boxes: [B,4] float32 — all on this
        device.  -> (losses [B,2] float32 = ssim | psnr, strips [B,S,7S,3] uint8, figs [B,7,S,S,3] float32 | None, status [B] int32), on
        the device, asynchronous on the current stream.  Check `status` (raise_for_status) once it is on the host."""
        rows10, masks, boxes = self.inputs(("rows10", rows10, torch.float32, 4), ("masks", masks, torch.uint8, 4), ("boxes", boxes, torch.float32, 2))
        b, s = rows10.shape[0], rows10.shape[1]
        if rows10.shape != (b, s, s, 10) or masks.shape != (b, 7, s, s) or boxes.shape != (b, 4):
            raise ValueError("shapes: rows10 [B,S,S,10], masks [B,7,S,S], boxes [B,4]; got %s %s %s" % (tuple(rows10.shape), tuple(masks.shape), tuple(boxes.shape)))
        scratch = self.scratch(b, s)
        losses, strips, status = self.empty((b, 2), torch.float32), self.empty((b, s, 7 * s, 3), torch.uint8), self.empty((b,), torch.int32)
        figs = self.empty((b, 7, s, s, 3), torch.float32) if want_figs else None
        self.call(rows10, masks, boxes, b, s, losses, strips, figs, status, scratch)
        return losses, strips, figs, status


def raise_for_status(status: Sequence[int], names: Optional[Sequence[str]] = None) -> None:
    """The reference raises (numpy's min of an empty array) where a mask it needs is empty: so does the device path, by item."""
    post_gpu.raise_for_status(status, names, STATUS_TEXT, "UCB post-processing of item")
