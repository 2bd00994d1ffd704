"""The RGB baseline's `FSRNet.test_step` post-processing (/root/reference/train_RGB_test.py:427-502) for a whole batch ON THE DEVICE:
binding of bsr_ucb_post_rgb (csrc/ucb_rgb_kernels.h).  blindshadowremoval_amd/ucb_post_rgb.py is the host statement of the same steps —
every figure of the two is bit-identical (tests/test_ucb_post_rgb_gpu.py); this module has no CPU fallback."""
from __future__ import annotations

import torch

from . import post_gpu
from .ucb_post_gpu import raise_for_status  # noqa: F401  (re-exported: the same status codes as bsr_ucb_post)


class UcbPostRgbDevice(post_gpu.PostDevice):
    """Reusable runner for one device: keeps its scratch buffer between calls."""
    SYMBOL = "bsr_ucb_post_rgb"
    SIZE_TEXT = "bsr_ucb_post_rgb supports S in {32, 64, 128, 256} (reference: 256), got %(s)d"

    def run(self, rows9: torch.Tensor, masks: torch.Tensor, boxes: torch.Tensor, want_figs: bool = False):
        """rows9: [B,S,S,9] float32 (input 3 | gt 3 | con 3), masks: [B,S,S] uint8 grey levels of the with-hair face mask, boxes: [B,4]
        float32 — all on this device.  -> (losses [B,2] float32 = ssim | psnr, strips [B,S,3S,3] uint8, figs [B,3,S,S,3] float32 | None,
        status [B] int32), on the device, asynchronous on the current stream.  Check `status` (raise_for_status) once it is on the host."""
        rows9, masks, boxes = self.inputs(("rows9", rows9, torch.float32, 4), ("masks", masks, torch.uint8, 3), ("boxes", boxes, torch.float32, 2))
        b, s = rows9.shape[0], rows9.shape[1]
        if rows9.shape != (b, s, s, 9) or masks.shape != (b, s, s) or boxes.shape != (b, 4):
            raise ValueError("shapes: rows9 [B,S,S,9], masks [B,S,S], boxes [B,4]; got %s %s %s" % (tuple(rows9.shape), tuple(masks.shape), tuple(boxes.shape)))
        scratch = self.scratch(b, s)
        losses, strips, status = self.empty((b, 2), torch.float32), self.empty((b, s, 3 * s, 3), torch.uint8), self.empty((b,), torch.int32)
        figs = self.empty((b, 3, s, s, 3), torch.float32) if want_figs else None
        self.call(rows9, masks, boxes, b, s, losses, strips, figs, status, scratch)
        return losses, strips, figs, status
