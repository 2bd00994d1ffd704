"""The TSM model's `FSRNet.test_step` post-processing (/root/reference/train_with_TSM.py:441-614) for a whole batch ON THE DEVICE: binding
of bsr_ucb_post_tsm (csrc/ucb_tsm_kernels.h).  blindshadowremoval_amd/ucb_post_tsm.py is the host statement of the same steps — every
decision and figure of the two is bit-identical (tests/test_ucb_post_tsm_gpu.py); this module has no CPU fallback."""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence

import torch

from . import _lib

STATUS_TEXT = {1: "the nose mask has no pixel of level 255 (the reference takes the bounding box of its pixels equal to 1)",
               2: "the crop box is larger than the image or empty"}

ROW_CHANNELS = 13         # input 3 | gt 3 | con of the image 3 | con of the mirror 3 | dif of the image 1


class UcbPostTsmDevice:
    """Reusable runner for one device: keeps its scratch buffer between calls."""

    def __init__(self, device: int):
        self.device = int(device)
        self._scratch: Optional[torch.Tensor] = None

    def run(self, rows: torch.Tensor, masks: torch.Tensor, boxes: torch.Tensor, want_figs: bool = False):
        """rows: [B,S,S,13] float32, masks: [B,3,S,S] uint8 grey levels of the with-hair face, face and nose masks, boxes: [B,4] float32
        — all on this device.  -> (losses [B,2] float32 = ssim | psnr, nose_stats [B,2] float64 = frac_nose_in_shadow | mean_intensity,
        strips [B,S,8S,3] uint8, figs [B,8,S,S,3] float32 | None, status [B] int32), on the device, asynchronous on the current stream.
        Check `status` (raise_for_status) once it is on the host."""
        dev = torch.device("cuda", self.device)
        for name, t, dt, nd in (("rows", rows, torch.float32, 4), ("masks", masks, torch.uint8, 4), ("boxes", boxes, torch.float32, 2)):
            if not isinstance(t, torch.Tensor) or t.dtype != dt or t.dim() != nd or t.device != dev:
                raise TypeError("%s must be a %s tensor with %d dims on %s" % (name, dt, nd, dev))
        rows, masks, boxes = rows.contiguous(), masks.contiguous(), boxes.contiguous()
        b, s = rows.shape[0], rows.shape[1]
        if rows.shape != (b, s, s, ROW_CHANNELS) or masks.shape != (b, 3, s, s) or boxes.shape != (b, 4):
            raise ValueError("shapes: rows [B,S,S,13], masks [B,3,S,S], boxes [B,4]; got %s %s %s" % (tuple(rows.shape), tuple(masks.shape), tuple(boxes.shape)))
        lib = _lib.load()
        need = int(lib.bsr_ucb_post_tsm_scratch_bytes(b, s))
        if need == 0:
            raise ValueError("bsr_ucb_post_tsm supports S in {32, 64, 128, 256} (reference: 256), got %d" % s)
        if self._scratch is None or self._scratch.numel() < need + 256:
            self._scratch = torch.empty(need + 256, dtype=torch.uint8, device=dev)
        base = self._scratch.data_ptr()
        base += (-base) % 256
        losses = torch.empty((b, 2), dtype=torch.float32, device=dev)
        nose_stats = torch.empty((b, 2), dtype=torch.float64, device=dev)
        strips = torch.empty((b, s, 8 * s, 3), dtype=torch.uint8, device=dev)
        figs = torch.empty((b, 8, s, s, 3), dtype=torch.float32, device=dev) if want_figs else None
        status = torch.empty((b,), dtype=torch.int32, device=dev)
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        with torch.cuda.device(self.device):
            rc = lib.bsr_ucb_post_tsm(self.device, p(rows), p(masks), p(boxes), b, s, p(losses), p(nose_stats), p(strips),
                                      p(figs) if figs is not None else None, p(status), ctypes.c_void_p(base),
                                      ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        _lib.check(rc, "bsr_ucb_post_tsm")
        return losses, nose_stats, strips, figs, status


def raise_for_status(status: Sequence[int], names: Optional[Sequence[str]] = None) -> None:
    """The reference raises (numpy's max of an empty array) where the nose mask is empty: so does the device path, by item."""
    for j, st in enumerate(status):
        if int(st) != 0:
            raise ValueError("TSM UCB post-processing of item %s: %s" % (names[j] if names is not None else j, STATUS_TEXT.get(int(st), "status %d" % int(st))))
