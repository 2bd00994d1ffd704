"""The GSC model's `FSRNet.test_step_sfw` scoring (/root/reference/train_test_GSC.py:808-832) for a whole batch ON THE DEVICE: binding of
bsr_sfw_score (csrc/sfw_kernels.h).  blindshadowremoval_amd/sfw_post.py is the host statement: mask_pred and the label plane are
bit-identical to it, the AUC too (exact integer Mann-Whitney count, one final division); this module has no CPU fallback."""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib

SFW_NONFINITE = 3           # status: a mask_pred value is NaN or infinite (csrc/sfw_kernels.h)


def raise_for_status(status: np.ndarray, names: Sequence[str]) -> None:
    """Raise for the first item whose scoring failed, as the reference's roc_auc_score would."""
    for j, s in enumerate(np.asarray(status).reshape(-1)):
        if s == SFW_NONFINITE:
            raise ValueError("SFW item %s: mask_pred contains NaN or infinity (roc_auc_score raises here)" % (names[j] if j < len(names) else j))
        if s != 0:
            raise RuntimeError("SFW item %s: scoring status %d" % (names[j] if j < len(names) else j, int(s)))


class SfwScoreDevice:
    """Reusable runner for one device: keeps its scratch buffer between calls."""

    def __init__(self, device: int):
        self.device = int(device)
        self._scratch: Optional[torch.Tensor] = None

    def run(self, rows3: torch.Tensor):
        """rows3: [B,S,S,3] float32 on this device = mask grey level | dif | face of row 0 of each item.  -> (losses [B,2] float32 =
        ssim | psnr, auc [B] float64, pred [B,S,S,1] float32 = dif * face, label [B,S,S,1] float32 = (mask == 2), status [B] int32), on the
        device, asynchronous on the current stream.  Check `status` (raise_for_status) once it is on the host."""
        dev = torch.device("cuda", self.device)
        if not isinstance(rows3, torch.Tensor) or rows3.dtype != torch.float32 or rows3.dim() != 4 or rows3.device != dev:
            raise TypeError("rows3 must be a float32 tensor with 4 dims on %s" % dev)
        rows3 = rows3.contiguous()
        b, s = rows3.shape[0], rows3.shape[1]
        if rows3.shape != (b, s, s, 3):
            raise ValueError("rows3 must be [B,S,S,3], got %s" % (tuple(rows3.shape),))
        lib = _lib.load()
        need = int(lib.bsr_sfw_score_scratch_bytes(b, s)) if b > 0 else 0
        if need == 0:
            raise ValueError("bsr_sfw_score supports B > 0 and S in {32, 64, 128, 256} (reference: 256), got B=%d S=%d" % (b, s))
        if self._scratch is None or self._scratch.numel() < need + 256:
            self._scratch = torch.empty(need + 256, dtype=torch.uint8, device=dev)
        base = self._scratch.data_ptr()
        base += (-base) % 256
        losses = torch.empty((b, 2), dtype=torch.float32, device=dev)
        auc = torch.empty((b,), dtype=torch.float64, device=dev)
        pred = torch.empty((b, s, s, 1), dtype=torch.float32, device=dev)
        label = torch.empty((b, s, s, 1), dtype=torch.float32, device=dev)
        status = torch.empty((b,), dtype=torch.int32, device=dev)
        ptr = lambda t: ctypes.c_void_p(t.data_ptr())
        with torch.cuda.device(self.device):
            rc = lib.bsr_sfw_score(self.device, ptr(rows3), b, s, ptr(losses), ptr(auc), ptr(pred), ptr(label), ptr(status), ctypes.c_void_p(base),
                                   ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        _lib.check(rc, "bsr_sfw_score")
        return losses, auc, pred, label, status
