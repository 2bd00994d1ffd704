"""The GSC model's `FSRNet.test_step_sfw` scoring (/root/reference/train_test_GSC.py:808-832) for a whole batch ON THE DEVICE: binding of
bsr_sfw_score (csrc/sfw_kernels.h).  blindshadowremoval_amd/sfw_post.py is the host statement: mask_pred and the label plane are
bit-identical to it, the AUC too (exact integer Mann-Whitney count, one final division); this module has no CPU fallback."""
from __future__ import annotations

from typing import Sequence

import numpy as np
import torch

from . import post_gpu

SFW_NONFINITE = 3           # status: a mask_pred value is NaN or infinite (csrc/sfw_kernels.h)


def raise_for_status(status: np.ndarray, names: Sequence[str]) -> None:
    """Raise for the first item whose scoring failed, as the reference's roc_auc_score would."""
    post_gpu.raise_for_status(status, names, {SFW_NONFINITE: "mask_pred contains NaN or infinity (roc_auc_score raises here)"}, "SFW item",
                              other="scoring status %d", other_type=RuntimeError)


class SfwScoreDevice(post_gpu.PostDevice):
    """Reusable runner for one device: keeps its scratch buffer between calls."""
    SYMBOL = "bsr_sfw_score"
    SIZE_TEXT = "bsr_sfw_score supports B > 0 and S in {32, 64, 128, 256} (reference: 256), got B=%(b)d S=%(s)d"
    TYPE_TEXT = "%(name)s must be a float32 tensor with %(dims)d dims on %(dev)s"

    def run(self, rows3: torch.Tensor):
        """rows3: [B,S,S,3] float32 on this device = mask grey level | dif | face of row 0 of each item.  -> (losses [B,2] float32 =
        ssim | psnr, auc [B] float64, pred [B,S,S,1] float32 = dif * face, label [B,S,S,1] float32 = (mask == 2), status [B] int32), on the
        device, asynchronous on the current stream.  Check `status` (raise_for_status) once it is on the host."""
        rows3, = self.inputs(("rows3", rows3, torch.float32, 4))
        b, s = rows3.shape[0], rows3.shape[1]
        if rows3.shape != (b, s, s, 3):
            raise ValueError("rows3 must be [B,S,S,3], got %s" % (tuple(rows3.shape),))
        scratch = self.scratch(b, s)
        losses, auc, status = self.empty((b, 2), torch.float32), self.empty((b,), torch.float64), self.empty((b,), torch.int32)
        pred, label = self.empty((b, s, s, 1), torch.float32), self.empty((b, s, s, 1), torch.float32)
        self.call(rows3, b, s, losses, auc, pred, label, status, scratch)
        return losses, auc, pred, label, status
