"""The device binding of train_step's reconstruction and gradient losses: bsr_train_losses (csrc/train_losses_kernels.h), held to
train_losses.py's host statement."""
from __future__ import annotations

import ctypes

import torch

from . import train_losses as host
from .post_gpu import PostDevice


class TrainLosses(PostDevice):
    """`TrainLosses(device).step_losses(img, gt, mask_sv, gs, con_rgb)` — recon_gs, recon_c and grad of the reference's train_step for a
    batch, on `device`."""
    SYMBOL = "bsr_train_losses"
    SIZE_TEXT = "train_losses takes 1..65535 items of side 32, 64, 128 or 256, got B=%(b)d S=%(s)d"

    def step_losses(self, img: torch.Tensor, gt: torch.Tensor, mask_sv: torch.Tensor, gs: torch.Tensor, con_rgb: torch.Tensor, figs: bool = False):
        """-> (losses float32 [3] = recon_gs, recon_c, grad (train_losses.LOSS_NAMES), sums float64 [B,K] (train_losses.SUM_NAMES)) on the
        device, asynchronously on the current stream; with `figs` also (mask_edge [B,S,S,1], bmaskgt [B,S,S,1], dif_grad [B,S,S,3]), the
        reference's figures 5, 6 and 8.  Everything is checked here, before any launch: TypeError / ValueError."""
        b, s = self.images((("img", img, 3), ("gt", gt, 3), ("mask_sv", mask_sv, 3), ("gs", gs, 1), ("con_rgb", con_rgb, 3)), 65535)
        losses = self.empty((3,), torch.float32)
        sums = self.empty((b, host.K), torch.float64)
        planes = (self.empty((b, s, s, 1), torch.float32), self.empty((b, s, s, 1), torch.float32), self.empty((b, s, s, 3), torch.float32)) if figs \
            else (None, None, None)
        scratch = self.scratch(b, s)
        self.call(img, gt, mask_sv, gs, con_rgb, b, s, sums, losses, planes[0], planes[1], planes[2], ctypes.c_void_p(scratch))
        return (losses, sums) + (planes if figs else ())
