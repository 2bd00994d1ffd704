"""The device binding of train_step's reconstruction and gradient losses and of their gradient with respect to gs and con_rgb:
bsr_train_losses and bsr_train_losses_grad (csrc/train_losses_kernels.h), held to train_losses.py's host statement."""
from __future__ import annotations

import ctypes
from typing import Dict

import torch

from . import _lib
from . import train_losses as host
from .post_gpu import PostDevice

G_TOTAL_WEIGHTS = host.G_TOTAL_WEIGHTS
IMAGES = (("img", 3), ("gt", 3), ("mask_sv", 3), ("gs", 1), ("con_rgb", 3))


class TrainLosses(PostDevice):
    """`TrainLosses(device).step_losses(img, gt, mask_sv, gs, con_rgb)` — recon_gs, recon_c and grad of the reference's train_step for a
    batch, on `device`.  `step_losses_grad` adds the gradient of their weighted sum with respect to gs and con_rgb, and `loss` is that
    weighted sum as a differentiable torch scalar."""
    SYMBOL, GRAD_SYMBOL = "bsr_train_losses", "bsr_train_losses_grad"
    GRAD_SCRATCH_QUERY = "bsr_train_losses_grad_scratch_bytes"
    SIZE_TEXT = "train_losses takes 1..65535 items of side 32, 64, 128 or 256, got B=%(b)d S=%(s)d"
    UPSTREAM_TEXT = "upstream must be a float32 tensor of three elements (the weights of recon_gs, recon_c and grad) on %s, or None"

    def __init__(self, device: int):
        super().__init__(device)
        self._weights: Dict[tuple, torch.Tensor] = {}          # loss()'s weights on the device

    def _images(self, tensors):
        return self.images([(name, t, c) for (name, c), t in zip(IMAGES, tensors)], 65535)

    def step_losses(self, img: torch.Tensor, gt: torch.Tensor, mask_sv: torch.Tensor, gs: torch.Tensor, con_rgb: torch.Tensor, figs: bool = False):
        """-> (losses float32 [3] = recon_gs, recon_c, grad (train_losses.LOSS_NAMES), sums float64 [B,K] (train_losses.SUM_NAMES)) on the
        device, asynchronously on the current stream; with `figs` also (mask_edge [B,S,S,1], bmaskgt [B,S,S,1], dif_grad [B,S,S,3]), the
        reference's figures 5, 6 and 8.  Everything is checked here, before any launch: TypeError / ValueError."""
        b, s = self._images((img, gt, mask_sv, gs, con_rgb))
        losses = self.empty((3,), torch.float32)
        sums = self.empty((b, host.K), torch.float64)
        planes = (self.empty((b, s, s, 1), torch.float32), self.empty((b, s, s, 1), torch.float32), self.empty((b, s, s, 3), torch.float32)) if figs \
            else (None, None, None)
        scratch = self.scratch(b, s)
        self.call(img, gt, mask_sv, gs, con_rgb, b, s, sums, losses, planes[0], planes[1], planes[2], ctypes.c_void_p(scratch))
        return (losses, sums) + (planes if figs else ())

    def step_losses_grad(self, img: torch.Tensor, gt: torch.Tensor, mask_sv: torch.Tensor, gs: torch.Tensor, con_rgb: torch.Tensor,
                         upstream: torch.Tensor = None, parts: bool = False):
        """-> (losses, sums, grad_gs float32 [B,S,S,1], grad_con float32 [B,S,S,3]) on the device, asynchronously on the current stream:
        step_losses' bytes and the gradient of upstream . (recon_gs, recon_c, grad) with respect to gs and con_rgb
        (train_losses.step_losses_grad).  `upstream`: a float32 device tensor of three elements, or None for ones.  With `parts` also
        (d_recon_c, d_grad) [B,S,S,3], the two summands of grad_con.  Everything is checked here, before any launch: TypeError /
        ValueError."""
        b, s = self._images((img, gt, mask_sv, gs, con_rgb))
        if upstream is not None and (not isinstance(upstream, torch.Tensor) or upstream.dtype != torch.float32 or tuple(upstream.shape) != (3,)
                                     or upstream.device != self._dev):
            raise TypeError(self.UPSTREAM_TEXT % (self._dev,))
        if upstream is not None:
            upstream = upstream.contiguous()
        losses = self.empty((3,), torch.float32)
        sums = self.empty((b, host.K), torch.float64)
        grad_gs, grad_con = self.empty((b, s, s, 1), torch.float32), self.empty((b, s, s, 3), torch.float32)
        two = (self.empty((b, s, s, 3), torch.float32), self.empty((b, s, s, 3), torch.float32)) if parts else (None, None)
        scratch = self.scratch(b, s, grad=True)
        self.call(img, gt, mask_sv, gs, con_rgb, upstream, b, s, sums, losses, grad_gs, grad_con, two[0], two[1], ctypes.c_void_p(scratch),
                  symbol=self.GRAD_SYMBOL)
        return (losses, sums, grad_gs, grad_con) + (two if parts else ())

    def gradients(self, b: int, s: int) -> Dict[str, torch.Tensor]:
        """Views of the maps g0..g4 [b, s >> l, s >> l, 3] that the last step_losses_grad call of these sizes left in the scratch, as
        train_losses.step_losses_grad names them.  Views, not copies: the next call writes over them."""
        lib = _lib.load()
        self.scratch(b, s, grad=True)
        return {"g%d" % l: self.view(int(lib.bsr_train_losses_grad_offset(b, s, l)), (b, s >> l, s >> l, 3)) for l in range(len(host.SCALES))}

    def loss(self, img: torch.Tensor, gt: torch.Tensor, mask_sv: torch.Tensor, gs: torch.Tensor, con_rgb: torch.Tensor, weights=G_TOTAL_WEIGHTS) -> torch.Tensor:
        """(w0 recon_gs + w1 recon_c) + w2 grad as a differentiable scalar: float32 [] whose backward hands its gradient to gs and con_rgb
        and None to every other input.  When gs or con_rgb requires a gradient, forward and backward run in one call here and the backward
        is one device multiply per output; nothing is synchronised."""
        w = tuple(float(x) for x in weights)
        if len(w) != 3:
            raise ValueError("weights must be three numbers: those of recon_gs, recon_c and grad")
        return _LossesTerm.apply(self, w, img, gt, mask_sv, gs, con_rgb)


class _LossesTerm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, runner, weights, img, gt, mask_sv, gs, con_rgb):
        tensors = [t.detach() if isinstance(t, torch.Tensor) else t for t in (img, gt, mask_sv, gs, con_rgb)]
        ctx.want = ctx.needs_input_grad[5], ctx.needs_input_grad[6]
        if any(ctx.want):
            runner._images(tensors)                                       # checked before the weights' upload
            up = runner._weights.get(weights)
            if up is None:                                                # uploaded once per set of weights
                up = runner._weights[weights] = torch.tensor(weights, dtype=torch.float32).to(runner._dev)
            losses, _, grad_gs, grad_con = runner.step_losses_grad(*tensors, upstream=up)
            ctx.save_for_backward(grad_gs, grad_con)
        else:
            losses = runner.step_losses(*tensors)[0]
        w = [torch.tensor(x, dtype=torch.float32) for x in weights]      # zero-dim host scalars: the products stay float32 on the device
        return (w[0] * losses[0] + w[1] * losses[1]) + w[2] * losses[2]

    @staticmethod
    def backward(ctx, grad_output):
        out = [None] * 7
        if any(ctx.want):
            grad_gs, grad_con = ctx.saved_tensors
            g = grad_output.to(torch.float32).reshape(())
            if ctx.want[0]:
                out[5] = grad_gs * g
            if ctx.want[1]:
                out[6] = grad_con * g
        return tuple(out)
