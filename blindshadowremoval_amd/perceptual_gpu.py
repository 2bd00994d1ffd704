"""The device binding of train_step's VGG19 perceptual term and of its gradient with respect to con_rgb: bsr_vgg_per_loss
(csrc/vgg_kernels.h) and bsr_vgg_per_loss_grad (csrc/vgg_grad_kernels.h), held to perceptual.py's host statement.  The checks, the
blobs, the calls and the differentiable scalar are post_gpu.WeightedTerm's; here are the names and what the network leaves in the
scratch."""
from __future__ import annotations

from typing import Dict

import torch

from . import _lib
from . import perceptual as host
from .pack import pack_vgg, pack_vgg_dgrad
from .post_gpu import WeightedTerm
from .weights import VGG_BLOCKS, VGG_LAYERS, load_vgg_weights


class Perceptual(WeightedTerm):
    """`Perceptual(device).per_loss(gt, con_rgb)` — per_loss of the reference's train_step for a batch, on `device`, after
    `load_weights(dict)` (the 26 VGG19 variables, weights.vgg_variable_shapes), `load_blob(bytes)` or `load_npz(path)`.
    `per_loss_grad(gt, con_rgb)` adds d per / d con_rgb, and `loss(gt, con_rgb)` is the term as a differentiable torch scalar; both
    need `load_weights` or `load_npz`, which also upload the gradient layers' blob (pack.pack_vgg_dgrad)."""
    SYMBOL, GRAD_SYMBOL = "bsr_vgg_per_loss", "bsr_vgg_per_loss_grad"
    SCRATCH_QUERY, GRAD_SCRATCH_QUERY = "bsr_vgg_scratch_bytes", "bsr_vgg_grad_scratch_bytes"
    BLOB_QUERY, DGRAD_BLOB_QUERY = "bsr_vgg_blob_bytes", "bsr_vgg_dgrad_blob_bytes"
    PACK, PACK_DGRAD = staticmethod(pack_vgg), staticmethod(pack_vgg_dgrad)
    IMAGES = ("gt", "con_rgb")
    MAX_B, N_LOSSES, K = host.MAX_B, 1, host.K
    SIZE_TEXT = "the perceptual term takes 1..4096 items of side 32, 64, 128 or 256, got B=%(b)d S=%(s)d"
    BLOB_TEXT = "a VGG19 blob holds %d bytes, got %d"
    NO_WEIGHTS_TEXT = "the perceptual term has no weights: call load_weights, load_blob or load_npz first"
    NO_GRAD_WEIGHTS_TEXT = "the perceptual gradient has no weights: call load_weights or load_npz first (load_blob brings the forward's alone)"

    def load_npz(self, path: str) -> None:
        """The `.npz` of weights.load_vgg_weights."""
        self.load_weights(load_vgg_weights(path))

    def activations(self, b: int, s: int) -> Dict[str, torch.Tensor]:
        """Copies of the activations the last call of these sizes left in the scratch, as perceptual.forward names them: `input`
        [2B,s,s,3], `block<b>_conv<i>`, `block<b>_pool`."""
        lib = _lib.load()
        self.scratch(b, s)

        def view(layer, side, c):
            return self.view(int(lib.bsr_vgg_act_offset(b, s, layer)), (2 * b, side, side, c))

        out = {"input": view(0, s, 8)[..., :3].clone()}
        layer = 1
        for blk, (ch, n) in enumerate(VGG_BLOCKS):
            for i in range(n):
                out["block%d_conv%d" % (blk + 1, i + 1)] = view(layer, s >> blk, ch).clone()
                layer += 1
        for blk in range(len(VGG_BLOCKS) - 1):
            out["block%d_pool" % (blk + 1)] = view(len(VGG_LAYERS) + 1 + blk, s >> (blk + 1), VGG_BLOCKS[blk][0]).clone()
        return out

    def per_loss(self, gt: torch.Tensor, con_rgb: torch.Tensor, keep: bool = False):
        """-> (loss float32 [1], sums float64 [B,5] (perceptual.PER_SUM_NAMES)) on the device, asynchronously on the current stream;
        with `keep` also the dict of activations (`activations`).  Everything is checked here, before any launch: TypeError /
        ValueError."""
        return self._forward((gt, con_rgb), keep)

    def per_loss_grad(self, gt: torch.Tensor, con_rgb: torch.Tensor, upstream: torch.Tensor = None, keep: bool = False):
        """-> (loss float32 [1], sums float64 [B,5], grad float32 [B,S,S,3] = d per / d con_rgb * upstream) on the device, asynchronously
        on the current stream; loss and sums are per_loss' bytes.  `upstream`: a float32 device tensor of one element, or None for 1.
        With `keep` also the dict of activations.  Everything is checked here, before any launch: TypeError / ValueError."""
        return self._grad((gt, con_rgb), upstream, keep)

    def grad_stage(self, gt: torch.Tensor, con_rgb: torch.Tensor, stop_after: int) -> torch.Tensor:
        """For the stage-by-stage tests: the chain stopped after `stop_after` (1..17) of its 18 backward launches -> a copy of the
        gradient buffer that launch wrote, flat (grad_stages() names the launches and gives the shapes)."""
        b, s = self._check((gt, con_rgb), grad=True)
        if not 1 <= int(stop_after) < len(grad_stages()):
            raise ValueError("stop_after must be 1..%d" % (len(grad_stages()) - 1))
        self._run((gt, con_rgb), b, s, grad=True, stop_after=stop_after)
        which = (int(stop_after) - 1) & 1
        self.scratch(b, s, grad=True)
        return self.view(int(_lib.load().bsr_vgg_grad_offset(b, s, which)), (b * s * s * 64,)).clone()

    def loss(self, gt: torch.Tensor, con_rgb: torch.Tensor) -> torch.Tensor:
        """per_loss as a differentiable scalar: float32 [1] with a grad_fn whose backward hands d per / d con_rgb * grad_output to
        con_rgb and None to gt.  When con_rgb requires a gradient, forward and backward run in one call here and the backward is one
        device multiply; nothing is synchronised."""
        return self._loss(gt, con_rgb)


def grad_stages():
    """The backward chain's 18 launches in order: ("seed" | "dgrad" | "unpool", layer name, the output's (side shift, channels)); the
    output of launch j = 1..17 is [B, S >> shift, S >> shift, channels], the last writes grad."""
    out = [("seed", VGG_LAYERS[-1], (4, 512))]
    ch = [c for c, n in VGG_BLOCKS for _ in range(n)]
    for i in range(len(VGG_LAYERS) - 1, -1, -1):
        blk = int(VGG_LAYERS[i][5]) - 1
        out.append(("dgrad", VGG_LAYERS[i], (blk, ch[i - 1] if i else 3)))
        if i and VGG_LAYERS[i].endswith("conv1"):
            out.append(("unpool", VGG_LAYERS[i - 1], (blk - 1, ch[i - 1])))
    return out
