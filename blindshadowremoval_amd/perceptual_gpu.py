"""The device binding of train_step's VGG19 perceptual term and of its gradient with respect to con_rgb: bsr_vgg_per_loss
(csrc/vgg_kernels.h) and bsr_vgg_per_loss_grad (csrc/vgg_grad_kernels.h), held to perceptual.py's host statement."""
from __future__ import annotations

import ctypes
from typing import Dict

import numpy as np
import torch

from . import _lib
from . import perceptual as host
from .pack import pack_vgg, pack_vgg_dgrad
from .post_gpu import PostDevice
from .weights import VGG_BLOCKS, VGG_LAYERS, load_vgg_weights


class Perceptual(PostDevice):
    """`Perceptual(device).per_loss(gt, con_rgb)` — per_loss of the reference's train_step for a batch, on `device`, after
    `load_weights(dict)`, `load_blob(bytes)` or `load_npz(path)`.  `per_loss_grad(gt, con_rgb)` adds d per / d con_rgb, and
    `loss(gt, con_rgb)` is the term as a differentiable torch scalar; both need `load_weights` or `load_npz`, which also upload the
    gradient layers' blob (pack.pack_vgg_dgrad)."""
    SYMBOL = "bsr_vgg_per_loss"
    SIZE_TEXT = "the perceptual term takes 1..4096 items of side 32, 64, 128 or 256, got B=%(b)d S=%(s)d"

    def __init__(self, device: int):
        super().__init__(device)
        self._blob = None
        self._dgrad_blob = None

    def load_weights(self, weights: Dict[str, np.ndarray]) -> None:
        """The 26 VGG19 variables (weights.vgg_variable_shapes) -> the packed blob on the device."""
        self.load_blob(pack_vgg(weights))
        dgrad = pack_vgg_dgrad(weights)
        assert len(dgrad) == int(_lib.load().bsr_vgg_dgrad_blob_bytes())
        self._dgrad_blob = torch.frombuffer(bytearray(dgrad), dtype=torch.uint8).to(self._dev)

    def load_blob(self, blob: bytes) -> None:
        """A blob of pack.pack_vgg.  ValueError unless it holds bsr_vgg_blob_bytes() bytes.  The forward's weights alone: a gradient
        blob loaded earlier is dropped with the weights it belonged to."""
        want = int(_lib.load().bsr_vgg_blob_bytes())
        if len(blob) != want:
            raise ValueError("a VGG19 blob holds %d bytes, got %d" % (want, len(blob)))
        self._dgrad_blob = None
        self._blob = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(self._dev)

    def load_npz(self, path: str) -> None:
        """The `.npz` of weights.load_vgg_weights."""
        self.load_weights(load_vgg_weights(path))

    def scratch(self, b: int, s: int, grad: bool = False) -> int:
        """The 256-byte aligned device address of at least bsr_vgg_scratch_bytes(b, s) bytes of scratch (the query is not named after
        SYMBOL, so PostDevice.scratch cannot find it); with `grad`, of bsr_vgg_grad_scratch_bytes(b, s): the same bytes followed by the
        two gradient buffers."""
        lib = _lib.load()
        need = int(lib.bsr_vgg_grad_scratch_bytes(b, s) if grad else lib.bsr_vgg_scratch_bytes(b, s))
        if need == 0:
            raise ValueError(self.SIZE_TEXT % {"b": b, "s": s})
        if self._scratch is None or self._scratch.numel() < need + 256:
            self._scratch = None
            self._scratch = torch.empty(need + 256, dtype=torch.uint8, device=self._dev)
        base = self._scratch.data_ptr()
        return base + (-base) % 256

    def _check_input(self, gt, con_rgb):
        spec = (("gt", gt), ("con_rgb", con_rgb))
        for name, t in spec:
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 4 or t.device != self._dev:
                raise TypeError("%s must be a float32 tensor [B,S,S,3] on %s" % (name, self._dev))
            if not t.is_contiguous():
                raise ValueError("%s must be contiguous (NHWC, dense)" % name)
        b, s = int(gt.shape[0]), int(gt.shape[1])
        if s not in host.SIZES or not 1 <= b <= host.MAX_B:
            raise ValueError(self.SIZE_TEXT % {"b": b, "s": s})
        for name, t in spec:
            if tuple(t.shape) != (b, s, s, 3):
                raise ValueError("%s must be [%d,%d,%d,3] like gt, got %s" % (name, b, s, s, tuple(t.shape)))
        return b, s

    def activations(self, b: int, s: int) -> Dict[str, torch.Tensor]:
        """Copies of the activations the last call of these sizes left in the scratch, as perceptual.forward names them: `input`
        [2B,s,s,3], `block<b>_conv<i>`, `block<b>_pool`."""
        lib = _lib.load()
        base = self.scratch(b, s) - self._scratch.data_ptr()

        def view(layer, side, c):
            off = base + int(lib.bsr_vgg_act_offset(b, s, layer))
            n = 2 * b * side * side * c
            return self._scratch[off:off + 4 * n].view(torch.float32).reshape(2 * b, side, side, c)

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
        b, s = self._check_input(gt, con_rgb)
        if self._blob is None:
            raise ValueError("the perceptual term has no weights: call load_weights, load_blob or load_npz first")
        loss = self.empty((1,), torch.float32)
        sums = self.empty((b, host.K), torch.float64)
        scratch = self.scratch(b, s)
        self.call(self._blob, ctypes.c_size_t(self._blob.numel()), gt, con_rgb, b, s, sums, loss, ctypes.c_void_p(scratch))
        out = (loss, sums)
        if keep:
            out += (self.activations(b, s),)
        return out

    def _check_grad(self, gt, con_rgb, upstream):
        b, s = self._check_input(gt, con_rgb)
        if upstream is not None and (not isinstance(upstream, torch.Tensor) or upstream.dtype != torch.float32 or upstream.numel() != 1
                                     or upstream.device != self._dev):
            raise TypeError("upstream must be a float32 tensor of one element on %s, or None" % (self._dev,))
        if self._blob is None or self._dgrad_blob is None:
            raise ValueError("the perceptual gradient has no weights: call load_weights or load_npz first (load_blob brings the forward's alone)")
        return b, s

    def _run_grad(self, gt, con_rgb, upstream, b, s, stop_after=None):
        loss = self.empty((1,), torch.float32)
        sums = self.empty((b, host.K), torch.float64)
        grad = self.empty((b, s, s, 3), torch.float32)
        scratch = self.scratch(b, s, grad=True)
        args = [self._blob, ctypes.c_size_t(self._blob.numel()), self._dgrad_blob, ctypes.c_size_t(self._dgrad_blob.numel()), gt, con_rgb, upstream, b, s,
                sums, loss, grad, ctypes.c_void_p(scratch)]
        if stop_after is None:
            self.call(*args, symbol="bsr_vgg_per_loss_grad")
        else:
            self.call(*args, int(stop_after), symbol="bsr_debug_vgg_per_loss_grad")
        return loss, sums, grad

    def per_loss_grad(self, gt: torch.Tensor, con_rgb: torch.Tensor, upstream: torch.Tensor = None, keep: bool = False):
        """-> (loss float32 [1], sums float64 [B,5], grad float32 [B,S,S,3] = d per / d con_rgb * upstream) on the device, asynchronously
        on the current stream; loss and sums are per_loss' bytes.  `upstream`: a float32 device tensor of one element, or None for 1.
        With `keep` also the dict of activations.  Everything is checked here, before any launch: TypeError / ValueError."""
        b, s = self._check_grad(gt, con_rgb, upstream)
        out = self._run_grad(gt, con_rgb, upstream, b, s)
        if keep:
            out += (self.activations(b, s),)
        return out

    def grad_stage(self, gt: torch.Tensor, con_rgb: torch.Tensor, stop_after: int) -> torch.Tensor:
        """For the stage-by-stage tests: the chain stopped after `stop_after` (1..17) of its 18 backward launches -> a copy of the
        gradient buffer that launch wrote, flat (grad_stages() names the launches and gives the shapes)."""
        b, s = self._check_grad(gt, con_rgb, None)
        if not 1 <= int(stop_after) < len(grad_stages()):
            raise ValueError("stop_after must be 1..%d" % (len(grad_stages()) - 1))
        self._run_grad(gt, con_rgb, None, b, s, stop_after)
        which = (int(stop_after) - 1) & 1
        lib = _lib.load()
        off = self.scratch(b, s, grad=True) - self._scratch.data_ptr() + int(lib.bsr_vgg_grad_offset(b, s, which))
        return self._scratch[off:off + 4 * b * s * s * 64].view(torch.float32).clone()

    def loss(self, gt: torch.Tensor, con_rgb: torch.Tensor) -> torch.Tensor:
        """per_loss as a differentiable scalar: float32 [1] with a grad_fn whose backward hands d per / d con_rgb * grad_output to
        con_rgb and None to gt.  When con_rgb requires a gradient, forward and backward run in one call here and the backward is one
        device multiply; nothing is synchronised."""
        return _PerLoss.apply(self, gt, con_rgb)


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


class _PerLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, runner, gt, con_rgb):
        if ctx.needs_input_grad[2]:
            loss, _, grad = runner.per_loss_grad(gt.detach(), con_rgb.detach())
            ctx.save_for_backward(grad)
        else:
            loss = runner.per_loss(gt.detach(), con_rgb.detach())[0]
        return loss

    @staticmethod
    def backward(ctx, grad_output):
        if not ctx.needs_input_grad[2]:
            return None, None, None
        grad, = ctx.saved_tensors
        return None, None, grad * grad_output.to(torch.float32).reshape(())
