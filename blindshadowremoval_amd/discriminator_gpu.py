"""The device binding of train_step's three discriminators and GAN losses and of the gen term's gradient with respect to con_rgb:
bsr_disc_losses (csrc/disc_kernels.h) and bsr_disc_gen_grad (csrc/disc_grad_kernels.h), held to discriminator.py's host statement."""
from __future__ import annotations

import ctypes
from typing import Dict

import numpy as np
import torch

from . import _lib
from . import discriminator as host
from .pack import pack_discriminators, pack_discriminators_dgrad
from .post_gpu import PostDevice
from .weights import N_LAYER_D


class Discriminators(PostDevice):
    """`Discriminators(device).gan_losses(gt, con_rgb, mask_sv)` — gen, disc_real and disc_fake of the reference's train_step for a
    batch, on `device`, after `load_weights(dict)` or `restore(ckpt_dir)`.  `gen_grad(gt, con_rgb, mask_sv)` adds d gen / d con_rgb, and
    `gen_loss(gt, con_rgb, mask_sv)` is the gen term as a differentiable torch scalar; both need `load_weights` or `restore`, which also
    upload the gradient layers' blob (pack.pack_discriminators_dgrad)."""
    SYMBOL = "bsr_disc_losses"
    SIZE_TEXT = "discriminators take 1..32767 items of side 32, 64, 128 or 256, got B=%(b)d S=%(s)d"

    def __init__(self, device: int):
        super().__init__(device)
        self._blob = None
        self._dgrad_blob = None

    def load_weights(self, weights: Dict[str, np.ndarray]) -> None:
        """The three discriminators' variables (weights.discriminator_variable_shapes) -> the packed blob on the device."""
        self.load_blob(pack_discriminators(weights))
        dgrad = pack_discriminators_dgrad(weights)
        assert len(dgrad) == int(_lib.load().bsr_disc_dgrad_blob_bytes())
        self._dgrad_blob = torch.frombuffer(bytearray(dgrad), dtype=torch.uint8).to(self._dev)

    def load_blob(self, blob: bytes) -> None:
        """A blob of pack.pack_discriminators.  ValueError unless it holds bsr_disc_blob_bytes() bytes.  The forward's weights alone: a
        gradient blob loaded earlier is dropped with the weights it belonged to."""
        want = int(_lib.load().bsr_disc_blob_bytes())
        if len(blob) != want:
            raise ValueError("a discriminator blob holds %d bytes, got %d" % (want, len(blob)))
        self._dgrad_blob = None
        self._blob = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(self._dev)

    def restore(self, ckpt_dir: str) -> None:
        """The `discriminator_{1,2,3}/*` variables of the latest checkpoint under `ckpt_dir`."""
        from .tf_bundle import latest_checkpoint, load_discriminator_weights
        prefix = latest_checkpoint(ckpt_dir)
        if prefix is None:
            raise FileNotFoundError("no checkpoint under %s" % ckpt_dir)
        self.load_weights(load_discriminator_weights(prefix))

    def scratch(self, b: int, s: int, grad: bool = False) -> int:
        """The 256-byte aligned device address of at least bsr_disc_losses_scratch_bytes(b, s) bytes of scratch; with `grad`, of
        bsr_disc_grad_scratch_bytes(b, s): the same bytes followed by the gradient maps."""
        if not grad:
            return super().scratch(b, s)
        need = int(_lib.load().bsr_disc_grad_scratch_bytes(b, s))
        if need == 0:
            raise ValueError(self.SIZE_TEXT % {"b": b, "s": s})
        if self._scratch is None or self._scratch.numel() < need + 256:
            self._scratch = None
            self._scratch = torch.empty(need + 256, dtype=torch.uint8, device=self._dev)
        base = self._scratch.data_ptr()
        return base + (-base) % 256

    def _check_input(self, gt, con_rgb, mask_sv):
        spec = (("gt", gt), ("con_rgb", con_rgb), ("mask_sv", mask_sv))
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
        """Copies of the activations the last call of these sizes left in the scratch: `d{k}/in` [2B,s,s,6], `d{k}/conv{i}`, `d{k}/out`
        [2B,h_k,h_k,1], as discriminator.forward names them."""
        lib = _lib.load()
        base = self.scratch(b, s) - self._scratch.data_ptr()
        out = {}
        for k in (1, 2, 3):
            sides = host.map_sides(s, k)
            for layer, side in enumerate(sides):
                c = 8 if layer == 0 else (host.DISC_CH[layer - 1] if layer <= N_LAYER_D else 1)
                off = base + int(lib.bsr_disc_act_offset(b, s, k, layer))
                n = 2 * b * side * side * c
                a = self._scratch[off:off + 4 * n].view(torch.float32).reshape(2 * b, side, side, c)
                name = "in" if layer == 0 else ("conv%d" % (layer - 1) if layer <= N_LAYER_D else "out")
                out["d%d/%s" % (k, name)] = (a[..., :6] if layer == 0 else a).clone()
        return out

    def gan_losses(self, gt: torch.Tensor, con_rgb: torch.Tensor, mask_sv: torch.Tensor, logits: bool = False, keep: bool = False):
        """-> (losses float32 [3] = gen, disc_real, disc_fake (discriminator.LOSS_NAMES), sums float64 [B,9] (discriminator.DISC_SUM_NAMES))
        on the device, asynchronously on the current stream; with `logits` also the three maps [2B,h_k,h_k] as a list; with `keep` also
        the dict of activations (`activations`).  Everything is checked here, before any launch: TypeError / ValueError."""
        b, s = self._check_input(gt, con_rgb, mask_sv)
        if self._blob is None:
            raise ValueError("the discriminators have no weights: call load_weights or restore first")
        losses = self.empty((3,), torch.float32)
        sums = self.empty((b, host.K), torch.float64)
        sides = [host.final_side(s, k) for k in (1, 2, 3)]
        flat = self.empty((sum(2 * b * h * h for h in sides),), torch.float32) if logits else None
        scratch = self.scratch(b, s)
        self.call(self._blob, ctypes.c_size_t(self._blob.numel()), gt, con_rgb, mask_sv, b, s, sums, losses, flat, ctypes.c_void_p(scratch))
        out = (losses, sums)
        if logits:
            maps, off = [], 0
            for h in sides:
                maps.append(flat[off:off + 2 * b * h * h].reshape(2 * b, h, h))
                off += 2 * b * h * h
            out += (maps,)
        if keep:
            out += (self.activations(b, s),)
        return out

    def _check_grad(self, gt, con_rgb, mask_sv, upstream):
        b, s = self._check_input(gt, con_rgb, mask_sv)
        if upstream is not None and (not isinstance(upstream, torch.Tensor) or upstream.dtype != torch.float32 or upstream.numel() != 1
                                     or upstream.device != self._dev):
            raise TypeError("upstream must be a float32 tensor of one element on %s, or None" % (self._dev,))
        if self._blob is None or self._dgrad_blob is None:
            raise ValueError("the discriminators' gradient has no weights: call load_weights or restore first (load_blob brings the forward's alone)")
        return b, s

    def _run_grad(self, gt, con_rgb, mask_sv, upstream, b, s, stop_after=None):
        losses = self.empty((3,), torch.float32)
        sums = self.empty((b, host.K), torch.float64)
        grad = self.empty((b, s, s, 3), torch.float32)
        scratch = self.scratch(b, s, grad=True)
        args = [self._blob, ctypes.c_size_t(self._blob.numel()), self._dgrad_blob, ctypes.c_size_t(self._dgrad_blob.numel()), gt, con_rgb, mask_sv, upstream,
                b, s, sums, losses, None, grad, ctypes.c_void_p(scratch)]
        if stop_after is None:
            self.call(*args, symbol="bsr_disc_gen_grad")
        else:
            self.call(*args, int(stop_after), symbol="bsr_debug_disc_gen_grad")
        return losses, sums, grad

    def gen_grad(self, gt: torch.Tensor, con_rgb: torch.Tensor, mask_sv: torch.Tensor, upstream: torch.Tensor = None, keep: bool = False):
        """-> (losses float32 [3], sums float64 [B,9], grad float32 [B,S,S,3] = d gen / d con_rgb * upstream) on the device, asynchronously
        on the current stream; losses, sums and the kept activations are gan_losses' bytes.  `upstream`: a float32 device tensor of one
        element, or None for 1.  With `keep` also the dict of activations.  Everything is checked here, before any launch: TypeError /
        ValueError."""
        b, s = self._check_grad(gt, con_rgb, mask_sv, upstream)
        out = self._run_grad(gt, con_rgb, mask_sv, upstream, b, s)
        if keep:
            out += (self.activations(b, s),)
        return out

    def gradients(self, b: int, s: int) -> Dict[str, torch.Tensor]:
        """Copies of the gradient maps the last gen_grad / grad_stages call of these sizes left in the scratch, as discriminator.gen_grad
        names them: `d{k}/in` [B,s,s,3], `d{k}/conv{i}` [B,.,.,n_ch[i]]."""
        lib = _lib.load()
        base = self.scratch(b, s, grad=True) - self._scratch.data_ptr()
        out = {}
        for k in (1, 2, 3):
            sides = host.map_sides(s, k)
            for layer in range(N_LAYER_D + 1):
                side, c = sides[layer], 4 if layer == 0 else host.DISC_CH[layer - 1]
                off = base + int(lib.bsr_disc_grad_offset(b, s, k, layer))
                a = self._scratch[off:off + 4 * b * side * side * c].view(torch.float32).reshape(b, side, side, c)
                out["d%d/%s" % (k, "in" if layer == 0 else "conv%d" % (layer - 1))] = (a[..., :3] if layer == 0 else a).clone()
        return out

    def grad_stages(self, gt: torch.Tensor, con_rgb: torch.Tensor, mask_sv: torch.Tensor, stop_after: int) -> Dict[str, torch.Tensor]:
        """For the stage-by-stage tests: the chain stopped after `stop_after` (0..6) of its backward launches (GRAD_LAUNCHES) ->
        `gradients`; the maps of launches that did not run hold whatever the scratch held."""
        b, s = self._check_grad(gt, con_rgb, mask_sv, None)
        if not 0 <= int(stop_after) <= len(GRAD_LAUNCHES):
            raise ValueError("stop_after must be 0..%d" % len(GRAD_LAUNCHES))
        self._run_grad(gt, con_rgb, mask_sv, None, b, s, stop_after)
        return self.gradients(b, s)

    def gen_loss(self, gt: torch.Tensor, con_rgb: torch.Tensor, mask_sv: torch.Tensor) -> torch.Tensor:
        """gen as a differentiable scalar: float32 [] with a grad_fn whose backward hands d gen / d con_rgb * grad_output to con_rgb and
        None to gt and mask_sv.  When con_rgb requires a gradient, forward and backward run in one call here and the backward is one
        device multiply; nothing is synchronised."""
        return _GenLoss.apply(self, gt, con_rgb, mask_sv)


# the backward chain's launches in order and the gradient map each writes (the last writes grad)
GRAD_LAUNCHES = (("head", "conv3"), ("dgrad", "conv2"), ("dgrad", "conv1"), ("dgrad", "conv0"), ("dgrad_in", "in"), ("gather", "grad"))


class _GenLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, runner, gt, con_rgb, mask_sv):
        if ctx.needs_input_grad[2]:
            losses, _, grad = runner.gen_grad(gt.detach(), con_rgb.detach(), mask_sv.detach())
            ctx.save_for_backward(grad)
        else:
            losses = runner.gan_losses(gt.detach(), con_rgb.detach(), mask_sv.detach())[0]
        return losses[0]

    @staticmethod
    def backward(ctx, grad_output):
        if not ctx.needs_input_grad[2]:
            return None, None, None, None
        grad, = ctx.saved_tensors
        return None, None, grad * grad_output.to(torch.float32).reshape(()), None
