"""The device binding of train_step's three discriminators and GAN losses: bsr_disc_losses (csrc/disc_kernels.h), held to
discriminator.py's host statement."""
from __future__ import annotations

import ctypes
from typing import Dict

import numpy as np
import torch

from . import _lib
from . import discriminator as host
from .pack import pack_discriminators
from .post_gpu import PostDevice
from .weights import N_LAYER_D


class Discriminators(PostDevice):
    """`Discriminators(device).gan_losses(gt, con_rgb, mask_sv)` — gen, disc_real and disc_fake of the reference's train_step for a
    batch, on `device`, after `load_weights(dict)` or `restore(ckpt_dir)`."""
    SYMBOL = "bsr_disc_losses"
    SIZE_TEXT = "discriminators take 1..32767 items of side 32, 64, 128 or 256, got B=%(b)d S=%(s)d"

    def __init__(self, device: int):
        super().__init__(device)
        self._blob = None

    def load_weights(self, weights: Dict[str, np.ndarray]) -> None:
        """The three discriminators' variables (weights.discriminator_variable_shapes) -> the packed blob on the device."""
        self.load_blob(pack_discriminators(weights))

    def load_blob(self, blob: bytes) -> None:
        """A blob of pack.pack_discriminators.  ValueError unless it holds bsr_disc_blob_bytes() bytes."""
        want = int(_lib.load().bsr_disc_blob_bytes())
        if len(blob) != want:
            raise ValueError("a discriminator blob holds %d bytes, got %d" % (want, len(blob)))
        self._blob = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(self._dev)

    def restore(self, ckpt_dir: str) -> None:
        """The `discriminator_{1,2,3}/*` variables of the latest checkpoint under `ckpt_dir`."""
        from .tf_bundle import latest_checkpoint, load_discriminator_weights
        prefix = latest_checkpoint(ckpt_dir)
        if prefix is None:
            raise FileNotFoundError("no checkpoint under %s" % ckpt_dir)
        self.load_weights(load_discriminator_weights(prefix))

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
