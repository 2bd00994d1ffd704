"""The device binding of train_step's VGG19 perceptual term: bsr_vgg_per_loss (csrc/vgg_kernels.h), held to perceptual.py's host
statement."""
from __future__ import annotations

import ctypes
from typing import Dict

import numpy as np
import torch

from . import _lib
from . import perceptual as host
from .pack import pack_vgg
from .post_gpu import PostDevice
from .weights import VGG_BLOCKS, VGG_LAYERS, load_vgg_weights


class Perceptual(PostDevice):
    """`Perceptual(device).per_loss(gt, con_rgb)` — per_loss of the reference's train_step for a batch, on `device`, after
    `load_weights(dict)`, `load_blob(bytes)` or `load_npz(path)`."""
    SYMBOL = "bsr_vgg_per_loss"
    SIZE_TEXT = "the perceptual term takes 1..4096 items of side 32, 64, 128 or 256, got B=%(b)d S=%(s)d"

    def __init__(self, device: int):
        super().__init__(device)
        self._blob = None

    def load_weights(self, weights: Dict[str, np.ndarray]) -> None:
        """The 26 VGG19 variables (weights.vgg_variable_shapes) -> the packed blob on the device."""
        self.load_blob(pack_vgg(weights))

    def load_blob(self, blob: bytes) -> None:
        """A blob of pack.pack_vgg.  ValueError unless it holds bsr_vgg_blob_bytes() bytes."""
        want = int(_lib.load().bsr_vgg_blob_bytes())
        if len(blob) != want:
            raise ValueError("a VGG19 blob holds %d bytes, got %d" % (want, len(blob)))
        self._blob = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(self._dev)

    def load_npz(self, path: str) -> None:
        """The `.npz` of weights.load_vgg_weights."""
        self.load_weights(load_vgg_weights(path))

    def scratch(self, b: int, s: int) -> int:
        """The 256-byte aligned device address of at least bsr_vgg_scratch_bytes(b, s) bytes of scratch (the query is not named after
        SYMBOL, so PostDevice.scratch cannot find it)."""
        need = int(_lib.load().bsr_vgg_scratch_bytes(b, s))
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
