"""The device binding of the shadow synthesis: bsr_shadow_synth (csrc/shadow_synth_kernels.h), held to shadow_synth.py's host statement."""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import shadow_synth as host
from .post_gpu import PostDevice


class ShadowSynth(PostDevice):
    """`ShadowSynth(device).process_mask(mask, gt, img_dark, face, draws)` — process_mask of the reference for a batch, on `device`."""
    SYMBOL = "bsr_shadow_synth"
    SIZE_TEXT = "process_mask takes 1..65535 items of side 32, 64, 128 or 256, got B=%(b)d S=%(s)d"

    def process_mask(self, mask: torch.Tensor, gt: torch.Tensor, img_dark: torch.Tensor, face: torch.Tensor, draws: Sequence[host.ShadowDraws],
                     out: Optional[Tuple[torch.Tensor, ...]] = None, aux: Optional[torch.Tensor] = None):
        """-> (img, mask_sv, mask_edge [B,S,S,3] float32, status [B] int32) on the device, asynchronously on the current stream.  `out`:
        four such tensors to write into.  `aux`: an optional float32 [B,3,S,S] that receives the Perlin map, the brightness mask and
        the composited mask.  Everything is checked here, before any launch: TypeError / ValueError."""
        b, s = self.images((("mask", mask, 1), ("gt", gt, 3), ("img_dark", img_dark, 3), ("face", face, 1)), 65535)
        if len(draws) != b:
            raise ValueError("process_mask: %d draws records for %d items" % (len(draws), b))
        blob = torch.from_numpy(host.pack_draws(draws, s).view(np.int32)).to(self._dev)          # ValueError: r too large for S, bad integers
        if out is None:
            out = tuple(self.empty((b, s, s, 3), torch.float32) for _ in range(3)) + (self.empty((b,), torch.int32),)
        else:
            if len(out) != 4:
                raise ValueError("out is (img, mask_sv, mask_edge, status)")
            for name, t, shape, dt in (("img", out[0], (b, s, s, 3), torch.float32), ("mask_sv", out[1], (b, s, s, 3), torch.float32),
                                       ("mask_edge", out[2], (b, s, s, 3), torch.float32), ("status", out[3], (b,), torch.int32)):
                if not isinstance(t, torch.Tensor) or t.dtype != dt or tuple(t.shape) != shape or t.device != self._dev or not t.is_contiguous():
                    raise ValueError("out: %s must be a contiguous %s tensor %s on %s" % (name, dt, shape, self._dev))
        if aux is not None and (not isinstance(aux, torch.Tensor) or aux.dtype != torch.float32 or tuple(aux.shape) != (b, 3, s, s)
                                or aux.device != self._dev or not aux.is_contiguous()):
            raise ValueError("aux must be a contiguous float32 tensor [%d,3,%d,%d] on %s" % (b, s, s, self._dev))
        scratch = self.scratch(b, s)
        self.call(mask, gt, img_dark, face, blob, ctypes.c_size_t(blob.numel() * 4), b, s, out[0], out[1], out[2], out[3],
                  aux if aux is not None else None, ctypes.c_void_p(scratch))
        return out
