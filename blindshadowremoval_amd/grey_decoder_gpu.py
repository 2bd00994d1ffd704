"""The device binding of the generator's grey decoder backward: bsr_grey_decoder_grad (csrc/grey_up_grad_kernels.h), held to
generator_grad.py's host statement (grey_decoder_grad).  A post_gpu.GradStage like clr_decoder_gpu.ColourDecoder: here are the stage's
declaration, its public calls and what the chain leaves in the scratch."""
from __future__ import annotations

from typing import Dict

import torch

from . import _lib
from .pack import pack_grey_decoder_grad
from .post_gpu import DENSE, STRIDED, GradStage
from .weights import generator_grey_decoder_trainable_names

# the chain's launches in order and what each writes
LAUNCHES = (("mask", "gz3 (only when maps are kept)"), ("wgrad3", "up3 kernel partials, S partials"), ("dgrad3", "gz2, d_x2"),
            ("wgrad2", "up2 kernel partials, S partials"), ("dgrad2", "gz1, d_x3"), ("wgrad1", "up1 kernel partials, S partials"),
            ("dgrad1", "d_x"), ("fold", "the three kernels, Wg, S"), ("finish", "bias, gamma, beta of the three layers"))
MAPS = (("gz1", 4, 96), ("gz2", 2, 64), ("gz3", 1, 64))        # name, the image's size over the map's, channels: bsr_grey_decoder_grad_offset's 0..2
LAYER_SHAPES = ((96, 257), (64, 160), (64, 128))               # (O, C) of up1..3
SIZE_TEXT = "the grey decoder takes B >= 1 images with H a multiple of 32 and W a multiple of 256, got B=%d H=%d W=%d"
NO_WEIGHTS_TEXT = "the grey decoder has no weights: call load_weights or restore first"


class GreyDecoder(GradStage):
    """`GreyDecoder(device).grey_decoder_grad(x, c2, c3, y, d_y)` — the gradients of the generator's grey decoder (up1, up2, up3;
    training=False; GSC width) on `device`, after `load_weights(dict)` (the generator's variables; ValueError for TSM and RGB weights) or
    `restore(ckpt_dir)`: d / d x at res_stack/2's output, the skip gradients d_x3 and d_x2, and the twelve variable gradients of
    weights.generator_grey_decoder_trainable_names().  `backward(generator, d_y)` reads x, c2, c3, y in place from the generator's
    workspace."""
    SYMBOL = "bsr_grey_decoder_grad"
    PACK, NAMES = staticmethod(pack_grey_decoder_grad), staticmethod(generator_grey_decoder_trainable_names)
    INPUTS = (("x", 257, 8, STRIDED), ("c2", 160, 4, STRIDED), ("c3", 128, 2, STRIDED), ("y", 64, 1, STRIDED), ("d_y", 64, 1, DENSE))
    LEAD = "d_y"
    OUTPUTS = (("d_x", 257, 8), ("d_x3", 64, 4), ("d_x2", 64, 2))
    TAKES_KEEP = True
    KEPT = ("gz1", "gz2", "gz3")
    MULTIPLES = (32, 256)
    IMAGE_DIMS = ".,."         # the images come at four sizes
    LIKE_TEXT, SIZE_TEXT, NO_WEIGHTS_TEXT, WHAT = "for this d_y", SIZE_TEXT, NO_WEIGHTS_TEXT, "the grey decoder"
    LAUNCHES = LAUNCHES
    LAST = "last_grey_decoder"

    def maps(self, b: int, h: int, w: int, keep: bool = True) -> Dict[str, torch.Tensor]:
        """Copies of what the last call of these sizes left in the scratch: `gz1` [B,H/4,W/4,96], `gz2` [B,H/2,W/2,64] (and `gz3`
        [B,H,W,64] when that call kept it), `Wg1..3` float64 [3,3,O,C] (the kernel gradients before the BN factor) and `S1..3` float64
        [O] (the sums of gz)."""
        lib = _lib.load()
        self.scratch4(b, h, w, keep)
        out = {name: self.view(int(lib.bsr_grey_decoder_grad_offset(b, h, w, i)), (b, h // div, w // div, c)).clone()
               for i, (name, div, c) in enumerate(MAPS) if keep or name != "gz3"}
        for i, (o, c) in enumerate(LAYER_SHAPES):
            out["Wg%d" % (i + 1)] = self.view(int(lib.bsr_grey_decoder_grad_offset(b, h, w, 3 + i)), (3, 3, o, c), torch.float64).clone()
            out["S%d" % (i + 1)] = self.view(int(lib.bsr_grey_decoder_grad_offset(b, h, w, 6 + i)), (o,), torch.float64).clone()
        return out

    def grey_decoder_grad(self, x: torch.Tensor, c2: torch.Tensor, c3: torch.Tensor, y: torch.Tensor, d_y: torch.Tensor, keep: bool = False):
        """x [B,H/8,W/8,257], c2 = cat[up1, x3] [B,H/4,W/4,160], c3 = cat[up2, x2] [B,H/2,W/2,128], y [B,H,W,64], d_y [B,H,W,64] ->
        dict(`d_x` [B,H/8,W/8,257], `d_x3` [B,H/4,W/4,64], `d_x2` [B,H/2,W/2,64] and the twelve variable gradients by name, views of one
        flat tensor which is under ""; with `keep` also copies of the stage maps `gz1`, `gz2`, `gz3`), float32 on the device,
        asynchronously on the current stream.  Everything is checked here, before any launch: TypeError / ValueError."""
        return self._grad(dict(x=x, c2=c2, c3=c3, y=y, d_y=d_y), keep)

    def backward(self, generator, d_y: torch.Tensor, keep: bool = False):
        """grey_decoder_grad with x, c2, c3, y read in place from `generator`'s workspace (Generator.last_grey_decoder: the last
        forward's, no copies), for a d_y of that forward's shape (HeadsGrad's).  The generator must be an fp32 GSC one on this device
        whose last forward ran on the current stream."""
        return self._backward(generator, dict(d_y=d_y), keep)
