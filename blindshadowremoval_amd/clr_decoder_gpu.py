"""The device binding of the generator's colour decoder backward: bsr_clr_decoder_grad (csrc/clr_up_grad_kernels.h), held to
generator_grad.py's host statement (decoder_grad).  A post_gpu.GradStage like clr_tail_gpu.ColourTail: here are the stage's declaration,
its public calls and what the chain leaves in the scratch."""
from __future__ import annotations

from typing import Dict

import torch

from . import _lib
from .pack import pack_clr_decoder_grad
from .post_gpu import DENSE, STRIDED, GradStage
from .weights import generator_decoder_trainable_names

# the chain's launches in order and what each writes
LAUNCHES = (("mask", "gz3 (only when maps are kept)"), ("wgrad3", "clr_up3 kernel partials, S partials"), ("dgrad3", "gz2"),
            ("wgrad2", "clr_up2 kernel partials, S partials"), ("dgrad2", "gz1"), ("wgrad1", "clr_up1 kernel partials, S partials"),
            ("dgrad1", "d_x"), ("fold", "the three kernels, Wg, S"), ("finish", "bias, gamma, beta of the three layers"))
MAPS = (("gz1", 4, 128), ("gz2", 2, 96), ("gz3", 1, 64))       # name, the image's size over the map's, channels: bsr_clr_decoder_grad_offset's 0..2
LAYER_SHAPES = ((128, 261), (96, 128), (64, 96))               # (O, C) of clr_up1..3
SIZE_TEXT = "the colour decoder takes B >= 1 images with H a multiple of 32 and W a multiple of 256, got B=%d H=%d W=%d"
NO_WEIGHTS_TEXT = "the colour decoder has no weights: call load_weights or restore first"


class ColourDecoder(GradStage):
    """`ColourDecoder(device).decoder_grad(x, f1, f2, f, d_f)` — the gradients of the generator's colour decoder (clr_up1, clr_up2,
    clr_up3; training=False; GSC width) on `device`, after `load_weights(dict)` (the generator's variables; ValueError for TSM weights)
    or `restore(ckpt_dir)`: d / d x at res_stack/5's output and the twelve variable gradients of
    weights.generator_decoder_trainable_names().  `backward(generator, d_f)` reads x, f1, f2, f in place from the generator's workspace."""
    SYMBOL = "bsr_clr_decoder_grad"
    PACK, NAMES = staticmethod(pack_clr_decoder_grad), staticmethod(generator_decoder_trainable_names)
    INPUTS = (("x", 261, 8, STRIDED), ("f1", 128, 4, STRIDED), ("f2", 96, 2, STRIDED), ("f", 64, 1, STRIDED), ("d_f", 64, 1, DENSE))
    LEAD = "d_f"
    OUTPUTS = (("d_x", 261, 8),)
    TAKES_KEEP = True
    KEPT = ("gz1", "gz2", "gz3")
    MULTIPLES = (32, 256)
    IMAGE_DIMS = ".,."         # the images come at four sizes
    LIKE_TEXT, SIZE_TEXT, NO_WEIGHTS_TEXT, WHAT = "for this d_f", SIZE_TEXT, NO_WEIGHTS_TEXT, "the colour decoder"
    LAUNCHES = LAUNCHES
    LAST = "last_decoder"

    def maps(self, b: int, h: int, w: int, keep: bool = True) -> Dict[str, torch.Tensor]:
        """Copies of what the last call of these sizes left in the scratch: `gz1` [B,H/4,W/4,128], `gz2` [B,H/2,W/2,96] (and `gz3`
        [B,H,W,64] when that call kept it), `Wg1..3` float64 [3,3,O,C] (the kernel gradients before the BN factor) and `S1..3` float64
        [O] (the sums of gz)."""
        lib = _lib.load()
        self.scratch4(b, h, w, keep)
        out = {name: self.view(int(lib.bsr_clr_decoder_grad_offset(b, h, w, i)), (b, h // div, w // div, c)).clone()
               for i, (name, div, c) in enumerate(MAPS) if keep or name != "gz3"}
        for i, (o, c) in enumerate(LAYER_SHAPES):
            out["Wg%d" % (i + 1)] = self.view(int(lib.bsr_clr_decoder_grad_offset(b, h, w, 3 + i)), (3, 3, o, c), torch.float64).clone()
            out["S%d" % (i + 1)] = self.view(int(lib.bsr_clr_decoder_grad_offset(b, h, w, 6 + i)), (o,), torch.float64).clone()
        return out

    def decoder_grad(self, x: torch.Tensor, f1: torch.Tensor, f2: torch.Tensor, f: torch.Tensor, d_f: torch.Tensor, keep: bool = False):
        """x [B,H/8,W/8,261], f1 [B,H/4,W/4,128], f2 [B,H/2,W/2,96], f [B,H,W,64], d_f [B,H,W,64] -> dict(`d_x` [B,H/8,W/8,261] and the
        twelve variable gradients by name, views of one flat tensor which is under ""; with `keep` also copies of the stage maps `gz1`,
        `gz2`, `gz3`), float32 on the device, asynchronously on the current stream.  Everything is checked here, before any launch:
        TypeError / ValueError."""
        return self._grad(dict(x=x, f1=f1, f2=f2, f=f, d_f=d_f), keep)

    def backward(self, generator, d_f: torch.Tensor, keep: bool = False):
        """decoder_grad with x, f1, f2, f read in place from `generator`'s workspace (Generator.last_decoder: the last forward's, no
        copies), for a d_f of that forward's shape.  The generator must be an fp32 GSC one on this device whose last forward ran on the
        current stream."""
        return self._backward(generator, dict(d_f=d_f), keep)
