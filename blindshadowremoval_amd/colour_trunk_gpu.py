"""The device binding of the backward of res_stack/4, res_stack/3 and the hole: bsr_colour_trunk_grad (csrc/colour_trunk_grad_kernels.h),
held to generator_grad.py's host statement (colour_trunk_grad).  A block_chain_gpu.BlockChainStage: here are its declaration, its public
calls and the hole's."""
from __future__ import annotations

from typing import Optional

import torch

from .block_chain_gpu import BlockChainStage
from .pack import pack_colour_trunk_grad
from .post_gpu import DENSE, OPTIONAL, STRIDED
from .weights import generator_colour_trunk_trainable_names

C_IN, C_Y = 261, 257
SIZE_TEXT = "the colour trunk takes B >= 1 grids with h a multiple of 4 and w a multiple of 32, got B=%d h=%d w=%d"
NO_WEIGHTS_TEXT = "the colour trunk has no weights: call load_weights or restore first"


ALIGN_TEXT = "%s must be 16-byte aligned (a contiguous view that starts at an odd storage offset is not), got address %#x"


def _aligned(**tensors) -> None:
    """ValueError for a tensor that does not start on a 16-byte boundary: the hole kernel reads and writes 16-byte words."""
    for name, t in tensors.items():
        if t is not None and t.data_ptr() % 16:
            raise ValueError(ALIGN_TEXT % (name, t.data_ptr()))


class ColourTrunk(BlockChainStage):
    """`ColourTrunk(device).colour_trunk_grad(y3x4, out4, y3x3, out3, xh, d_xin, d_x)` — the gradients of the generator's res_stack/4,
    res_stack/3 and the hole x_hole = x (1 - bmask) (training=False; GSC width) on `device`, after `load_weights(dict)` (the generator's
    variables; ValueError for TSM weights) or `restore(ckpt_dir)`: `d_res2`, the complete gradient at res_stack/2's output — the colour
    branch's through the hole plus the grey branch's `d_x` — and the 44 variable gradients of
    weights.generator_colour_trunk_trainable_names().  `backward(generator, d_xin, d_x)` reads y3x4, out4, y3x3, out3, xh in place from
    the generator's workspace."""
    SYMBOL = "bsr_colour_trunk_grad"
    BLOCKS, TAIL = (4, 3), ("hole", "d_res2")          # in the chain's order; the hole reads block 3's d_xin
    PACK, NAMES = staticmethod(pack_colour_trunk_grad), staticmethod(generator_colour_trunk_trainable_names)
    INPUTS = (("y3x4", C_Y, 1, STRIDED), ("out4", C_IN, 1, STRIDED), ("y3x3", C_Y, 1, STRIDED), ("out3", C_IN, 1, STRIDED), ("xh", C_IN, 1, STRIDED),
              ("d_xin", C_IN, 1, DENSE), ("d_x", C_Y, 1, OPTIONAL))
    LEAD = "d_xin"
    OUTPUTS = (("d_res2", C_Y, 1),)
    MULTIPLES = (4, 32)
    DIMS = IMAGE_DIMS = "h,w"
    LIKE_TEXT, SIZE_TEXT, NO_WEIGHTS_TEXT, WHAT = "for this d_xin", SIZE_TEXT, NO_WEIGHTS_TEXT, "the colour trunk"
    LAST = "last_colour_trunk"

    def colour_trunk_grad(self, y3x4: torch.Tensor, out4: torch.Tensor, y3x3: torch.Tensor, out3: torch.Tensor, xh: torch.Tensor, d_xin: torch.Tensor,
                          d_x: Optional[torch.Tensor] = None, keep: bool = False):
        """y3x<b> [B,h,w,257] = block b's bnorm3 output + the first 257 channels of its input, out<b> [B,h,w,261] its output (block 4's
        input is out3), xh [B,h,w,261] block 3's input (channel 257 is bmask, in {0, 1}), d_xin [B,h,w,261] the gradient at res_stack/5's
        input, d_x [B,h,w,257] the grey decoder's gradient at res_stack/2's output (None: nothing) -> dict(`d_res2` [B,h,w,257] and the 44
        variable gradients by name, views of one flat tensor which is under ""; with `keep` also `a1_<b>`, `a2_<b>` per block and the
        intermediate data gradients `d_y3_<b>`, `d_skip_<b>`, `d_xin4`, `d_xin3`), float32 on the device, asynchronously on the current
        stream.  Everything is checked here, before any launch: TypeError / ValueError."""
        return self._grad(dict(y3x4=y3x4, out4=out4, y3x3=y3x3, out3=out3, xh=xh, d_xin=d_xin, d_x=d_x), keep)

    def backward(self, generator, d_xin: torch.Tensor, d_x: Optional[torch.Tensor] = None, keep: bool = False):
        """colour_trunk_grad with y3x4, out4, y3x3, out3, xh read in place from `generator`'s workspace (Generator.last_colour_trunk: the
        last forward's, no copies), for a d_xin [B,H/8,W/8,261] of that forward's shape (BottleneckGrad's `d_xin`) and GreyDecoder's `d_x`.
        The generator must be an fp32 GSC one on this device whose last forward ran on the current stream."""
        return self._backward(generator, dict(d_xin=d_xin, d_x=d_x), keep)

    def hole_grad(self, xh: torch.Tensor, d_xin3: torch.Tensor, d_x: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The chain's last launch alone (bsr_debug_hole_grad), for the tests and the bench tool: xh [B,h,w,261] (channel 257 is bmask),
        d_xin3 [B,h,w,261], d_x [B,h,w,257] or None -> d_res2 [B,h,w,257] = d_xin3[..., :257] (1 - bmask) + d_x.  It needs no weights.
        Everything is checked here, before the launch: TypeError / ValueError."""
        self._image("d_xin3", d_xin3, C_IN)
        b, h, w = (int(d) for d in d_xin3.shape[:3])
        for name, t, c in (("d_xin3", d_xin3, C_IN), ("xh", xh, C_IN), ("d_x", d_x, C_Y)):
            if t is None:
                continue
            self._image(name, t, c)
            if tuple(t.shape) != (b, h, w, c):
                raise ValueError("%s must be [%d,%d,%d,%d] for this d_xin3, got %s" % (name, b, h, w, c, tuple(t.shape)))
        if b < 1 or h < 1 or w < 1 or h % self.MULTIPLES[0] or w % self.MULTIPLES[1]:
            raise ValueError(SIZE_TEXT % (b, h, w))
        _aligned(d_xin3=d_xin3, d_x=d_x)
        out = self.empty((b, h, w, C_Y), torch.float32)
        self.call(xh, C_IN, d_xin3, d_x, b, h, w, out, symbol="bsr_debug_hole_grad")
        return out

    def _check(self, given, in_place: bool = False):
        """GradStage's checks, then the 16-byte alignment the hole kernel needs of d_x."""
        sizes = super()._check(given, in_place)
        _aligned(d_x=given["d_x"])
        return sizes

    def stages(self, y3x4, out4, y3x3, out3, xh, d_xin, d_x, n):
        """The chain stopped after `n` of its launches (`LAUNCHES`) -> `maps`, `d_res2` and the flat gradient buffer under ""."""
        return super().stages(y3x4, out4, y3x3, out3, xh, d_xin, d_x, n)


BLOCKS, LAUNCHES, DATA, KEPT = ColourTrunk.BLOCKS, ColourTrunk.LAUNCHES, ColourTrunk.DATA, ColourTrunk.KEPT
