"""The device binding of the backward of res_stack/4, res_stack/3 and the hole: bsr_colour_trunk_grad (csrc/colour_trunk_grad_kernels.h),
held to generator_grad.py's host statement (colour_trunk_grad).  A post_gpu.GradStage like bottleneck_grad_gpu.BottleneckGrad: here are
the stage's declaration, its public calls and what the chain leaves in the scratch."""
from __future__ import annotations

from typing import Dict, Optional

import torch

from . import _lib, bottleneck_grad_gpu, nonlocal_grad_gpu
from .pack import pack_colour_trunk_grad
from .post_gpu import DENSE, OPTIONAL, STRIDED, GradStage
from .weights import generator_colour_trunk_trainable_names

BLOCKS = (4, 3)                # in the chain's order
# the chain's launches in order and what each writes: the two existing chains per block, their names prefixed, and the hole
LAUNCHES = tuple(("%s%d.%s" % (tag, b, name), "block %d: %s" % (b, what)) for b in BLOCKS
                 for tag, chain in (("nl", nonlocal_grad_gpu.LAUNCHES), ("bn", bottleneck_grad_gpu.LAUNCHES))
                 for name, what in chain) + (("hole", "d_res2"),)
N_NL_MAPS, N_BN_MAPS = 10, 8   # bsr_nonlocal_grad_offset's and bsr_bottleneck_grad_offset's maps: a block's take 18 of bsr_colour_trunk_grad_offset's
# the intermediate data gradients: name -> (bsr_colour_trunk_grad_offset's map, channels)
DATA = {"d_y3_4": (36, 257), "d_skip_4": (37, 261), "d_xin4": (38, 261), "d_y3_3": (39, 257), "d_skip_3": (40, 261), "d_xin3": (41, 261)}
KEPT = tuple("a%d_%d" % (j, b) for b in BLOCKS for j in (1, 2)) + tuple(DATA)
C_IN, C_Y = 261, 257
SIZE_TEXT = "the colour trunk takes B >= 1 grids with h a multiple of 4 and w a multiple of 32, got B=%d h=%d w=%d"
NO_WEIGHTS_TEXT = "the colour trunk has no weights: call load_weights or restore first"


ALIGN_TEXT = "%s must be 16-byte aligned (a contiguous view that starts at an odd storage offset is not), got address %#x"


def _aligned(**tensors) -> None:
    """ValueError for a tensor that does not start on a 16-byte boundary: the hole kernel reads and writes 16-byte words."""
    for name, t in tensors.items():
        if t is not None and t.data_ptr() % 16:
            raise ValueError(ALIGN_TEXT % (name, t.data_ptr()))


class ColourTrunk(GradStage):
    """`ColourTrunk(device).colour_trunk_grad(y3x4, out4, y3x3, out3, xh, d_xin, d_x)` — the gradients of the generator's res_stack/4,
    res_stack/3 and the hole x_hole = x (1 - bmask) (training=False; GSC width) on `device`, after `load_weights(dict)` (the generator's
    variables; ValueError for TSM weights) or `restore(ckpt_dir)`: `d_res2`, the complete gradient at res_stack/2's output — the colour
    branch's through the hole plus the grey branch's `d_x` — and the 44 variable gradients of
    weights.generator_colour_trunk_trainable_names().  `backward(generator, d_xin, d_x)` reads y3x4, out4, y3x3, out3, xh in place from
    the generator's workspace."""
    SYMBOL = "bsr_colour_trunk_grad"
    PACK, NAMES = staticmethod(pack_colour_trunk_grad), staticmethod(generator_colour_trunk_trainable_names)
    INPUTS = (("y3x4", C_Y, 1, STRIDED), ("out4", C_IN, 1, STRIDED), ("y3x3", C_Y, 1, STRIDED), ("out3", C_IN, 1, STRIDED), ("xh", C_IN, 1, STRIDED),
              ("d_xin", C_IN, 1, DENSE), ("d_x", C_Y, 1, OPTIONAL))
    LEAD = "d_xin"
    OUTPUTS = (("d_res2", C_Y, 1),)
    KEPT = KEPT
    MULTIPLES = (4, 32)
    DIMS = IMAGE_DIMS = "h,w"
    LIKE_TEXT, SIZE_TEXT, NO_WEIGHTS_TEXT, WHAT = "for this d_xin", SIZE_TEXT, NO_WEIGHTS_TEXT, "the colour trunk"
    LAUNCHES = LAUNCHES
    LAST = "last_colour_trunk"

    def maps(self, b: int, h: int, w: int) -> Dict[str, torch.Tensor]:
        """Copies of what the last call of these sizes left in the scratch: per block b = 4, 3 NonLocalGrad.maps' under `nl<b>.<name>` and
        BottleneckGrad.maps' under `bn<b>.<name>` (each sub-chain has a region of its own), the bottlenecks' `a1_<b>`, `a2_<b>` again
        under the names the host statement gives them, and the intermediate data gradients `d_y3_<b>` [B,h,w,257], `d_skip_<b>`, `d_xin4`,
        `d_xin3` [B,h,w,261]."""
        lib = _lib.load()
        self.scratch3(b, h, w)
        out = {}
        for k, block in enumerate(BLOCKS):
            first = k * (N_NL_MAPS + N_BN_MAPS)
            nl = nonlocal_grad_gpu.read_maps(self.view, lambda i: int(lib.bsr_colour_trunk_grad_offset(b, h, w, first + i)), b, h * w)
            bn = bottleneck_grad_gpu.read_maps(self.view, lambda i: int(lib.bsr_colour_trunk_grad_offset(b, h, w, first + N_NL_MAPS + i)), b, h, w)
            out.update(("nl%d.%s" % (block, name), t) for name, t in nl.items())
            out.update(("bn%d.%s" % (block, name), t) for name, t in bn.items())
            out["a1_%d" % block], out["a2_%d" % block] = bn["a1"], bn["a2"]
        for name, (index, c) in DATA.items():
            out[name] = self.view(int(lib.bsr_colour_trunk_grad_offset(b, h, w, index)), (b, h, w, c)).clone()
        return out

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
