"""The device binding of the backward of res_stack/2, res_stack/1 and res_stack/0: bsr_lower_trunk_grad
(csrc/lower_trunk_grad_kernels.h), held to generator_grad.py's host statement (lower_trunk_grad).  A post_gpu.GradStage like
colour_trunk_gpu.ColourTrunk: here are the stage's declaration, its public calls and what the chain leaves in the scratch."""
from __future__ import annotations

from typing import Dict

import torch

from . import _lib, bottleneck_grad_gpu, nonlocal_grad_gpu
from .pack import LOWER_TRUNK_WIDTHS, pack_lower_trunk_grad
from .post_gpu import DENSE, STRIDED, GradStage
from .weights import generator_lower_trunk_trainable_names

BLOCKS = (2, 1, 0)             # in the chain's order
# the chain's launches in order and what each writes: the two existing chains per block, their names prefixed
LAUNCHES = tuple(("%s%d.%s" % (tag, b, name), "block %d: %s" % (b, what)) for b in BLOCKS
                 for tag, chain in (("nl", nonlocal_grad_gpu.LAUNCHES), ("bn", bottleneck_grad_gpu.LAUNCHES))
                 for name, what in chain)
N_NL_MAPS, N_BN_MAPS = 10, 8   # bsr_nonlocal_grad_offset's and bsr_bottleneck_grad_offset's maps: a block's take 18 of bsr_lower_trunk_grad_offset's
C_Y, C_X0 = 257, 99
# the intermediate data gradients: name -> (bsr_lower_trunk_grad_offset's map, channels)
DATA = {"d_y3_2": (54, C_Y), "d_skip_2": (55, C_Y), "d_xin2": (56, C_Y), "d_y3_1": (57, C_Y), "d_skip_1": (58, C_Y), "d_xin1": (59, C_Y),
        "d_y3_0": (60, C_Y), "d_skip_0": (61, C_X0)}
KEPT = tuple("a%d_%d" % (j, b) for b in BLOCKS for j in (1, 2)) + tuple(DATA)
SIZE_TEXT = "the lower trunk takes B >= 1 grids with h a multiple of 4 and w a multiple of 32, got B=%d h=%d w=%d"
NO_WEIGHTS_TEXT = "the lower trunk has no weights: call load_weights or restore first"


class LowerTrunk(GradStage):
    """`LowerTrunk(device).lower_trunk_grad(y3x2, out2, y3x1, out1, y3x0, out0, x0, d_res2)` — the gradients of the generator's
    res_stack/2, res_stack/1 and res_stack/0, the blocks both branches share (training=False; GSC width), on `device`, after
    `load_weights(dict)` (the generator's variables; ValueError for TSM and RGB weights) or `restore(ckpt_dir)`: `d_x0`, the gradient at
    x0 = cat[down3's output 96 | the resized uv 3], and the 66 variable gradients of weights.generator_lower_trunk_trainable_names().
    `backward(generator, d_res2)` reads the seven tensors in place from the generator's workspace."""
    SYMBOL = "bsr_lower_trunk_grad"
    PACK, NAMES = staticmethod(pack_lower_trunk_grad), staticmethod(generator_lower_trunk_trainable_names)
    INPUTS = (("y3x2", C_Y, 1, STRIDED), ("out2", C_Y, 1, STRIDED), ("y3x1", C_Y, 1, STRIDED), ("out1", C_Y, 1, STRIDED), ("y3x0", C_Y, 1, STRIDED),
              ("out0", C_Y, 1, STRIDED), ("x0", C_X0, 1, STRIDED), ("d_res2", C_Y, 1, DENSE))
    LEAD = "d_res2"
    OUTPUTS = (("d_x0", C_X0, 1),)
    KEPT = KEPT
    MULTIPLES = (4, 32)
    DIMS = IMAGE_DIMS = "h,w"
    LIKE_TEXT, SIZE_TEXT, NO_WEIGHTS_TEXT, WHAT = "for this d_res2", SIZE_TEXT, NO_WEIGHTS_TEXT, "the lower trunk"
    LAUNCHES = LAUNCHES
    LAST = "last_lower_trunk"

    def maps(self, b: int, h: int, w: int) -> Dict[str, torch.Tensor]:
        """Copies of what the last call of these sizes left in the scratch: per block b = 2, 1, 0 NonLocalGrad.maps' under `nl<b>.<name>`
        and BottleneckGrad.maps' under `bn<b>.<name>` at the block's input width (each sub-chain has a region of its own), the
        bottlenecks' `a1_<b>`, `a2_<b>` again under the names the host statement gives them, and the intermediate data gradients
        `d_y3_<b>`, `d_skip_<b>`, `d_xin2`, `d_xin1` [B,h,w,257] (`d_skip_0` [B,h,w,99])."""
        lib = _lib.load()
        self.scratch3(b, h, w)
        out = {}
        for k, block in enumerate(BLOCKS):
            first = k * (N_NL_MAPS + N_BN_MAPS)
            nl = nonlocal_grad_gpu.read_maps(self.view, lambda i: int(lib.bsr_lower_trunk_grad_offset(b, h, w, first + i)), b, h * w)
            bn = bottleneck_grad_gpu.read_maps(self.view, lambda i: int(lib.bsr_lower_trunk_grad_offset(b, h, w, first + N_NL_MAPS + i)), b, h, w,
                                               LOWER_TRUNK_WIDTHS[block])
            out.update(("nl%d.%s" % (block, name), t) for name, t in nl.items())
            out.update(("bn%d.%s" % (block, name), t) for name, t in bn.items())
            out["a1_%d" % block], out["a2_%d" % block] = bn["a1"], bn["a2"]
        for name, (index, c) in DATA.items():
            out[name] = self.view(int(lib.bsr_lower_trunk_grad_offset(b, h, w, index)), (b, h, w, c)).clone()
        return out

    def lower_trunk_grad(self, y3x2: torch.Tensor, out2: torch.Tensor, y3x1: torch.Tensor, out1: torch.Tensor, y3x0: torch.Tensor, out0: torch.Tensor,
                         x0: torch.Tensor, d_res2: torch.Tensor, keep: bool = False):
        """y3x<b> [B,h,w,257] = block b's bnorm3 output + its input zero-padded to 257 channels, out<b> [B,h,w,257] its output (block 2's
        input is out1, block 1's out0), x0 [B,h,w,99] block 0's input, d_res2 [B,h,w,257] the complete gradient at res_stack/2's output ->
        dict(`d_x0` [B,h,w,99] and the 66 variable gradients by name, views of one flat tensor which is under ""; with `keep` also
        `a1_<b>`, `a2_<b>` per block and the intermediate data gradients `d_y3_<b>`, `d_skip_<b>`, `d_xin2`, `d_xin1`), float32 on the
        device, asynchronously on the current stream.  Everything is checked here, before any launch: TypeError / ValueError."""
        return self._grad(dict(y3x2=y3x2, out2=out2, y3x1=y3x1, out1=out1, y3x0=y3x0, out0=out0, x0=x0, d_res2=d_res2), keep)

    def backward(self, generator, d_res2: torch.Tensor, keep: bool = False):
        """lower_trunk_grad with the seven tensors read in place from `generator`'s workspace (Generator.last_lower_trunk: the last
        forward's, no copies), for a d_res2 [B,H/8,W/8,257] of that forward's shape (ColourTrunk's `d_res2`).  The generator must be an
        fp32 GSC one on this device whose last forward ran on the current stream."""
        return self._backward(generator, dict(d_res2=d_res2), keep)

    def stages(self, y3x2, out2, y3x1, out1, y3x0, out0, x0, d_res2, n):
        """The chain stopped after `n` of its launches (`LAUNCHES`) -> `maps`, `d_x0` and the flat gradient buffer under ""."""
        return super().stages(y3x2, out2, y3x1, out1, y3x0, out0, x0, d_res2, n)
