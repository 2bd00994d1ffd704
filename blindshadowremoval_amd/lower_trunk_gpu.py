"""The device binding of the backward of res_stack/2, res_stack/1 and res_stack/0: bsr_lower_trunk_grad (csrc/block_chain_grad.h), held to
generator_grad.py's host statement (lower_trunk_grad).  A block_chain_gpu.BlockChainStage: here are its declaration and public calls."""
from __future__ import annotations

import torch

from .block_chain_gpu import BlockChainStage
from .pack import pack_lower_trunk_grad
from .post_gpu import DENSE, STRIDED
from .weights import generator_lower_trunk_trainable_names

C_Y, C_X0 = 257, 99
SIZE_TEXT = "the lower trunk takes B >= 1 grids with h a multiple of 4 and w a multiple of 32, got B=%d h=%d w=%d"
NO_WEIGHTS_TEXT = "the lower trunk has no weights: call load_weights or restore first"


class LowerTrunk(BlockChainStage):
    """`LowerTrunk(device).lower_trunk_grad(y3x2, out2, y3x1, out1, y3x0, out0, x0, d_res2)` — the gradients of the generator's
    res_stack/2, res_stack/1 and res_stack/0, the blocks both branches share (training=False; GSC width), on `device`, after
    `load_weights(dict)` (the generator's variables; ValueError for TSM and RGB weights) or `restore(ckpt_dir)`: `d_x0`, the gradient at
    x0 = cat[down3's output 96 | the resized uv 3], and the 66 variable gradients of weights.generator_lower_trunk_trainable_names().
    `backward(generator, d_res2)` reads the seven tensors in place from the generator's workspace."""
    SYMBOL = "bsr_lower_trunk_grad"
    BLOCKS = (2, 1, 0)         # in the chain's order; no tail: block 0's d_xin is d_x0
    PACK, NAMES = staticmethod(pack_lower_trunk_grad), staticmethod(generator_lower_trunk_trainable_names)
    INPUTS = (("y3x2", C_Y, 1, STRIDED), ("out2", C_Y, 1, STRIDED), ("y3x1", C_Y, 1, STRIDED), ("out1", C_Y, 1, STRIDED), ("y3x0", C_Y, 1, STRIDED),
              ("out0", C_Y, 1, STRIDED), ("x0", C_X0, 1, STRIDED), ("d_res2", C_Y, 1, DENSE))
    LEAD = "d_res2"
    OUTPUTS = (("d_x0", C_X0, 1),)
    MULTIPLES = (4, 32)
    DIMS = IMAGE_DIMS = "h,w"
    LIKE_TEXT, SIZE_TEXT, NO_WEIGHTS_TEXT, WHAT = "for this d_res2", SIZE_TEXT, NO_WEIGHTS_TEXT, "the lower trunk"
    LAST = "last_lower_trunk"

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


BLOCKS, LAUNCHES, DATA, KEPT = LowerTrunk.BLOCKS, LowerTrunk.LAUNCHES, LowerTrunk.DATA, LowerTrunk.KEPT
