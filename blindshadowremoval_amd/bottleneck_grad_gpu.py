"""The device binding of the backward of res_stack/5's lower half — conv1/bnorm1/relu1, conv2/bnorm2/relu2, conv3/bnorm3 and the sum
with what the skip carries: bsr_bottleneck_grad (csrc/bottleneck_grad_kernels.h), held to generator_grad.py's host statement
(bottleneck_grad).  A post_gpu.GradStage like nonlocal_grad_gpu.NonLocalGrad: here are the stage's declaration, its public calls and what
the chain leaves in the scratch."""
from __future__ import annotations

import functools
from typing import Dict, Optional

import torch

from . import _lib
from .pack import pack_bottleneck_grad
from .post_gpu import DENSE, OPTIONAL, STRIDED, GradStage
from .weights import generator_bottleneck_trainable_names

# the chain's launches in order and what each writes
LAUNCHES = (("entry", "xp, dyp, S3 partials"), ("a1", "a1"), ("a2", "a2"), ("gz2", "gz2"), ("gz1", "gz1"), ("wgrad_conv2", "a1^T gz2 partials per tap"),
            ("wgrad_conv3", "a2^T d_y3 partials"), ("wgrad_conv1", "xin^T gz1 partials"), ("dgrad", "d_xin"), ("colsum", "S2, S1 partials"),
            ("fold", "the three kernels, Wg"), ("finish", "the biases, gammas, betas, S"))
# name -> (bsr_bottleneck_grad_offset's map, columns, columns kept)
MAPS = {"xp": (0, 272, 261), "dyp": (1, 272, 257), "a1": (2, 128, 128), "a2": (3, 128, 128), "gz2": (4, 128, 128), "gz1": (5, 128, 128)}
KEPT = ("gz2", "gz1", "a1", "a2")
C_IN, C_Y, D = 261, 257, 128
SIZE_TEXT = "the bottleneck takes B >= 1 grids with h a multiple of 4 and w a multiple of 32, got B=%d h=%d w=%d"
NO_WEIGHTS_TEXT = "the bottleneck has no weights: call load_weights or restore first"


def read_maps(view, offset, b: int, h: int, w: int, width: int = C_IN) -> Dict[str, torch.Tensor]:
    """Copies of the chain's maps out of a scratch: `view`(byte offset, shape[, dtype]) gives a tensor over it, `offset`(index) the byte
    offset of bsr_bottleneck_grad_offset's map `index` (colour_trunk_gpu and lower_trunk_gpu read each block's region with its own).
    `width`: the block's input width, 261 (blocks 3..5), 257 (blocks 1, 2) or 99 (block 0) — xp's rows are `width` rounded up to 16
    floats and Wg1 is [width,128]."""
    out = {}
    for name, (index, cols, kept) in MAPS.items():
        if name == "xp":
            cols, kept = (width + 15) // 16 * 16, width
        out[name] = view(offset(index), (b, h, w, cols))[..., :kept].clone()
    wg = view(offset(6), (width * D + 9 * D * D + D * C_Y,), torch.float64)
    out["Wg1"] = wg[:width * D].reshape(width, D).clone()
    out["Wg2"] = wg[width * D:width * D + 9 * D * D].reshape(3, 3, D, D).clone()
    out["Wg3"] = wg[width * D + 9 * D * D:].reshape(D, C_Y).clone()
    s = view(offset(7), (2 * D + C_Y,), torch.float64)
    out["S1"], out["S2"], out["S3"] = s[:D].clone(), s[D:2 * D].clone(), s[2 * D:].clone()
    return out


class BottleneckGrad(GradStage):
    """`BottleneckGrad(device).bottleneck_grad(xin, d_y3, d_skip)` — the gradients of the lower half of the generator's res_stack/5
    (training=False; GSC width) on `device`, after `load_weights(dict)` (the generator's variables; ValueError for TSM weights;
    `block=3` or `4` reads that block's, whose shapes are the same) or `restore(ckpt_dir)`: `d_xin` at the block's input and the twelve
    variable gradients of weights.generator_bottleneck_trainable_names().  `backward(generator, d_y3, d_skip)` reads xin in place from the
    generator's workspace."""
    SYMBOL = "bsr_bottleneck_grad"
    PACK, NAMES = staticmethod(pack_bottleneck_grad), staticmethod(generator_bottleneck_trainable_names)
    INPUTS = (("xin", C_IN, 1, STRIDED), ("d_y3", C_Y, 1, DENSE), ("d_skip", C_IN, 1, OPTIONAL))
    LEAD = "d_y3"
    OUTPUTS = (("d_xin", C_IN, 1),)
    KEPT = KEPT
    MULTIPLES = (4, 32)
    DIMS = IMAGE_DIMS = "h,w"
    LIKE_TEXT, SIZE_TEXT, NO_WEIGHTS_TEXT, WHAT = "for this d_y3", SIZE_TEXT, NO_WEIGHTS_TEXT, "the bottleneck"
    LAUNCHES = LAUNCHES
    LAST = "last_block5_input"

    def load_weights(self, weights, block: int = 5) -> None:
        """The generator's variables (res_stack/<block>'s are read) -> the chain's blob on the device."""
        self.PACK = functools.partial(pack_bottleneck_grad, block=block)
        super().load_weights(weights)

    def maps(self, b: int, h: int, w: int) -> Dict[str, torch.Tensor]:
        """Copies of what the last call of these sizes left in the scratch: `xp` [B,h,w,261] and `dyp` [B,h,w,257] (the padded copies of
        xin and d_y3), `a1`, `a2`, `gz2`, `gz1` [B,h,w,128], the kernel gradients before the BN factor `Wg1` [261,128], `Wg2`
        [3,3,128,128], `Wg3` [128,257] and the column sums `S1`, `S2` [128], `S3` [257] of gz1, gz2, d_y3, the last six float64."""
        lib = _lib.load()
        self.scratch3(b, h, w)
        return read_maps(self.view, lambda index: int(lib.bsr_bottleneck_grad_offset(b, h, w, index)), b, h, w)

    def bottleneck_grad(self, xin: torch.Tensor, d_y3: torch.Tensor, d_skip: Optional[torch.Tensor] = None, keep: bool = False):
        """xin [B,h,w,261] the block's input, d_y3 [B,h,w,257] the gradient at bnorm3's output, d_skip [B,h,w,261] what the skip carries
        (None: nothing) -> dict(`d_xin` [B,h,w,261] and the twelve variable gradients by name, views of one flat tensor which is under "";
        with `keep` also the stage maps `gz2`, `gz1`, `a1`, `a2`), float32 on the device, asynchronously on the current stream.  Everything
        is checked here, before any launch: TypeError / ValueError."""
        return self._grad(dict(xin=xin, d_y3=d_y3, d_skip=d_skip), keep)

    def backward(self, generator, d_y3: torch.Tensor, d_skip: Optional[torch.Tensor] = None, keep: bool = False):
        """bottleneck_grad with xin read in place from `generator`'s workspace (Generator.last_block5_input: the last forward's, no copy),
        for a d_y3 [B,H/8,W/8,257] of that forward's shape (NonLocalGrad's `d_y3` and `d_skip`).  The generator must be an fp32 GSC one on
        this device whose last forward ran on the current stream."""
        return self._backward(generator, dict(d_y3=d_y3, d_skip=d_skip), keep)

    def stages(self, xin, d_y3, d_skip, n):
        """The chain stopped after `n` of its launches (`LAUNCHES`) -> `maps`, `d_xin` and the flat gradient buffer under ""."""
        return super().stages(xin, d_y3, d_skip, n)
