"""The device binding of a chain of residual blocks' backward (csrc/block_chain_grad.h): what colour_trunk_gpu.ColourTrunk and
lower_trunk_gpu.LowerTrunk share."""
from __future__ import annotations

from typing import Dict

import torch

from . import _lib, bottleneck_grad_gpu, nonlocal_grad_gpu
from .pack import BLOCK_WIDTHS
from .post_gpu import GradStage

N_NL_MAPS, N_BN_MAPS = 10, 8   # bsr_nonlocal_grad_offset's and bsr_bottleneck_grad_offset's maps: a block's take 18 of the stage's
C_Y = 257


class BlockChainStage(GradStage):
    """A GradStage over BLOCKS, in the chain's order.  A subclass gets `LAUNCHES`, the two existing chains per block with their names
    prefixed and then TAIL; `DATA`, name -> (bsr_<stage>_grad_offset's map, channels) of `d_y3_<b>`, `d_skip_<b>`, `d_xin<b>` behind the
    blocks' maps (the last block's d_xin is a map only when a tail reads it: otherwise it is the stage's output); and `KEPT`."""
    BLOCKS = ()
    TAIL = None                # (name, what it writes) of the launch after the last block, or None

    def __init_subclass__(cls, **kw):
        super().__init_subclass__(**kw)
        cls.LAUNCHES = tuple(("%s%d.%s" % (tag, b, name), "block %d: %s" % (b, what)) for b in cls.BLOCKS
                             for tag, chain in (("nl", nonlocal_grad_gpu.LAUNCHES), ("bn", bottleneck_grad_gpu.LAUNCHES))
                             for name, what in chain) + ((cls.TAIL,) if cls.TAIL else ())
        names = [(n % b, c) for b in cls.BLOCKS for n, c in (("d_y3_%d", C_Y), ("d_skip_%d", BLOCK_WIDTHS[b]), ("d_xin%d", BLOCK_WIDTHS[b]))]
        first = len(cls.BLOCKS) * (N_NL_MAPS + N_BN_MAPS)
        cls.DATA = {name: (first + i, c) for i, (name, c) in enumerate(names if cls.TAIL else names[:-1])}
        cls.KEPT = tuple("a%d_%d" % (j, b) for b in cls.BLOCKS for j in (1, 2)) + tuple(cls.DATA)

    def maps(self, b: int, h: int, w: int) -> Dict[str, torch.Tensor]:
        """Copies of what the last call of these sizes left in the scratch: per block NonLocalGrad.maps' under `nl<b>.<name>` and
        BottleneckGrad.maps' under `bn<b>.<name>` at the block's input width, the bottlenecks' `a1_<b>`, `a2_<b>` again under the names
        the host statement gives them, and the intermediate data gradients of `DATA`."""
        offset = getattr(_lib.load(), self.SYMBOL + "_offset")
        self.scratch3(b, h, w)
        out = {}
        for k, block in enumerate(self.BLOCKS):
            first = k * (N_NL_MAPS + N_BN_MAPS)
            nl = nonlocal_grad_gpu.read_maps(self.view, lambda i: int(offset(b, h, w, first + i)), b, h * w)
            bn = bottleneck_grad_gpu.read_maps(self.view, lambda i: int(offset(b, h, w, first + N_NL_MAPS + i)), b, h, w, BLOCK_WIDTHS[block])
            out.update(("nl%d.%s" % (block, name), t) for name, t in nl.items())
            out.update(("bn%d.%s" % (block, name), t) for name, t in bn.items())
            out["a1_%d" % block], out["a2_%d" % block] = bn["a1"], bn["a2"]
        for name, (index, c) in self.DATA.items():
            out[name] = self.view(int(offset(b, h, w, index)), (b, h, w, c)).clone()
        return out
