"""The device binding of the backward of res_stack/5's upper half — relu3, the skip and the non-local block: bsr_nonlocal_grad
(csrc/nonlocal_grad_kernels.h), held to generator_grad.py's host statement (nonlocal_grad).  A post_gpu.GradStage like
clr_decoder_gpu.ColourDecoder: here are the stage's declaration, its public calls and what the chain leaves in the scratch."""
from __future__ import annotations

from typing import Dict

import torch

from . import _lib
from .pack import pack_nonlocal_grad
from .post_gpu import DENSE, STRIDED, GradStage
from .weights import generator_nonlocal_trainable_names

# the chain's launches in order and what each writes
LAUNCHES = (("entry", "d_skip, dz, y3, Sz partials"), ("project", "theta | phi | g"), ("stats", "L = (m, r), A"), ("dA", "dA, D"),
            ("key", "d_phi, d_g"), ("query", "d_theta"), ("wgrad_qkv", "X^T [d_theta | d_phi | d_g] partials"),
            ("wgrad_w", "A^T dz partials"), ("colsum", "bias partials"), ("dgrad", "d_y3"), ("fold", "the four kernels, Wgd"),
            ("finish", "the biases, gamma, beta, Sz"))
# name, columns (0: a vector per token), first column, columns kept (1: that column as a vector): bsr_nonlocal_grad_offset's 0..7
MAPS = (("y3", 272, 0, 257), ("dz", 272, 0, 257), ("theta", 384, 0, 128), ("phi", 384, 128, 128), ("g", 384, 256, 128), ("A", 128, 0, 128),
        ("m", 2, 0, 1), ("r", 2, 1, 1), ("dA", 128, 0, 128), ("D", 0, 0, 0), ("d_theta", 384, 0, 128), ("d_phi", 384, 128, 128), ("d_g", 384, 256, 128))
MAP_INDEX = {"y3": 0, "dz": 1, "theta": 2, "phi": 2, "g": 2, "A": 3, "m": 4, "r": 4, "dA": 5, "D": 6, "d_theta": 7, "d_phi": 7, "d_g": 7}
KEPT = ("gz", "dA", "D", "d_theta", "d_phi", "d_g", "A")
C_IN, C_NL = 261, 257
SIZE_TEXT = "the non-local block takes B >= 1 grids with h a multiple of 4 and w a multiple of 32, got B=%d h=%d w=%d"
NO_WEIGHTS_TEXT = "the non-local block has no weights: call load_weights or restore first"


def read_maps(view, offset, b: int, t: int) -> Dict[str, torch.Tensor]:
    """Copies of the chain's maps out of a scratch: `view`(byte offset, shape[, dtype]) gives a tensor over it, `offset`(index) the byte
    offset of bsr_nonlocal_grad_offset's map `index` (colour_trunk_gpu reads each block's region with its own)."""
    out = {}
    for name, cols, first, kept in MAPS:
        off = offset(MAP_INDEX[name])
        if cols == 0:
            out[name] = view(off, (b, t)).clone()
        elif kept == 1:
            out[name] = view(off, (b, t, cols))[..., first].clone()
        else:
            out[name] = view(off, (b, t, cols))[..., first:first + kept].clone()
    out["Wgd"] = view(offset(8), (128, C_NL), torch.float64).clone()
    out["Sz"] = view(offset(9), (C_NL,), torch.float64).clone()
    return out


class NonLocalGrad(GradStage):
    """`NonLocalGrad(device).nonlocal_grad(y3x, xin, out, d_out)` — the gradients of the upper half of the generator's res_stack/5
    (training=False; GSC width) on `device`, after `load_weights(dict)` (the generator's variables; ValueError for TSM weights) or
    `restore(ckpt_dir)`: `d_y3` at bnorm3's output, `d_skip` at the block's input and the ten variable gradients of
    weights.generator_nonlocal_trainable_names().  `backward(generator, d_x)` reads y3x, xin, out in place from the generator's workspace."""
    SYMBOL = "bsr_nonlocal_grad"
    PACK, NAMES = staticmethod(pack_nonlocal_grad), staticmethod(generator_nonlocal_trainable_names)
    INPUTS = (("y3x", C_NL, 1, STRIDED), ("xin", C_IN, 1, STRIDED), ("out", C_IN, 1, STRIDED), ("d_out", C_IN, 1, DENSE))
    LEAD = "d_out"
    OUTPUTS = (("d_y3", C_NL, 1), ("d_skip", C_IN, 1))
    KEPT = KEPT[1:]            # gz is d_skip itself
    MULTIPLES = (4, 32)
    DIMS = IMAGE_DIMS = "h,w"
    LIKE_TEXT, SIZE_TEXT, NO_WEIGHTS_TEXT, WHAT = "for this d_out", SIZE_TEXT, NO_WEIGHTS_TEXT, "the non-local block"
    LAUNCHES = LAUNCHES
    LAST = "last_block5"

    def maps(self, b: int, h: int, w: int) -> Dict[str, torch.Tensor]:
        """Copies of what the last call of these sizes left in the scratch, T = h w: `y3`, `dz` [B,T,257], `theta`, `phi`, `g`, `A`, `dA`,
        `d_theta`, `d_phi`, `d_g` [B,T,128], `m`, `r` (the softmax rows' maximum and 1 / sum exp(S - m)), `D` [B,T], `Wgd` float64
        [128,257] (w's kernel gradient before the BN factor) and `Sz` float64 [257]."""
        lib = _lib.load()
        self.scratch3(b, h, w)
        return read_maps(self.view, lambda index: int(lib.bsr_nonlocal_grad_offset(b, h, w, index)), b, h * w)

    def _result(self, outs, b, h, w, keep):
        out = super()._result(outs, b, h, w, keep)
        if keep:
            out["gz"] = out["d_skip"]
        return out

    def nonlocal_grad(self, y3x: torch.Tensor, xin: torch.Tensor, out: torch.Tensor, d_out: torch.Tensor, keep: bool = False):
        """y3x [B,h,w,257] = bnorm3's output + the first 257 channels of xin, xin [B,h,w,261] the block's input, out [B,h,w,261] its
        output, d_out [B,h,w,261] -> dict(`d_y3` [B,h,w,257], `d_skip` [B,h,w,261] and the ten variable gradients by name, views of one
        flat tensor which is under ""; with `keep` also the stage maps `gz` (= d_skip), `dA`, `D`, `d_theta`, `d_phi`, `d_g`, `A`), float32
        on the device, asynchronously on the current stream.  Everything is checked here, before any launch: TypeError / ValueError."""
        return self._grad(dict(y3x=y3x, xin=xin, out=out, d_out=d_out), keep)

    def backward(self, generator, d_x: torch.Tensor, keep: bool = False):
        """nonlocal_grad with y3x, xin, out read in place from `generator`'s workspace (Generator.last_block5: the last forward's, no
        copies), for a d_x [B,H/8,W/8,261] of that forward's shape (ColourDecoder's `d_x`).  The generator must be an fp32 GSC one on this
        device whose last forward ran on the current stream."""
        return self._backward(generator, dict(d_out=d_x), keep, lead="d_x")
