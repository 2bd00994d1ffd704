"""The device binding of the backward of the generator's grey heads — conv2 (7x7, 64 -> 1, tanh: mask), conv3 (7x7, 64 -> 1: con) and
gs = gray(inputs) (1 + mask) + con: bsr_heads_grad (csrc/heads_grad_kernels.h), held to generator_grad.py's host statement (heads_grad).
A post_gpu.GradStage like clr_tail_gpu.ColourTail: here are the stage's declaration, its public calls and what the chain leaves in the
scratch."""
from __future__ import annotations

from typing import Dict

import torch

from . import _lib
from .pack import pack_heads_grad
from .post_gpu import DENSE, STRIDED, GradStage
from .weights import generator_heads_trainable_names

# the chain's launches in order and what each writes
LAUNCHES = (("entry", "g2 = (g_m, g_con), mask, the column sums' partials"), ("dgrad", "d_y"), ("wgrad", "the kernel gradients' partials"),
            ("fold", "the two kernels, Wg"), ("finish", "the two biases, S"))
KEPT = ("g_m", "mask")
SIZE_TEXT = "the heads take B >= 1 images with H a multiple of 8 and W a multiple of 32, got B=%d H=%d W=%d"
NO_WEIGHTS_TEXT = "the heads have no weights: call load_weights or restore first"


class HeadsGrad(GradStage):
    """`HeadsGrad(device).heads_grad(inputs, mask22, y, d_gs)` — the gradients of the generator's grey heads (conv2, conv3;
    training=False) on `device`, after `load_weights(dict)` (the generator's variables, GSC or TSM; ValueError for RGB weights) or
    `restore(ckpt_dir)`: `d_y` at up3's output and the four variable gradients of weights.generator_heads_trainable_names().  `d_gs` is
    the complete gradient at gs (ColourTail's `d_gs`); `inputs` and `mask22` are the forward's input and output.
    `backward(generator, inputs, mask22, d_gs)` reads y in place from the generator's workspace."""
    SYMBOL = "bsr_heads_grad"
    PACK, NAMES = staticmethod(pack_heads_grad), staticmethod(generator_heads_trainable_names)
    INPUTS = (("inputs", 3, 1, DENSE), ("mask22", 3, 1, DENSE), ("y", 64, 1, STRIDED), ("d_gs", 1, 1, DENSE))
    LEAD = "d_gs"
    OUTPUTS = (("d_y", 64, 1),)
    KEPT = KEPT
    MULTIPLES = (8, 32)
    LIKE_TEXT, SIZE_TEXT, NO_WEIGHTS_TEXT, WHAT = "like d_gs", SIZE_TEXT, NO_WEIGHTS_TEXT, "the heads"
    LAUNCHES = LAUNCHES
    LAST = "last_y"

    def maps(self, b: int, h: int, w: int) -> Dict[str, torch.Tensor]:
        """Copies of what the last call of these sizes left in the scratch: `g_m`, `g_con`, `mask` [B,H,W,1], the kernel gradients `Wg`
        float64 [2,7,7,64] (head 0 the mask head conv2, 1 the con head conv3) and `S` float64 [2], the sums of g_m and g_con."""
        lib = _lib.load()
        self.scratch3(b, h, w)
        g2 = self.view(int(lib.bsr_heads_grad_offset(b, h, w, 0)), (b, h, w, 2))
        return {"g_m": g2[..., 0:1].clone(), "g_con": g2[..., 1:2].clone(),
                "mask": self.view(int(lib.bsr_heads_grad_offset(b, h, w, 1)), (b, h, w, 1)).clone(),
                "Wg": self.view(int(lib.bsr_heads_grad_offset(b, h, w, 2)), (2, 7, 7, 64), torch.float64).clone(),
                "S": self.view(int(lib.bsr_heads_grad_offset(b, h, w, 3)), (2,), torch.float64).clone()}

    def heads_grad(self, inputs: torch.Tensor, mask22: torch.Tensor, y: torch.Tensor, d_gs: torch.Tensor, keep: bool = False):
        """inputs, mask22 [B,H,W,3], y [B,H,W,64], d_gs [B,H,W,1] -> dict(`d_y` [B,H,W,64] and the four variable gradients by name, views
        of one flat tensor which is under ""; with `keep` also the stage maps `g_m`, `mask`), float32 on the device, asynchronously on the
        current stream.  Everything is checked here, before any launch: TypeError / ValueError."""
        return self._grad(dict(inputs=inputs, mask22=mask22, y=y, d_gs=d_gs), keep)

    def backward(self, generator, inputs: torch.Tensor, mask22: torch.Tensor, d_gs: torch.Tensor, keep: bool = False):
        """heads_grad with y read in place from `generator`'s workspace (Generator.last_y: the last forward's, no copy), for a d_gs of that
        forward's shape.  The generator must be an fp32 GSC or TSM one on this device whose last forward ran on the current stream."""
        return self._backward(generator, dict(inputs=inputs, mask22=mask22, d_gs=d_gs), keep)

    def stages(self, inputs, mask22, y, d_gs, n):
        """The chain stopped after `n` of its launches (`LAUNCHES`) -> `maps`, `d_y` and the flat gradient buffer under ""."""
        return super().stages(inputs, mask22, y, d_gs, n)
