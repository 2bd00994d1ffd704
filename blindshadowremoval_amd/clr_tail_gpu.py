"""The device binding of the generator's colour tail backward: bsr_clr_tail_grad (csrc/clr_tail_grad_kernels.h), held to
generator_grad.py's host statement (tail_grad).  A post_gpu.GradStage: here are the stage's declaration, its public calls and what the
chain leaves in the scratch."""
from __future__ import annotations

from typing import Dict, Optional

import torch

from . import _lib
from .pack import pack_clr_tail_grad
from .post_gpu import DENSE, OPTIONAL, STRIDED, GradStage
from .weights import generator_tail_trainable_names

# the chain's launches in order and what each writes
LAUNCHES = (("conv_n16", "a1"), ("pixel", "gz1, a2, the 1x1 partial sums"), ("wgrad", "clr_conv1 kernel partials"), ("dgrad", "d_f, d_gs"),
            ("fold", "clr_conv1 kernel, W1, S"), ("finish", "bias, gamma, beta, clr_conv2 and clr_conv3 kernels"))
MAPS = ("a1", "a2", "gz1")          # the kept maps [B,H,W,16], bsr_clr_tail_grad_offset's 0..2
SIZE_TEXT = "the colour tail takes B >= 1 images with H a multiple of 8 and W a multiple of 32, got B=%d H=%d W=%d"
NO_WEIGHTS_TEXT = "the colour tail has no weights: call load_weights or restore first"


class ColourTail(GradStage):
    """`ColourTail(device).tail_grad(gs, f, g_con, g_gs)` — the gradients of the generator's colour tail (clr_conv1, clr_conv2,
    clr_conv3; training=False) on `device`, after `load_weights(dict)` (the generator's variables) or `restore(ckpt_dir)`:
    d / d f at clr_up3's output, the complete d / d gs, and the ten variable gradients of weights.generator_tail_trainable_names().
    `backward(generator, gs, g_con, g_gs)` reads f in place from the generator's workspace."""
    SYMBOL = "bsr_clr_tail_grad"
    PACK, NAMES = staticmethod(pack_clr_tail_grad), staticmethod(generator_tail_trainable_names)
    INPUTS = (("gs", 1, 1, DENSE), ("f", 64, 1, STRIDED), ("g_con", 3, 1, DENSE), ("g_gs", 1, 1, OPTIONAL))
    LEAD = "gs"
    OUTPUTS = (("d_f", 64, 1), ("d_gs", 1, 1))
    TAKES_KEEP = True
    KEPT = ("a1", "a2")
    MULTIPLES = (8, 32)
    LIKE_TEXT, SIZE_TEXT, NO_WEIGHTS_TEXT, WHAT = "like gs", SIZE_TEXT, NO_WEIGHTS_TEXT, "the colour tail"
    LAUNCHES = LAUNCHES
    LAST = "last_f"

    def maps(self, b: int, h: int, w: int, keep: bool = True) -> Dict[str, torch.Tensor]:
        """Copies of what the last call of these sizes left in the scratch: `a1`, `gz1` (and `a2` when that call kept it) [B,H,W,16],
        `W1` float64 [3,3,65,16] (the kernel gradient before the BN factor) and `S` float64 [339] (the 1x1 layers' sums: a1 (x) gz2
        [16,16], a2 (x) G [16,3], sum G [3], sum gz1 [16], sum gz2 [16])."""
        lib = _lib.load()
        self.scratch3(b, h, w)
        out = {name: self.view(int(lib.bsr_clr_tail_grad_offset(b, h, w, i)), (b, h, w, 16)).clone()
               for i, name in enumerate(MAPS) if keep or name != "a2"}
        out["W1"] = self.view(int(lib.bsr_clr_tail_grad_offset(b, h, w, 5)), (3, 3, 65, 16), torch.float64).clone()
        out["S"] = self.view(int(lib.bsr_clr_tail_grad_offset(b, h, w, 6)), (339,), torch.float64).clone()
        return out

    def tail_grad(self, gs: torch.Tensor, f: torch.Tensor, g_con: torch.Tensor, g_gs: Optional[torch.Tensor] = None, keep: bool = False):
        """gs [B,H,W,1], f [B,H,W,64], g_con [B,H,W,3], g_gs [B,H,W,1] or None -> dict(`d_f` [B,H,W,64], `d_gs` [B,H,W,1], and the ten
        variable gradients by name, views of one flat tensor which is under ""; with `keep` also copies of the activations `a1`, `a2`),
        float32 on the device, asynchronously on the current stream.  Everything is checked here, before any launch: TypeError /
        ValueError."""
        return self._grad(dict(gs=gs, f=f, g_con=g_con, g_gs=g_gs), keep)

    def backward(self, generator, gs: torch.Tensor, g_con: torch.Tensor, g_gs: Optional[torch.Tensor] = None, keep: bool = False):
        """tail_grad with f read in place from `generator`'s workspace (Generator.last_f: the last forward's f, no copy), for a gs of
        that forward's shape.  The generator must be an fp32 one on this device whose last forward ran on the current stream."""
        return self._backward(generator, dict(gs=gs, g_con=g_con, g_gs=g_gs), keep)
