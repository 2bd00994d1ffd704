"""The device binding of the generator's colour tail backward: bsr_clr_tail_grad (csrc/clr_tail_grad_kernels.h), held to
generator_grad.py's host statement (tail_grad).  Built on post_gpu.PostDevice: the cached scratch sized by the named query, float32 views
into it and the library call on the current stream; here are the checks, the blob, and what the chain leaves in the scratch."""
from __future__ import annotations

import ctypes
import math
from typing import Dict, Optional

import torch

from . import _lib
from .pack import pack_clr_tail_grad
from .post_gpu import PostDevice
from .weights import generator_tail_trainable_names, generator_variable_shapes

# the chain's launches in order and what each writes
LAUNCHES = (("conv_n16", "a1"), ("pixel", "gz1, a2, the 1x1 partial sums"), ("wgrad", "clr_conv1 kernel partials"), ("dgrad", "d_f, d_gs"),
            ("fold", "clr_conv1 kernel, W1, S"), ("finish", "bias, gamma, beta, clr_conv2 and clr_conv3 kernels"))
MAPS = ("a1", "a2", "gz1")          # the kept maps [B,H,W,16], bsr_clr_tail_grad_offset's 0..2
SIZE_TEXT = "the colour tail takes B >= 1 images with H a multiple of 8 and W a multiple of 32, got B=%d H=%d W=%d"
NO_WEIGHTS_TEXT = "the colour tail has no weights: call load_weights or restore first"


class ColourTail(PostDevice):
    """`ColourTail(device).tail_grad(gs, f, g_con, g_gs)` — the gradients of the generator's colour tail (clr_conv1, clr_conv2,
    clr_conv3; training=False) on `device`, after `load_weights(dict)` (the generator's variables) or `restore(ckpt_dir)`:
    d / d f at clr_up3's output, the complete d / d gs, and the ten variable gradients of weights.generator_tail_trainable_names().
    `backward(generator, gs, g_con, g_gs)` reads f in place from the generator's workspace."""
    SYMBOL = "bsr_clr_tail_grad"

    def __init__(self, device: int):
        super().__init__(device)
        self._blob: Optional[torch.Tensor] = None

    def load_weights(self, weights) -> None:
        """The generator's variables (the colour tail's 16 are read) -> the chain's blob on the device."""
        blob = pack_clr_tail_grad(weights)
        assert len(blob) == int(_lib.load().bsr_clr_tail_grad_blob_bytes())
        self._blob = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(self._dev)

    def restore(self, ckpt_dir: str) -> None:
        """The `generator/*` variables of the latest checkpoint under `ckpt_dir`."""
        from .tf_bundle import latest_checkpoint, load_generator_weights
        prefix = latest_checkpoint(ckpt_dir)
        if prefix is None:
            raise FileNotFoundError("no checkpoint under %s" % ckpt_dir)
        self.load_weights(load_generator_weights(prefix))

    # -- checks, all before any launch ------------------------------------------------------------
    def _image(self, name: str, t, c: int, shape=None):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 4 or t.device != self._dev:
            raise TypeError("%s must be a float32 tensor [B,H,W,%d] on %s" % (name, c, self._dev))
        if not t.is_contiguous():
            raise ValueError("%s must be contiguous (NHWC, dense)" % name)
        if shape is not None and tuple(t.shape) != shape + (c,):
            raise ValueError("%s must be [%d,%d,%d,%d] like gs, got %s" % ((name,) + shape + (c, tuple(t.shape))))

    def _check(self, gs, g_con, g_gs, f=None):
        """The images in their order (gs, f, g_con, g_gs), the sizes, the weights -> (b, h, w)."""
        self._image("gs", gs, 1)
        shape = tuple(int(d) for d in gs.shape[:3])
        if tuple(gs.shape[3:]) != (1,):
            raise ValueError("gs must be [B,H,W,1], got %s" % (tuple(gs.shape),))
        if f is not None:
            self._image("f", f, 64, shape)
        self._image("g_con", g_con, 3, shape)
        if g_gs is not None:
            self._image("g_gs", g_gs, 1, shape)
        b, h, w = shape
        if b < 1 or h < 1 or w < 1 or h % 8 or w % 32:
            raise ValueError(SIZE_TEXT % (b, h, w))
        if self._blob is None:
            raise ValueError(NO_WEIGHTS_TEXT)
        return b, h, w

    def scratch3(self, b: int, h: int, w: int) -> int:
        """The 256-byte aligned device address of at least bsr_clr_tail_grad_scratch_bytes(b, h, w) bytes of scratch."""
        need = int(_lib.load().bsr_clr_tail_grad_scratch_bytes(b, h, w))
        if need == 0:
            raise ValueError(SIZE_TEXT % (b, h, w))
        if self._scratch is None or self._scratch.numel() < need + 256:
            self._scratch = None
            self._scratch = torch.empty(need + 256, dtype=torch.uint8, device=self._dev)
        base = self._scratch.data_ptr()
        return base + (-base) % 256

    def view64(self, offset: int, shape) -> torch.Tensor:
        """The float64 tensor `shape` that starts `offset` bytes past the scratch's aligned address: a view."""
        offset += (-self._scratch.data_ptr()) % 256
        return self._scratch[offset:offset + 8 * math.prod(shape)].view(torch.float64).reshape(shape)

    # -- the call ---------------------------------------------------------------------------------
    def _run(self, gs, f_ptr: int, f_cs: int, g_con, g_gs, b: int, h: int, w: int, keep: bool, stop_after: Optional[int] = None):
        lib = _lib.load()
        d_f = self.empty((b, h, w, 64), torch.float32)
        d_gs = self.empty((b, h, w, 1), torch.float32)
        flat = self.empty((int(lib.bsr_clr_tail_grad_floats()),), torch.float32)
        if stop_after is not None:
            for t in (d_f, d_gs, flat):
                t.zero_()                      # a stopped chain leaves what it did not write at 0
        args = [self._blob, ctypes.c_size_t(self._blob.numel()), gs, ctypes.c_void_p(f_ptr), int(f_cs), g_con, g_gs, b, h, w, d_f, d_gs, flat,
                1 if keep else 0, ctypes.c_void_p(self.scratch3(b, h, w))]
        symbol = self.SYMBOL
        if stop_after is not None:
            args.append(int(stop_after))
            symbol = "bsr_debug_clr_tail_grad"
        self.call(*args, symbol=symbol)
        return d_f, d_gs, flat

    @staticmethod
    def split_grads(flat: torch.Tensor) -> Dict[str, torch.Tensor]:
        """The flat buffer of bsr_clr_tail_grad -> name -> a view of it in the variable's shape, for
        weights.generator_tail_trainable_names(); the flat tensor itself under the key ""."""
        lib = _lib.load()
        shapes = generator_variable_shapes()
        out = {"": flat}
        for index, name in enumerate(generator_tail_trainable_names()):
            off = int(lib.bsr_clr_tail_grad_var_offset(index))
            out[name] = flat[off:off + math.prod(shapes[name])].reshape(shapes[name])
        return out

    def maps(self, b: int, h: int, w: int, keep: bool = True) -> Dict[str, torch.Tensor]:
        """Copies of what the last call of these sizes left in the scratch: `a1`, `gz1` (and `a2` when that call kept it) [B,H,W,16],
        `W1` float64 [3,3,65,16] (the kernel gradient before the BN factor) and `S` float64 [339] (the 1x1 layers' sums: a1 (x) gz2
        [16,16], a2 (x) G [16,3], sum G [3], sum gz1 [16], sum gz2 [16])."""
        lib = _lib.load()
        self.scratch3(b, h, w)
        out = {name: self.view(int(lib.bsr_clr_tail_grad_offset(b, h, w, i)), (b, h, w, 16)).clone()
               for i, name in enumerate(MAPS) if keep or name != "a2"}
        out["W1"] = self.view64(int(lib.bsr_clr_tail_grad_offset(b, h, w, 5)), (3, 3, 65, 16)).clone()
        out["S"] = self.view64(int(lib.bsr_clr_tail_grad_offset(b, h, w, 6)), (339,)).clone()
        return out

    def _result(self, d_f, d_gs, flat, b, h, w, keep):
        out = self.split_grads(flat)
        out["d_f"], out["d_gs"] = d_f, d_gs
        if keep:
            kept = self.maps(b, h, w)
            out["a1"], out["a2"] = kept["a1"], kept["a2"]
        return out

    def tail_grad(self, gs: torch.Tensor, f: torch.Tensor, g_con: torch.Tensor, g_gs: Optional[torch.Tensor] = None, keep: bool = False):
        """gs [B,H,W,1], f [B,H,W,64], g_con [B,H,W,3], g_gs [B,H,W,1] or None -> dict(`d_f` [B,H,W,64], `d_gs` [B,H,W,1], and the ten
        variable gradients by name, views of one flat tensor which is under ""; with `keep` also copies of the activations `a1`, `a2`),
        float32 on the device, asynchronously on the current stream.  Everything is checked here, before any launch: TypeError /
        ValueError."""
        b, h, w = self._check(gs, g_con, g_gs, f)
        return self._result(*self._run(gs, f.data_ptr(), 64, g_con, g_gs, b, h, w, keep), b, h, w, keep)

    def backward(self, generator, gs: torch.Tensor, g_con: torch.Tensor, g_gs: Optional[torch.Tensor] = None, keep: bool = False):
        """tail_grad with f read in place from `generator`'s workspace (Generator.last_f: the last forward's f, no copy), for a gs of
        that forward's shape.  The generator must be an fp32 one on this device whose last forward ran on the current stream."""
        b, h, w = self._check(gs, g_con, g_gs)
        ptr, cs, shape = generator.last_f()
        if generator._device != self.device:
            raise ValueError("the generator lives on cuda:%s, the colour tail on %s" % (generator._device, self._dev))
        if tuple(shape[:3]) != (b, h, w):
            raise ValueError("the generator's last forward was %s, gs is %s" % (tuple(shape[:3]), (b, h, w)))
        return self._result(*self._run(gs, ptr, cs, g_con, g_gs, b, h, w, keep), b, h, w, keep)

    def stages(self, gs, f, g_con, g_gs, n: int) -> Dict[str, torch.Tensor]:
        """For the stage-by-stage tests: the chain stopped after `n` (0..6) of its launches (LAUNCHES), activations kept -> `maps`, plus
        `d_f`, `d_gs` and the flat gradient buffer under "", zero where no launch wrote; the maps of launches that did not run hold
        whatever the scratch held."""
        b, h, w = self._check(gs, g_con, g_gs, f)
        if not 0 <= int(n) <= len(LAUNCHES):
            raise ValueError("stop_after must be 0..%d" % len(LAUNCHES))
        d_f, d_gs, flat = self._run(gs, f.data_ptr(), 64, g_con, g_gs, b, h, w, True, stop_after=int(n))
        out = self.maps(b, h, w)
        out.update({"d_f": d_f, "d_gs": d_gs, "": flat})
        return out
