"""The device binding of the generator's colour decoder backward: bsr_clr_decoder_grad (csrc/clr_up_grad_kernels.h), held to
generator_grad.py's host statement (decoder_grad).  Built on post_gpu.PostDevice like clr_tail_gpu.ColourTail: the cached scratch sized
by the named query, views into it and the library call on the current stream; here are the checks, the blob, and what the chain leaves
in the scratch."""
from __future__ import annotations

import ctypes
import math
from typing import Dict, Optional

import torch

from . import _lib
from .pack import pack_clr_decoder_grad
from .post_gpu import PostDevice
from .weights import generator_decoder_trainable_names, generator_variable_shapes

# the chain's launches in order and what each writes
LAUNCHES = (("mask", "gz3 (only when maps are kept)"), ("wgrad3", "clr_up3 kernel partials, S partials"), ("dgrad3", "gz2"),
            ("wgrad2", "clr_up2 kernel partials, S partials"), ("dgrad2", "gz1"), ("wgrad1", "clr_up1 kernel partials, S partials"),
            ("dgrad1", "d_x"), ("fold", "the three kernels, Wg, S"), ("finish", "bias, gamma, beta of the three layers"))
MAPS = (("gz1", 4, 128), ("gz2", 2, 96), ("gz3", 1, 64))       # name, the image's size over the map's, channels: bsr_clr_decoder_grad_offset's 0..2
LAYER_SHAPES = ((128, 261), (96, 128), (64, 96))               # (O, C) of clr_up1..3
SIZE_TEXT = "the colour decoder takes B >= 1 images with H a multiple of 32 and W a multiple of 256, got B=%d H=%d W=%d"
NO_WEIGHTS_TEXT = "the colour decoder has no weights: call load_weights or restore first"


class ColourDecoder(PostDevice):
    """`ColourDecoder(device).decoder_grad(x, f1, f2, f, d_f)` — the gradients of the generator's colour decoder (clr_up1, clr_up2,
    clr_up3; training=False; GSC width) on `device`, after `load_weights(dict)` (the generator's variables) or `restore(ckpt_dir)`:
    d / d x at res_stack/5's output and the twelve variable gradients of weights.generator_decoder_trainable_names().
    `backward(generator, d_f)` reads x, f1, f2, f in place from the generator's workspace."""
    SYMBOL = "bsr_clr_decoder_grad"

    def __init__(self, device: int):
        super().__init__(device)
        self._blob: Optional[torch.Tensor] = None

    def load_weights(self, weights) -> None:
        """The generator's variables (the colour decoder's 18 are read) -> the chain's blob on the device.  ValueError for TSM weights."""
        blob = pack_clr_decoder_grad(weights)
        assert len(blob) == int(_lib.load().bsr_clr_decoder_grad_blob_bytes())
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
            raise TypeError("%s must be a float32 tensor [B,.,.,%d] on %s" % (name, c, self._dev))
        if not t.is_contiguous():
            raise ValueError("%s must be contiguous (NHWC, dense)" % name)
        if shape is not None and tuple(t.shape) != shape + (c,):
            raise ValueError("%s must be [%d,%d,%d,%d] for this d_f, got %s" % ((name,) + shape + (c, tuple(t.shape))))

    def _check(self, d_f, acts=None):
        """d_f first (it gives the sizes), then x, f1, f2, f in that order, then the sizes and the weights -> (b, h, w), the image's."""
        self._image("d_f", d_f, 64)
        b, h, w = (int(d) for d in d_f.shape[:3])
        if int(d_f.shape[3]) != 64:
            raise ValueError("d_f must be [B,H,W,64], got %s" % (tuple(d_f.shape),))
        if acts is not None:
            for (name, c, div), t in zip((("x", 261, 8), ("f1", 128, 4), ("f2", 96, 2), ("f", 64, 1)), acts):
                self._image(name, t, c, (b, h // div, w // div))
        if b < 1 or h < 1 or w < 1 or h % 32 or w % 256:
            raise ValueError(SIZE_TEXT % (b, h, w))
        if self._blob is None:
            raise ValueError(NO_WEIGHTS_TEXT)
        return b, h, w

    def scratch4(self, b: int, h: int, w: int, keep: bool) -> int:
        """The 256-byte aligned device address of at least bsr_clr_decoder_grad_scratch_bytes(b, h, w, keep) bytes of scratch."""
        need = int(_lib.load().bsr_clr_decoder_grad_scratch_bytes(b, h, w, 1 if keep else 0))
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
    def _run(self, ptrs, strides, d_f, b: int, h: int, w: int, keep: bool, stop_after: Optional[int] = None):
        """ptrs, strides: the device addresses and floats between pixels of x, f1, f2, f -> (d_x, the flat gradient buffer)."""
        lib = _lib.load()
        d_x = self.empty((b, h // 8, w // 8, 261), torch.float32)
        flat = self.empty((int(lib.bsr_clr_decoder_grad_floats()),), torch.float32)
        if stop_after is not None:
            d_x.zero_()
            flat.zero_()                       # a stopped chain leaves what it did not write at 0
        args = [self._blob, ctypes.c_size_t(self._blob.numel())]
        for ptr, cs in zip(ptrs, strides):
            args += [ctypes.c_void_p(ptr), int(cs)]
        args += [d_f, b, h, w, d_x, flat, 1 if keep else 0, ctypes.c_void_p(self.scratch4(b, h, w, keep))]
        symbol = self.SYMBOL
        if stop_after is not None:
            args.append(int(stop_after))
            symbol = "bsr_debug_clr_decoder_grad"
        self.call(*args, symbol=symbol)
        return d_x, flat

    @staticmethod
    def split_grads(flat: torch.Tensor) -> Dict[str, torch.Tensor]:
        """The flat buffer of bsr_clr_decoder_grad -> name -> a view of it in the variable's shape, for
        weights.generator_decoder_trainable_names(); the flat tensor itself under the key ""."""
        lib = _lib.load()
        shapes = generator_variable_shapes()
        out = {"": flat}
        for index, name in enumerate(generator_decoder_trainable_names()):
            off = int(lib.bsr_clr_decoder_grad_var_offset(index))
            out[name] = flat[off:off + math.prod(shapes[name])].reshape(shapes[name])
        return out

    def maps(self, b: int, h: int, w: int, keep: bool = True) -> Dict[str, torch.Tensor]:
        """Copies of what the last call of these sizes left in the scratch: `gz1` [B,H/4,W/4,128], `gz2` [B,H/2,W/2,96] (and `gz3`
        [B,H,W,64] when that call kept it), `Wg1..3` float64 [3,3,O,C] (the kernel gradients before the BN factor) and `S1..3` float64
        [O] (the sums of gz)."""
        lib = _lib.load()
        self.scratch4(b, h, w, keep)
        out = {name: self.view(int(lib.bsr_clr_decoder_grad_offset(b, h, w, i)), (b, h // div, w // div, c)).clone()
               for i, (name, div, c) in enumerate(MAPS) if keep or name != "gz3"}
        for i, (o, c) in enumerate(LAYER_SHAPES):
            out["Wg%d" % (i + 1)] = self.view64(int(lib.bsr_clr_decoder_grad_offset(b, h, w, 3 + i)), (3, 3, o, c)).clone()
            out["S%d" % (i + 1)] = self.view64(int(lib.bsr_clr_decoder_grad_offset(b, h, w, 6 + i)), (o,)).clone()
        return out

    def _result(self, d_x, flat, b, h, w, keep):
        out = self.split_grads(flat)
        out["d_x"] = d_x
        if keep:
            kept = self.maps(b, h, w)
            for name, _, _ in MAPS:
                out[name] = kept[name]
        return out

    def decoder_grad(self, x: torch.Tensor, f1: torch.Tensor, f2: torch.Tensor, f: torch.Tensor, d_f: torch.Tensor, keep: bool = False):
        """x [B,H/8,W/8,261], f1 [B,H/4,W/4,128], f2 [B,H/2,W/2,96], f [B,H,W,64], d_f [B,H,W,64] -> dict(`d_x` [B,H/8,W/8,261] and the
        twelve variable gradients by name, views of one flat tensor which is under ""; with `keep` also copies of the stage maps `gz1`,
        `gz2`, `gz3`), float32 on the device, asynchronously on the current stream.  Everything is checked here, before any launch:
        TypeError / ValueError."""
        b, h, w = self._check(d_f, (x, f1, f2, f))
        return self._result(*self._run([t.data_ptr() for t in (x, f1, f2, f)], (261, 128, 96, 64), d_f, b, h, w, keep), b, h, w, keep)

    def backward(self, generator, d_f: torch.Tensor, keep: bool = False):
        """decoder_grad with x, f1, f2, f read in place from `generator`'s workspace (Generator.last_decoder: the last forward's, no
        copies), for a d_f of that forward's shape.  The generator must be an fp32 GSC one on this device whose last forward ran on the
        current stream."""
        b, h, w = self._check(d_f)
        ptrs, x_cs, shape = generator.last_decoder()
        if generator._device != self.device:
            raise ValueError("the generator lives on cuda:%s, the colour decoder on %s" % (generator._device, self._dev))
        if tuple(shape[:3]) != (b, h, w):
            raise ValueError("the generator's last forward was %s, d_f is %s" % (tuple(shape[:3]), (b, h, w)))
        return self._result(*self._run(ptrs, (x_cs, 128, 96, 64), d_f, b, h, w, keep), b, h, w, keep)

    def stages(self, x, f1, f2, f, d_f, n: int) -> Dict[str, torch.Tensor]:
        """For the stage-by-stage tests: the chain stopped after `n` (0..9) of its launches (LAUNCHES), maps kept -> `maps`, plus `d_x`
        and the flat gradient buffer under "", zero where no launch wrote; the maps of launches that did not run hold whatever the
        scratch held."""
        b, h, w = self._check(d_f, (x, f1, f2, f))
        if not 0 <= int(n) <= len(LAUNCHES):
            raise ValueError("stop_after must be 0..%d" % len(LAUNCHES))
        d_x, flat = self._run([t.data_ptr() for t in (x, f1, f2, f)], (261, 128, 96, 64), d_f, b, h, w, True, stop_after=int(n))
        out = self.maps(b, h, w)
        out.update({"d_x": d_x, "": flat})
        return out
