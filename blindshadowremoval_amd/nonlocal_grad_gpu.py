"""The device binding of the backward of res_stack/5's upper half — relu3, the skip and the non-local block: bsr_nonlocal_grad
(csrc/nonlocal_grad_kernels.h), held to generator_grad.py's host statement (nonlocal_grad).  Built on post_gpu.PostDevice like
clr_decoder_gpu.ColourDecoder: the cached scratch sized by the named query, views into it and the library call on the current stream;
here are the checks, the blob, and what the chain leaves in the scratch."""
from __future__ import annotations

import ctypes
import math
from typing import Dict, Optional

import torch

from . import _lib
from .pack import pack_nonlocal_grad
from .post_gpu import PostDevice
from .weights import generator_nonlocal_trainable_names, generator_variable_shapes

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


class NonLocalGrad(PostDevice):
    """`NonLocalGrad(device).nonlocal_grad(y3x, xin, out, d_out)` — the gradients of the upper half of the generator's res_stack/5
    (training=False; GSC width) on `device`, after `load_weights(dict)` (the generator's variables) or `restore(ckpt_dir)`: `d_y3` at
    bnorm3's output, `d_skip` at the block's input and the ten variable gradients of weights.generator_nonlocal_trainable_names().
    `backward(generator, d_x)` reads y3x, xin, out in place from the generator's workspace."""
    SYMBOL = "bsr_nonlocal_grad"

    def __init__(self, device: int):
        super().__init__(device)
        self._blob: Optional[torch.Tensor] = None

    def load_weights(self, weights) -> None:
        """The generator's variables (res_stack/5/non_local's 12 are read) -> the chain's blob on the device.  ValueError for TSM weights."""
        blob = pack_nonlocal_grad(weights)
        assert len(blob) == int(_lib.load().bsr_nonlocal_grad_blob_bytes())
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
            raise TypeError("%s must be a float32 tensor [B,h,w,%d] on %s" % (name, c, self._dev))
        if not t.is_contiguous():
            raise ValueError("%s must be contiguous (NHWC, dense)" % name)
        if shape is not None and tuple(t.shape) != shape + (c,):
            raise ValueError("%s must be [%d,%d,%d,%d] for this d_out, got %s" % ((name,) + shape + (c, tuple(t.shape))))

    def _check(self, d_out, acts=None):
        """d_out first (it gives the sizes), then y3x, xin, out in that order, then the sizes and the weights -> (b, h, w), the grid's."""
        self._image("d_out", d_out, C_IN)
        b, h, w = (int(d) for d in d_out.shape[:3])
        if int(d_out.shape[3]) != C_IN:
            raise ValueError("d_out must be [B,h,w,%d], got %s" % (C_IN, tuple(d_out.shape)))
        if acts is not None:
            for (name, c), t in zip((("y3x", C_NL), ("xin", C_IN), ("out", C_IN)), acts):
                self._image(name, t, c, (b, h, w))
        if b < 1 or h < 1 or w < 1 or h % 4 or w % 32:
            raise ValueError(SIZE_TEXT % (b, h, w))
        if self._blob is None:
            raise ValueError(NO_WEIGHTS_TEXT)
        return b, h, w

    def scratch3(self, b: int, h: int, w: int) -> int:
        """The 256-byte aligned device address of at least bsr_nonlocal_grad_scratch_bytes(b, h, w) bytes of scratch."""
        need = int(_lib.load().bsr_nonlocal_grad_scratch_bytes(b, h, w))
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
    def _run(self, ptrs, strides, d_out, b: int, h: int, w: int, stop_after: Optional[int] = None):
        """ptrs, strides: the device addresses and floats between pixels of y3x, xin, out -> (d_y3, d_skip, the flat gradient buffer)."""
        lib = _lib.load()
        d_y3 = self.empty((b, h, w, C_NL), torch.float32)
        d_skip = self.empty((b, h, w, C_IN), torch.float32)
        flat = self.empty((int(lib.bsr_nonlocal_grad_floats()),), torch.float32)
        if stop_after is not None:
            for t in (d_y3, d_skip, flat):
                t.zero_()                      # a stopped chain leaves what it did not write at 0
        args = [self._blob, ctypes.c_size_t(self._blob.numel())]
        for ptr, cs in zip(ptrs, strides):
            args += [ctypes.c_void_p(ptr), int(cs)]
        args += [d_out, b, h, w, d_y3, d_skip, flat, ctypes.c_void_p(self.scratch3(b, h, w))]
        symbol = self.SYMBOL
        if stop_after is not None:
            args.append(int(stop_after))
            symbol = "bsr_debug_nonlocal_grad"
        self.call(*args, symbol=symbol)
        return d_y3, d_skip, flat

    @staticmethod
    def split_grads(flat: torch.Tensor) -> Dict[str, torch.Tensor]:
        """The flat buffer of bsr_nonlocal_grad -> name -> a view of it in the variable's shape, for
        weights.generator_nonlocal_trainable_names(); the flat tensor itself under the key ""."""
        lib = _lib.load()
        shapes = generator_variable_shapes()
        out = {"": flat}
        for index, name in enumerate(generator_nonlocal_trainable_names()):
            off = int(lib.bsr_nonlocal_grad_var_offset(index))
            out[name] = flat[off:off + math.prod(shapes[name])].reshape(shapes[name])
        return out

    def maps(self, b: int, h: int, w: int) -> Dict[str, torch.Tensor]:
        """Copies of what the last call of these sizes left in the scratch, T = h w: `y3`, `dz` [B,T,257], `theta`, `phi`, `g`, `A`, `dA`,
        `d_theta`, `d_phi`, `d_g` [B,T,128], `m`, `r` (the softmax rows' maximum and 1 / sum exp(S - m)), `D` [B,T], `Wgd` float64 [128,257] (w's kernel gradient before the BN factor) and `Sz`
        float64 [257]."""
        lib = _lib.load()
        self.scratch3(b, h, w)
        t = h * w
        out = {}
        for name, cols, first, kept in MAPS:
            off = int(lib.bsr_nonlocal_grad_offset(b, h, w, MAP_INDEX[name]))
            if cols == 0:
                out[name] = self.view(off, (b, t)).clone()
            elif kept == 1:
                out[name] = self.view(off, (b, t, cols))[..., first].clone()
            else:
                out[name] = self.view(off, (b, t, cols))[..., first:first + kept].clone()
        out["Wgd"] = self.view64(int(lib.bsr_nonlocal_grad_offset(b, h, w, 8)), (128, C_NL)).clone()
        out["Sz"] = self.view64(int(lib.bsr_nonlocal_grad_offset(b, h, w, 9)), (C_NL,)).clone()
        return out

    def _result(self, d_y3, d_skip, flat, b, h, w, keep):
        out = self.split_grads(flat)
        out["d_y3"], out["d_skip"] = d_y3, d_skip
        if keep:
            kept = self.maps(b, h, w)
            out["gz"] = d_skip
            for name in KEPT[1:]:
                out[name] = kept[name]
        return out

    def nonlocal_grad(self, y3x: torch.Tensor, xin: torch.Tensor, out: torch.Tensor, d_out: torch.Tensor, keep: bool = False):
        """y3x [B,h,w,257] = bnorm3's output + the first 257 channels of xin, xin [B,h,w,261] the block's input, out [B,h,w,261] its
        output, d_out [B,h,w,261] -> dict(`d_y3` [B,h,w,257], `d_skip` [B,h,w,261] and the ten variable gradients by name, views of one
        flat tensor which is under ""; with `keep` also the stage maps `gz` (= d_skip), `dA`, `D`, `d_theta`, `d_phi`, `d_g`, `A`), float32
        on the device, asynchronously on the current stream.  Everything is checked here, before any launch: TypeError / ValueError."""
        b, h, w = self._check(d_out, (y3x, xin, out))
        return self._result(*self._run([t.data_ptr() for t in (y3x, xin, out)], (C_NL, C_IN, C_IN), d_out, b, h, w), b, h, w, keep)

    def backward(self, generator, d_x: torch.Tensor, keep: bool = False):
        """nonlocal_grad with y3x, xin, out read in place from `generator`'s workspace (Generator.last_block5: the last forward's, no
        copies), for a d_x [B,H/8,W/8,261] of that forward's shape (ColourDecoder's `d_x`).  The generator must be an fp32 GSC one on this
        device whose last forward ran on the current stream."""
        b, h, w = self._check(d_x)
        ptrs, strides, shape = generator.last_block5()
        if generator._device != self.device:
            raise ValueError("the generator lives on cuda:%s, the non-local block on %s" % (generator._device, self._dev))
        if tuple(shape[:3]) != (b, h, w):
            raise ValueError("the generator's last forward was %s, d_x is %s" % (tuple(shape[:3]), (b, h, w)))
        return self._result(*self._run(ptrs, strides, d_x, b, h, w), b, h, w, keep)

    def stages(self, y3x, xin, out, d_out, n: int) -> Dict[str, torch.Tensor]:
        """For the stage-by-stage tests: the chain stopped after `n` (0..12) of its launches (LAUNCHES) -> `maps`, plus `d_y3`, `d_skip`
        and the flat gradient buffer under "", zero where no launch wrote; the maps of launches that did not run hold whatever the
        scratch held."""
        b, h, w = self._check(d_out, (y3x, xin, out))
        if not 0 <= int(n) <= len(LAUNCHES):
            raise ValueError("stop_after must be 0..%d" % len(LAUNCHES))
        d_y3, d_skip, flat = self._run([t.data_ptr() for t in (y3x, xin, out)], (C_NL, C_IN, C_IN), d_out, b, h, w, stop_after=int(n))
        res = self.maps(b, h, w)
        res.update({"d_y3": d_y3, "d_skip": d_skip, "": flat})
        return res
