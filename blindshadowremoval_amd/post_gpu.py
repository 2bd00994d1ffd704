"""What the device bindings of single library entry points share.  `PostDevice`, under the evaluation runners (ucb_post_gpu,
ucb_post_rgb_gpu, ucb_post_tsm_gpu, sfw_post_gpu) and train_step's terms (shadow_synth_gpu, train_losses_gpu): the input checks, a
cached scratch buffer aligned to 256 bytes and sized by a named query, float32 views into it, the library call on the current stream,
and the per-item status check.  `WeightedTerm`, under the two terms that carry weights and a backward chain (discriminator_gpu,
perceptual_gpu): the two blobs, the forward and gradient calls, and the term as a differentiable scalar.  `GradStage`, under the stages
of the generator's backward pass (clr_tail_gpu, clr_decoder_gpu, nonlocal_grad_gpu): the blob, the ordered checks, the entry point's
argument layout from the stage's declaration, and the gradients by variable name."""
from __future__ import annotations

import ctypes
import math
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import _lib

SIZES = (32, 64, 128, 256)        # the sides the post-processing and training entry points take


class PostDevice:
    """Reusable runner of one library entry point `SYMBOL` on one device: keeps its scratch buffer between calls.  A subclass's run()
    checks its inputs (`inputs` or `images`), sizes the scratch (`scratch`), allocates its outputs (`empty`) and calls the library
    (`call`)."""
    SYMBOL = ""
    SCRATCH_QUERY = ""    # the library's size query for (B, S); `SYMBOL`_scratch_bytes when empty
    GRAD_SCRATCH_QUERY = ""        # of a term with a backward chain: the size query of its gradient call
    SIZE_TEXT = ""        # the ValueError text when the query refuses (B, S); %(b)d / %(s)d are filled in
    TYPE_TEXT = "%(name)s must be a %(dtype)s tensor with %(dims)d dims on %(dev)s"

    def __init__(self, device: int):
        self.device = int(device)
        self._dev = torch.device("cuda", self.device)
        self._scratch: Optional[torch.Tensor] = None

    def inputs(self, *spec):
        """spec: (name, tensor, dtype, dims) per input -> the tensors, contiguous.  TypeError unless each is such a tensor on this device."""
        for name, t, dt, nd in spec:
            if not isinstance(t, torch.Tensor) or t.dtype != dt or t.dim() != nd or t.device != self._dev:
                raise TypeError(self.TYPE_TEXT % {"name": name, "dtype": dt, "dims": nd, "dev": self._dev})
        return [t.contiguous() for _, t, _, _ in spec]

    def images(self, spec, cap: int):
        """spec: (name, tensor, channels) per image, one of them named gt -> (b, s) of gt.  TypeError unless each is a float32 tensor of 4
        dims on this device; ValueError unless each is dense, s is one of SIZES, 1 <= b <= `cap` and each is [b,s,s,channels]."""
        for name, t, c in spec:
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 4 or t.device != self._dev:
                raise TypeError("%s must be a float32 tensor [B,S,S,%d] on %s" % (name, c, self._dev))
            if not t.is_contiguous():
                raise ValueError("%s must be contiguous (NHWC, dense)" % name)
        b, s = next((int(t.shape[0]), int(t.shape[1])) for name, t, _ in spec if name == "gt")
        if s not in SIZES or not 1 <= b <= cap:
            raise ValueError(self.SIZE_TEXT % {"b": b, "s": s})
        for name, t, c in spec:
            if tuple(t.shape) != (b, s, s, c):
                raise ValueError("%s must be [%d,%d,%d,%d] like gt, got %s" % (name, b, s, s, c, tuple(t.shape)))
        return b, s

    def scratch(self, b: int, s: int, grad: bool = False) -> int:
        """The 256-byte aligned device address of at least `SCRATCH_QUERY`(b, s) bytes of scratch; with `grad`, of
        `GRAD_SCRATCH_QUERY`(b, s): the same bytes followed by the gradient maps; `grad` may also name a size query of a further chain
        itself.  A buffer that is too small is released before the larger one is allocated."""
        query = grad if isinstance(grad, str) else self.GRAD_SCRATCH_QUERY if grad else self.SCRATCH_QUERY or self.SYMBOL + "_scratch_bytes"
        need = int(getattr(_lib.load(), query)(b, s))
        if need == 0:
            raise ValueError(self.SIZE_TEXT % {"b": b, "s": s})
        return self.reserve(need)

    def reserve(self, need: int) -> int:
        """The 256-byte aligned device address of at least `need` bytes of the cached scratch."""
        if self._scratch is None or self._scratch.numel() < need + 256:
            self._scratch = None
            self._scratch = torch.empty(need + 256, dtype=torch.uint8, device=self._dev)
        base = self._scratch.data_ptr()
        return base + (-base) % 256

    def view(self, offset: int, shape, dtype=torch.float32) -> torch.Tensor:
        """The `dtype` tensor `shape` that starts `offset` bytes past the scratch's aligned address: a view, not a copy."""
        offset += (-self._scratch.data_ptr()) % 256
        return self._scratch[offset:offset + dtype.itemsize * math.prod(shape)].view(dtype).reshape(shape)

    def empty(self, shape, dtype) -> torch.Tensor:
        return torch.empty(shape, dtype=dtype, device=self._dev)

    def call(self, *args, symbol: Optional[str] = None) -> None:
        """`SYMBOL` (or `symbol`)(device, *args, current stream): tensors go as their device addresses, None as a null pointer.
        Asynchronous."""
        lib = _lib.load()
        symbol = symbol or self.SYMBOL
        ptrs = [ctypes.c_void_p(a.data_ptr()) if isinstance(a, torch.Tensor) else a for a in args]
        with torch.cuda.device(self.device):
            rc = getattr(lib, symbol)(self.device, *ptrs, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        _lib.check(rc, symbol)


class WeightedTerm(PostDevice):
    """A term of train_step that carries weights and a backward chain to con_rgb: `SYMBOL` is its forward, `GRAD_SYMBOL` the forward
    followed by the chain, bsr_debug_<GRAD_SYMBOL> the same stopped after `stop_after` of the chain's launches.  The subclass names its
    symbols, queries, pack functions, images, cap and texts, turns its losses into the scalar (`_scalar`), adds its own outputs to a call
    (`_extra`) and names what the calls leave in the scratch (`activations`)."""
    GRAD_SYMBOL = ""
    BLOB_QUERY = DGRAD_BLOB_QUERY = ""         # the sizes of the forward's and the gradient layers' blob
    PACK = PACK_DGRAD = None                   # weights dict -> those blobs (pack.py), as staticmethods
    IMAGES = ()                                # the image arguments' names in the entry points' order, [B,S,S,3] each
    MAX_B = 0
    N_LOSSES = K = 0                           # the losses tensor's floats, the columns of sums
    BLOB_TEXT = NO_WEIGHTS_TEXT = NO_GRAD_WEIGHTS_TEXT = ""

    def __init__(self, device: int):
        super().__init__(device)
        self._blob = None
        self._dgrad_blob = None

    def _upload(self, blob: bytes) -> torch.Tensor:
        return torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(self._dev)

    def load_weights(self, weights: Dict[str, np.ndarray]) -> None:
        """The term's variables -> the forward's packed blob (`PACK`) and the gradient layers' (`PACK_DGRAD`) on the device."""
        self.load_blob(self.PACK(weights))
        dgrad = self.PACK_DGRAD(weights)
        assert len(dgrad) == int(getattr(_lib.load(), self.DGRAD_BLOB_QUERY)())
        self._dgrad_blob = self._upload(dgrad)

    def load_blob(self, blob: bytes) -> None:
        """A blob of `PACK`.  ValueError unless it holds `BLOB_QUERY`() bytes.  The forward's weights alone: a gradient blob loaded earlier
        is dropped with the weights it belonged to."""
        want = int(getattr(_lib.load(), self.BLOB_QUERY)())
        if len(blob) != want:
            raise ValueError(self.BLOB_TEXT % (want, len(blob)))
        self._dgrad_blob = None
        self._blob = self._upload(blob)

    def _check(self, images, upstream=None, grad: bool = False):
        """Everything a call checks before any launch, in this order: the images, `upstream`, the weights -> (b, s)."""
        b, s = self.images([(name, t, 3) for name, t in zip(self.IMAGES, images)], self.MAX_B)
        if upstream is not None and (not isinstance(upstream, torch.Tensor) or upstream.dtype != torch.float32 or upstream.numel() != 1
                                     or upstream.device != self._dev):
            raise TypeError("upstream must be a float32 tensor of one element on %s, or None" % (self._dev,))
        if self._blob is None or (grad and self._dgrad_blob is None):
            raise ValueError(self.NO_GRAD_WEIGHTS_TEXT if grad else self.NO_WEIGHTS_TEXT)
        return b, s

    def _scalar(self, losses: torch.Tensor) -> torch.Tensor:
        """The term's own loss out of the losses tensor."""
        return losses

    def _extra(self, b: int, s: int, **want):
        """The subclass's own outputs -> (what the entry points take for them after losses, what a call returns for them after sums)."""
        return (), ()

    def _run(self, images, b: int, s: int, upstream=None, grad: bool = False, stop_after: Optional[int] = None, keep: bool = False, **want):
        """One checked call -> (losses, sums, the subclass's own outputs, with `grad` the gradient [b,s,s,3], with `keep` the
        activations)."""
        losses = self.empty((self.N_LOSSES,), torch.float32)
        sums = self.empty((b, self.K), torch.float64)
        extra, out = self._extra(b, s, **want)
        out = (losses, sums) + out
        args = [self._blob, ctypes.c_size_t(self._blob.numel())]
        if grad:
            args += [self._dgrad_blob, ctypes.c_size_t(self._dgrad_blob.numel())]
        args += images
        if grad:
            args.append(upstream)
        args += [b, s, sums, losses, *extra]
        if grad:
            out += (self.empty((b, s, s, 3), torch.float32),)
            args.append(out[-1])
        args.append(ctypes.c_void_p(self.scratch(b, s, grad)))
        symbol = self.GRAD_SYMBOL if grad else self.SYMBOL
        if stop_after is not None:
            args.append(int(stop_after))
            symbol = symbol.replace("bsr_", "bsr_debug_", 1)
        self.call(*args, symbol=symbol)
        return out + (self.activations(b, s),) if keep else out

    def _forward(self, images, keep: bool = False, **want):
        b, s = self._check(images)
        return self._run(images, b, s, keep=keep, **want)

    def _grad(self, images, upstream, keep: bool = False):
        b, s = self._check(images, upstream, grad=True)
        return self._run(images, b, s, upstream, grad=True, keep=keep)

    def _loss(self, *images) -> torch.Tensor:
        return _TermLoss.apply(self, *images)


class _TermLoss(torch.autograd.Function):
    """A WeightedTerm's scalar with d scalar / d con_rgb: when con_rgb requires a gradient, forward and backward run in one call in
    forward() and backward() is one device multiply; every other input gets None."""
    @staticmethod
    def forward(ctx, runner, *images):
        ctx.con_rgb = 1 + runner.IMAGES.index("con_rgb")
        detached = [t.detach() for t in images]
        if ctx.needs_input_grad[ctx.con_rgb]:
            losses, _, grad = runner._grad(detached, None)
            ctx.save_for_backward(grad)
        else:
            losses = runner._forward(detached)[0]
        return runner._scalar(losses)

    @staticmethod
    def backward(ctx, grad_output):
        out = [None] * len(ctx.needs_input_grad)
        if ctx.needs_input_grad[ctx.con_rgb]:
            grad, = ctx.saved_tensors
            out[ctx.con_rgb] = grad * grad_output.to(torch.float32).reshape(())
        return tuple(out)


DENSE, STRIDED, OPTIONAL = "dense", "strided", "optional"


class GradStage(PostDevice):
    """A stage of the generator's backward pass: `SYMBOL`(blob, bytes, the inputs, B, H, W, the outputs, the flat gradient buffer[, keep],
    scratch), bsr_debug_<SYMBOL> the same stopped after `stop_after` of the chain's launches, and the queries <SYMBOL>_blob_bytes,
    _scratch_bytes, _floats, _var_offset.  The subclass declares the attributes below and keeps what it reads out of the scratch (`maps`)
    and its public calls, which hand their tensors over by name."""
    PACK = NAMES = None        # weights dict -> the blob (pack.py); the trainable variables' names in the flat buffer's order: staticmethods
    INPUTS = ()                # (name, channels, the sizes' divisor, kind) in the entry point's order.  DENSE: a tensor; STRIDED: (address,
    #                            floats between pixels), a tensor or the generator's own; OPTIONAL: a dense tensor or None
    LEAD = ""                  # the dense input that gives (B, H, W)
    OUTPUTS = ()               # (name, channels, divisor) in the entry point's order, ahead of the flat buffer
    TAKES_KEEP = False         # the entry point has a `keep` argument
    KEPT = ()                  # what a call with keep=True adds to its result, out of `maps`
    MULTIPLES = (1, 1)         # the size rule: H and W are multiples of these
    DIMS = IMAGE_DIMS = "H,W"  # how the texts spell the lead's sizes, and an image's
    LIKE_TEXT = SIZE_TEXT = NO_WEIGHTS_TEXT = WHAT = ""
    LAUNCHES = ()
    LAST = ""                  # the Generator method that gives the strided inputs in place: (addresses, strides, the forward's shape)

    def __init__(self, device: int):
        super().__init__(device)
        self._blob: Optional[torch.Tensor] = None

    def load_weights(self, weights) -> None:
        """The generator's variables (the stage's own are read) -> the chain's blob on the device."""
        blob = self.PACK(weights)
        assert len(blob) == int(getattr(_lib.load(), self.SYMBOL + "_blob_bytes")())
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
            raise TypeError("%s must be a float32 tensor [B,%s,%d] on %s" % (name, self.IMAGE_DIMS, c, self._dev))
        if not t.is_contiguous():
            raise ValueError("%s must be contiguous (NHWC, dense)" % name)
        if shape is not None and tuple(t.shape) != shape + (c,):
            raise ValueError("%s must be [%d,%d,%d,%d] %s, got %s" % ((name,) + shape + (c, self.LIKE_TEXT, tuple(t.shape))))

    def _check(self, given, in_place: bool = False):
        """given: name -> tensor.  `LEAD` first, then the other inputs in their order (with `in_place` the dense ones alone), then the
        size rule, then the weights -> (b, h, w)."""
        lead = given[self.LEAD]
        channels = next(c for name, c, _, _ in self.INPUTS if name == self.LEAD)
        self._image(self.LEAD, lead, channels)
        b, h, w = (int(d) for d in lead.shape[:3])
        if int(lead.shape[3]) != channels:
            raise ValueError("%s must be [B,%s,%d], got %s" % (self.LEAD, self.DIMS, channels, tuple(lead.shape)))
        for name, c, div, kind in self.INPUTS:
            if name != self.LEAD and not (kind == STRIDED and in_place) and not (kind == OPTIONAL and given[name] is None):
                self._image(name, given[name], c, (b, h // div, w // div))
        if b < 1 or h < 1 or w < 1 or h % self.MULTIPLES[0] or w % self.MULTIPLES[1]:
            raise ValueError(self.SIZE_TEXT % (b, h, w))
        if self._blob is None:
            raise ValueError(self.NO_WEIGHTS_TEXT)
        return b, h, w

    def stage_scratch(self, b: int, h: int, w: int, keep: bool = False) -> int:
        """The 256-byte aligned device address of at least <SYMBOL>_scratch_bytes(b, h, w[, keep]) bytes of scratch."""
        query = self.SYMBOL + "_scratch_bytes"
        sizes = (b, h, w, 1 if keep else 0)[:len(_lib.SIGNATURES[query][1])]
        need = int(getattr(_lib.load(), query)(*sizes))
        if need == 0:
            raise ValueError(self.SIZE_TEXT % (b, h, w))
        return self.reserve(need)

    scratch3 = scratch4 = stage_scratch

    # -- the call ---------------------------------------------------------------------------------
    def _run(self, given, strided, b: int, h: int, w: int, keep: bool, stop_after: Optional[int] = None):
        """strided: name -> (device address, floats between pixels) of the STRIDED inputs; None: the tensors of `given`, dense -> the
        outputs, then the flat gradient buffer."""
        lib = _lib.load()
        outs = [self.empty((b, h // div, w // div, c), torch.float32) for _, c, div in self.OUTPUTS]
        outs.append(self.empty((int(getattr(lib, self.SYMBOL + "_floats")()),), torch.float32))
        if stop_after is not None:
            for t in outs:
                t.zero_()                      # a stopped chain leaves what it did not write at 0
        args = [self._blob, ctypes.c_size_t(self._blob.numel())]
        for name, c, _, kind in self.INPUTS:
            if kind == STRIDED:
                ptr, cs = strided[name] if strided is not None else (given[name].data_ptr(), c)
                args += [ctypes.c_void_p(ptr), int(cs)]
            else:
                args.append(given[name])
        args += [b, h, w, *outs]
        if self.TAKES_KEEP:
            args.append(1 if keep else 0)
        args.append(ctypes.c_void_p(self.stage_scratch(b, h, w, keep)))
        symbol = self.SYMBOL
        if stop_after is not None:
            args.append(int(stop_after))
            symbol = symbol.replace("bsr_", "bsr_debug_", 1)
        self.call(*args, symbol=symbol)
        return outs

    @classmethod
    def split_grads(cls, flat: torch.Tensor) -> Dict[str, torch.Tensor]:
        """The flat buffer of `SYMBOL` -> name -> a view of it in the variable's shape, for `NAMES`(); the flat tensor itself under the
        key ""."""
        from .weights import generator_variable_shapes
        var_offset = getattr(_lib.load(), cls.SYMBOL + "_var_offset")
        shapes = generator_variable_shapes()
        out = {"": flat}
        for index, name in enumerate(cls.NAMES()):
            off = int(var_offset(index))
            out[name] = flat[off:off + math.prod(shapes[name])].reshape(shapes[name])
        return out

    def _result(self, outs, b: int, h: int, w: int, keep: bool):
        out = self.split_grads(outs[-1])
        out.update(zip((name for name, _, _ in self.OUTPUTS), outs))
        if keep:
            kept = self.maps(b, h, w)
            out.update((name, kept[name]) for name in self.KEPT)
        return out

    def _grad(self, given, keep: bool):
        """The public call on tensors: everything is checked before any launch (TypeError / ValueError)."""
        b, h, w = self._check(given)
        return self._result(self._run(given, None, b, h, w, keep), b, h, w, keep)

    def _backward(self, generator, given, keep: bool, lead: str = ""):
        """The public call with the STRIDED inputs read in place from `generator`'s workspace (`LAST`: the last forward's, no copies),
        for a `LEAD` (called `lead` by the caller) of that forward's shape."""
        b, h, w = self._check(given, in_place=True)
        ptrs, strides, shape = getattr(generator, self.LAST)()
        if generator._device != self.device:
            raise ValueError("the generator lives on cuda:%s, %s on %s" % (generator._device, self.WHAT, self._dev))
        if tuple(shape[:3]) != (b, h, w):
            raise ValueError("the generator's last forward was %s, %s is %s" % (tuple(shape[:3]), lead or self.LEAD, (b, h, w)))
        in_place = [(name, c) for name, c, _, kind in self.INPUTS if kind == STRIDED]
        ptrs = ptrs if isinstance(ptrs, (tuple, list)) else (ptrs,)
        strides = strides if isinstance(strides, (tuple, list)) else (strides,)
        strides = tuple(strides) + tuple(c for _, c in in_place[len(strides):])      # a stride the generator does not give is the channels
        strided = {name: (ptr, cs) for (name, _), ptr, cs in zip(in_place, ptrs, strides)}
        return self._result(self._run(given, strided, b, h, w, keep), b, h, w, keep)

    def stages(self, *tensors) -> Dict[str, torch.Tensor]:
        """For the stage-by-stage tests: stages(the inputs in their order, n), the chain stopped after `n` of its launches (`LAUNCHES`),
        everything kept -> `maps`, plus the outputs and the flat gradient buffer under "", zero where no launch wrote; the maps of
        launches that did not run hold whatever the scratch held."""
        *tensors, n = tensors
        given = dict(zip((name for name, _, _, _ in self.INPUTS), tensors))
        b, h, w = self._check(given)
        if not 0 <= int(n) <= len(self.LAUNCHES):
            raise ValueError("stop_after must be 0..%d" % len(self.LAUNCHES))
        outs = self._run(given, None, b, h, w, True, stop_after=int(n))
        out = self.maps(b, h, w)
        out.update(zip([name for name, _, _ in self.OUTPUTS] + [""], outs))
        return out


def raise_for_status(status, names: Optional[Sequence[str]], texts: Dict[int, str], prefix: str, other: str = "status %d",
                     other_type: type = ValueError) -> None:
    """Raise for the first item whose status is not 0: "<prefix> <name>: <text>", the item's name (its index when `names` has none for
    it).  A status in `texts` raises ValueError; any other raises `other_type` with the text `other` % status."""
    for j, st in enumerate(np.asarray(status).reshape(-1)):
        st = int(st)
        if st != 0:
            name = names[j] if names is not None and j < len(names) else j
            if st in texts:
                raise ValueError("%s %s: %s" % (prefix, name, texts[st]))
            raise other_type("%s %s: %s" % (prefix, name, other % st))
