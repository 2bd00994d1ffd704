"""What the device bindings of single library entry points share.  `PostDevice`, under the evaluation runners (ucb_post_gpu,
ucb_post_rgb_gpu, ucb_post_tsm_gpu, sfw_post_gpu) and train_step's terms (shadow_synth_gpu, train_losses_gpu): the input checks, a
cached scratch buffer aligned to 256 bytes and sized by a named query, float32 views into it, the library call on the current stream,
and the per-item status check.  `WeightedTerm`, under the two terms that carry weights and a backward chain (discriminator_gpu,
perceptual_gpu): the two blobs, the forward and gradient calls, and the term as a differentiable scalar."""
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
        if self._scratch is None or self._scratch.numel() < need + 256:
            self._scratch = None
            self._scratch = torch.empty(need + 256, dtype=torch.uint8, device=self._dev)
        base = self._scratch.data_ptr()
        return base + (-base) % 256

    def view(self, offset: int, shape) -> torch.Tensor:
        """The float32 tensor `shape` that starts `offset` bytes past the scratch's aligned address: a view, not a copy."""
        offset += (-self._scratch.data_ptr()) % 256
        return self._scratch[offset:offset + 4 * math.prod(shape)].view(torch.float32).reshape(shape)

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
