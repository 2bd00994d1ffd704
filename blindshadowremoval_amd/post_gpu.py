"""What the device post-processing bindings share (ucb_post_gpu, ucb_post_rgb_gpu, ucb_post_tsm_gpu, sfw_post_gpu): the input checks,
a cached scratch buffer aligned to 256 bytes, the library call on the current stream, and the per-item status check."""
from __future__ import annotations

import ctypes
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import _lib


class PostDevice:
    """Reusable runner of one library entry point `SYMBOL` on one device: keeps its scratch buffer between calls.  A subclass's run()
    checks its inputs (`inputs`), sizes the scratch (`scratch`), allocates its outputs (`empty`) and calls the library (`call`)."""
    SYMBOL = ""
    SIZE_TEXT = ""        # the ValueError text when `SYMBOL`_scratch_bytes refuses (B, S); %(b)d / %(s)d are filled in
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

    def scratch(self, b: int, s: int) -> int:
        """The 256-byte aligned device address of at least `SYMBOL`_scratch_bytes(b, s) bytes of scratch."""
        need = int(getattr(_lib.load(), self.SYMBOL + "_scratch_bytes")(b, s))
        if need == 0:
            raise ValueError(self.SIZE_TEXT % {"b": b, "s": s})
        if self._scratch is None or self._scratch.numel() < need + 256:
            self._scratch = torch.empty(need + 256, dtype=torch.uint8, device=self._dev)
        base = self._scratch.data_ptr()
        return base + (-base) % 256

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
