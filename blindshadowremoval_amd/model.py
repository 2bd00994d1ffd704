"""Drop-in counterpart of the reference's ``Generator`` (/root/reference/model.py:198-290) for
inference on MI355X: same constructor, same call signature and return order, NHWC float32 tensors —
backed by libbsr_hip (hand-written gfx950 kernels) through the C ABI of include/bsr_hip.h.

    gen = Generator()
    gen.load_weights(weights)                    # dict: reference checkpoint names -> numpy arrays
    gs, con_rgb, mask22, dif = gen(inputs, uv, reg, chuck=1, training=False)

``reg`` and ``chuck`` are accepted and unused, exactly as in the reference's GSC forward
(``ShareLayer`` is constructed but never called there: model.py:221 vs :228-290).
"""
from __future__ import annotations

import ctypes
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib
from .pack import DTYPES, pack_generator
from .tf_bundle import latest_checkpoint, load_generator_weights


class Generator:
    _NAME = "Generator"      # the class name the "no weights" refusal states (GeneratorTSM says Generator too)

    def __init__(self, downsize: int = 1, n_res: int = 6, device: Optional[int] = None, dtype: str = "f32"):
        """``dtype``: "f32" (fp32 matrix cores — the measured path and the default), "f32x3" (split-precision fp32 on the fp16 matrix
        cores: same end-to-end tolerance, ~1.9x faster, activations must stay below 65520 in magnitude — a violation is detected on
        the device and raised by ``check_range()`` / the next call, never silent) or "f16" (BASELINE configs[3])."""
        if dtype not in DTYPES:
            raise ValueError("dtype must be 'f32' (the measured path), 'f32x3' (split-precision fp32 on the 16-bit matrix cores) or "
                             "'f16' (fp16 operands on the 3x3-conv path, BASELINE configs[3])")
        self.dtype = dtype
        if n_res != 6:
            raise ValueError("the GSC generator has n_res=6 (/root/reference/model.py:199)")
        self.n_res = n_res
        self.n_ch = [32, 64, 64, 96, 128, 256, 256]
        self._device = device
        self._handle: Optional[ctypes.c_void_p] = None
        self._lib = None
        self._shape: Optional[Tuple[int, int, int]] = None

    # -- weights ----------------------------------------------------------------------------
    def load_weights(self, weights: Dict[str, np.ndarray]) -> "Generator":
        """``weights``: the reference's ``generator/...`` variables by checkpoint name
        (``conv1/conv/kernel`` HWIO, ConvT kernels ``[kh,kw,out,in]``, BN gamma/beta/moving_*)."""
        if not torch.cuda.is_available():
            raise RuntimeError("blindshadowremoval_amd.Generator needs a ROCm GPU: there is no CPU path")
        lib = _lib.load()
        dev = torch.cuda.current_device() if self._device is None else int(self._device)
        blob = pack_generator(weights, self.dtype)
        handle = ctypes.c_void_p()
        buf = (ctypes.c_char * len(blob)).from_buffer_copy(blob)
        with torch.cuda.device(dev):
            rc = lib.bsr_create(ctypes.byref(handle), dev, ctypes.cast(buf, ctypes.c_void_p), len(blob), DTYPES[self.dtype])
        _lib.check(rc, "bsr_create")
        self.close()
        self._lib, self._handle, self._device = lib, handle, dev
        return self

    def restore(self, checkpoint_dir: str) -> int:
        """Counterpart of ``tf.train.latest_checkpoint`` + ``checkpoint.restore(...).expect_partial()``
        (/root/reference/train_test_GSC.py:362-367).  Returns the epoch parsed from the file name, 0 if none."""
        prefix = latest_checkpoint(checkpoint_dir)
        if not prefix:
            return 0
        self.load_weights(load_generator_weights(prefix))
        return int(prefix.split("-")[-1])

    def close(self) -> None:
        if self._handle is not None and self._lib is not None:
            self._lib.bsr_destroy(self._handle)
        self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- forward ----------------------------------------------------------------------------
    def _require_weights(self) -> None:
        if self._handle is None:
            raise RuntimeError("%s has no weights: call load_weights() or restore() first" % self._NAME)

    def _prepare(self, inputs, uv, same_size: bool = True):
        """The checks every forward starts with, in their order; returns (dev, inputs, uv, B, H, W) with both tensors on the device.
        ``same_size=False``: the TSM path, which checks ``reg`` next and then states its own (square) size rule."""
        self._require_weights()
        dev = self._device
        inputs = self._check_input(inputs, "inputs", dev)
        uv = self._check_input(uv, "uv", dev)
        B, H, W, _ = inputs.shape
        if same_size:
            if uv.shape != inputs.shape:
                raise ValueError("inputs %s and uv %s must have the same shape" % (tuple(inputs.shape), tuple(uv.shape)))
            if H % 32 or W % 256:
                raise ValueError("H must be a multiple of 32 and W of 256 (reference IMG_SIZE = 256), got %dx%d" % (H, W))
        return dev, inputs, uv, B, H, W

    @staticmethod
    def _new_outputs(B: int, H: int, W: int, device):
        return tuple(torch.empty((B, H, W, c), dtype=torch.float32, device=device) for c in (1, 3, 3, 1))      # gs, con_rgb, mask22, dif

    def _check_input(self, t: torch.Tensor, name: str, dev: int) -> torch.Tensor:
        if not isinstance(t, torch.Tensor):
            t = torch.as_tensor(np.asarray(t))
        if t.dim() != 4 or t.shape[-1] != 3:
            raise ValueError("%s must be [B,H,W,3] NHWC, got %s" % (name, tuple(t.shape)))
        if t.dtype != torch.float32:
            raise TypeError("%s must be float32, got %s" % (name, t.dtype))
        if t.device.type != "cuda" or t.device.index != dev:
            t = t.to("cuda:%d" % dev)
        return t.contiguous()

    @staticmethod
    def _check_out(out, B: int, H: int, W: int, dev: int):
        """Caller-supplied output buffers go to the library as raw pointers: refuse anything it would write out of bounds."""
        if not isinstance(out, (tuple, list)) or len(out) != 4:
            raise ValueError("out must be a tuple (gs, con_rgb, mask22, dif)")
        for t, c, name in zip(out, (1, 3, 3, 1), ("gs", "con_rgb", "mask22", "dif")):
            if not isinstance(t, torch.Tensor) or tuple(t.shape) != (B, H, W, c):
                raise ValueError("out[%s] must be a tensor of shape %s, got %s" % (name, (B, H, W, c), tuple(getattr(t, "shape", ()))))
            if t.dtype != torch.float32:
                raise TypeError("out[%s] must be float32, got %s" % (name, t.dtype))
            if t.device.type != "cuda" or t.device.index != dev:
                raise ValueError("out[%s] must live on cuda:%d, got %s" % (name, dev, t.device))
            if not t.is_contiguous():
                raise ValueError("out[%s] must be contiguous (dense NHWC)" % name)
        return tuple(out)

    def __call__(self, inputs, uv, reg=None, chuck: int = 1, training: bool = False,
                 out: Optional[Tuple[torch.Tensor, ...]] = None, packed_out: Optional[torch.Tensor] = None):
        """``packed_out``: optional [B,H,W,4] float32 CUDA tensor; con_rgb | dif are then written straight into it (bsr_forward_packed:
        the multi-GPU all-gather payload) and the returned con_rgb / dif are views of it."""
        if training:
            raise NotImplementedError("only the inference path (training=False) is implemented "
                                      "(/root/reference/train_test_GSC.py:404,856)")
        dev, inputs, uv, B, H, W = self._prepare(inputs, uv)
        with torch.cuda.device(dev):
            gs, con_rgb, mask22, dif = self._new_outputs(B, H, W, inputs.device) if out is None else self._check_out(out, B, H, W, dev)
            stream = torch.cuda.current_stream().cuda_stream
            if packed_out is not None:
                if (not isinstance(packed_out, torch.Tensor) or tuple(packed_out.shape) != (B, H, W, 4) or packed_out.dtype != torch.float32
                        or packed_out.device.type != "cuda" or packed_out.device.index != dev or not packed_out.is_contiguous()):
                    raise ValueError("packed_out must be a contiguous float32 [B,H,W,4] tensor on cuda:%d" % dev)
                rc = self._lib.bsr_forward_packed(self._handle, inputs.data_ptr(), uv.data_ptr(), B, H, W, gs.data_ptr(), packed_out.data_ptr(),
                                                  mask22.data_ptr(), stream)
                con_rgb, dif = packed_out[..., :3], packed_out[..., 3:]
            else:
                rc = self._lib.bsr_forward(self._handle, inputs.data_ptr(), uv.data_ptr(), B, H, W, gs.data_ptr(), con_rgb.data_ptr(),
                                           mask22.data_ptr(), dif.data_ptr(), stream)
        _lib.check(rc, "bsr_forward")
        self._shape = (B, H, W)
        return gs, con_rgb, mask22, dif

    # -- TSM variant ------------------------------------------------------------------------
    def call_tsm(self, inputs, uv, reg, frame: int, share: bool = True, chuck: int = 1, training: bool = False):
        """``Generator.call(inputs, uv, reg, frame, share, chuck, training)`` of /root/reference/model_with_TSM.py:261-325
        (call site /root/reference/train_with_TSM.py:676).  Needs TSM weights (291-channel ``res_stack/0/conv1``)."""
        if training:
            raise NotImplementedError("only the inference path (training=False) is implemented")
        dev, inputs, uv, B, H, W = self._prepare(inputs, uv, same_size=False)
        if not isinstance(reg, torch.Tensor):
            reg = torch.as_tensor(np.asarray(reg))
        if reg.dim() != 4 or reg.shape[-1] != 6 or reg.shape[:3] != inputs.shape[:3] or reg.dtype != torch.float32:
            raise ValueError("reg must be float32 [B,H,W,6] (reg_in | reg_out), got %s %s" % (tuple(reg.shape), reg.dtype))
        reg = reg.to("cuda:%d" % dev).contiguous()
        if H != W or H % 256:
            raise ValueError("the TSM path needs square images with H a multiple of 256, got %dx%d" % (H, W))
        if frame <= 0 or B % frame:
            raise ValueError("batch %d is not a multiple of frame %d" % (B, frame))
        with torch.cuda.device(dev):
            gs, con_rgb, mask22, dif = self._new_outputs(B, H, W, inputs.device)
            stream = torch.cuda.current_stream().cuda_stream
            rc = self._lib.bsr_forward_tsm(self._handle, inputs.data_ptr(), uv.data_ptr(), reg.data_ptr(), B, H, W, int(frame), 1 if share else 0,
                                           gs.data_ptr(), con_rgb.data_ptr(), mask22.data_ptr(), dif.data_ptr(), stream)
        _lib.check(rc, "bsr_forward_tsm")
        self._shape = (B, H, W)
        return gs, con_rgb, mask22, dif

    def check_range(self) -> None:
        """16-bit modes (dtype "f32x3" / "f16"): synchronise the current stream and raise ``_lib.RangeError`` if any forward since
        the last call converted an activation of magnitude >= 65520 to fp16 (its outputs hold inf / NaN where the fp32 path stays
        finite: discard them and re-run on a ``dtype="f32"`` generator).  The kernels detect this on the device (bsr_check_range in
        include/bsr_hip.h); without a call the NEXT forward after a completed overflowing one raises instead.  No-op for "f32"."""
        self._require_weights()
        with torch.cuda.device(self._device):
            rc = self._lib.bsr_check_range(self._handle, torch.cuda.current_stream().cuda_stream)
        _lib.check(rc, "bsr_check_range")

    def peek_range(self) -> None:
        """``check_range`` for a pipelined caller: no stream synchronisation and the condition is not cleared — raises
        ``_lib.RangeError`` if any forward that has COMPLETED so far overflowed fp16 (bsr_peek_range).  No-op for "f32"."""
        self._require_weights()
        _lib.check(self._lib.bsr_peek_range(self._handle), "bsr_peek_range")

    # -- test / measurement hooks -----------------------------------------------------------
    def probe(self, name: str) -> torch.Tensor:
        """Intermediate of the last forward as a dense NHWC tensor (see bsr_probe in include/bsr_hip.h)."""
        if self._shape is None:
            raise RuntimeError("probe() needs a forward first")
        shape = (ctypes.c_int * 4)()
        with torch.cuda.device(self._device):
            stream = torch.cuda.current_stream().cuda_stream
            # first call with zero capacity only reports the shape (the copy is refused with BSR_ERR_ARG) ...
            rc = self._lib.bsr_probe(self._handle, name.encode(), ctypes.c_void_p(8), 0, ctypes.byref(shape), stream)
            if rc not in (0, 1) or shape[0] == 0:
                _lib.check(rc if rc else 4, "bsr_probe")
            n = shape[0] * shape[1] * shape[2] * shape[3]
            dst = torch.empty(n, dtype=torch.float32, device="cuda:%d" % self._device)
            # ... the second one copies into an exactly sized tensor
            _lib.check(self._lib.bsr_probe(self._handle, name.encode(), dst.data_ptr(), dst.numel(), ctypes.byref(shape), stream), "bsr_probe")
        return dst.reshape(shape[0], shape[1], shape[2], shape[3])

    def last_f(self) -> Tuple[int, int, Tuple[int, int, int, int]]:
        """(device address, floats between pixels, (B, H, W, 64)) of the last forward's f — clr_up3's output, the colour tail's input —
        in the handle's workspace (bsr_last_f): no copy; valid until the next forward on this generator.  fp32 generators only:
        RuntimeError before any forward and for the 16-bit modes."""
        self._require_weights()
        ptr, cs, shape = ctypes.c_void_p(), ctypes.c_int(), (ctypes.c_int * 4)()
        _lib.check(self._lib.bsr_last_f(self._handle, ctypes.byref(ptr), ctypes.byref(cs), ctypes.byref(shape)), "bsr_last_f")
        return int(ptr.value), int(cs.value), (shape[0], shape[1], shape[2], shape[3])

    def last_decoder(self) -> Tuple[Tuple[int, int, int, int], int, Tuple[int, int, int, int]]:
        """((x, f1, f2, f) device addresses, x's floats between pixels, (B, H, W, 64)) of the last forward's colour decoder tensors in the
        handle's workspace (bsr_last_decoder): x = res_stack/5's output [B,H/8,W/8,261 of x_cs], f1 [B,H/4,W/4,128], f2 [B,H/2,W/2,96],
        f [B,H,W,64], the last three dense.  No copy; valid until the next forward on this generator.  fp32 GSC generators only:
        RuntimeError before any forward, for the 16-bit modes and for TSM weights."""
        self._require_weights()
        ptrs = [ctypes.c_void_p() for _ in range(4)]
        cs, shape = ctypes.c_int(), (ctypes.c_int * 4)()
        _lib.check(self._lib.bsr_last_decoder(self._handle, ctypes.byref(ptrs[0]), ctypes.byref(cs), ctypes.byref(ptrs[1]), ctypes.byref(ptrs[2]),
                                              ctypes.byref(ptrs[3]), ctypes.byref(shape)), "bsr_last_decoder")
        return tuple(int(p.value) for p in ptrs), int(cs.value), (shape[0], shape[1], shape[2], shape[3])

    def last_block5(self) -> Tuple[Tuple[int, int, int], Tuple[int, int, int], Tuple[int, int, int, int]]:
        """((y3x, xin, out) device addresses, their floats between pixels, (B, H/8, W/8, 261)) of what the last forward kept of res_stack/5
        in the handle's workspace (bsr_last_block5): y3x = bnorm3's output + pad(xin) (257 channels read), xin the block's input, out its
        output.  No copy; valid until the next forward on this generator.  fp32 GSC generators only: RuntimeError before any forward, for
        the 16-bit modes and for TSM weights."""
        self._require_weights()
        ptrs = [ctypes.c_void_p() for _ in range(3)]
        y_cs, x_cs, shape = ctypes.c_int(), ctypes.c_int(), (ctypes.c_int * 4)()
        _lib.check(self._lib.bsr_last_block5(self._handle, ctypes.byref(ptrs[0]), ctypes.byref(y_cs), ctypes.byref(ptrs[1]), ctypes.byref(ptrs[2]),
                                             ctypes.byref(x_cs), ctypes.byref(shape)), "bsr_last_block5")
        return tuple(int(p.value) for p in ptrs), (int(y_cs.value), int(x_cs.value), int(x_cs.value)), (shape[0], shape[1], shape[2], shape[3])

    def last_block5_input(self) -> Tuple[int, int, Tuple[int, int, int, int]]:
        """(xin's device address, its floats between pixels, (B, H/8, W/8, 261)) of res_stack/5's input in the handle's workspace: what
        last_block5 gives for xin, under the same conditions."""
        ptrs, strides, shape = self.last_block5()
        return ptrs[1], strides[1], shape

    def last_block(self, block: int) -> Tuple[Tuple[int, int, int], Tuple[int, int, int], Tuple[int, int, int, int]]:
        """last_block5's triple for res_stack/`block`, block 3, 4 or 5 (bsr_last_block): y3x and out are the block's own, xin is xh =
        cat[x_hole | bmask | uv] for block 3 and the block below's output for blocks 4 and 5.  Under last_block5's conditions."""
        self._require_weights()
        ptrs = [ctypes.c_void_p() for _ in range(3)]
        y_cs, x_cs, shape = ctypes.c_int(), ctypes.c_int(), (ctypes.c_int * 4)()
        _lib.check(self._lib.bsr_last_block(self._handle, int(block), ctypes.byref(ptrs[0]), ctypes.byref(y_cs), ctypes.byref(ptrs[1]),
                                            ctypes.byref(ptrs[2]), ctypes.byref(x_cs), ctypes.byref(shape)), "bsr_last_block")
        return tuple(int(p.value) for p in ptrs), (int(y_cs.value), int(x_cs.value), int(x_cs.value)), (shape[0], shape[1], shape[2], shape[3])

    def last_colour_trunk(self) -> Tuple[Tuple[int, int, int, int, int], Tuple[int, int, int, int, int], Tuple[int, int, int, int]]:
        """((y3x4, out4, y3x3, out3, xh) device addresses, their floats between pixels, (B, H/8, W/8, 261)) of what the last forward kept
        of res_stack/4 and res_stack/3 in the handle's workspace (last_block(4) and last_block(3)): block 4's input is out3, block 3's
        is xh, whose channel 257 is bmask.  No copy; valid until the next forward on this generator.  Under last_block5's conditions."""
        (y4, _, o4), (y4_cs, _, o4_cs), shape = self.last_block(4)      # block 4's xin is out3 (bsr_last_block)
        (y3, xh, o3), (y3_cs, xh_cs, o3_cs), _ = self.last_block(3)
        return (y4, o4, y3, o3, xh), (y4_cs, o4_cs, y3_cs, o3_cs, xh_cs), shape

    def last_lower_trunk(self) -> Tuple[Tuple[int, ...], Tuple[int, ...], Tuple[int, int, int, int]]:
        """((y3x2, out2, y3x1, out1, y3x0, out0, x0) device addresses, their floats between pixels, (B, H/8, W/8, 257)) of what the last
        forward kept of res_stack/2, /1 and /0 in the handle's workspace (bsr_last_lower_trunk): block 2's input is out1, block 1's is
        out0, block 0's is x0 = cat[down3's output 96 | the resized uv 3].  No copy; valid until the next forward on this generator.
        Under last_block5's conditions."""
        self._require_weights()
        ptrs, strides, shape = (ctypes.c_void_p * 7)(), (ctypes.c_int * 7)(), (ctypes.c_int * 4)()
        _lib.check(self._lib.bsr_last_lower_trunk(self._handle, ctypes.byref(ptrs), ctypes.byref(strides), ctypes.byref(shape)), "bsr_last_lower_trunk")
        return tuple(int(p or 0) for p in ptrs), tuple(int(s) for s in strides), (shape[0], shape[1], shape[2], shape[3])

    def last_y(self) -> Tuple[int, int, Tuple[int, int, int, int]]:
        """(y's device address, its floats between pixels, (B, H, W, 64)) of the last forward's y, up3's output and the grey heads' input,
        in the handle's workspace (bsr_last_y): no copy; valid until the next forward on this generator.  Under last_f's conditions."""
        self._require_weights()
        ptr, cs, shape = ctypes.c_void_p(), ctypes.c_int(), (ctypes.c_int * 4)()
        _lib.check(self._lib.bsr_last_y(self._handle, ctypes.byref(ptr), ctypes.byref(cs), ctypes.byref(shape)), "bsr_last_y")
        return int(ptr.value), int(cs.value), (shape[0], shape[1], shape[2], shape[3])

    def last_grey_decoder(self) -> Tuple[Tuple[int, int, int, int], Tuple[int, int, int, int], Tuple[int, int, int, int]]:
        """((x, c2, c3, y) device addresses, their floats between pixels, (B, H, W, 64)) of the last forward's grey decoder tensors in the
        handle's workspace (bsr_last_grey_decoder): x = res_stack/2's output [B,H/8,W/8,257 of x_cs], c2 = [up1 96 | x3 64] at
        [B,H/4,W/4], c3 = [up2 64 | x2 64] at [B,H/2,W/2], y = up3's output [B,H,W,64].  No copy; valid until the next forward on this
        generator.  Under last_decoder's conditions."""
        self._require_weights()
        ptrs = [ctypes.c_void_p() for _ in range(4)]
        cs = [ctypes.c_int() for _ in range(4)]
        shape = (ctypes.c_int * 4)()
        args = [ctypes.byref(v) for pair in zip(ptrs, cs) for v in pair]
        _lib.check(self._lib.bsr_last_grey_decoder(self._handle, *args, ctypes.byref(shape)), "bsr_last_grey_decoder")
        return tuple(int(p.value) for p in ptrs), tuple(int(c.value) for c in cs), (shape[0], shape[1], shape[2], shape[3])

    def set_timing(self, enable: bool) -> None:
        _lib.check(self._lib.bsr_set_timing(self._handle, 1 if enable else 0), "bsr_set_timing")

    def get_timing(self) -> Dict[str, Tuple[float, int]]:
        ms = (ctypes.c_float * _lib.NUM_CLASSES)()
        n = (ctypes.c_int * _lib.NUM_CLASSES)()
        _lib.check(self._lib.bsr_get_timing(self._handle, ctypes.byref(ms), ctypes.byref(n)), "bsr_get_timing")
        return {name: (float(ms[i]), int(n[i])) for i, name in enumerate(_lib.CLASS_NAMES)}


    def get_launch_timing(self):
        """[(layer name, ms, class name)] of the last timed forward, in launch order (bsr_timing_entry)."""
        out = []
        name = ctypes.create_string_buffer(64)
        ms, cls = ctypes.c_float(), ctypes.c_int()
        for i in range(self._lib.bsr_timing_launches(self._handle)):
            _lib.check(self._lib.bsr_timing_entry(self._handle, i, name, 64, ctypes.byref(ms), ctypes.byref(cls)), "bsr_timing_entry")
            out.append((name.value.decode(), float(ms.value), _lib.CLASS_NAMES[cls.value]))
        return out


class GeneratorTSM(Generator):
    """Drop-in for ``Generator`` of /root/reference/model_with_TSM.py:231-325 (temporal-sharing variant, BASELINE config 5):
    ``gen(inputs, uv, reg, frame, share, chuck, training)``."""

    def __call__(self, inputs, uv, reg, frame, share=True, chuck: int = 1, training: bool = False):
        return self.call_tsm(inputs, uv, reg, frame, share, chuck, training)


class GeneratorRGB(Generator):
    """Drop-in for ``Generator`` of /root/reference/model_RGB.py:198-266, the paper's single-stage RGB baseline (call site
    /root/reference/train_RGB_test.py:414): one decoder predicts the shadow-free RGB image directly.

        gen = GeneratorRGB()
        gen.load_weights(weights)                    # model_RGB.py variables (generator_variable_shapes("rgb"))
        con = gen(inputs, uv, reg, chuck=4, training=False)

    ``reg`` and ``chuck`` are accepted and unused, as in the reference's ``call``.  fp32 only (``dtype="f32"``)."""
    _NAME = "GeneratorRGB"

    def __init__(self, downsize: int = 1, n_res: int = 6, device: Optional[int] = None, dtype: str = "f32"):
        if dtype != "f32":
            raise ValueError("GeneratorRGB is provided in dtype 'f32' only (the RGB baseline has no 'f32x3' / 'f16' path), got %r" % (dtype,))
        super().__init__(downsize, n_res, device, dtype)

    def load_weights(self, weights: Dict[str, np.ndarray]) -> "GeneratorRGB":
        from .weights import detect_variant
        if detect_variant(weights) != "rgb":
            raise ValueError("GeneratorRGB needs the RGB baseline's weights (model_RGB.py: 256-wide res_stack/0/conv1), got %s weights"
                             % detect_variant(weights))
        return super().load_weights(weights)

    def __call__(self, inputs, uv, reg=None, chuck: int = 1, training: bool = False, out: Optional[torch.Tensor] = None):
        """``out``: optional caller-supplied [B,H,W,3] float32 CUDA tensor for ``con``.  Returns ``con`` [B,H,W,3]."""
        if training:
            raise NotImplementedError("only the inference path (training=False) is implemented (/root/reference/train_RGB_test.py:414)")
        dev, inputs, uv, B, H, W = self._prepare(inputs, uv)
        with torch.cuda.device(dev):
            if out is None:
                con = torch.empty((B, H, W, 3), dtype=torch.float32, device=inputs.device)
            else:
                if (not isinstance(out, torch.Tensor) or tuple(out.shape) != (B, H, W, 3) or out.dtype != torch.float32
                        or out.device.type != "cuda" or out.device.index != dev or not out.is_contiguous()):
                    raise ValueError("out must be a contiguous float32 [B,H,W,3] tensor on cuda:%d" % dev)
                con = out
            stream = torch.cuda.current_stream().cuda_stream
            rc = self._lib.bsr_forward_rgb(self._handle, inputs.data_ptr(), uv.data_ptr(), B, H, W, con.data_ptr(), stream)
        _lib.check(rc, "bsr_forward_rgb")
        self._shape = (B, H, W)
        return con

    def reserve(self, B: int, H: int, W: int) -> None:
        """Allocate the workspace for forwards up to [B,H,W] now: later forwards of that size allocate nothing (bsr_reserve)."""
        self._require_weights()
        _lib.check(self._lib.bsr_reserve(self._handle, int(B), int(H), int(W)), "bsr_reserve")

    def workspace_bytes(self, B: int, H: int, W: int) -> int:
        return int(self._lib.bsr_handle_workspace_bytes(self._handle, int(B), int(H), int(W)))

    def call_tsm(self, *a, **k):
        raise TypeError("GeneratorRGB has no TSM forward")
