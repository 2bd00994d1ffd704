"""The device binding of the generator's colour tail backward (clr_tail_gpu.ColourTail) and its C entry points refuse bad arguments
before anything touches a GPU: the runner's image checks in their order, the sizes, the weights, the size queries and the entry points'
argument checks (all ahead of the device switch; no pointer is dereferenced).  Every text is asserted whole.  Everything here runs on a
CPU-only box; the GPU test holds the same refusals and that nothing was launched."""
import ctypes

import pytest
import torch

from blindshadowremoval_amd import _lib
from blindshadowremoval_amd.build import build_library
from blindshadowremoval_amd.clr_tail_gpu import LAUNCHES, NO_WEIGHTS_TEXT, SIZE_TEXT, ColourTail
from on_dev0 import BSR_ERR_ARG, DEV, P, d0

SPEC = (("gs", 1), ("f", 64), ("g_con", 3), ("g_gs", 1))


def _images(b=1, h=8, w=32):
    return [d0(b, h, w, c) for _, c in SPEC]


def refused(runner, error, args):
    with pytest.raises(error) as e:
        runner.tail_grad(*args)
    assert type(e.value) is error
    return str(e.value)


def test_runner_image_checks():
    runner = ColourTail(0)
    good = _images()
    for k, (name, c) in enumerate(SPEC):
        def swapped(t):
            return good[:k] + [t] + good[k + 1:]
        for bad in (torch.zeros(1, 8, 32, c), d0(1, 8, 32, c, dtype=torch.float64), d0(1, 8, 32)):           # host, dtype, dims
            assert refused(runner, TypeError, swapped(bad)) == "%s must be a float32 tensor [B,H,W,%d] on %s" % (name, c, DEV)
        strided = d0(1, 8, 32, 2 * c)[..., ::2]
        assert tuple(strided.shape) == (1, 8, 32, c) and not strided.is_contiguous()
        assert refused(runner, ValueError, swapped(strided)) == "%s must be contiguous (NHWC, dense)" % name
        if name == "gs":
            assert refused(runner, ValueError, swapped(d0(1, 8, 32, 2))) == "gs must be [B,H,W,1], got (1, 8, 32, 2)"
            assert refused(runner, ValueError, swapped(d0(2, 8, 32, 1))) == "f must be [2,8,32,64] like gs, got (1, 8, 32, 64)"
        else:
            assert refused(runner, ValueError, swapped(d0(1, 8, 32, c + 1))) == "%s must be [1,8,32,%d] like gs, got (1, 8, 32, %d)" % (name, c, c + 1)
            assert refused(runner, ValueError, swapped(d0(2, 8, 32, c))) == "%s must be [1,8,32,%d] like gs, got (2, 8, 32, %d)" % (name, c, c)
    for b, h, w in ((1, 12, 32), (1, 8, 48), (0, 8, 32), (1, 4, 32)):
        assert refused(runner, ValueError, _images(b, h, w)) == SIZE_TEXT % (b, h, w)
    # a type mistake in a later image comes before a size the chain does not take, and both before the weights
    assert refused(runner, TypeError, _images(1, 12, 32)[:-1] + [torch.zeros(1, 12, 32, 1)]) == "g_gs must be a float32 tensor [B,H,W,1] on %s" % (DEV,)
    assert refused(runner, ValueError, good) == NO_WEIGHTS_TEXT
    assert refused(runner, ValueError, good[:3] + [None]) == NO_WEIGHTS_TEXT
    with pytest.raises(ValueError) as e:                 # the weights come before stop_after's range
        runner.stages(*good, 99)
    assert str(e.value) == NO_WEIGHTS_TEXT
    with pytest.raises(ValueError) as e:
        runner.backward(object(), good[0], good[2], good[3])
    assert str(e.value) == NO_WEIGHTS_TEXT
    assert runner._scratch is None and len(LAUNCHES) == 6


@pytest.fixture(scope="module")
def lib():
    build_library()            # no-op when the in-tree .so is fresh
    return _lib.load()


def test_size_queries(lib):
    assert lib.bsr_clr_tail_grad_blob_bytes() == 30080 * 4
    assert lib.bsr_clr_tail_grad_floats() == 9763
    assert [lib.bsr_clr_tail_grad_var_offset(i) for i in range(10)] == [0, 9360, 9376, 9392, 9408, 9664, 9680, 9696, 9712, 9760]
    size_max = ctypes.c_size_t(-1).value
    assert lib.bsr_clr_tail_grad_var_offset(-1) == lib.bsr_clr_tail_grad_var_offset(10) == size_max
    for b, h, w in ((0, 8, 32), (1, 12, 32), (1, 8, 48), (1, 0, 32), (1, 8, 0), (-1, 8, 32), (1 << 12, 1 << 8, 1 << 8)):
        assert lib.bsr_clr_tail_grad_scratch_bytes(b, h, w) == 0, (b, h, w)
        assert lib.bsr_clr_tail_grad_partials(b, h, w) == 0
        assert lib.bsr_clr_tail_grad_offset(b, h, w, 0) == size_max
    # three maps of 16 floats a pixel, then the partials: one workgroup each at one tile
    maps = 8 * 32 * 16 * 4
    assert [lib.bsr_clr_tail_grad_offset(1, 8, 32, m) for m in range(4)] == [0, maps, 2 * maps, 3 * maps]
    assert lib.bsr_clr_tail_grad_offset(1, 8, 32, 7) == lib.bsr_clr_tail_grad_offset(1, 8, 32, -1) == size_max
    assert lib.bsr_clr_tail_grad_scratch_bytes(1, 8, 32) == 3 * maps + 2816 + 4 * 160 * 16 * 4 + 75008 + 2816      # each part rounded up to 256 bytes
    assert [lib.bsr_clr_tail_grad_partials(b, h, w) for b, h, w in ((1, 8, 32), (2, 16, 64), (3, 24, 96), (1, 32, 256), (32, 256, 256))] == [1, 2, 7, 8, 160]
    assert lib.bsr_clr_tail_grad_scratch_bytes(32, 256, 256) > lib.bsr_clr_tail_grad_scratch_bytes(1, 32, 256) > 0


SLOTS = "d_blob blob_bytes gs f f_cs g_con g_gs? B H W d_f d_gs grads keep scratch"


@pytest.mark.parametrize("fn", ("bsr_clr_tail_grad", "bsr_debug_clr_tail_grad"))
def test_entry_point_argument_checks(lib, fn):
    slots = (SLOTS + (" stop_after" if "debug" in fn else "")).split()

    def refused(**over):
        """The code and the text of the call with the named arguments replaced."""
        args = [0]
        for slot in slots:
            value = {"B": 2, "H": 8, "W": 32, "f_cs": 64, "keep": 0, "stop_after": 1, "blob_bytes": lib.bsr_clr_tail_grad_blob_bytes()}.get(
                slot, None if slot.endswith("?") else P)
            args.append(over.get(slot.rstrip("?"), value))
        assert set(over) <= set(s.rstrip("?") for s in slots)
        return getattr(lib, fn)(*args, None), lib.bsr_last_error().decode()

    def text(what):
        return (BSR_ERR_ARG, fn + ": " + what)

    required = [s for s in slots if not s.endswith("?") and s not in ("B", "H", "W", "f_cs", "keep", "stop_after", "blob_bytes")]
    assert required == ["d_blob", "gs", "f", "g_con", "d_f", "d_gs", "grads", "scratch"]
    for slot in required:
        assert refused(**{slot: None}) == text("null argument"), slot
    size = "B must be positive, H a multiple of 8 and W a multiple of 32 (conv_n16_kernel's tile), at most 2^26 pixels in all"
    for over in (dict(B=0), dict(H=12), dict(W=48), dict(H=0), dict(B=1 << 12, H=1 << 8, W=1 << 8)):
        assert refused(**over) == text(size), over
    assert refused(blob_bytes=lib.bsr_clr_tail_grad_blob_bytes() - 4) == text("blob_bytes must be bsr_clr_tail_grad_blob_bytes() (pack.pack_clr_tail_grad)")
    for f_cs in (63, 0, 66):
        assert refused(f_cs=f_cs) == text("f_cs must be a multiple of 4 and at least 64")
    for slot in ("d_blob", "f", "d_f"):
        assert refused(**{slot: P + 4}) == text("d_blob, f and d_f must be 16-byte aligned"), slot
    for slot in ("gs", "g_con", "g_gs", "d_gs", "grads"):
        assert refused(**{slot: P + 2}) == text("gs, g_con, g_gs, d_gs and grads must be 4-byte aligned"), slot
    assert refused(scratch=P + 8) == text("scratch must be 256-byte aligned")
    if "stop_after" in slots:
        for stop in (-1, 7):
            assert refused(stop_after=stop) == text("stop_after must be 0..6")


def test_last_f_refuses_null_arguments(lib):
    shape, cs, ptr = (ctypes.c_int * 4)(), ctypes.c_int(), ctypes.c_void_p()
    assert lib.bsr_last_f(None, ctypes.byref(ptr), ctypes.byref(cs), ctypes.byref(shape)) == BSR_ERR_ARG
    assert lib.bsr_last_error().decode() == "bsr_last_f: null argument"
