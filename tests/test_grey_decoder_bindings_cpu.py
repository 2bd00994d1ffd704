"""The device binding of the generator's grey decoder backward (grey_decoder_gpu.GreyDecoder) and its C entry points refuse bad
arguments before anything touches a GPU: the runner's image checks in their order, the sizes, the weights, the size queries and the
entry points' argument checks (all ahead of the device switch; no pointer is dereferenced).  Every text is asserted whole.  Everything
here runs on a CPU-only box; the GPU test holds the same refusals and that nothing was launched."""
import ctypes

import pytest
import torch

from blindshadowremoval_amd import _lib
from blindshadowremoval_amd.build import build_library
from blindshadowremoval_amd.grey_decoder_gpu import LAUNCHES, NO_WEIGHTS_TEXT, SIZE_TEXT, GreyDecoder
from on_dev0 import BSR_ERR_ARG, DEV, P, d0

SPEC = (("x", 257, 8), ("c2", 160, 4), ("c3", 128, 2), ("y", 64, 1), ("d_y", 64, 1))


def _images(b=1, h=32, w=256):
    return [d0(b, h // div, w // div, c) for _, c, div in SPEC]


def refused(runner, error, args):
    with pytest.raises(error) as e:
        runner.grey_decoder_grad(*args)
    assert type(e.value) is error
    return str(e.value)


def test_the_declaration():
    from blindshadowremoval_amd import GreyDecoder as exported
    from blindshadowremoval_amd.post_gpu import DENSE, STRIDED, GradStage
    assert exported is GreyDecoder and issubclass(GreyDecoder, GradStage)
    assert GreyDecoder.INPUTS == (("x", 257, 8, STRIDED), ("c2", 160, 4, STRIDED), ("c3", 128, 2, STRIDED), ("y", 64, 1, STRIDED), ("d_y", 64, 1, DENSE))
    assert GreyDecoder.LEAD == "d_y" and GreyDecoder.OUTPUTS == (("d_x", 257, 8), ("d_x3", 64, 4), ("d_x2", 64, 2))
    assert GreyDecoder.MULTIPLES == (32, 256) and GreyDecoder.TAKES_KEEP and GreyDecoder.KEPT == ("gz1", "gz2", "gz3")
    assert GreyDecoder.LAST == "last_grey_decoder" and GreyDecoder.SYMBOL == "bsr_grey_decoder_grad"
    assert [n for n, _ in LAUNCHES] == ["mask", "wgrad3", "dgrad3", "wgrad2", "dgrad2", "wgrad1", "dgrad1", "fold", "finish"]
    assert len(GreyDecoder.NAMES()) == 12


def test_runner_image_checks():
    runner = GreyDecoder(0)
    good = _images()
    for k, (name, c, div) in enumerate(SPEC):
        def swapped(t):
            return good[:k] + [t] + good[k + 1:]
        h, w = 32 // div, 256 // div
        for bad in (torch.zeros(1, h, w, c), d0(1, h, w, c, dtype=torch.float64), d0(1, h, w)):           # host, dtype, dims
            assert refused(runner, TypeError, swapped(bad)) == "%s must be a float32 tensor [B,.,.,%d] on %s" % (name, c, DEV)
        strided = d0(1, h, w, 2 * c)[..., ::2]
        assert tuple(strided.shape) == (1, h, w, c) and not strided.is_contiguous()
        assert refused(runner, ValueError, swapped(strided)) == "%s must be contiguous (NHWC, dense)" % name
        if name == "d_y":
            assert refused(runner, ValueError, swapped(d0(1, 32, 256, 65))) == "d_y must be [B,H,W,64], got (1, 32, 256, 65)"
            assert refused(runner, ValueError, swapped(d0(2, 32, 256, 64))) == "x must be [2,4,32,257] for this d_y, got (1, 4, 32, 257)"
        else:
            assert refused(runner, ValueError, swapped(d0(1, h, w, c + 1))) == "%s must be [1,%d,%d,%d] for this d_y, got (1, %d, %d, %d)" % (name, h, w, c, h, w, c + 1)
            assert refused(runner, ValueError, swapped(d0(2, h, w, c))) == "%s must be [1,%d,%d,%d] for this d_y, got (2, %d, %d, %d)" % (name, h, w, c, h, w, c)
    for b, h, w in ((1, 48, 256), (1, 32, 128), (1, 16, 256), (1, 32, 384)):
        assert refused(runner, ValueError, _images(b, h, w)) == SIZE_TEXT % (b, h, w)
    # a type mistake in an image comes before a size the chain does not take, and both before the weights
    assert refused(runner, TypeError, [torch.zeros(1, 6, 32, 257)] + _images(1, 48, 256)[1:]) == "x must be a float32 tensor [B,.,.,257] on %s" % (DEV,)
    assert refused(runner, ValueError, good) == NO_WEIGHTS_TEXT
    with pytest.raises(ValueError) as e:                 # the weights come before stop_after's range
        runner.stages(*good, 99)
    assert str(e.value) == NO_WEIGHTS_TEXT
    with pytest.raises(ValueError) as e:
        runner.backward(object(), good[4])
    assert str(e.value) == NO_WEIGHTS_TEXT
    assert runner._scratch is None and len(LAUNCHES) == 9


@pytest.fixture(scope="module")
def lib():
    build_library()            # no-op when the in-tree .so is fresh
    return _lib.load()


def test_size_queries(lib):
    assert lib.bsr_grey_decoder_grad_blob_bytes() == 803552 * 4
    assert lib.bsr_grey_decoder_grad_floats() == 388608
    assert [lib.bsr_grey_decoder_grad_var_offset(i) for i in range(12)] == [0, 222048, 222144, 222240, 222336, 314496, 314560, 314624, 314688, 388416,
                                                                           388480, 388544]
    size_max = ctypes.c_size_t(-1).value
    assert lib.bsr_grey_decoder_grad_var_offset(-1) == lib.bsr_grey_decoder_grad_var_offset(12) == size_max
    for b, h, w in ((0, 32, 256), (1, 48, 256), (1, 32, 128), (1, 0, 256), (1, 32, 0), (-1, 32, 256), (1 << 12, 1 << 8, 1 << 8)):
        assert lib.bsr_grey_decoder_grad_scratch_bytes(b, h, w, 0) == lib.bsr_grey_decoder_grad_scratch_bytes(b, h, w, 1) == 0, (b, h, w)
        assert [lib.bsr_grey_decoder_grad_partials(b, h, w, layer) for layer in (1, 2, 3)] == [0, 0, 0]
        assert lib.bsr_grey_decoder_grad_offset(b, h, w, 0) == size_max
    assert lib.bsr_grey_decoder_grad_offset(1, 32, 256, 9) == lib.bsr_grey_decoder_grad_offset(1, 32, 256, -1) == size_max
    assert lib.bsr_grey_decoder_grad_partials(1, 32, 256, 0) == lib.bsr_grey_decoder_grad_partials(1, 32, 256, 4) == 0
    # the scratch: per layer the partials, Wg and S, then gz1 and gz2; gz3 is the last part and there only with keep
    offs = [lib.bsr_grey_decoder_grad_offset(1, 32, 256, m) for m in range(9)]
    assert all(o % 256 == 0 for o in offs)
    gz1, gz2, gz3 = offs[:3]
    assert gz2 - gz1 == 8 * 64 * 96 * 4 and gz3 - gz2 == 16 * 128 * 64 * 4
    assert lib.bsr_grey_decoder_grad_scratch_bytes(1, 32, 256, 0) == gz3
    assert lib.bsr_grey_decoder_grad_scratch_bytes(1, 32, 256, 1) == gz3 + 32 * 256 * 64 * 4
    assert offs[3] == 1 * 9 * 96 * 288 * 4 + 1 * 3 * 256 * 8 and offs[6] - offs[3] == 9 * 96 * 257 * 8
    assert lib.bsr_grey_decoder_grad_scratch_bytes(32, 256, 256, 0) > lib.bsr_grey_decoder_grad_scratch_bytes(1, 32, 256, 0)


@pytest.mark.parametrize("B,H,W", ((1, 32, 256), (2, 64, 256), (3, 96, 256), (1, 32, 512), (8, 256, 256), (32, 256, 256), (64, 256, 512)))
def test_partials_follow_their_rule(lib, B, H, W):
    """P = min(cap, ceil(tiles / 3)) with 4 x 16 coarse tiles and caps 85, 51, 128: at the caps 9 P = 765 workgroups are three rounds of
    256 places, 10 P = 510 and 4 P = 512 one round of 512."""
    caps = (85, 51, 128)
    for layer in (1, 2, 3):
        tiles = B * ((H >> (4 - layer)) // 4) * ((W >> (4 - layer)) // 16)
        assert lib.bsr_grey_decoder_grad_partials(B, H, W, layer) == min(caps[layer - 1], -(-tiles // 3)), layer
    if (B, H, W) == (32, 256, 256):
        assert [lib.bsr_grey_decoder_grad_partials(B, H, W, layer) for layer in (1, 2, 3)] == [85, 51, 128]


SLOTS = "d_blob blob_bytes x x_cs c2 c2_cs c3 c3_cs y y_cs d_y B H W d_x d_x3 d_x2 grads keep scratch"
INTS = {"B": 2, "H": 32, "W": 256, "x_cs": 264, "c2_cs": 160, "c3_cs": 128, "y_cs": 64, "keep": 0, "stop_after": 1}


@pytest.mark.parametrize("fn", ("bsr_grey_decoder_grad", "bsr_debug_grey_decoder_grad"))
def test_entry_point_argument_checks(lib, fn):
    slots = (SLOTS + (" stop_after" if "debug" in fn else "")).split()

    def refused(**over):
        """The code and the text of the call with the named arguments replaced."""
        args = [0]
        for slot in slots:
            value = dict(INTS, blob_bytes=lib.bsr_grey_decoder_grad_blob_bytes()).get(slot, P)
            args.append(over.get(slot, value))
        assert set(over) <= set(slots)
        return getattr(lib, fn)(*args, None), lib.bsr_last_error().decode()

    def text(what):
        return (BSR_ERR_ARG, fn + ": " + what)

    required = [s for s in slots if s not in INTS and s != "blob_bytes"]
    assert required == ["d_blob", "x", "c2", "c3", "y", "d_y", "d_x", "d_x3", "d_x2", "grads", "scratch"]
    for slot in required:
        assert refused(**{slot: None}) == text("null argument"), slot
    size = "B must be positive, H a multiple of 32 and W a multiple of 256 (the generator's rule), at most 2^26 pixels in all"
    for over in (dict(B=0), dict(H=48), dict(W=128), dict(H=0), dict(B=1 << 12, H=1 << 8, W=1 << 8)):
        assert refused(**over) == text(size), over
    # a TSM blob (up1 291 wide) would be longer: any other length is refused with the text that says so
    assert refused(blob_bytes=lib.bsr_grey_decoder_grad_blob_bytes() + 9 * 96 * (291 - 257) * 4) == text(
        "blob_bytes must be bsr_grey_decoder_grad_blob_bytes() (pack.pack_grey_decoder_grad; the GSC width 257 only, not TSM's 291)")
    assert refused(x_cs=256) == text("x_cs must be at least 257")
    for over in (dict(c2_cs=156), dict(c2_cs=162), dict(c3_cs=124), dict(c3_cs=130), dict(y_cs=60), dict(y_cs=66)):
        assert refused(**over) == text("c2_cs, c3_cs, y_cs must be multiples of 4 and at least 160, 128, 64"), over
    for slot in ("d_blob", "c2", "c3", "y", "d_y", "d_x3", "d_x2"):
        assert refused(**{slot: P + 4}) == text("d_blob, c2, c3, y, d_y, d_x3 and d_x2 must be 16-byte aligned"), slot
    for slot in ("x", "d_x", "grads"):
        assert refused(**{slot: P + 2}) == text("x, d_x and grads must be 4-byte aligned"), slot
    assert refused(scratch=P + 8) == text("scratch must be 256-byte aligned")
    if "stop_after" in slots:
        for stop in (-1, 10):
            assert refused(stop_after=stop) == text("stop_after must be 0..9")


def test_last_grey_decoder_refuses_null_arguments(lib):
    shape = (ctypes.c_int * 4)()
    ptrs, cs = [ctypes.c_void_p() for _ in range(4)], [ctypes.c_int() for _ in range(4)]
    args = [ctypes.byref(v) for pair in zip(ptrs, cs) for v in pair]
    assert lib.bsr_last_grey_decoder(None, *args, ctypes.byref(shape)) == BSR_ERR_ARG
    assert lib.bsr_last_error().decode() == "bsr_last_grey_decoder: null argument"
    assert lib.bsr_abi_version() == 8
