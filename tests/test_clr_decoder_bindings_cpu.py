"""The device binding of the generator's colour decoder backward (clr_decoder_gpu.ColourDecoder) and its C entry points refuse bad
arguments before anything touches a GPU: the runner's image checks in their order, the sizes, the weights, the size queries and the
entry points' argument checks (all ahead of the device switch; no pointer is dereferenced).  Every text is asserted whole.  Everything
here runs on a CPU-only box; the GPU test holds the same refusals and that nothing was launched."""
import ctypes

import pytest
import torch

from blindshadowremoval_amd import _lib
from blindshadowremoval_amd.build import build_library
from blindshadowremoval_amd.clr_decoder_gpu import LAUNCHES, NO_WEIGHTS_TEXT, SIZE_TEXT, ColourDecoder
from on_dev0 import BSR_ERR_ARG, DEV, P, d0

SPEC = (("x", 261, 8), ("f1", 128, 4), ("f2", 96, 2), ("f", 64, 1), ("d_f", 64, 1))


def _images(b=1, h=32, w=256):
    return [d0(b, h // div, w // div, c) for _, c, div in SPEC]


def refused(runner, error, args):
    with pytest.raises(error) as e:
        runner.decoder_grad(*args)
    assert type(e.value) is error
    return str(e.value)


def test_runner_image_checks():
    runner = ColourDecoder(0)
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
        if name == "d_f":
            assert refused(runner, ValueError, swapped(d0(1, 32, 256, 65))) == "d_f must be [B,H,W,64], got (1, 32, 256, 65)"
            assert refused(runner, ValueError, swapped(d0(2, 32, 256, 64))) == "x must be [2,4,32,261] for this d_f, got (1, 4, 32, 261)"
        else:
            assert refused(runner, ValueError, swapped(d0(1, h, w, c + 1))) == "%s must be [1,%d,%d,%d] for this d_f, got (1, %d, %d, %d)" % (name, h, w, c, h, w, c + 1)
            assert refused(runner, ValueError, swapped(d0(2, h, w, c))) == "%s must be [1,%d,%d,%d] for this d_f, got (2, %d, %d, %d)" % (name, h, w, c, h, w, c)
    for b, h, w in ((1, 48, 256), (1, 32, 128), (1, 16, 256), (1, 32, 384)):
        assert refused(runner, ValueError, _images(b, h, w)) == SIZE_TEXT % (b, h, w)
    # a type mistake in an image comes before a size the chain does not take, and both before the weights
    assert refused(runner, TypeError, [torch.zeros(1, 6, 32, 261)] + _images(1, 48, 256)[1:]) == "x must be a float32 tensor [B,.,.,261] on %s" % (DEV,)
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
    assert lib.bsr_clr_decoder_grad_blob_bytes() == 965376 * 4
    assert lib.bsr_clr_decoder_grad_floats() == 467424
    assert [lib.bsr_clr_decoder_grad_var_offset(i) for i in range(12)] == [0, 300672, 300800, 300928, 301056, 411648, 411744, 411840, 411936, 467232,
                                                                          467296, 467360]
    size_max = ctypes.c_size_t(-1).value
    assert lib.bsr_clr_decoder_grad_var_offset(-1) == lib.bsr_clr_decoder_grad_var_offset(12) == size_max
    for b, h, w in ((0, 32, 256), (1, 48, 256), (1, 32, 128), (1, 0, 256), (1, 32, 0), (-1, 32, 256), (1 << 12, 1 << 8, 1 << 8)):
        assert lib.bsr_clr_decoder_grad_scratch_bytes(b, h, w, 0) == lib.bsr_clr_decoder_grad_scratch_bytes(b, h, w, 1) == 0, (b, h, w)
        assert [lib.bsr_clr_decoder_grad_partials(b, h, w, layer) for layer in (1, 2, 3)] == [0, 0, 0]
        assert lib.bsr_clr_decoder_grad_offset(b, h, w, 0) == size_max
    assert lib.bsr_clr_decoder_grad_offset(1, 32, 256, 9) == lib.bsr_clr_decoder_grad_offset(1, 32, 256, -1) == size_max
    assert lib.bsr_clr_decoder_grad_partials(1, 32, 256, 0) == lib.bsr_clr_decoder_grad_partials(1, 32, 256, 4) == 0
    # P = min(cap, ceil(tiles / 3)) with 4 x 16 coarse tiles and caps 64, 85, 256
    for (b, h, w), want in (((1, 32, 256), [1, 3, 11]), ((2, 64, 256), [3, 11, 43]), ((3, 96, 256), [6, 24, 96]), ((1, 32, 512), [2, 6, 22]),
                            ((32, 256, 256), [64, 85, 256])):
        assert [lib.bsr_clr_decoder_grad_partials(b, h, w, layer) for layer in (1, 2, 3)] == want, (b, h, w)
    # the scratch: per layer the partials, Wg and S, then gz1 and gz2; gz3 is the last part and there only with keep
    offs = [lib.bsr_clr_decoder_grad_offset(1, 32, 256, m) for m in range(9)]
    assert all(o % 256 == 0 for o in offs)
    gz1, gz2, gz3 = offs[:3]
    assert gz2 - gz1 == 8 * 64 * 128 * 4 and gz3 - gz2 == 16 * 128 * 96 * 4
    assert lib.bsr_clr_decoder_grad_scratch_bytes(1, 32, 256, 0) == gz3
    assert lib.bsr_clr_decoder_grad_scratch_bytes(1, 32, 256, 1) == gz3 + 32 * 256 * 64 * 4
    assert offs[3] == 1 * 9 * 128 * 288 * 4 + 1 * 4 * 256 * 8 and offs[6] - offs[3] == 9 * 128 * 261 * 8
    assert lib.bsr_clr_decoder_grad_scratch_bytes(32, 256, 256, 0) > lib.bsr_clr_decoder_grad_scratch_bytes(1, 32, 256, 0)


SLOTS = "d_blob blob_bytes x x_cs f1 f1_cs f2 f2_cs f f_cs d_f B H W d_x grads keep scratch"
INTS = {"B": 2, "H": 32, "W": 256, "x_cs": 264, "f1_cs": 128, "f2_cs": 96, "f_cs": 64, "keep": 0, "stop_after": 1}


@pytest.mark.parametrize("fn", ("bsr_clr_decoder_grad", "bsr_debug_clr_decoder_grad"))
def test_entry_point_argument_checks(lib, fn):
    slots = (SLOTS + (" stop_after" if "debug" in fn else "")).split()

    def refused(**over):
        """The code and the text of the call with the named arguments replaced."""
        args = [0]
        for slot in slots:
            value = dict(INTS, blob_bytes=lib.bsr_clr_decoder_grad_blob_bytes()).get(slot, P)
            args.append(over.get(slot, value))
        assert set(over) <= set(slots)
        return getattr(lib, fn)(*args, None), lib.bsr_last_error().decode()

    def text(what):
        return (BSR_ERR_ARG, fn + ": " + what)

    required = [s for s in slots if s not in INTS and s != "blob_bytes"]
    assert required == ["d_blob", "x", "f1", "f2", "f", "d_f", "d_x", "grads", "scratch"]
    for slot in required:
        assert refused(**{slot: None}) == text("null argument"), slot
    size = "B must be positive, H a multiple of 32 and W a multiple of 256 (the generator's rule), at most 2^26 pixels in all"
    for over in (dict(B=0), dict(H=48), dict(W=128), dict(H=0), dict(B=1 << 12, H=1 << 8, W=1 << 8)):
        assert refused(**over) == text(size), over
    # a TSM blob (clr_up1 877 wide) would be longer: any other length is refused with the text that says so
    assert refused(blob_bytes=lib.bsr_clr_decoder_grad_blob_bytes() + 9 * 128 * (877 - 261) * 4) == text(
        "blob_bytes must be bsr_clr_decoder_grad_blob_bytes() (pack.pack_clr_decoder_grad; the GSC width 261 only, not TSM's 877)")
    assert refused(x_cs=260) == text("x_cs must be at least 261")
    for over in (dict(f1_cs=127), dict(f1_cs=130), dict(f2_cs=92), dict(f2_cs=98), dict(f_cs=60), dict(f_cs=66)):
        assert refused(**over) == text("f1_cs, f2_cs, f_cs must be multiples of 4 and at least 128, 96, 64"), over
    for slot in ("d_blob", "f1", "f2", "f", "d_f"):
        assert refused(**{slot: P + 4}) == text("d_blob, f1, f2, f and d_f must be 16-byte aligned"), slot
    for slot in ("x", "d_x", "grads"):
        assert refused(**{slot: P + 2}) == text("x, d_x and grads must be 4-byte aligned"), slot
    assert refused(scratch=P + 8) == text("scratch must be 256-byte aligned")
    if "stop_after" in slots:
        for stop in (-1, 10):
            assert refused(stop_after=stop) == text("stop_after must be 0..9")


def test_last_decoder_refuses_null_arguments(lib):
    shape, cs = (ctypes.c_int * 4)(), ctypes.c_int()
    ptrs = [ctypes.c_void_p() for _ in range(4)]
    assert lib.bsr_last_decoder(None, ctypes.byref(ptrs[0]), ctypes.byref(cs), ctypes.byref(ptrs[1]), ctypes.byref(ptrs[2]), ctypes.byref(ptrs[3]),
                                ctypes.byref(shape)) == BSR_ERR_ARG
    assert lib.bsr_last_error().decode() == "bsr_last_decoder: null argument"


def test_the_command_refuses_decoder_without_tail(capsys):
    from blindshadowremoval_amd import objective
    with pytest.raises(SystemExit):
        objective.main(["nowhere", "--vgg", "none.npz", "--grad-total", "--decoder"])
    assert "--decoder goes with --grad-total --tail" in capsys.readouterr().err
    with pytest.raises(ValueError, match="--decoder goes with --grad-total --tail"):
        objective.score_folder("nowhere", "none.npz", grad_total=True, decoder=True)
    assert len(objective.decoder_grad_names()) == 26
