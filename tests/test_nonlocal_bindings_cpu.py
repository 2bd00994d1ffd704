"""The device binding of the backward of res_stack/5's upper half (nonlocal_grad_gpu.NonLocalGrad) and its C entry points refuse bad
arguments before anything touches a GPU: the runner's image checks in their order, the sizes, the weights, the size queries and the
entry points' argument checks (all ahead of the device switch; no pointer is dereferenced).  Every text is asserted whole.  Everything
here runs on a CPU-only box; the GPU test holds the same refusals and that nothing was launched."""
import ctypes

import pytest
import torch

from blindshadowremoval_amd import _lib
from blindshadowremoval_amd.build import build_library
from blindshadowremoval_amd.nonlocal_grad_gpu import LAUNCHES, NO_WEIGHTS_TEXT, SIZE_TEXT, NonLocalGrad
from on_dev0 import BSR_ERR_ARG, DEV, P, d0

SPEC = (("y3x", 257), ("xin", 261), ("out", 261), ("d_out", 261))


def _images(b=1, h=4, w=32):
    return [d0(b, h, w, c) for _, c in SPEC]


def refused(runner, error, args):
    with pytest.raises(error) as e:
        runner.nonlocal_grad(*args)
    assert type(e.value) is error
    return str(e.value)


def test_runner_image_checks():
    runner = NonLocalGrad(0)
    good = _images()
    h, w = 4, 32
    for k, (name, c) in enumerate(SPEC):
        def swapped(t):
            return good[:k] + [t] + good[k + 1:]
        for bad in (torch.zeros(1, h, w, c), d0(1, h, w, c, dtype=torch.float64), d0(1, h, w)):           # host, dtype, dims
            assert refused(runner, TypeError, swapped(bad)) == "%s must be a float32 tensor [B,h,w,%d] on %s" % (name, c, DEV)
        strided = d0(1, h, w, 2 * c)[..., ::2]
        assert tuple(strided.shape) == (1, h, w, c) and not strided.is_contiguous()
        assert refused(runner, ValueError, swapped(strided)) == "%s must be contiguous (NHWC, dense)" % name
        if name == "d_out":
            assert refused(runner, ValueError, swapped(d0(1, 4, 32, 262))) == "d_out must be [B,h,w,261], got (1, 4, 32, 262)"
            assert refused(runner, ValueError, swapped(d0(2, 4, 32, 261))) == "y3x must be [2,4,32,257] for this d_out, got (1, 4, 32, 257)"
        else:
            assert refused(runner, ValueError, swapped(d0(1, h, w, c + 1))) == "%s must be [1,%d,%d,%d] for this d_out, got (1, %d, %d, %d)" % (name, h, w, c, h, w, c + 1)
            assert refused(runner, ValueError, swapped(d0(2, h, w, c))) == "%s must be [1,%d,%d,%d] for this d_out, got (2, %d, %d, %d)" % (name, h, w, c, h, w, c)
    for b, h, w in ((1, 6, 32), (1, 4, 16), (1, 2, 32), (1, 4, 48)):
        assert refused(runner, ValueError, _images(b, h, w)) == SIZE_TEXT % (b, h, w)
    # a type mistake in an image comes before a size the chain does not take, and both before the weights
    assert refused(runner, TypeError, [torch.zeros(1, 6, 32, 257)] + _images(1, 6, 32)[1:]) == "y3x must be a float32 tensor [B,h,w,257] on %s" % (DEV,)
    assert refused(runner, ValueError, good) == NO_WEIGHTS_TEXT
    with pytest.raises(ValueError) as e:                 # the weights come before stop_after's range
        runner.stages(*good, 99)
    assert str(e.value) == NO_WEIGHTS_TEXT
    with pytest.raises(ValueError) as e:
        runner.backward(object(), good[3])
    assert str(e.value) == NO_WEIGHTS_TEXT
    assert runner._scratch is None and len(LAUNCHES) == 12


@pytest.fixture(scope="module")
def lib():
    build_library()            # no-op when the in-tree .so is fresh
    return _lib.load()


def test_size_queries(lib):
    assert lib.bsr_nonlocal_grad_blob_bytes() == (272 * 384 + 384 + 272 * 128 + 384 * 384 + 128 * 257 + 4 * 257) * 4
    assert lib.bsr_nonlocal_grad_floats() == 132739
    assert [lib.bsr_nonlocal_grad_var_offset(i) for i in range(10)] == [0, 32896, 33024, 65920, 66048, 98944, 99072, 131968, 132225, 132482]
    size_max = ctypes.c_size_t(-1).value
    assert lib.bsr_nonlocal_grad_var_offset(-1) == lib.bsr_nonlocal_grad_var_offset(10) == size_max
    for b, h, w in ((0, 4, 32), (1, 6, 32), (1, 4, 16), (1, 0, 32), (1, 4, 0), (-1, 4, 32), (1 << 10, 1 << 6, 1 << 6)):
        assert lib.bsr_nonlocal_grad_scratch_bytes(b, h, w) == 0, (b, h, w)
        assert lib.bsr_nonlocal_grad_partials(b, h, w) == 0
        assert lib.bsr_nonlocal_grad_offset(b, h, w, 0) == size_max
    assert lib.bsr_nonlocal_grad_offset(1, 4, 32, 10) == lib.bsr_nonlocal_grad_offset(1, 4, 32, -1) == size_max
    # one row slice per 128 tokens, at most 64
    for (b, h, w), want in (((1, 4, 32), 1), ((2, 8, 32), 4), ((3, 12, 32), 9), ((1, 4, 64), 2), ((1, 32, 32), 8), ((32, 32, 32), 64)):
        assert lib.bsr_nonlocal_grad_partials(b, h, w) == want, (b, h, w)
    # the scratch: y3, dz [N][272], theta | phi | g [N][384], A [N][128], (m, r) [N][2], dA [N][128], D [N], the three gradients [N][384], Wgd, Sz
    offs = [lib.bsr_nonlocal_grad_offset(1, 4, 32, m) for m in range(10)]
    assert all(o % 256 == 0 for o in offs) and offs[0] == 0
    n = 128
    assert [b - a for a, b in zip(offs, offs[1:])] == [n * 272 * 4, n * 272 * 4, n * 384 * 4, n * 128 * 4, n * 2 * 4, n * 128 * 4, n * 4, n * 384 * 4,
                                                      128 * 257 * 8]
    assert lib.bsr_nonlocal_grad_scratch_bytes(1, 4, 32) > offs[9] + 257 * 8
    assert lib.bsr_nonlocal_grad_scratch_bytes(32, 32, 32) > lib.bsr_nonlocal_grad_scratch_bytes(1, 4, 32)


SLOTS = "d_blob blob_bytes y3x y3x_cs xin xin_cs out out_cs d_out B h w d_y3 d_skip grads scratch"
INTS = {"B": 2, "h": 4, "w": 32, "y3x_cs": 288, "xin_cs": 264, "out_cs": 264, "stop_after": 1}


@pytest.mark.parametrize("fn", ("bsr_nonlocal_grad", "bsr_debug_nonlocal_grad"))
def test_entry_point_argument_checks(lib, fn):
    slots = (SLOTS + (" stop_after" if "debug" in fn else "")).split()

    def refused(**over):
        """The code and the text of the call with the named arguments replaced."""
        args = [0]
        for slot in slots:
            value = dict(INTS, blob_bytes=lib.bsr_nonlocal_grad_blob_bytes()).get(slot, P)
            args.append(over.get(slot, value))
        assert set(over) <= set(slots)
        return getattr(lib, fn)(*args, None), lib.bsr_last_error().decode()

    def text(what):
        return (BSR_ERR_ARG, fn + ": " + what)

    required = [s for s in slots if s not in INTS and s != "blob_bytes"]
    assert required == ["d_blob", "y3x", "xin", "out", "d_out", "d_y3", "d_skip", "grads", "scratch"]
    for slot in required:
        assert refused(**{slot: None}) == text("null argument"), slot
    size = "B must be positive, h a multiple of 4 and w a multiple of 32 (the generator's rule at 1/8 resolution), at most 2^21 tokens in all"
    for over in (dict(B=0), dict(h=6), dict(w=16), dict(h=0), dict(B=1 << 10, h=1 << 6, w=1 << 6)):
        assert refused(**over) == text(size), over
    # a blob of any other length is refused with the text that says so
    assert refused(blob_bytes=lib.bsr_nonlocal_grad_blob_bytes() + 4) == text(
        "blob_bytes must be bsr_nonlocal_grad_blob_bytes() (pack.pack_nonlocal_grad; the GSC width 261 only, not TSM's 877)")
    for over in (dict(y3x_cs=256), dict(xin_cs=260), dict(out_cs=260)):
        assert refused(**over) == text("y3x_cs must be at least 257, xin_cs and out_cs at least 261"), over
    assert refused(d_blob=P + 4) == text("d_blob must be 16-byte aligned")
    for slot in ("y3x", "xin", "out", "d_out", "d_y3", "d_skip", "grads"):
        assert refused(**{slot: P + 2}) == text("y3x, xin, out, d_out, d_y3, d_skip and grads must be 4-byte aligned"), slot
    assert refused(scratch=P + 8) == text("scratch must be 256-byte aligned")
    if "stop_after" in slots:
        for stop in (-1, 13):
            assert refused(stop_after=stop) == text("stop_after must be 0..12")


def test_last_block5_refuses_null_arguments(lib):
    shape, y_cs, x_cs = (ctypes.c_int * 4)(), ctypes.c_int(), ctypes.c_int()
    ptrs = [ctypes.c_void_p() for _ in range(3)]
    assert lib.bsr_last_block5(None, ctypes.byref(ptrs[0]), ctypes.byref(y_cs), ctypes.byref(ptrs[1]), ctypes.byref(ptrs[2]), ctypes.byref(x_cs),
                               ctypes.byref(shape)) == BSR_ERR_ARG
    assert lib.bsr_last_error().decode() == "bsr_last_block5: null argument"


def test_the_command_refuses_nonlocal_without_decoder(capsys):
    from blindshadowremoval_amd import NonLocalGrad as exported
    from blindshadowremoval_amd import objective
    assert exported is NonLocalGrad
    with pytest.raises(SystemExit):
        objective.main(["nowhere", "--vgg", "none.npz", "--grad-total", "--tail", "--nonlocal"])
    assert "--nonlocal goes with --grad-total --tail --decoder" in capsys.readouterr().err
    with pytest.raises(ValueError, match="--nonlocal goes with --grad-total --tail --decoder"):
        objective.score_folder("nowhere", "none.npz", grad_total=True, tail=True, nonlocal_=True)
    names = objective.nonlocal_grad_names()
    assert len(names) == 24 and names[:4] == ["d_y3_l1", "d_y3_linf", "d_skip_l1", "d_skip_linf"]
