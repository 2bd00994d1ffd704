"""The device binding of the backward of res_stack/5's lower half (bottleneck_grad_gpu.BottleneckGrad) and its C entry points refuse bad
arguments before anything touches a GPU: the runner's image checks in their order, the sizes, the weights, the size queries and the
entry points' argument checks (all ahead of the device switch; no pointer is dereferenced).  Every text is asserted whole.  Everything
here runs on a CPU-only box; the GPU test holds the same refusals and that nothing was launched."""
import ctypes

import pytest
import torch

from blindshadowremoval_amd import _lib
from blindshadowremoval_amd.bottleneck_grad_gpu import KEPT, LAUNCHES, NO_WEIGHTS_TEXT, SIZE_TEXT, BottleneckGrad
from blindshadowremoval_amd.build import build_library
from blindshadowremoval_amd.post_gpu import DENSE, OPTIONAL, STRIDED
from on_dev0 import BSR_ERR_ARG, DEV, P, d0

SPEC = (("xin", 261), ("d_y3", 257), ("d_skip", 261))


def _images(b=1, h=4, w=32):
    return [d0(b, h, w, c) for _, c in SPEC]


def refused(runner, error, args):
    with pytest.raises(error) as e:
        runner.bottleneck_grad(*args)
    assert type(e.value) is error
    return str(e.value)


def test_the_declaration():
    assert BottleneckGrad.INPUTS == (("xin", 261, 1, STRIDED), ("d_y3", 257, 1, DENSE), ("d_skip", 261, 1, OPTIONAL))
    assert BottleneckGrad.LEAD == "d_y3" and BottleneckGrad.OUTPUTS == (("d_xin", 261, 1),) and BottleneckGrad.MULTIPLES == (4, 32)
    assert BottleneckGrad.KEPT == KEPT == ("gz2", "gz1", "a1", "a2") and BottleneckGrad.LAST == "last_block5_input"
    assert BottleneckGrad.SYMBOL == "bsr_bottleneck_grad" and len(LAUNCHES) == 12


def test_runner_image_checks():
    runner = BottleneckGrad(0)
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
        if name == "d_y3":
            assert refused(runner, ValueError, swapped(d0(1, 4, 32, 258))) == "d_y3 must be [B,h,w,257], got (1, 4, 32, 258)"
            assert refused(runner, ValueError, swapped(d0(2, 4, 32, 257))) == "xin must be [2,4,32,261] for this d_y3, got (1, 4, 32, 261)"
        else:
            assert refused(runner, ValueError, swapped(d0(1, h, w, c + 1))) == "%s must be [1,%d,%d,%d] for this d_y3, got (1, %d, %d, %d)" % (name, h, w, c, h, w, c + 1)
            assert refused(runner, ValueError, swapped(d0(2, h, w, c))) == "%s must be [1,%d,%d,%d] for this d_y3, got (2, %d, %d, %d)" % (name, h, w, c, h, w, c)
    for b, h, w in ((1, 6, 32), (1, 4, 16), (1, 2, 32), (1, 4, 48)):
        assert refused(runner, ValueError, _images(b, h, w)) == SIZE_TEXT % (b, h, w)
        assert refused(runner, ValueError, _images(b, h, w)[:2]) == SIZE_TEXT % (b, h, w)                 # d_skip may be left out
    # a type mistake in an image comes before a size the chain does not take, and both before the weights
    assert refused(runner, TypeError, [torch.zeros(1, 6, 32, 261)] + _images(1, 6, 32)[1:]) == "xin must be a float32 tensor [B,h,w,261] on %s" % (DEV,)
    assert refused(runner, ValueError, good) == NO_WEIGHTS_TEXT
    assert refused(runner, ValueError, good[:2] + [None]) == NO_WEIGHTS_TEXT
    with pytest.raises(ValueError) as e:                 # the weights come before stop_after's range
        runner.stages(*good, 99)
    assert str(e.value) == NO_WEIGHTS_TEXT
    for d_skip in (good[2], None):
        with pytest.raises(ValueError) as e:
            runner.backward(object(), good[1], d_skip)
        assert str(e.value) == NO_WEIGHTS_TEXT
    with pytest.raises(TypeError) as e:                  # in place the dense inputs alone are checked, d_skip among them
        runner.backward(object(), good[1], torch.zeros(1, 4, 32, 261))
    assert str(e.value) == "d_skip must be a float32 tensor [B,h,w,261] on %s" % (DEV,)
    assert runner._scratch is None


@pytest.fixture(scope="module")
def lib():
    build_library()            # no-op when the in-tree .so is fresh
    return _lib.load()


def test_size_queries(lib):
    k2 = 9 * 128 * 128
    assert lib.bsr_bottleneck_grad_blob_bytes() == (272 * 128 + 128 + k2 + 128 + 272 * 128 + k2 + 128 * 384 + 261 * 128 + k2 + 128 * 257 + 8 * 128
                                                    + 4 * 257) * 4
    assert lib.bsr_bottleneck_grad_floats() == 215299
    assert [lib.bsr_bottleneck_grad_var_offset(i) for i in range(12)] == [0, 33408, 33536, 180992, 181120, 214016, 214273, 214401, 214529, 214657,
                                                                          214785, 215042]
    size_max = ctypes.c_size_t(-1).value
    assert lib.bsr_bottleneck_grad_var_offset(-1) == lib.bsr_bottleneck_grad_var_offset(12) == size_max
    for b, h, w in ((0, 4, 32), (1, 6, 32), (1, 4, 16), (1, 0, 32), (1, 4, 0), (-1, 4, 32), (1 << 10, 1 << 6, 1 << 6)):
        assert lib.bsr_bottleneck_grad_scratch_bytes(b, h, w) == 0, (b, h, w)
        assert lib.bsr_bottleneck_grad_partials(b, h, w) == 0
        assert lib.bsr_bottleneck_grad_offset(b, h, w, 0) == size_max
    assert lib.bsr_bottleneck_grad_offset(1, 4, 32, 8) == lib.bsr_bottleneck_grad_offset(1, 4, 32, -1) == size_max
    # one row slice per 128 pixels, at most 64
    for (b, h, w), want in (((1, 4, 32), 1), ((2, 8, 32), 4), ((3, 12, 32), 9), ((1, 4, 64), 2), ((1, 32, 32), 8), ((32, 32, 32), 64)):
        assert lib.bsr_bottleneck_grad_partials(b, h, w) == want, (b, h, w)
    # the scratch: xin, d_y3 [N][272], a1, a2, gz2, gz1 [N][128], Wg, S
    offs = [lib.bsr_bottleneck_grad_offset(1, 4, 32, m) for m in range(8)]
    assert all(o % 256 == 0 for o in offs) and offs[0] == 0
    n = 128
    assert [b - a for a, b in zip(offs, offs[1:])] == [n * 272 * 4, n * 272 * 4, n * 128 * 4, n * 128 * 4, n * 128 * 4, n * 128 * 4,
                                                      (261 * 128 + k2 + 128 * 257) * 8]
    assert lib.bsr_bottleneck_grad_scratch_bytes(1, 4, 32) > offs[7] + 513 * 8
    assert lib.bsr_bottleneck_grad_scratch_bytes(32, 32, 32) > lib.bsr_bottleneck_grad_scratch_bytes(1, 4, 32)


SLOTS = "d_blob blob_bytes xin xin_cs d_y3 d_skip B h w d_xin grads scratch"
INTS = {"B": 2, "h": 4, "w": 32, "xin_cs": 264, "stop_after": 1}


@pytest.mark.parametrize("fn", ("bsr_bottleneck_grad", "bsr_debug_bottleneck_grad"))
def test_entry_point_argument_checks(lib, fn):
    slots = (SLOTS + (" stop_after" if "debug" in fn else "")).split()

    def refused(**over):
        """The code and the text of the call with the named arguments replaced."""
        args = [0]
        for slot in slots:
            value = dict(INTS, blob_bytes=lib.bsr_bottleneck_grad_blob_bytes()).get(slot, P)
            args.append(over.get(slot, value))
        assert set(over) <= set(slots)
        return getattr(lib, fn)(*args, None), lib.bsr_last_error().decode()

    def text(what):
        return (BSR_ERR_ARG, fn + ": " + what)

    for slot in ("d_blob", "xin", "d_y3", "d_xin", "grads", "scratch"):             # d_skip may be null
        assert refused(**{slot: None}) == text("null argument"), slot
    size = "B must be positive, h a multiple of 4 and w a multiple of 32 (the generator's rule at 1/8 resolution), at most 2^21 pixels in all"
    for over in (dict(B=0), dict(h=6), dict(w=16), dict(h=0), dict(B=1 << 10, h=1 << 6, w=1 << 6)):
        assert refused(**over) == text(size), over
        assert refused(d_skip=None, **over) == text(size), over
    assert refused(blob_bytes=lib.bsr_bottleneck_grad_blob_bytes() + 4) == text(
        "blob_bytes must be bsr_bottleneck_grad_blob_bytes() (pack.pack_bottleneck_grad; the GSC width 261 only, not TSM's 877)")
    assert refused(xin_cs=260) == text("xin_cs must be at least 261")
    assert refused(d_blob=P + 4) == text("d_blob must be 16-byte aligned")
    for slot in ("xin", "d_y3", "d_skip", "d_xin", "grads"):
        assert refused(**{slot: P + 2}) == text("xin, d_y3, d_skip, d_xin and grads must be 4-byte aligned"), slot
    assert refused(scratch=P + 8) == text("scratch must be 256-byte aligned")
    if "stop_after" in slots:
        for stop in (-1, 13):
            assert refused(stop_after=stop) == text("stop_after must be 0..12")


def test_the_command_refuses_bottleneck_without_nonlocal(capsys):
    from blindshadowremoval_amd import BottleneckGrad as exported
    from blindshadowremoval_amd import objective
    assert exported is BottleneckGrad
    with pytest.raises(SystemExit):
        objective.main(["nowhere", "--vgg", "none.npz", "--grad-total", "--tail", "--decoder", "--bottleneck"])
    assert "--bottleneck goes with --grad-total --tail --decoder --nonlocal" in capsys.readouterr().err
    with pytest.raises(ValueError, match="--bottleneck goes with --grad-total --tail --decoder --nonlocal"):
        objective.score_folder("nowhere", "none.npz", grad_total=True, tail=True, decoder=True, bottleneck=True)
    names = objective.bottleneck_grad_names()
    assert len(names) == 26 and names[:4] == ["d_xin_l1", "d_xin_linf", "res_stack/5/conv1/kernel_l1", "res_stack/5/conv1/kernel_linf"]
    assert objective.STAGES == ("tail", "decoder", "nonlocal", "bottleneck")
