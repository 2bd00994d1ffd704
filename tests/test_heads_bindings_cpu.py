"""The device binding of the backward of the generator's grey heads (heads_grad_gpu.HeadsGrad) and its C entry points refuse bad
arguments before anything touches a GPU: the runner's image checks in their order, the sizes, the weights, the size queries and the
entry points' argument checks (all ahead of the device switch; no pointer is dereferenced).  Every text is asserted whole.  Everything
here runs on a CPU-only box; the GPU test holds the same refusals and that nothing was launched."""
import ctypes

import pytest
import torch

from blindshadowremoval_amd import _lib
from blindshadowremoval_amd.build import build_library
from blindshadowremoval_amd.heads_grad_gpu import KEPT, LAUNCHES, NO_WEIGHTS_TEXT, SIZE_TEXT, HeadsGrad
from blindshadowremoval_amd.post_gpu import DENSE, STRIDED
from on_dev0 import BSR_ERR_ARG, DEV, P, d0

import heads_grad_cases as cases

SPEC = (("inputs", 3), ("mask22", 3), ("y", 64), ("d_gs", 1))


def _images(b=1, h=8, w=32):
    return [d0(b, h, w, c) for _, c in SPEC]


def refused(runner, error, args):
    with pytest.raises(error) as e:
        runner.heads_grad(*args)
    assert type(e.value) is error
    return str(e.value)


def test_the_declaration():
    assert HeadsGrad.INPUTS == (("inputs", 3, 1, DENSE), ("mask22", 3, 1, DENSE), ("y", 64, 1, STRIDED), ("d_gs", 1, 1, DENSE))
    assert HeadsGrad.LEAD == "d_gs" and HeadsGrad.OUTPUTS == (("d_y", 64, 1),) and HeadsGrad.MULTIPLES == (8, 32)
    assert HeadsGrad.KEPT == KEPT == ("g_m", "mask") and HeadsGrad.LAST == "last_y"
    assert HeadsGrad.SYMBOL == "bsr_heads_grad" and [name for name, _ in LAUNCHES] == ["entry", "dgrad", "wgrad", "fold", "finish"]
    assert HeadsGrad.NAMES() == list(cases.NAMES)


def test_runner_image_checks():
    runner = HeadsGrad(0)
    good = _images()
    h, w = 8, 32
    for k, (name, c) in enumerate(SPEC):
        def swapped(t):
            return good[:k] + [t] + good[k + 1:]
        for bad in (torch.zeros(1, h, w, c), d0(1, h, w, c, dtype=torch.float64), d0(1, h, w)):           # host, dtype, dims
            assert refused(runner, TypeError, swapped(bad)) == "%s must be a float32 tensor [B,H,W,%d] on %s" % (name, c, DEV)
        strided = d0(1, h, w, 2 * c)[..., ::2]
        assert tuple(strided.shape) == (1, h, w, c) and not strided.is_contiguous()
        assert refused(runner, ValueError, swapped(strided)) == "%s must be contiguous (NHWC, dense)" % name
        if name == "d_gs":
            assert refused(runner, ValueError, swapped(d0(1, 8, 32, 2))) == "d_gs must be [B,H,W,1], got (1, 8, 32, 2)"
            assert refused(runner, ValueError, swapped(d0(2, 8, 32, 1))) == "inputs must be [2,8,32,3] like d_gs, got (1, 8, 32, 3)"
        else:
            assert refused(runner, ValueError, swapped(d0(1, h, w, c + 1))) == "%s must be [1,%d,%d,%d] like d_gs, got (1, %d, %d, %d)" % (name, h, w, c, h, w, c + 1)
            assert refused(runner, ValueError, swapped(d0(2, h, w, c))) == "%s must be [1,%d,%d,%d] like d_gs, got (2, %d, %d, %d)" % (name, h, w, c, h, w, c)
    for b, h, w in ((1, 12, 32), (1, 8, 16), (1, 4, 32), (1, 8, 48)):
        assert refused(runner, ValueError, _images(b, h, w)) == SIZE_TEXT % (b, h, w)
    # a type mistake in an image comes before a size the chain does not take, and both before the weights
    assert refused(runner, TypeError, [torch.zeros(1, 12, 32, 3)] + _images(1, 12, 32)[1:]) == "inputs must be a float32 tensor [B,H,W,3] on %s" % (DEV,)
    assert refused(runner, ValueError, good) == NO_WEIGHTS_TEXT
    with pytest.raises(ValueError) as e:                 # the weights come before stop_after's range
        runner.stages(*good, 99)
    assert str(e.value) == NO_WEIGHTS_TEXT
    with pytest.raises(ValueError) as e:
        runner.backward(object(), good[0], good[1], good[3])
    assert str(e.value) == NO_WEIGHTS_TEXT
    with pytest.raises(TypeError) as e:                  # in place the dense inputs alone are checked
        runner.backward(object(), good[0], torch.zeros(1, 8, 32, 3), good[3])
    assert str(e.value) == "mask22 must be a float32 tensor [B,H,W,3] on %s" % (DEV,)
    assert runner._scratch is None
    with pytest.raises(ValueError) as e:
        from blindshadowremoval_amd.weights import init_weights
        runner.load_weights(init_weights(1, variant="rgb"))
    from blindshadowremoval_amd import pack
    assert str(e.value) == pack.HEADS_RGB_TEXT and runner._blob is None


@pytest.fixture(scope="module")
def lib():
    build_library()            # no-op when the in-tree .so is fresh
    return _lib.load()


def test_size_queries(lib):
    assert lib.bsr_heads_grad_blob_bytes() == 100 * 64 * 4
    assert lib.bsr_heads_grad_floats() == 6274
    assert [lib.bsr_heads_grad_var_offset(i) for i in range(4)] == [0, 3136, 3137, 6273]
    size_max = ctypes.c_size_t(-1).value
    assert lib.bsr_heads_grad_var_offset(-1) == lib.bsr_heads_grad_var_offset(4) == size_max
    for b, h, w in ((0, 8, 32), (1, 12, 32), (1, 8, 16), (1, 0, 32), (1, 8, 0), (-1, 8, 32), (1 << 10, 1 << 9, 1 << 9)):
        assert lib.bsr_heads_grad_scratch_bytes(b, h, w) == 0, (b, h, w)
        assert lib.bsr_heads_grad_partials(b, h, w) == 0
        assert lib.bsr_heads_grad_offset(b, h, w, 0) == size_max
    assert lib.bsr_heads_grad_offset(1, 8, 32, 4) == lib.bsr_heads_grad_offset(1, 8, 32, -1) == size_max
    # slices of whole 8 x 32 tiles: half as many as tiles, rounded up, at most 256.  The device tests' (24, 96, 3) and (40, 32, 1) run more
    # than one slice with a tile count that is no multiple of the slice count
    for (h, w, b), (tiles, slices) in cases.SLICES.items():
        assert b * h * w == 256 * tiles and lib.bsr_heads_grad_partials(b, h, w) == slices, (h, w, b)
    assert sorted(cases.SLICES) == sorted(cases.GPU_SIZES)
    assert any(s > 1 and t % s for t, s in cases.SLICES.values())
    assert lib.bsr_heads_grad_partials(32, 256, 256) == 256 and lib.bsr_heads_grad_partials(3, 256, 256) == 256 and lib.bsr_heads_grad_partials(1, 256, 256) == 128
    # the scratch: g2 [N][2], mask [N], Wg float64 [2][49][64], S float64 [2], then the sums' and the kernel gradients' partials
    offs = [lib.bsr_heads_grad_offset(1, 8, 32, m) for m in range(4)]
    assert all(o % 256 == 0 for o in offs) and offs[0] == 0
    assert [b - a for a, b in zip(offs, offs[1:])] == [256 * 2 * 4, 256 * 4, 2 * 49 * 64 * 8]
    assert lib.bsr_heads_grad_scratch_bytes(1, 8, 32) == offs[3] + 256 + 256 + 4 * 112 * 64 * 4
    assert lib.bsr_heads_grad_scratch_bytes(32, 256, 256) > lib.bsr_heads_grad_scratch_bytes(1, 8, 32)


SLOTS = "d_blob blob_bytes inputs mask22 y y_cs d_gs B H W d_y grads scratch"
INTS = {"B": 2, "H": 8, "W": 32, "y_cs": 64, "stop_after": 1}


@pytest.mark.parametrize("fn", ("bsr_heads_grad", "bsr_debug_heads_grad"))
def test_entry_point_argument_checks(lib, fn):
    slots = (SLOTS + (" stop_after" if "debug" in fn else "")).split()

    def refused(**over):
        """The code and the text of the call with the named arguments replaced."""
        args = [0]
        for slot in slots:
            value = dict(INTS, blob_bytes=lib.bsr_heads_grad_blob_bytes()).get(slot, P)
            args.append(over.get(slot, value))
        assert set(over) <= set(slots)
        return getattr(lib, fn)(*args, None), lib.bsr_last_error().decode()

    def text(what):
        return (BSR_ERR_ARG, fn + ": " + what)

    for slot in ("d_blob", "inputs", "mask22", "y", "d_gs", "d_y", "grads", "scratch"):
        assert refused(**{slot: None}) == text("null argument"), slot
    size = "B must be positive, H a multiple of 8 and W a multiple of 32 (the forward heads' tile), at most 2^26 pixels in all"
    for over in (dict(B=0), dict(H=12), dict(W=16), dict(H=0), dict(B=1 << 10, H=1 << 9, W=1 << 9)):
        assert refused(**over) == text(size), over
    assert refused(blob_bytes=lib.bsr_heads_grad_blob_bytes() + 4) == text("blob_bytes must be bsr_heads_grad_blob_bytes() (pack.pack_heads_grad)")
    for y_cs in (60, 66, 0):
        assert refused(y_cs=y_cs) == text("y_cs must be a multiple of 4 and at least 64")
    for slot in ("d_blob", "y", "d_y"):
        assert refused(**{slot: P + 4}) == text("d_blob, y and d_y must be 16-byte aligned"), slot
    for slot in ("inputs", "mask22", "d_gs", "grads"):
        assert refused(**{slot: P + 2}) == text("inputs, mask22, d_gs and grads must be 4-byte aligned"), slot
    assert refused(scratch=P + 8) == text("scratch must be 256-byte aligned")
    if "stop_after" in slots:
        for stop in (-1, 6):
            assert refused(stop_after=stop) == text("stop_after must be 0..5")


def test_last_y_refuses_null_arguments(lib):
    ptr, cs, shape = ctypes.c_void_p(), ctypes.c_int(), (ctypes.c_int * 4)()
    assert lib.bsr_last_y(None, ctypes.byref(ptr), ctypes.byref(cs), ctypes.byref(shape)) == BSR_ERR_ARG
    assert lib.bsr_last_error().decode() == "bsr_last_y: null argument"
    assert "bsr_last_y" in _lib.EXPORTS and "bsr_heads_grad" in _lib.EXPORTS and "bsr_debug_heads_grad" in _lib.EXPORTS


def test_the_command_refuses_heads_without_tail(capsys):
    from blindshadowremoval_amd import HeadsGrad as exported
    from blindshadowremoval_amd import objective
    assert exported is HeadsGrad
    with pytest.raises(SystemExit):
        objective.main(["nowhere", "--vgg", "none.npz", "--grad-total", "--heads"])
    assert "--heads goes with --grad-total --tail" in capsys.readouterr().err
    with pytest.raises(ValueError, match="--heads goes with --grad-total --tail"):
        objective.score_folder("nowhere", "none.npz", grad_total=True, heads=True)
    names = objective.heads_grad_names()
    assert len(names) == 10 and names[:4] == ["d_y_l1", "d_y_linf", "conv2/conv/kernel_l1", "conv2/conv/kernel_linf"]
    assert objective.STAGES == ("tail", "decoder", "nonlocal", "bottleneck")          # the colour branch's chain of flags is as it was
