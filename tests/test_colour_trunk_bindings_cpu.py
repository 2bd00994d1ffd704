"""The device binding of the backward of res_stack/4, res_stack/3 and the hole (colour_trunk_gpu.ColourTrunk) and its C entry points
refuse bad arguments before anything touches a GPU: the runner's image checks in their order, the sizes, the weights, the size queries
and the entry points' argument checks (all ahead of the device switch; no pointer is dereferenced).  Every text is asserted whole.
Everything here runs on a CPU-only box; the GPU test holds that nothing was launched."""
import ctypes
import math

import pytest
import torch

from blindshadowremoval_amd import _lib, pack
from blindshadowremoval_amd.build import build_library
from blindshadowremoval_amd.colour_trunk_gpu import ALIGN_TEXT, LAUNCHES, NO_WEIGHTS_TEXT, SIZE_TEXT, ColourTrunk
from blindshadowremoval_amd.weights import (generator_bottleneck_trainable_names, generator_colour_trunk_trainable_names,
                                            generator_nonlocal_trainable_names, generator_variable_shapes, init_weights)
from on_dev0 import BSR_ERR_ARG, DEV, P, d0

SPEC = (("y3x4", 257), ("out4", 261), ("y3x3", 257), ("out3", 261), ("xh", 261), ("d_xin", 261), ("d_x", 257))
c_i, c_v, c_sz = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t


def _images(b=1, h=4, w=32):
    return [d0(b, h, w, c) for _, c in SPEC]


def refused(runner, error, args):
    with pytest.raises(error) as e:
        runner.colour_trunk_grad(*args)
    assert type(e.value) is error
    return str(e.value)


def test_the_declaration_and_the_exports():
    import blindshadowremoval_amd as package
    from blindshadowremoval_amd import objective
    from blindshadowremoval_amd.post_gpu import DENSE, OPTIONAL, STRIDED, GradStage
    assert package.ColourTrunk is ColourTrunk and "ColourTrunk" in package.__all__ and issubclass(ColourTrunk, GradStage)
    assert ColourTrunk.SYMBOL == "bsr_colour_trunk_grad" and ColourTrunk.LAST == "last_colour_trunk" and ColourTrunk.LEAD == "d_xin"
    assert ColourTrunk.INPUTS == (("y3x4", 257, 1, STRIDED), ("out4", 261, 1, STRIDED), ("y3x3", 257, 1, STRIDED), ("out3", 261, 1, STRIDED),
                                  ("xh", 261, 1, STRIDED), ("d_xin", 261, 1, DENSE), ("d_x", 257, 1, OPTIONAL))
    assert ColourTrunk.OUTPUTS == (("d_res2", 257, 1),) and ColourTrunk.MULTIPLES == (4, 32) and not ColourTrunk.TAKES_KEEP
    assert ColourTrunk.KEPT == ("a1_4", "a2_4", "a1_3", "a2_3", "d_y3_4", "d_skip_4", "d_xin4", "d_y3_3", "d_skip_3", "d_xin3")
    from blindshadowremoval_amd import bottleneck_grad_gpu, nonlocal_grad_gpu
    names = [n for n, _ in LAUNCHES]
    assert len(names) == 49 and ColourTrunk.LAUNCHES is LAUNCHES and names[-1] == "hole"
    want = []
    for b in (4, 3):
        want += ["nl%d.%s" % (b, n) for n, _ in nonlocal_grad_gpu.LAUNCHES] + ["bn%d.%s" % (b, n) for n, _ in bottleneck_grad_gpu.LAUNCHES]
    assert names[:48] == want and names[0] == "nl4.entry" and names[12] == "bn4.entry" and names[24] == "nl3.entry" and names[47] == "bn3.finish"
    assert hasattr(package.Generator, "last_block") and hasattr(package.Generator, "last_colour_trunk")
    # the table of the objective command is not touched: its rows follow in a change that may edit its test
    assert [s.name for s in objective.BACKWARD] == ["tail", "decoder", "nonlocal", "bottleneck", "heads"]


def test_the_names():
    names = generator_colour_trunk_trainable_names()
    shapes = generator_variable_shapes()
    per_block = [generator_bottleneck_trainable_names(b) + generator_nonlocal_trainable_names(b) for b in (3, 4)]
    assert names == per_block[0] + per_block[1] and len(names) == 44 == ColourTrunk.NAMES().__len__()
    assert names == [n for n in shapes if n.split("/")[1] in ("3", "4") and n.startswith("res_stack/") and "moving_" not in n]
    assert sum(math.prod(shapes[n]) for n in names) == 2 * (215299 + 132739) == 696076


def test_the_signatures():
    five = [c_v, c_i] * 5
    assert _lib.SIGNATURES["bsr_colour_trunk_grad"] == (c_i, [c_i, c_v, c_sz] + five + [c_v, c_v, c_i, c_i, c_i, c_v, c_v, c_v, c_v])
    assert _lib.SIGNATURES["bsr_debug_colour_trunk_grad"] == (c_i, [c_i, c_v, c_sz] + five + [c_v, c_v, c_i, c_i, c_i, c_v, c_v, c_v, c_i, c_v])
    assert _lib.SIGNATURES["bsr_colour_trunk_grad_blob_bytes"] == _lib.SIGNATURES["bsr_colour_trunk_grad_floats"] == (c_sz, [])
    assert _lib.SIGNATURES["bsr_colour_trunk_grad_scratch_bytes"] == (c_sz, [c_i, c_i, c_i])
    assert _lib.SIGNATURES["bsr_colour_trunk_grad_var_offset"] == (c_sz, [c_i])
    assert _lib.SIGNATURES["bsr_colour_trunk_grad_offset"] == (c_sz, [c_i, c_i, c_i, c_i])
    ptr = ctypes.POINTER
    assert _lib.SIGNATURES["bsr_last_block"] == (c_i, [c_v, c_i, ptr(c_v), ptr(c_i), ptr(c_v), ptr(c_v), ptr(c_i), ptr(c_i * 4)])
    assert _lib.SIGNATURES["bsr_last_block"][1][2:] == _lib.SIGNATURES["bsr_last_block5"][1][1:]
    for name in ("bsr_last_block", "bsr_colour_trunk_grad", "bsr_debug_colour_trunk_grad", "bsr_colour_trunk_grad_offset"):
        assert name in _lib.EXPORTS


def test_runner_checks_come_before_any_library_call(monkeypatch):
    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "load", no_library)
    runner = ColourTrunk(0)
    good = _images()
    for k, (name, c) in enumerate(SPEC):
        def swapped(t):
            return good[:k] + [t] + good[k + 1:]
        for bad in (torch.zeros(1, 4, 32, c), d0(1, 4, 32, c, dtype=torch.float64), d0(1, 4, 32)):           # host, dtype, dims
            assert refused(runner, TypeError, swapped(bad)) == "%s must be a float32 tensor [B,h,w,%d] on %s" % (name, c, DEV)
        strided = d0(1, 4, 32, 2 * c)[..., ::2]
        assert tuple(strided.shape) == (1, 4, 32, c) and not strided.is_contiguous()
        assert refused(runner, ValueError, swapped(strided)) == "%s must be contiguous (NHWC, dense)" % name
        if name == "d_xin":
            assert refused(runner, ValueError, swapped(d0(1, 4, 32, 257))) == "d_xin must be [B,h,w,261], got (1, 4, 32, 257)"
            assert refused(runner, ValueError, swapped(d0(2, 4, 32, 261))) == "y3x4 must be [2,4,32,257] for this d_xin, got (1, 4, 32, 257)"
        else:
            assert refused(runner, ValueError, swapped(d0(1, 4, 32, c + 1))) == "%s must be [1,4,32,%d] for this d_xin, got (1, 4, 32, %d)" % (name, c, c + 1)
            assert refused(runner, ValueError, swapped(d0(2, 4, 32, c))) == "%s must be [1,4,32,%d] for this d_xin, got (2, 4, 32, %d)" % (name, c, c)
    for b, h, w in ((1, 6, 32), (1, 4, 16), (1, 2, 32), (1, 4, 48)):
        assert refused(runner, ValueError, _images(b, h, w)) == SIZE_TEXT % (b, h, w)
    # a type mistake comes before a size the chain does not take, and both before the weights; no d_x is no mistake
    assert refused(runner, TypeError, [torch.zeros(1, 6, 32, 257)] + _images(1, 6, 32)[1:]) == "y3x4 must be a float32 tensor [B,h,w,257] on %s" % (DEV,)
    assert refused(runner, ValueError, good) == refused(runner, ValueError, good[:6] + [None]) == refused(runner, ValueError, good[:6]) == NO_WEIGHTS_TEXT
    with pytest.raises(ValueError) as e:                 # the weights come before stop_after's range
        runner.stages(*good, 99)
    assert str(e.value) == NO_WEIGHTS_TEXT
    with pytest.raises(ValueError) as e:
        runner.backward(object(), good[5], good[6])
    assert str(e.value) == NO_WEIGHTS_TEXT
    assert runner._scratch is None and runner._blob is None
    assert SIZE_TEXT % (1, 6, 32) == "the colour trunk takes B >= 1 grids with h a multiple of 4 and w a multiple of 32, got B=1 h=6 w=32"
    assert NO_WEIGHTS_TEXT == "the colour trunk has no weights: call load_weights or restore first"


@pytest.fixture(scope="module")
def lib():
    build_library()            # no-op when the in-tree .so is fresh
    return _lib.load()


def test_the_blob_is_the_four_packs_joined(lib):
    wt = init_weights(3)
    parts = [pack.pack_nonlocal_grad(wt, 4), pack.pack_bottleneck_grad(wt, 4), pack.pack_nonlocal_grad(wt, 3), pack.pack_bottleneck_grad(wt, 3)]
    blob = pack.pack_colour_trunk_grad(wt)
    assert blob == b"".join(parts) and len(set(parts)) == 4
    assert lib.bsr_colour_trunk_grad_blob_bytes() == len(blob) == 2 * (lib.bsr_nonlocal_grad_blob_bytes() + lib.bsr_bottleneck_grad_blob_bytes())
    assert all(len(p) % 16 == 0 for p in parts)          # every sub-blob keeps the 16-byte alignment of the whole
    with pytest.raises(ValueError) as e:
        pack.pack_colour_trunk_grad(init_weights(3, variant="tsm"))
    assert str(e.value) == pack.NONLOCAL_TSM_TEXT


def test_size_queries(lib):
    assert lib.bsr_colour_trunk_grad_floats() == 696076
    shapes = generator_variable_shapes()
    off = 0
    for index, name in enumerate(generator_colour_trunk_trainable_names()):
        assert lib.bsr_colour_trunk_grad_var_offset(index) == off, (index, name)
        off += math.prod(shapes[name])
    assert off == 696076
    size_max = ctypes.c_size_t(-1).value
    assert lib.bsr_colour_trunk_grad_var_offset(-1) == lib.bsr_colour_trunk_grad_var_offset(44) == size_max
    # a block's part of the flat buffer is the two existing buffers end to end
    bn, nl = lib.bsr_bottleneck_grad_floats(), lib.bsr_nonlocal_grad_floats()
    for first in (0, 22):
        base = lib.bsr_colour_trunk_grad_var_offset(first)
        assert [lib.bsr_colour_trunk_grad_var_offset(first + i) - base for i in range(12)] == [lib.bsr_bottleneck_grad_var_offset(i) for i in range(12)]
        assert [lib.bsr_colour_trunk_grad_var_offset(first + 12 + i) - base - bn for i in range(10)] == [lib.bsr_nonlocal_grad_var_offset(i) for i in range(10)]
    assert lib.bsr_colour_trunk_grad_var_offset(22) == bn + nl
    for b, h, w in ((0, 4, 32), (1, 6, 32), (1, 4, 16), (1, 0, 32), (1, 4, 0), (-1, 4, 32), (1 << 12, 1 << 5, 1 << 5)):
        assert lib.bsr_colour_trunk_grad_scratch_bytes(b, h, w) == 0, (b, h, w)
        assert lib.bsr_colour_trunk_grad_offset(b, h, w, 0) == size_max
    assert lib.bsr_colour_trunk_grad_offset(1, 4, 32, 42) == lib.bsr_colour_trunk_grad_offset(1, 4, 32, -1) == size_max
    # the scratch: the four sub-chains' regions in the order of the launches, each whole, then the six intermediate data gradients
    for b, h, w in ((1, 4, 32), (3, 12, 32), (32, 32, 32)):
        offs = [lib.bsr_colour_trunk_grad_offset(b, h, w, m) for m in range(42)]
        assert all(o % 256 == 0 for o in offs) and offs == sorted(offs) and len(set(offs)) == 42
        nl_bytes, bn_bytes = lib.bsr_nonlocal_grad_scratch_bytes(b, h, w), lib.bsr_bottleneck_grad_scratch_bytes(b, h, w)
        regions = [0, nl_bytes, nl_bytes + bn_bytes, 2 * nl_bytes + bn_bytes]
        assert [offs[0], offs[10], offs[18], offs[28]] == regions
        for k, base in enumerate(regions):
            first = (0, 10, 18, 28)[k]
            query = lib.bsr_bottleneck_grad_offset if k % 2 else lib.bsr_nonlocal_grad_offset
            assert [offs[first + i] - base for i in range(8 if k % 2 else 10)] == [query(b, h, w, i) for i in range(8 if k % 2 else 10)]
        n = b * h * w
        assert offs[36] == 2 * (nl_bytes + bn_bytes)
        assert [offs[m + 1] - offs[m] for m in range(36, 41)] == [n * c * 4 for c in (257, 261, 261, 257, 261)]
        assert lib.bsr_colour_trunk_grad_scratch_bytes(b, h, w) == offs[41] + n * 261 * 4
    assert lib.bsr_colour_trunk_grad_scratch_bytes(32, 32, 32) == 1155558400          # 32 items of 256 x 256: profiles/colour_trunk_grad_resources.md


SLOTS = "d_blob blob_bytes y3x4 y3x4_cs out4 out4_cs y3x3 y3x3_cs out3 out3_cs xh xh_cs d_xin d_x B h w d_res2 grads scratch"
INTS = {"B": 2, "h": 4, "w": 32, "y3x4_cs": 288, "out4_cs": 264, "y3x3_cs": 288, "out3_cs": 264, "xh_cs": 264, "stop_after": 1}


@pytest.mark.parametrize("fn", ("bsr_colour_trunk_grad", "bsr_debug_colour_trunk_grad"))
def test_entry_point_argument_checks(lib, fn):
    slots = (SLOTS + (" stop_after" if "debug" in fn else "")).split()

    def refused(**over):
        """The code and the text of the call with the named arguments replaced."""
        args = [0]
        for slot in slots:
            value = dict(INTS, blob_bytes=lib.bsr_colour_trunk_grad_blob_bytes()).get(slot, P)
            args.append(over.get(slot, value))
        assert set(over) <= set(slots)
        return getattr(lib, fn)(*args, None), lib.bsr_last_error().decode()

    def text(what):
        return (BSR_ERR_ARG, fn + ": " + what)

    required = [s for s in slots if s not in INTS and s not in ("blob_bytes", "d_x")]
    assert required == ["d_blob", "y3x4", "out4", "y3x3", "out3", "xh", "d_xin", "d_res2", "grads", "scratch"]
    for slot in required:
        assert refused(**{slot: None}) == text("null argument"), slot
    size = "B must be positive, h a multiple of 4 and w a multiple of 32 (the generator's rule at 1/8 resolution), at most 2^21 pixels in all"
    for over in (dict(B=0), dict(h=6), dict(w=16), dict(h=0), dict(B=1 << 12, h=1 << 5, w=1 << 5)):
        assert refused(**over) == text(size), over
    for nbytes in (16, lib.bsr_bottleneck_grad_blob_bytes() + lib.bsr_nonlocal_grad_blob_bytes()):
        assert refused(blob_bytes=nbytes) == text(
            "blob_bytes must be bsr_colour_trunk_grad_blob_bytes() (pack.pack_colour_trunk_grad; the GSC width 261 only, not TSM's 877)")
    for over in (dict(y3x4_cs=256), dict(y3x3_cs=256), dict(out4_cs=260), dict(out3_cs=260), dict(xh_cs=260)):
        assert refused(**over) == text("y3x4_cs and y3x3_cs must be at least 257, out4_cs, out3_cs and xh_cs at least 261"), over
    for slot in ("d_blob", "d_x", "d_res2"):
        assert refused(**{slot: P + 4}) == text("d_blob, d_x and d_res2 must be 16-byte aligned"), slot
    for slot in ("y3x4", "out4", "y3x3", "out3", "xh", "d_xin", "grads"):
        assert refused(**{slot: P + 2}) == text("y3x4, out4, y3x3, out3, xh, d_xin and grads must be 4-byte aligned"), slot
    assert refused(scratch=P + 8) == text("scratch must be 256-byte aligned")
    if "stop_after" in slots:
        for stop in (-1, 50):
            assert refused(stop_after=stop) == text("stop_after must be 0..49")


def _odd_view(*shape):
    """A dense float32 tensor that reports cuda:0 and starts 4 bytes past a 16-byte boundary."""
    from on_dev0 import OnDev0
    t = torch.zeros(math.prod(shape) + 1)[1:].view(shape).as_subclass(OnDev0)
    assert t.is_contiguous() and t.data_ptr() % 16 == 4
    return t


def test_a_misaligned_d_x_is_refused_before_any_library_call(monkeypatch):
    runner = ColourTrunk(0)
    runner._blob = torch.zeros(16, dtype=torch.uint8)        # stands for loaded weights: the alignment comes after them
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was reached"))
    odd = _odd_view(1, 4, 32, 257)
    for call in (lambda: runner.colour_trunk_grad(*_images()[:6], odd), lambda: runner.stages(*_images()[:6], odd, 3)):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == ALIGN_TEXT % ("d_x", odd.data_ptr())
    assert "16-byte aligned" in ALIGN_TEXT


def test_the_hole_hook_argument_checks(lib, monkeypatch):
    assert _lib.SIGNATURES["bsr_debug_hole_grad"] == (c_i, [c_i, c_v, c_i, c_v, c_v, c_i, c_i, c_i, c_v, c_v])

    def refused(xh=P, xh_cs=264, d_xin3=P, d_x=P, B=2, h=4, w=32, d_res2=P):
        return lib.bsr_debug_hole_grad(0, xh, xh_cs, d_xin3, d_x, B, h, w, d_res2, None), lib.bsr_last_error().decode()

    def text(what):
        return (BSR_ERR_ARG, "bsr_debug_hole_grad: " + what)

    for slot in ("xh", "d_xin3", "d_res2"):
        assert refused(**{slot: None}) == text("null argument"), slot
    size = "B must be positive, h a multiple of 4 and w a multiple of 32 (the generator's rule at 1/8 resolution), at most 2^21 pixels in all"
    for over in (dict(B=0), dict(h=6), dict(w=16), dict(B=1 << 12, h=1 << 5, w=1 << 5)):
        assert refused(**over) == text(size), over
    assert refused(xh_cs=257) == text("xh_cs must be at least 258")
    for slot in ("d_xin3", "d_x", "d_res2"):
        assert refused(**{slot: P + 4}) == text("d_xin3, d_x and d_res2 must be 16-byte aligned"), slot
    assert refused(xh=P + 2) == text("xh must be 4-byte aligned")
    # the runner's own checks come before the library
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was reached"))
    runner = ColourTrunk(0)
    with pytest.raises(TypeError) as e:
        runner.hole_grad(d0(1, 4, 32, 261), torch.zeros(1, 4, 32, 261))
    assert str(e.value) == "d_xin3 must be a float32 tensor [B,h,w,261] on %s" % (DEV,)
    with pytest.raises(ValueError) as e:
        runner.hole_grad(d0(1, 4, 32, 260), d0(1, 4, 32, 261))
    assert str(e.value) == "xh must be [1,4,32,261] for this d_xin3, got (1, 4, 32, 260)"
    with pytest.raises(ValueError) as e:
        runner.hole_grad(d0(1, 4, 32, 261), d0(1, 4, 32, 261), d0(2, 4, 32, 257))
    assert str(e.value) == "d_x must be [1,4,32,257] for this d_xin3, got (2, 4, 32, 257)"
    # a contiguous view that starts one float into its storage is refused here, not by the entry point
    for name, c, args in (("d_xin3", 261, lambda t: (d0(1, 4, 32, 261), t)), ("d_x", 257, lambda t: (d0(1, 4, 32, 261), d0(1, 4, 32, 261), t))):
        odd = _odd_view(1, 4, 32, c)
        with pytest.raises(ValueError) as e:
            runner.hole_grad(*args(odd))
        assert str(e.value) == ALIGN_TEXT % (name, odd.data_ptr())
    with pytest.raises(ValueError) as e:
        runner.hole_grad(d0(1, 6, 32, 261), d0(1, 6, 32, 261), d0(1, 6, 32, 257))
    assert str(e.value) == SIZE_TEXT % (1, 6, 32)


def test_last_block_refuses_null_arguments(lib):
    shape = (ctypes.c_int * 4)()
    ptrs, cs = [ctypes.c_void_p() for _ in range(3)], [ctypes.c_int() for _ in range(2)]
    args = [ctypes.byref(ptrs[0]), ctypes.byref(cs[0]), ctypes.byref(ptrs[1]), ctypes.byref(ptrs[2]), ctypes.byref(cs[1]), ctypes.byref(shape)]
    for block in (3, 4):
        assert lib.bsr_last_block(None, block, *args) == BSR_ERR_ARG
        assert lib.bsr_last_error().decode() == "bsr_last_block: null argument"
    assert lib.bsr_last_block5(None, *args) == BSR_ERR_ARG
    assert lib.bsr_last_error().decode() == "bsr_last_block5: null argument"
    assert lib.bsr_abi_version() == 8                    # a handle needs a device: the refusal of other blocks is held on the GPU
