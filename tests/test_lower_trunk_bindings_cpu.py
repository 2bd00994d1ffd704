"""The device binding of the backward of res_stack/2, res_stack/1 and res_stack/0 (lower_trunk_gpu.LowerTrunk) and its C entry points
refuse bad arguments before anything touches a GPU: the runner's image checks in their order, the sizes, the weights, the size queries
and the entry points' argument checks (all ahead of the device switch; no pointer is dereferenced).  Every text is asserted whole.
The blob is the six packs joined, the flat buffer follows the names, the scratch is the six regions and the eight data gradients.
Everything here runs on a CPU-only box; the GPU test holds that nothing was launched."""
import ctypes
import math

import numpy as np
import pytest
import torch

from blindshadowremoval_amd import _lib, pack
from blindshadowremoval_amd.build import build_library
from blindshadowremoval_amd.lower_trunk_gpu import DATA, LAUNCHES, NO_WEIGHTS_TEXT, SIZE_TEXT, LowerTrunk
from blindshadowremoval_amd.weights import (generator_bottleneck_trainable_names, generator_lower_trunk_trainable_names,
                                            generator_nonlocal_trainable_names, generator_variable_shapes, init_weights)
from on_dev0 import BSR_ERR_ARG, DEV, P, d0

SPEC = (("y3x2", 257), ("out2", 257), ("y3x1", 257), ("out1", 257), ("y3x0", 257), ("out0", 257), ("x0", 99), ("d_res2", 257))
WIDTHS = {0: 99, 1: 257, 2: 257}
c_i, c_v, c_sz = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t


def _images(b=1, h=4, w=32):
    return [d0(b, h, w, c) for _, c in SPEC]


def refused(runner, error, args):
    with pytest.raises(error) as e:
        runner.lower_trunk_grad(*args)
    assert type(e.value) is error
    return str(e.value)


def test_the_declaration_and_the_exports():
    import blindshadowremoval_amd as package
    from blindshadowremoval_amd import bottleneck_grad_gpu, nonlocal_grad_gpu, objective
    from blindshadowremoval_amd.post_gpu import DENSE, STRIDED, GradStage
    assert package.LowerTrunk is LowerTrunk and "LowerTrunk" in package.__all__ and issubclass(LowerTrunk, GradStage)
    assert LowerTrunk.SYMBOL == "bsr_lower_trunk_grad" and LowerTrunk.LAST == "last_lower_trunk" and LowerTrunk.LEAD == "d_res2"
    assert LowerTrunk.INPUTS == tuple((n, c, 1, STRIDED) for n, c in SPEC[:7]) + (("d_res2", 257, 1, DENSE),)
    assert LowerTrunk.OUTPUTS == (("d_x0", 99, 1),) and LowerTrunk.MULTIPLES == (4, 32) and not LowerTrunk.TAKES_KEEP
    assert LowerTrunk.KEPT == ("a1_2", "a2_2", "a1_1", "a2_1", "a1_0", "a2_0", "d_y3_2", "d_skip_2", "d_xin2", "d_y3_1", "d_skip_1", "d_xin1",
                               "d_y3_0", "d_skip_0")
    assert tuple(DATA) == LowerTrunk.KEPT[6:] and [DATA[k] for k in DATA] == [(54 + i, 99 if k == "d_skip_0" else 257) for i, k in enumerate(DATA)]
    names = [n for n, _ in LAUNCHES]
    want = []
    for b in (2, 1, 0):
        want += ["nl%d.%s" % (b, n) for n, _ in nonlocal_grad_gpu.LAUNCHES] + ["bn%d.%s" % (b, n) for n, _ in bottleneck_grad_gpu.LAUNCHES]
    assert len(names) == 72 and LowerTrunk.LAUNCHES is LAUNCHES and names == want
    assert names[0] == "nl2.entry" and names[12] == "bn2.entry" and names[24] == "nl1.entry" and names[48] == "nl0.entry" and names[71] == "bn0.finish"
    assert hasattr(package.Generator, "last_lower_trunk")
    # the table of the objective command is not touched
    assert [s.name for s in objective.BACKWARD] == ["tail", "decoder", "nonlocal", "bottleneck", "heads"]


def test_the_names():
    names = generator_lower_trunk_trainable_names()
    shapes = generator_variable_shapes()
    per_block = [generator_bottleneck_trainable_names(b) + generator_nonlocal_trainable_names(b) for b in (0, 1, 2)]
    assert names == per_block[0] + per_block[1] + per_block[2] and len(names) == 66 == len(LowerTrunk.NAMES()) and len(set(names)) == 66
    assert sorted(names) == sorted(n for n in shapes if n.startswith(("res_stack/0/", "res_stack/1/", "res_stack/2/")) and "moving_" not in n)
    counts = [sum(math.prod(shapes[n]) for n in block) for block in per_block]
    assert counts == [194563 + 132739, 214787 + 132739, 214787 + 132739] and sum(counts) == 1022354


def test_the_signatures():
    seven = [c_v, c_i] * 7
    assert _lib.SIGNATURES["bsr_lower_trunk_grad"] == (c_i, [c_i, c_v, c_sz] + seven + [c_v, c_i, c_i, c_i, c_v, c_v, c_v, c_v])
    assert _lib.SIGNATURES["bsr_debug_lower_trunk_grad"] == (c_i, [c_i, c_v, c_sz] + seven + [c_v, c_i, c_i, c_i, c_v, c_v, c_v, c_i, c_v])
    assert _lib.SIGNATURES["bsr_lower_trunk_grad_blob_bytes"] == _lib.SIGNATURES["bsr_lower_trunk_grad_floats"] == (c_sz, [])
    assert _lib.SIGNATURES["bsr_lower_trunk_grad_scratch_bytes"] == (c_sz, [c_i, c_i, c_i])
    assert _lib.SIGNATURES["bsr_lower_trunk_grad_var_offset"] == (c_sz, [c_i])
    assert _lib.SIGNATURES["bsr_lower_trunk_grad_offset"] == (c_sz, [c_i, c_i, c_i, c_i])
    ptr = ctypes.POINTER
    assert _lib.SIGNATURES["bsr_last_lower_trunk"] == (c_i, [c_v, ptr(c_v * 7), ptr(c_i * 7), ptr(c_i * 4)])
    for name in ("bsr_last_lower_trunk", "bsr_lower_trunk_grad", "bsr_debug_lower_trunk_grad", "bsr_lower_trunk_grad_offset"):
        assert name in _lib.EXPORTS


def test_runner_checks_come_before_any_library_call(monkeypatch):
    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "load", no_library)
    runner = LowerTrunk(0)
    good = _images()
    for k, (name, c) in enumerate(SPEC):
        def swapped(t):
            return good[:k] + [t] + good[k + 1:]
        for bad in (torch.zeros(1, 4, 32, c), d0(1, 4, 32, c, dtype=torch.float64), d0(1, 4, 32)):           # host, dtype, dims
            assert refused(runner, TypeError, swapped(bad)) == "%s must be a float32 tensor [B,h,w,%d] on %s" % (name, c, DEV)
        strided = d0(1, 4, 32, 2 * c)[..., ::2]
        assert tuple(strided.shape) == (1, 4, 32, c) and not strided.is_contiguous()
        assert refused(runner, ValueError, swapped(strided)) == "%s must be contiguous (NHWC, dense)" % name
        if name == "d_res2":
            assert refused(runner, ValueError, swapped(d0(1, 4, 32, 261))) == "d_res2 must be [B,h,w,257], got (1, 4, 32, 261)"
            assert refused(runner, ValueError, swapped(d0(2, 4, 32, 257))) == "y3x2 must be [2,4,32,257] for this d_res2, got (1, 4, 32, 257)"
        else:
            assert refused(runner, ValueError, swapped(d0(1, 4, 32, c + 1))) == "%s must be [1,4,32,%d] for this d_res2, got (1, 4, 32, %d)" % (name, c, c + 1)
            assert refused(runner, ValueError, swapped(d0(2, 4, 32, c))) == "%s must be [1,4,32,%d] for this d_res2, got (2, 4, 32, %d)" % (name, c, c)
    # block 0's input is 99 wide: the forward's 120-float rows are not a dense x0
    assert refused(runner, ValueError, good[:6] + [d0(1, 4, 32, 120), good[7]]) == "x0 must be [1,4,32,99] for this d_res2, got (1, 4, 32, 120)"
    for b, h, w in ((1, 6, 32), (1, 4, 16), (1, 2, 32), (1, 4, 48)):
        assert refused(runner, ValueError, _images(b, h, w)) == SIZE_TEXT % (b, h, w)
    # a type mistake comes before a size the chain does not take, and both before the weights
    assert refused(runner, TypeError, [torch.zeros(1, 6, 32, 257)] + _images(1, 6, 32)[1:]) == "y3x2 must be a float32 tensor [B,h,w,257] on %s" % (DEV,)
    assert refused(runner, ValueError, good) == NO_WEIGHTS_TEXT
    with pytest.raises(ValueError) as e:                 # the weights come before stop_after's range
        runner.stages(*good, 99)
    assert str(e.value) == NO_WEIGHTS_TEXT
    with pytest.raises(ValueError) as e:
        runner.backward(object(), good[7])
    assert str(e.value) == NO_WEIGHTS_TEXT
    assert runner._scratch is None and runner._blob is None
    assert SIZE_TEXT % (1, 6, 32) == "the lower trunk takes B >= 1 grids with h a multiple of 4 and w a multiple of 32, got B=1 h=6 w=32"
    assert NO_WEIGHTS_TEXT == "the lower trunk has no weights: call load_weights or restore first"


def test_the_packs_refuse_other_widths_and_keep_their_guards():
    """TSM's blocks 0..2 are 291 wide and the RGB baseline's 513: refused by the lower trunk's pack, first thing.  The existing packs keep
    their own guards: blocks 0..2 do not go through pack_bottleneck_grad or bottleneck_grad_record, nor through pack_nonlocal_grad."""
    wt = init_weights(3)
    for variant, got in (("tsm", (1, 1, 291, 128)), ("rgb", (1, 1, 99, 256))):
        other = init_weights(3, variant=variant)
        with pytest.raises(ValueError) as e:
            pack.pack_lower_trunk_grad(other)
        shape = tuple(np.shape(other["res_stack/2/conv1/kernel"]))
        assert str(e.value) == pack.LOWER_TRUNK_TEXT % (2, 257, shape) and "291 wide" in pack.LOWER_TRUNK_TEXT and "513" in pack.LOWER_TRUNK_TEXT
    for block in (0, 1, 2, 6):
        with pytest.raises(ValueError) as e:
            pack.pack_bottleneck_grad(wt, block)
        assert str(e.value) == pack.BOTTLENECK_BLOCK_TEXT % (block,)
        with pytest.raises(ValueError) as e:
            pack.bottleneck_grad_record(wt, block)
        assert str(e.value) == pack.BOTTLENECK_BLOCK_TEXT % (block,)
    for block in (0, 1, 2):
        with pytest.raises(ValueError) as e:
            pack.pack_nonlocal_grad(wt, block)
        assert str(e.value) == pack.NONLOCAL_TSM_TEXT
    with pytest.raises(ValueError) as e:
        LowerTrunk(0).load_weights(init_weights(3, variant="tsm"))
    assert str(e.value).startswith("the lower trunk's device chain takes the GSC widths only: res_stack/2/conv1/kernel must be [1,1,257,128]")


def test_the_layout_at_the_three_widths():
    assert pack.bottleneck_grad_layout() == pack.bottleneck_grad_layout(261) and pack.BOTTLENECK_WIDTH == 261
    assert pack.LOWER_TRUNK_WIDTHS == WIDTHS
    for width, xp, w1t in ((261, 272, 384), (257, 272, 384), (99, 112, 128)):
        layout, total = pack.bottleneck_grad_layout(width)
        shapes = {name: shape for name, _, shape in layout}
        assert shapes["w1f"] == (xp, 128) and shapes["w1t"] == (128, w1t) and shapes["k1"] == (width, 128) and shapes["w3t"] == (272, 128)
        assert total == sum(math.prod(s) for s in shapes.values()) and total % 4 == 0
        assert [off for _, off, _ in layout] == [sum(math.prod(s) for _, _, s in layout[:i]) for i in range(len(layout))]


@pytest.fixture(scope="module")
def lib():
    build_library()            # no-op when the in-tree .so is fresh
    return _lib.load()


def test_the_blob_is_the_six_packs_joined(lib):
    wt = init_weights(3)
    blob = pack.pack_lower_trunk_grad(wt)
    parts = pack.lower_trunk_grad_parts()
    assert [(k, b) for k, b, _ in parts] == [("nl", 2), ("bn", 2), ("nl", 1), ("bn", 1), ("nl", 0), ("bn", 0)]
    assert all(n % 4 == 0 for _, _, n in parts)             # every sub-blob keeps the 16-byte alignment of the whole
    assert lib.bsr_lower_trunk_grad_blob_bytes() == len(blob) == 4 * sum(n for _, _, n in parts)
    assert lib.bsr_nonlocal_grad_blob_bytes() == 4 * parts[0][2] and parts[1][2] == parts[3][2] > parts[5][2]
    # a part is what the existing packs write for a block of these shapes: the non-local blob does not carry the input's width, and
    # the bottleneck blob at the width 261 with conv1's rows 257..260 zero holds block 2's at 257 in the same places
    at = 0
    rec = pack.unpack_lower_trunk_grad(blob)
    for kind, b, n in parts:
        part = blob[4 * at:4 * (at + n)]
        if kind == "nl":
            as5 = {name.replace("res_stack/%d/" % b, "res_stack/5/"): v for name, v in wt.items() if name.startswith("res_stack/%d/" % b)}
            as5["res_stack/5/conv1/kernel"] = wt["res_stack/5/conv1/kernel"]
            assert part == pack.pack_nonlocal_grad(as5)
        else:
            layout, _ = pack.bottleneck_grad_layout(WIDTHS[b])
            for name, off, shape in layout:
                got = np.frombuffer(part, np.float32)[off:off + math.prod(shape)].reshape(shape)
                assert got.tobytes() == rec["bn%d.%s" % (b, name)].tobytes(), (b, name)
            k1 = np.asarray(wt["res_stack/%d/conv1/kernel" % b], np.float32)[0, 0]
            assert rec["bn%d.k1" % b].tobytes() == k1.tobytes() and rec["bn%d.k1" % b].shape == (WIDTHS[b], 128)
            w1f, w1t = rec["bn%d.w1f" % b], rec["bn%d.w1t" % b]
            assert not w1f[WIDTHS[b]:].any() and not w1t[:, WIDTHS[b]:].any() and w1f[:WIDTHS[b]].any()
            np.testing.assert_array_equal(w1t[:, :WIDTHS[b]], w1f[:WIDTHS[b]].T)
        at += n
    assert len(rec) == 3 * (6 + 13)
    with pytest.raises(ValueError, match="a lower trunk gradient blob holds %d bytes, got 16" % len(blob)):
        pack.unpack_lower_trunk_grad(b"\0" * 16)
    wide = dict(wt)
    wide["res_stack/4/conv1/kernel"] = np.concatenate([wt["res_stack/2/conv1/kernel"], np.zeros((1, 1, 4, 128), np.float32)], axis=2)
    for n in wt:
        if n.startswith("res_stack/2/") and n != "res_stack/2/conv1/kernel":
            wide[n.replace("res_stack/2/", "res_stack/4/")] = wt[n]
    at261 = pack.unpack_bottleneck_grad(pack.pack_bottleneck_grad(wide, 4))
    for name in ("w1f", "b1f", "w2f", "b2f", "w3t", "w2t", "w1t", "k2", "k3", "vecs1", "vecs2", "vecs3"):
        assert at261[name].tobytes() == rec["bn2." + name].tobytes(), name
    assert at261["k1"][:257].tobytes() == rec["bn2.k1"].tobytes()


def test_size_queries(lib):
    assert lib.bsr_lower_trunk_grad_floats() == 1022354
    shapes = generator_variable_shapes()
    off = 0
    for index, name in enumerate(generator_lower_trunk_trainable_names()):
        assert lib.bsr_lower_trunk_grad_var_offset(index) == off, (index, name)
        off += math.prod(shapes[name])
    assert off == 1022354
    size_max = ctypes.c_size_t(-1).value
    assert lib.bsr_lower_trunk_grad_var_offset(-1) == lib.bsr_lower_trunk_grad_var_offset(66) == size_max
    # the wide blocks' parts of the flat buffer are the two existing buffers end to end but for conv1's four rows fewer
    nl = lib.bsr_nonlocal_grad_floats()
    for first in (22, 44):
        base = lib.bsr_lower_trunk_grad_var_offset(first)
        assert [lib.bsr_lower_trunk_grad_var_offset(first + i) - base for i in range(1, 12)] == [lib.bsr_bottleneck_grad_var_offset(i) - 4 * 128
                                                                                                  for i in range(1, 12)]
        nl0 = lib.bsr_lower_trunk_grad_var_offset(first + 12)
        assert [lib.bsr_lower_trunk_grad_var_offset(first + 12 + i) - nl0 for i in range(10)] == [lib.bsr_nonlocal_grad_var_offset(i) for i in range(10)]
    assert lib.bsr_lower_trunk_grad_var_offset(22) == 194563 + nl and lib.bsr_lower_trunk_grad_var_offset(44) == 194563 + 214787 + 2 * nl
    for b, h, w in ((0, 4, 32), (1, 6, 32), (1, 4, 16), (1, 0, 32), (1, 4, 0), (-1, 4, 32), (1 << 12, 1 << 5, 1 << 5)):
        assert lib.bsr_lower_trunk_grad_scratch_bytes(b, h, w) == 0, (b, h, w)
        assert lib.bsr_lower_trunk_grad_offset(b, h, w, 0) == size_max
    assert lib.bsr_lower_trunk_grad_offset(1, 4, 32, 62) == lib.bsr_lower_trunk_grad_offset(1, 4, 32, -1) == size_max
    # the scratch: the six sub-chains' regions in the order of the launches, each whole, then the eight intermediate data gradients
    for b, h, w in ((1, 4, 32), (3, 12, 32), (32, 32, 32)):
        offs = [lib.bsr_lower_trunk_grad_offset(b, h, w, m) for m in range(62)]
        assert all(o % 256 == 0 for o in offs) and offs == sorted(offs) and len(set(offs)) == 62
        nl_bytes, bn_bytes = lib.bsr_nonlocal_grad_scratch_bytes(b, h, w), lib.bsr_bottleneck_grad_scratch_bytes(b, h, w)
        n = b * h * w
        # block 2's and 1's bottleneck regions: the 261-wide chain's less the four rows of Wg1 (float64, rounded up to 256 bytes)
        pad = lambda x: (x + 255) // 256 * 256                                       # noqa: E731
        bn257 = bn_bytes - pad((261 * 128 + 9 * 128 * 128 + 128 * 257) * 8) + pad((257 * 128 + 9 * 128 * 128 + 128 * 257) * 8)
        assert [offs[0], offs[10], offs[18], offs[28], offs[36]] == [0, nl_bytes, nl_bytes + bn257, 2 * nl_bytes + bn257, 2 * (nl_bytes + bn257)]
        for first in (0, 18, 36):
            assert [offs[first + i] - offs[first] for i in range(10)] == [lib.bsr_nonlocal_grad_offset(b, h, w, i) for i in range(10)]
        for first in (10, 28):
            assert [offs[first + i] - offs[first] for i in range(7)] == [lib.bsr_bottleneck_grad_offset(b, h, w, i) for i in range(7)]
        # block 0's bottleneck region: xp is 112 floats a pixel, not 272
        assert offs[46] == offs[36] + nl_bytes and offs[47] - offs[46] == pad(n * 112 * 4) and offs[48] - offs[47] == pad(n * 272 * 4)
        assert [offs[m + 1] - offs[m] for m in range(54, 61)] == [pad(n * c * 4) for c in (257, 257, 257, 257, 257, 257, 257)]
        assert lib.bsr_lower_trunk_grad_scratch_bytes(b, h, w) == offs[61] + pad(n * 99 * 4)
        assert offs[54] - offs[46] < bn257                                           # the narrow block's region is the smaller


SLOTS = "d_blob blob_bytes y3x2 y3x2_cs out2 out2_cs y3x1 y3x1_cs out1 out1_cs y3x0 y3x0_cs out0 out0_cs x0 x0_cs d_res2 B h w d_x0 grads scratch"
INTS = {"B": 2, "h": 4, "w": 32, "y3x2_cs": 288, "out2_cs": 264, "y3x1_cs": 288, "out1_cs": 264, "y3x0_cs": 288, "out0_cs": 264, "x0_cs": 120,
        "stop_after": 1}


@pytest.mark.parametrize("fn", ("bsr_lower_trunk_grad", "bsr_debug_lower_trunk_grad"))
def test_entry_point_argument_checks(lib, fn):
    slots = (SLOTS + (" stop_after" if "debug" in fn else "")).split()

    def refused(**over):
        """The code and the text of the call with the named arguments replaced."""
        args = [0]
        for slot in slots:
            value = dict(INTS, blob_bytes=lib.bsr_lower_trunk_grad_blob_bytes()).get(slot, P)
            args.append(over.get(slot, value))
        assert set(over) <= set(slots)
        return getattr(lib, fn)(*args, None), lib.bsr_last_error().decode()

    def text(what):
        return (BSR_ERR_ARG, fn + ": " + what)

    required = [s for s in slots if s not in INTS and s != "blob_bytes"]
    assert required == ["d_blob", "y3x2", "out2", "y3x1", "out1", "y3x0", "out0", "x0", "d_res2", "d_x0", "grads", "scratch"]
    for slot in required:
        assert refused(**{slot: None}) == text("null argument"), slot
    size = "B must be positive, h a multiple of 4 and w a multiple of 32 (the generator's rule at 1/8 resolution), at most 2^21 pixels in all"
    for over in (dict(B=0), dict(h=6), dict(w=16), dict(h=0), dict(B=1 << 12, h=1 << 5, w=1 << 5)):
        assert refused(**over) == text(size), over
    for nbytes in (16, lib.bsr_colour_trunk_grad_blob_bytes(), lib.bsr_lower_trunk_grad_blob_bytes() + 16):
        assert refused(blob_bytes=nbytes) == text(
            "blob_bytes must be bsr_lower_trunk_grad_blob_bytes() (pack.pack_lower_trunk_grad; the GSC widths 99 and 257 only, not TSM's 291 or RGB's 513)")
    for over in (dict(y3x2_cs=256), dict(y3x1_cs=256), dict(y3x0_cs=256), dict(out2_cs=256), dict(out1_cs=256), dict(out0_cs=256), dict(x0_cs=98)):
        assert refused(**over) == text("y3x2_cs, y3x1_cs, y3x0_cs, out2_cs, out1_cs and out0_cs must be at least 257, x0_cs at least 99"), over
    assert refused(d_blob=P + 4) == text("d_blob must be 16-byte aligned")
    for slot in required[1:-1]:
        assert refused(**{slot: P + 2}) == text("y3x2, out2, y3x1, out1, y3x0, out0, x0, d_res2, d_x0 and grads must be 4-byte aligned"), slot
    assert refused(scratch=P + 8) == text("scratch must be 256-byte aligned")
    if "stop_after" in slots:
        for stop in (-1, 73):
            assert refused(stop_after=stop) == text("stop_after must be 0..72")


def test_last_lower_trunk_refuses_null_arguments(lib):
    ptrs, strides, shape = (ctypes.c_void_p * 7)(), (ctypes.c_int * 7)(), (ctypes.c_int * 4)()
    assert lib.bsr_last_lower_trunk(None, ctypes.byref(ptrs), ctypes.byref(strides), ctypes.byref(shape)) == BSR_ERR_ARG
    assert lib.bsr_last_error().decode() == "bsr_last_lower_trunk: null argument"
    assert lib.bsr_abi_version() == 8                    # a handle needs a device: the other refusals are held on the GPU
