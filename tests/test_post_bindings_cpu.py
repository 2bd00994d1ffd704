"""The device post-processing bindings (ucb_post_gpu, ucb_post_rgb_gpu, ucb_post_tsm_gpu, sfw_post_gpu) and their C entry points refuse
bad arguments before anything touches a GPU: the runners' input checks, the scratch sizes, the entry points' argument checks (all ahead
of the device switch; no pointer is dereferenced) and the per-item status texts.  Everything here runs on a CPU-only box."""
import numpy as np
import pytest
import torch

from blindshadowremoval_amd import _lib
from blindshadowremoval_amd import sfw_post_gpu, ucb_post_gpu, ucb_post_rgb_gpu, ucb_post_tsm_gpu
from blindshadowremoval_amd.build import build_library
from on_dev0 import BSR_ERR_ARG, DEV, P, d0

S_TEXT = "supports S in {32, 64, 128, 256} (reference: 256)"
U8 = torch.uint8

# runner, good inputs (B = 2, S = 32) by name, the shape message's head, then the message of a good shape at S = 16
RUNNERS = [
    (ucb_post_gpu.UcbPostDevice, [("rows10", (2, 32, 32, 10), torch.float32), ("masks", (2, 7, 32, 32), U8), ("boxes", (2, 4), torch.float32)],
     "shapes: rows10 [B,S,S,10], masks [B,7,S,S], boxes [B,4]; got ", "bsr_ucb_post " + S_TEXT + ", got 16"),
    (ucb_post_rgb_gpu.UcbPostRgbDevice, [("rows9", (2, 32, 32, 9), torch.float32), ("masks", (2, 32, 32), U8), ("boxes", (2, 4), torch.float32)],
     "shapes: rows9 [B,S,S,9], masks [B,S,S], boxes [B,4]; got ", "bsr_ucb_post_rgb " + S_TEXT + ", got 16"),
    (ucb_post_tsm_gpu.UcbPostTsmDevice, [("rows", (2, 32, 32, 13), torch.float32), ("masks", (2, 3, 32, 32), U8), ("boxes", (2, 4), torch.float32)],
     "shapes: rows [B,S,S,13], masks [B,3,S,S], boxes [B,4]; got ", "bsr_ucb_post_tsm " + S_TEXT + ", got 16"),
    (sfw_post_gpu.SfwScoreDevice, [("rows3", (2, 32, 32, 3), torch.float32)],
     "rows3 must be [B,S,S,3], got ", "bsr_sfw_score supports B > 0 and S in {32, 64, 128, 256} (reference: 256), got B=2 S=16"),
]


def _at_s16(shape):
    return tuple(16 if d == 32 else d for d in shape)


@pytest.mark.parametrize("cls,spec,shape_msg,s_msg", RUNNERS, ids=[r[0].__name__ for r in RUNNERS])
def test_runner_input_checks(cls, spec, shape_msg, s_msg):
    run = cls(device=0).run
    good = [d0(*shp, dtype=dt) for _, shp, dt in spec]
    for k, (name, shp, dt) in enumerate(spec):
        dt_text = "float32" if cls is sfw_post_gpu.SfwScoreDevice else dt          # the SFW runner names its dtype without "torch."
        type_msg = "%s must be a %s tensor with %d dims on %s" % (name, dt_text, len(shp), DEV)
        for bad in (torch.zeros(shp, dtype=dt),                                          # on the host
                    d0(*shp, dtype=torch.float64 if dt == torch.float32 else torch.int32),  # wrong dtype
                    d0(*shp[:-1], dtype=dt)):                                           # wrong number of dims
            args = list(good)
            args[k] = bad
            with pytest.raises(TypeError) as e:
                run(*args)
            assert str(e.value) == type_msg
        args = list(good)
        wrong = list(shp)
        wrong[-1] += 1
        args[k] = d0(*wrong, dtype=dt)
        with pytest.raises(ValueError) as e:
            run(*args)
        got = tuple(tuple(a.shape) for a in args)
        assert str(e.value) == shape_msg + ("%s %s %s" % got if len(got) == 3 else "%s" % (got[0],))
    with pytest.raises(ValueError) as e:                        # a consistent shape of a size the library does not take
        run(*[d0(*_at_s16(shp), dtype=dt) for _, shp, dt in spec])
    assert str(e.value) == s_msg


def test_empty_batch_is_refused():
    with pytest.raises(ValueError) as e:
        ucb_post_gpu.UcbPostDevice(0).run(d0(0, 32, 32, 10), d0(0, 7, 32, 32, dtype=U8), d0(0, 4))
    assert str(e.value) == "bsr_ucb_post " + S_TEXT + ", got 32"
    with pytest.raises(ValueError) as e:
        sfw_post_gpu.SfwScoreDevice(0).run(d0(0, 32, 32, 3))
    assert str(e.value) == "bsr_sfw_score supports B > 0 and S in {32, 64, 128, 256} (reference: 256), got B=0 S=32"


@pytest.fixture(scope="module")
def lib():
    build_library()            # no-op when the in-tree .so is fresh
    return _lib.load()


SCRATCH = {   # (B, S) -> bytes; every pair not listed is 0 (B < 1, or S outside {32, 64, 128, 256})
    "bsr_ucb_post_scratch_bytes": {(1, 32): 112384, (1, 256): 7154176, (16, 32): 1798144, (16, 256): 114466816},
    "bsr_ucb_post_rgb_scratch_bytes": {(1, 32): 24832, (1, 256): 1576960, (16, 32): 397312, (16, 256): 25231360},
    "bsr_ucb_post_tsm_scratch_bytes": {(1, 32): 54784, (1, 256): 3485952, (16, 32): 876544, (16, 256): 55775232},
    "bsr_sfw_score_scratch_bytes": {(1, 32): 16640, (1, 256): 266496, (16, 32): 266240, (16, 256): 4263936},
}


@pytest.mark.parametrize("fn", sorted(SCRATCH))
def test_scratch_bytes(lib, fn):
    for b in (0, 1, 16):
        for s in (16, 32, 256, 512):
            assert getattr(lib, fn)(b, s) == SCRATCH[fn].get((b, s), 0), (fn, b, s)


def _ucb_args(B, S, scratch, n_out):
    # device, rows, masks, boxes, B, S, outputs (losses, [nose_stats,] strips, figs, status), scratch, stream
    return [0, P, P, P, B, S] + [P] * n_out + [scratch, None]


ENTRIES = {
    "bsr_ucb_post": lambda B=2, S=32, scratch=P: _ucb_args(B, S, scratch, 4),
    "bsr_ucb_post_rgb": lambda B=2, S=32, scratch=P: _ucb_args(B, S, scratch, 4),
    "bsr_ucb_post_tsm": lambda B=2, S=32, scratch=P: _ucb_args(B, S, scratch, 5),
    "bsr_sfw_score": lambda B=2, S=32, scratch=P: [0, P, B, S, P, P, P, P, P, scratch, None],
}


@pytest.mark.parametrize("fn", sorted(ENTRIES))
def test_entry_point_argument_checks(lib, fn):
    call = getattr(lib, fn)
    ok = ENTRIES[fn]()
    for i, a in enumerate(ok):                 # each required pointer (not figs, not the stream) set to null in turn
        if a != P or (fn != "bsr_sfw_score" and i == len(ok) - 4):
            continue
        args = list(ok)
        args[i] = None
        assert call(*args) == BSR_ERR_ARG, (fn, i)
        assert lib.bsr_last_error().decode() == fn + ": null argument"
    size_text = fn + ": B must be positive and S one of 32, 64, 128, 256 (reference: 256)"
    for b, s in ((0, 32), (-1, 32), (2, 16), (2, 48), (2, 512)):
        assert call(*ENTRIES[fn](B=b, S=s)) == BSR_ERR_ARG, (fn, b, s)
        assert lib.bsr_last_error().decode() == size_text
    for off in (1, 16, 128):
        assert call(*ENTRIES[fn](scratch=P + off)) == BSR_ERR_ARG, (fn, off)
        assert lib.bsr_last_error().decode() == fn + ": scratch must be 256-byte aligned"


UCB_TEXTS = {1: "a segmentation mask the reference takes a bounding box of (nose / mouth / forehead / face) is empty after the resize",
             2: "the crop box is larger than the image or empty"}
TSM_TEXTS = {1: "the nose mask has no pixel of level 255 (the reference takes the bounding box of its pixels equal to 1)",
             2: "the crop box is larger than the image or empty"}


@pytest.mark.parametrize("mod,prefix,texts", [(ucb_post_gpu, "UCB post-processing", UCB_TEXTS), (ucb_post_rgb_gpu, "UCB post-processing", UCB_TEXTS),
                                              (ucb_post_tsm_gpu, "TSM UCB post-processing", TSM_TEXTS)], ids=["ucb", "rgb", "tsm"])
def test_ucb_raise_for_status(mod, prefix, texts):
    mod.raise_for_status([0, 0, 0])
    mod.raise_for_status(np.zeros(3, np.int32), ["a", "b", "c"])
    for st in (1, 2, 3, 7, -1):
        text = texts.get(st, "status %d" % st)
        for names, who in ((None, "1"), (["a", "b", "c"], "b")):
            with pytest.raises(ValueError) as e:
                mod.raise_for_status(np.array([0, st, 1], np.int32), names)
            assert str(e.value) == "%s of item %s: %s" % (prefix, who, text)


def test_sfw_raise_for_status():
    sfw_post_gpu.raise_for_status(np.zeros(3, np.int32), ["a", "b", "c"])
    sfw_post_gpu.raise_for_status(np.zeros((2, 1), np.int32), [])
    with pytest.raises(ValueError) as e:
        sfw_post_gpu.raise_for_status(np.array([0, 3, 1], np.int32), ["a", "b", "c"])
    assert str(e.value) == "SFW item b: mask_pred contains NaN or infinity (roc_auc_score raises here)"
    with pytest.raises(ValueError) as e:
        sfw_post_gpu.raise_for_status(np.array([[0], [3]], np.int32), ["a"])           # fewer names than items: the index
    assert str(e.value) == "SFW item 1: mask_pred contains NaN or infinity (roc_auc_score raises here)"
    for st in (1, 2, 4, 9, -1):
        with pytest.raises(RuntimeError) as e:
            sfw_post_gpu.raise_for_status(np.array([0, st, 3], np.int32), ["a", "b", "c"])
        assert not isinstance(e.value, ValueError)
        assert str(e.value) == "SFW item b: scoring status %d" % st
        with pytest.raises(RuntimeError) as e:
            sfw_post_gpu.raise_for_status(np.array([0, st], np.int32), ["a"])
        assert str(e.value) == "SFW item 1: scoring status %d" % st
