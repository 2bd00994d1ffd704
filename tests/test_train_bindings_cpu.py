"""The device bindings of train_step's terms (shadow_synth_gpu, train_losses_gpu, discriminator_gpu, perceptual_gpu) and their C entry
points refuse bad arguments before anything touches a GPU: the runners' image checks in their order, the gradient calls' `upstream` and
weight checks, the blob sizes, the scratch sizes and the entry points' argument checks (all ahead of the device switch; no pointer is
dereferenced).  Every text is asserted whole.  Everything here runs on a CPU-only box; the GPU tests hold the same refusals and that
nothing was launched."""
import pytest
import torch

from blindshadowremoval_amd import _lib
from blindshadowremoval_amd.build import build_library
from blindshadowremoval_amd.discriminator_gpu import Discriminators
from blindshadowremoval_amd.perceptual_gpu import Perceptual
from blindshadowremoval_amd.shadow_synth_gpu import ShadowSynth
from blindshadowremoval_amd.train_losses_gpu import TrainLosses
from on_dev0 import BSR_ERR_ARG, DEV, P, d0

DISC_SIZE = "discriminators take 1..32767 items of side 32, 64, 128 or 256, got B=%d S=%d"
VGG_SIZE = "the perceptual term takes 1..4096 items of side 32, 64, 128 or 256, got B=%d S=%d"
DISC_IMAGES = (("gt", 3), ("con_rgb", 3), ("mask_sv", 3))
VGG_IMAGES = (("gt", 3), ("con_rgb", 3))

# id, class, the call of a fresh runner's images, the images (name, channels) in the call's order, the size text
RUNNERS = [
    ("ShadowSynth", ShadowSynth, lambda r, *t: r.process_mask(*t, ()), (("mask", 1), ("gt", 3), ("img_dark", 3), ("face", 1)),
     "process_mask takes 1..65535 items of side 32, 64, 128 or 256, got B=%d S=%d"),
    ("TrainLosses", TrainLosses, lambda r, *t: r.step_losses(*t), (("img", 3), ("gt", 3), ("mask_sv", 3), ("gs", 1), ("con_rgb", 3)),
     "train_losses takes 1..65535 items of side 32, 64, 128 or 256, got B=%d S=%d"),
    ("gan_losses", Discriminators, lambda r, *t: r.gan_losses(*t), DISC_IMAGES, DISC_SIZE),
    ("gen_grad", Discriminators, lambda r, *t: r.gen_grad(*t), DISC_IMAGES, DISC_SIZE),
    ("per_loss", Perceptual, lambda r, *t: r.per_loss(*t), VGG_IMAGES, VGG_SIZE),
    ("per_loss_grad", Perceptual, lambda r, *t: r.per_loss_grad(*t), VGG_IMAGES, VGG_SIZE),
]


def _images(spec, b=1, s=32):
    return [d0(b, s, s, c) for _, c in spec]


@pytest.mark.parametrize("cls,call,spec,size_text", [r[1:] for r in RUNNERS], ids=[r[0] for r in RUNNERS])
def test_runner_image_checks(cls, call, spec, size_text):
    runner = cls(0)

    def refused(error, args):
        with pytest.raises(error) as e:
            call(runner, *args)
        assert type(e.value) is error
        return str(e.value)

    good = _images(spec)
    for k, (name, c) in enumerate(spec):
        def swapped(t):
            return good[:k] + [t] + good[k + 1:]
        for bad in (torch.zeros(1, 32, 32, c), d0(1, 32, 32, c, dtype=torch.float64), d0(1, 32, 32)):      # host, dtype, dims
            assert refused(TypeError, swapped(bad)) == "%s must be a float32 tensor [B,S,S,%d] on %s" % (name, c, DEV)
        strided = d0(1, 32, 32, 2 * c)[..., ::2]
        assert tuple(strided.shape) == (1, 32, 32, c) and not strided.is_contiguous() and strided.device == DEV
        assert refused(ValueError, swapped(strided)) == "%s must be contiguous (NHWC, dense)" % name
        assert refused(ValueError, swapped(d0(1, 32, 32, c + 1))) == "%s must be [1,32,32,%d] like gt, got (1, 32, 32, %d)" % (name, c, c + 1)
        if name == "gt":            # b and s are gt's: another batch in gt is the first other image's mistake
            first, c1 = [x for x in spec if x[0] != "gt"][0]
            assert refused(ValueError, swapped(d0(2, 32, 32, c))) == "%s must be [2,32,32,%d] like gt, got (1, 32, 32, %d)" % (first, c1, c1)
        else:
            assert refused(ValueError, swapped(d0(2, 32, 32, c))) == "%s must be [1,32,32,%d] like gt, got (2, 32, 32, %d)" % (name, c, c)
            assert refused(ValueError, swapped(d0(1, 64, 64, c))) == "%s must be [1,32,32,%d] like gt, got (1, 64, 64, %d)" % (name, c, c)
    assert refused(ValueError, _images(spec, s=48)) == size_text % (1, 48)
    assert refused(ValueError, _images(spec, b=0)) == size_text % (0, 32)
    # a type mistake in a later image comes before a size the term does not take
    assert refused(TypeError, _images(spec, s=48)[:-1] + [torch.zeros(1, 48, 48, spec[-1][1])]) == \
        "%s must be a float32 tensor [B,S,S,%d] on %s" % (spec[-1][0], spec[-1][1], DEV)


def test_perceptual_batch_cap():
    runner = Perceptual(0)
    big = _images(VGG_IMAGES, b=4097)
    for call in (runner.per_loss, runner.per_loss_grad, runner.loss):
        with pytest.raises(ValueError) as e:
            call(*big)
        assert str(e.value) == VGG_SIZE % (4097, 32)


UPSTREAM_TEXT = "upstream must be a float32 tensor of one element on %s, or None" % (DEV,)
NO_WEIGHTS = {
    Discriminators: ("the discriminators have no weights: call load_weights or restore first",
                     "the discriminators' gradient has no weights: call load_weights or restore first (load_blob brings the forward's alone)"),
    Perceptual: ("the perceptual term has no weights: call load_weights, load_blob or load_npz first",
                 "the perceptual gradient has no weights: call load_weights or load_npz first (load_blob brings the forward's alone)"),
}
# class, images, forward, gradient, the differentiable scalar, the stage-by-stage call
TERMS = [(Discriminators, DISC_IMAGES, "gan_losses", "gen_grad", "gen_loss", "grad_stages"),
         (Perceptual, VGG_IMAGES, "per_loss", "per_loss_grad", "loss", "grad_stage")]


@pytest.mark.parametrize("cls,spec,fwd,grad,scalar,stage", TERMS, ids=[t[0].__name__ for t in TERMS])
def test_grad_checks_in_order(cls, spec, fwd, grad, scalar, stage):
    runner = cls(0)                     # fresh: no weights
    good = _images(spec)
    for bad in (d0(1, dtype=torch.float64), d0(2), torch.zeros(1), 1.0):
        with pytest.raises(TypeError) as e:
            getattr(runner, grad)(*good, upstream=bad)
        assert str(e.value) == UPSTREAM_TEXT
    with pytest.raises(TypeError) as e:             # the images come before upstream
        getattr(runner, grad)(*(good[:-1] + [torch.zeros(1, 32, 32, 3)]), upstream=1.0)
    assert str(e.value) == "%s must be a float32 tensor [B,S,S,3] on %s" % (spec[-1][0], DEV)
    fwd_text, grad_text = NO_WEIGHTS[cls]
    for call, args, text in ((fwd, good, fwd_text), (grad, good, grad_text), (grad, good + [d0(1)], grad_text),
                             (stage, good + [99], grad_text),        # the weights come before stop_after's range
                             (scalar, good, fwd_text)):               # no input needs a gradient: the forward's path
        with pytest.raises(ValueError) as e:
            getattr(runner, call)(*args)
        assert str(e.value) == text, call
    needs = list(good)
    needs[1] = d0(1, 32, 32, 3).requires_grad_()    # con_rgb needs a gradient: the gradient's path
    with pytest.raises(ValueError) as e:
        getattr(runner, scalar)(*needs)
    assert str(e.value) == grad_text
    assert runner._scratch is None


def test_blob_sizes():
    for cls, text in ((Discriminators, "a discriminator blob holds 1440048 bytes, got 1024"), (Perceptual, "a VGG19 blob holds 51791360 bytes, got 1024")):
        runner = cls(0)
        with pytest.raises(ValueError) as e:
            runner.load_blob(b"\0" * 1024)
        assert str(e.value) == text
        assert runner._blob is None and runner._dgrad_blob is None


@pytest.fixture(scope="module")
def lib():
    build_library()            # no-op when the in-tree .so is fresh
    return _lib.load()


# query -> (the largest batch it takes, bytes at (1, 32), (2, 64), (1, 256))
SCRATCH = {
    "bsr_train_losses_scratch_bytes": (65535, 33536, 266752, 2131968),
    "bsr_shadow_synth_scratch_bytes": (65535, 13568, 107008, 852224),
    "bsr_disc_losses_scratch_bytes": (32767, 208128, 1656576, 13249280),
    "bsr_disc_grad_scratch_bytes": (32767, 290304, 2312448, 18496256),
    "bsr_vgg_scratch_bytes": (4096, 2687232, 21496832, 171974400),
    "bsr_vgg_grad_scratch_bytes": (4096, 3211520, 25691136, 205528832),
}


@pytest.mark.parametrize("fn", sorted(SCRATCH))
def test_scratch_bytes(lib, fn):
    query = getattr(lib, fn)
    cap, *want = SCRATCH[fn]
    assert [query(1, 32), query(2, 64), query(1, 256)] == want
    for b, s in ((0, 32), (1, 16), (1, 48), (1, 512), (cap + 1, 32)):
        assert query(b, s) == 0, (fn, b, s)
    assert query(cap, 32) > 0


# The entry points' arguments after `device` and before `stream`, as include/bsr_hip.h declares them; `?` marks a pointer that may be null.
DISC_GRAD = "d_blob blob_bytes d_dgrad_blob dgrad_bytes gt con_rgb mask_sv upstream? B S sums losses3 logits? grad scratch"
VGG_GRAD = "d_blob blob_bytes d_dgrad_blob dgrad_bytes gt con_rgb upstream? B S sums loss1 grad scratch"
ENTRIES = {
    "bsr_train_losses": "img gt mask_sv gs con_rgb B S sums losses3 mask_edge? bmaskgt? dif_grad? scratch",
    "bsr_disc_losses": "d_blob blob_bytes gt con_rgb mask_sv B S sums losses3 logits? scratch",
    "bsr_disc_gen_grad": DISC_GRAD,
    "bsr_debug_disc_gen_grad": DISC_GRAD + " stop_after",
    "bsr_vgg_per_loss": "d_blob blob_bytes gt con_rgb B S sums loss1 scratch",
    "bsr_vgg_per_loss_grad": VGG_GRAD,
    "bsr_debug_vgg_per_loss_grad": VGG_GRAD + " stop_after",
}
# by the entry point's family: the largest batch, the blob queries and the pack functions their messages name, the chain's length
FAMILY = {
    "train": (65535, None, None, None, None, None),
    "disc": (32767, "bsr_disc_blob_bytes", "pack.pack_discriminators", "bsr_disc_dgrad_blob_bytes", "pack.pack_discriminators_dgrad", 6),
    "vgg": (4096, "bsr_vgg_blob_bytes", "pack.pack_vgg", "bsr_vgg_dgrad_blob_bytes", "pack.pack_vgg_dgrad", 18),
}


@pytest.mark.parametrize("fn", sorted(ENTRIES))
def test_entry_point_argument_checks(lib, fn):
    slots = ENTRIES[fn].split()
    cap, blob_query, blob_pack, dgrad_query, dgrad_pack, launches = FAMILY[[k for k in FAMILY if "_" + k + "_" in fn][0]]

    def refused(**over):
        """The code and the text of the call with the named arguments replaced."""
        args = [0]
        for slot in slots:
            value = {"B": 2, "S": 32, "stop_after": 1, "blob_bytes": blob_query and getattr(lib, blob_query)(),
                     "dgrad_bytes": dgrad_query and getattr(lib, dgrad_query)()}.get(slot, None if slot.endswith("?") else P)
            args.append(over.get(slot.rstrip("?"), value))
        assert set(over) <= set(s.rstrip("?") for s in slots)
        return getattr(lib, fn)(*args, None), lib.bsr_last_error().decode()

    def text(what):
        return (BSR_ERR_ARG, fn + ": " + what)

    required = [s for s in slots if not s.endswith("?") and s not in ("B", "S", "stop_after", "blob_bytes", "dgrad_bytes")]
    assert len(required) >= 6 and "scratch" in required and "sums" in required
    for slot in required:
        assert refused(**{slot: None}) == text("null argument"), slot
    for b, s in ((0, 32), (2, 16), (2, 48)):
        assert refused(B=b, S=s) == text("B must be positive and S one of 32, 64, 128, 256 (reference: 256)"), (b, s)
    assert refused(B=cap + 1) == text("B must be 1..%d" % cap)
    assert refused(scratch=P + 8) == text("scratch must be 256-byte aligned")
    assert refused(sums=P + 4) == text("sums must be 8-byte aligned")
    if "blob_bytes" in slots:
        assert refused(blob_bytes=getattr(lib, blob_query)() - 4) == text("blob_bytes must be %s() (%s)" % (blob_query, blob_pack))
        if "dgrad_bytes" not in slots:
            assert refused(d_blob=P + 4) == text("d_blob must be 16-byte aligned")
    if "dgrad_bytes" in slots:
        assert refused(dgrad_bytes=getattr(lib, dgrad_query)() - 4) == text("dgrad_bytes must be %s() (%s)" % (dgrad_query, dgrad_pack))
        for blob in ("d_blob", "d_dgrad_blob"):
            assert refused(**{blob: P + 4}) == text("d_blob and d_dgrad_blob must be 16-byte aligned")
    if "stop_after" in slots:
        for stop in (-1, launches + 1):
            assert refused(stop_after=stop) == text("stop_after must be 0..%d" % launches)
