"""The objective of the reference's `train_step`: how its terms are weighted and added into g_total_loss, d_total_loss and one gradient
(train_test_GSC.py:301-336), and the folder scoring of the three commands that evaluate terms of it.  The terms themselves are stated in
train_losses.py (recon_gs, recon_c, grad), discriminator.py (gen, disc_real, disc_fake) and perceptual.py (per).

THE TOTALS, float32 in the reference's order:
  g_total_loss(recon_gs, recon_c, grad, gen, per) = ((recon * 400 + gen) + per * .005) + grad * 2,   recon = (recon_gs + recon_c) / 2
  d_total_loss(disc_real, disc_fake)              = disc_real + disc_fake

THE TOTAL GRADIENT, d g_total_loss / d (con_rgb, gs).  grad_gs is step_losses_grad's under train_losses.G_TOTAL_WEIGHTS: no other term reads
gs.  grad_con = (step_losses_grad's grad_con + gen_grad's grad) + per_loss_grad's grad under PER_WEIGHT, three float32 tensors added in
that order.  BACKWARD, the one table of the generator's backward stages, takes both on through the generator: the stages' order, what
each takes from whom and what each needs of the forward.  host_walk and device_walk run its wanted rows over one context dict, and the
flags, their help and their refusals are read from the same rows.

THE ROUTES.  HostRoute states all of that over the host statements, DeviceRoute over TrainLosses, Discriminators, Perceptual and the
stages' runners, with the same methods; a command chooses one before its loop.  The methods take (img, gt, mask_sv, gs, con_rgb) as `bring`
returns them and return losses as float32 numpy arrays and gradients in the route's own type: numpy arrays or device tensors.

`python -m blindshadowremoval_amd.objective FOLDER --vgg FILE.npz [--ckpt DIR] [--batch N] [--host] [--grad] [--grad-total] [--<stage> ...]` evaluates
the whole objective on a folder written by `python -m blindshadowremoval_amd.shadow_synth` (folder_steps): ALL_NAMES per batch and as
step-weighted means, on the device route or with --host on the host route.  With --grad each batch's line also carries per_grad_l1 and
per_grad_linf, the L1 and L-infinity norms of the perceptual term's share of the total gradient; with --grad-total instead
TOTAL_GRAD_NAMES, the norms of the total gradient; with a stage's flag beside it and its ancestors' flags also stage_grad_names(stage),
those of the gradients the stage hands on and of its variables'.  `python -m blindshadowremoval_amd.perceptual` is the same command under its earlier name.
"""
from __future__ import annotations

import contextlib
import functools
import itertools
import keyword
import os
import sys
from typing import Callable, Dict, List, NamedTuple, Optional, Tuple

import numpy as np

from . import discriminator as disc
from . import generator_grad
from . import perceptual as vgg19
from . import train_losses as tl
from .perceptual import GRAD_NAMES
from .weights import load_vgg_weights

f32 = np.float32
PER_WEIGHT = f32(.005)                # per_loss' weight in g_total_loss
LOGGED = ("recon_gs", "recon_c", "grad", "gen", "disc_real", "disc_fake")
ALL_NAMES = LOGGED + ("per", "g_total", "d_total")
TOTAL_GRAD_NAMES = ("g_total_grad_con_l1", "g_total_grad_con_linf", "g_total_grad_gs_l1", "g_total_grad_gs_linf")


def g_total_loss(recon_gs, recon_c, grad, gen, per) -> np.float32:
    """train_step's g_total_loss from its five float32 terms, in the reference's order."""
    recon_gs, recon_c, grad, gen, per = (f32(v) for v in (recon_gs, recon_c, grad, gen, per))
    recon = (recon_gs + recon_c) / f32(2)
    return f32(f32(f32(recon * f32(400)) + gen) + f32(per * f32(.005))) + f32(grad * f32(2))


def d_total_loss(disc_real, disc_fake) -> np.float32:
    return f32(disc_real) + f32(disc_fake)


def loss_record(three, gan, per) -> Dict[str, float]:
    """The losses of the three terms (float32 [3], [3], [1]) -> ALL_NAMES -> value: the six logged losses, per and the two totals."""
    vals = [float(v) for v in three] + [float(v) for v in gan] + [float(per[0])]
    vals.append(float(g_total_loss(three[0], three[1], three[2], gan[0], per[0])))
    vals.append(float(d_total_loss(gan[1], gan[2])))
    return dict(zip(ALL_NAMES, vals))


# ---- the generator's backward pass: one table of its stages, walked by both routes
class Stage(NamedTuple):
    """A stage of the backward pass.  `name` is also its flag --<name>; `parent` the stage whose data gradients it takes; `device` the
    package's runner class; `takes` the context names its `backward` takes after the generator, in that order; `probes` what `host`
    needs of the forward, as Generator.probe's names; `host` the adaptor (gen_w, context, probes) -> the stage's statement of
    generator_grad.  What it adds to the context, `gives`, are the data gradients that lead generator_grad's <NAME>_NORM_NAMES."""
    name: str
    parent: Optional[str]
    device: str
    takes: Tuple[str, ...]
    probes: Tuple[str, ...]
    host: Callable
    help: str

    @property
    def dest(self) -> str:                 # score_folder's keyword and argparse's attribute: `nonlocal` is a Python keyword
        return self.name + "_" * keyword.iskeyword(self.name)

    @property
    def gives(self) -> Tuple[str, ...]:    # a variable's name has a "/", a data gradient's has none
        return tuple(itertools.takewhile(lambda n: "/" not in n, getattr(generator_grad, self.name.upper() + "_NORM_NAMES")))


# The context starts as {img, gs, mask22, grad_con, grad_gs}; each stage that runs adds its `gives`.  The rows' order is the walks' and
# the printed columns': the colour branch from the output down, then the grey branch.  A new stage adds one row with its host adaptor.
# The non-local block's y3 is y3x5 - pad(res4) in float32, as the device chain forms it, and the heads' mask the one the forward wrote.
BACKWARD = (
    Stage("tail", None, "ColourTail", ("gs", "grad_con", "grad_gs"), ("f",),
          lambda w, c, p: generator_grad.tail_grad(w, c["gs"], p["f"], c["grad_con"], c["grad_gs"]),
          "also the norms of d g_total_loss / d f, the complete d / d gs and the colour tail's ten variable gradients"),
    Stage("decoder", "tail", "ColourDecoder", ("d_f",), ("res5", "f1", "f2", "f"),
          lambda w, c, p: generator_grad.decoder_grad(w, p["res5"], c["d_f"], acts=p),
          "also the norms of d g_total_loss / d x at res_stack/5's output and the colour decoder's twelve variable gradients"),
    Stage("nonlocal", "decoder", "NonLocalGrad", ("d_x",), ("y3x5", "res4", "res5"),
          lambda w, c, p: generator_grad.nonlocal_grad(w, (p["y3x5"][..., :257] - p["res4"][..., :257]).astype(f32), p["res4"], c["d_x"], acts={"out": p["res5"]}),
          "also the norms of d g_total_loss / d y3 at res_stack/5's bnorm3 output, of what the block's skip carries to its input, and of the non-local block's ten variable gradients"),
    Stage("bottleneck", "nonlocal", "BottleneckGrad", ("d_y3", "d_skip"), ("res4",),
          lambda w, c, p: generator_grad.bottleneck_grad(w, p["res4"], c["d_y3"], c["d_skip"]),
          "also the norms of d g_total_loss / d xin at res_stack/5's input and of the twelve variable gradients of the block's conv1, conv2, conv3 and their batch norms"),
    Stage("heads", "tail", "HeadsGrad", ("img", "mask22", "d_gs"), ("y",),
          lambda w, c, p: generator_grad.heads_grad(w, c["img"], p["y"], c["d_gs"].astype(f32), acts={"mask": (c["mask22"][..., 0:1] - c["mask22"][..., 2:3]).astype(f32)}),
          "after the other columns the norms of d g_total_loss / d y at up3's output and of the four variable gradients of the grey heads conv2 and conv3, from the tail's complete d / d gs"),
)
_ROWS = {s.name: s for s in BACKWARD}


def _above(stage: str) -> Tuple[str, ...]:
    """The stage's ancestors, the root first."""
    parent = _ROWS[stage].parent
    return () if parent is None else _above(parent) + (parent,)


STAGES = _above("bottleneck") + ("bottleneck",)            # the colour branch's chain of flags


def stage_goes_with(stage: str) -> str:
    """The flags a stage's flag needs beside it, as the refusals and the help texts spell them."""
    return " ".join(["--grad-total"] + ["--" + s for s in _above(stage)])


def refusal(wanted, grad_total: bool) -> Optional[str]:
    """None, or for the first row that is wanted without --grad-total and all of its ancestors the text that says so."""
    for s in BACKWARD:
        if s.name in wanted and not (grad_total and all(a in wanted for a in _above(s.name))):
            return "--%s goes with %s" % (s.name, stage_goes_with(s.name))
    return None


def stage_grad_names(stage: str) -> List[str]:
    """`<name>_l1`, `<name>_linf` for generator_grad's <STAGE>_NORM_NAMES: the stage's data gradients (tail: d_f, d_gs; decoder: d_x;
    nonlocal: d_y3, d_skip; bottleneck: d_xin; heads: d_y), then its variables."""
    return [n + s for n in getattr(generator_grad, stage.upper() + "_NORM_NAMES") for s in ("_l1", "_linf")]


tail_grad_names, decoder_grad_names, nonlocal_grad_names, bottleneck_grad_names, heads_grad_names = (
    functools.partial(stage_grad_names, s.name) for s in BACKWARD)


def _walk(wanted, context, run) -> Dict[str, dict]:
    """`run(row, context)` for every wanted row in the table's order, each on the context the rows before it have added to -> stage
    name -> its result."""
    context, out = dict(context), {}
    for s in BACKWARD:
        if s.name in wanted:
            out[s.name] = run(s, context)
            context.update((n, out[s.name][n]) for n in s.gives)
    return out


def device_runners(wanted, gen_w, device: int = 0) -> Dict[str, object]:
    """Stage name -> the wanted rows' runners with the generator's weights loaded."""
    import blindshadowremoval_amd as package
    runners = {s.name: getattr(package, s.device)(device) for s in BACKWARD if s.name in wanted}
    for runner in runners.values():
        runner.load_weights(gen_w)
    return runners


def device_walk(runners, generator, context, keep=()) -> Dict[str, dict]:
    """The backward pass of `generator`'s last forward over device_runners' stages, in place in its workspace -> stage name -> the
    runner's result; the stages named in `keep` also give their kept maps."""
    return _walk(runners, context, lambda s, c: runners[s.name].backward(generator, *[c[n] for n in s.takes], keep=s.name in keep))


def host_walk(wanted, gen_w, context, probes) -> Dict[str, dict]:
    """The same over the host statements, on numpy arrays: `probes` is Generator.probe's name -> array for the wanted rows' `probes`."""
    return _walk(wanted, context, lambda s, c: s.host(gen_w, c, probes))


def _stage_norms(stage: str, grads) -> List[float]:
    """stage_grad_names(stage)'s values of a stage's result on either route: name -> numpy array or device tensor."""
    arrays = {k: t.cpu().numpy() if hasattr(t, "cpu") else t for k, t in grads.items()}
    return [v for pair in getattr(generator_grad, stage + "_norms")(arrays).values() for v in pair]


# ---- the two routes
class HostRoute:
    """The objective over the three host statements, on numpy arrays."""

    def __init__(self, disc_w, vgg_w, gen_w=None, wanted=()):
        self.disc_w, self.vgg_w, self.gen_w = disc_w, vgg_w, gen_w
        self.wanted = tuple(wanted)            # the stages stage_norms walks

    def bring(self, im_d, gt_a, mask_a, gs, con_rgb, generator=None, mask22=None):
        """A step of folder_steps -> (img, gt, mask_sv, gs, con_rgb) as the methods take them, and what the wanted stages need of the
        forward: copies of their probes by name, and of mask22 if one of them takes it."""
        import torch
        torch.cuda.synchronize(im_d.device)
        kept = {k: generator.probe(k).cpu().numpy() for k in sorted({k for name in self.wanted for k in _ROWS[name].probes})}
        if mask22 is not None:                 # handed out when a wanted stage takes it
            kept["mask22"] = mask22.cpu().numpy()
        return (im_d.cpu().numpy(), gt_a, mask_a, gs.cpu().numpy(), con_rgb.cpu().numpy()), kept

    def losses(self, img, gt, mask_sv, gs, con_rgb, per_grad: bool = False):
        """The terms' losses for a batch: float32 (recon_gs, recon_c, grad), (gen, disc_real, disc_fake), (per,); then None, or with
        `per_grad` the perceptual share of the total gradient, PER_WEIGHT d per / d con_rgb."""
        per = vgg19.per_loss_grad(self.vgg_w, gt, con_rgb, upstream=PER_WEIGHT) if per_grad else vgg19.per_loss(self.vgg_w, gt, con_rgb)
        return (tl.step_losses(img, gt, mask_sv, gs, con_rgb)["losses"], disc.gan_losses(self.disc_w, gt, con_rgb, mask_sv)["losses"],
                per["loss"], per.get("grad"))

    def total_grad(self, img, gt, mask_sv, gs, con_rgb):
        """The terms' losses as `losses` gives them, then d g_total_loss / d con_rgb and d g_total_loss / d gs."""
        three = tl.step_losses_grad(img, gt, mask_sv, gs, con_rgb, upstream=np.array(tl.G_TOTAL_WEIGHTS, f32))
        gan = disc.gen_grad(self.disc_w, gt, con_rgb, mask_sv)["grad"].astype(f32)
        per = vgg19.per_loss_grad(self.vgg_w, gt, con_rgb, upstream=PER_WEIGHT)
        grad_con = (three["grad_con"] + gan) + np.asarray(per["grad"], f32)
        return three["losses"], disc.gan_losses(self.disc_w, gt, con_rgb, mask_sv)["losses"], per["loss"], grad_con, three["grad_gs"]

    def stage_norms(self, context, kept) -> Dict[str, List[float]]:
        """The walks' first context and `bring`'s second result -> wanted stage -> stage_grad_names(stage)'s values, in the table's order."""
        return {stage: _stage_norms(stage, grads) for stage, grads in host_walk(self.wanted, self.gen_w, context, kept).items()}


class DeviceRoute:
    """The objective over TrainLosses, Discriminators, Perceptual and the wanted stages' runners, on tensors of the device."""

    def __init__(self, disc_w, vgg_w, gen_w=None, device: int = 0, wanted=()):
        import torch
        from . import Discriminators, Perceptual, TrainLosses
        self.dev = torch.device("cuda", device)
        self.three, self.gan, self.per = TrainLosses(device), Discriminators(device), Perceptual(device)
        self.gan.load_weights(disc_w)
        self.per.load_weights(vgg_w)
        self.runners = device_runners(wanted, gen_w, device)
        self.three_weights = torch.tensor(tl.G_TOTAL_WEIGHTS, dtype=torch.float32).to(self.dev)
        self.per_weight = torch.tensor([float(PER_WEIGHT)], dtype=torch.float32, device=self.dev)

    def bring(self, im_d, gt_a, mask_a, gs, con_rgb, generator=None, mask22=None):
        import torch
        return (im_d, torch.from_numpy(gt_a).to(self.dev), torch.from_numpy(mask_a).to(self.dev), gs, con_rgb), dict(generator=generator, mask22=mask22)

    def losses(self, img, gt, mask_sv, gs, con_rgb, per_grad: bool = False):
        three, gan = self.three.step_losses(img, gt, mask_sv, gs, con_rgb)[0].cpu().numpy(), self.gan.gan_losses(gt, con_rgb, mask_sv)[0].cpu().numpy()
        if not per_grad:
            return three, gan, self.per.per_loss(gt, con_rgb)[0].cpu().numpy(), None
        per = self.per.per_loss_grad(gt, con_rgb, upstream=self.per_weight)
        return three, gan, per[0].cpu().numpy(), per[2]

    def total_grad(self, img, gt, mask_sv, gs, con_rgb):
        three = self.three.step_losses_grad(img, gt, mask_sv, gs, con_rgb, upstream=self.three_weights)
        gan = self.gan.gen_grad(gt, con_rgb, mask_sv)
        per = self.per.per_loss_grad(gt, con_rgb, upstream=self.per_weight)
        grad_con = (three[3] + gan[2]) + per[2]
        return three[0].cpu().numpy(), gan[0].cpu().numpy(), per[0].cpu().numpy(), grad_con, three[2]

    def stage_norms(self, context, kept) -> Dict[str, List[float]]:
        return {stage: _stage_norms(stage, grads) for stage, grads in device_walk(self.runners, kept["generator"], context).items()}


def _norms(grad) -> List[float]:
    """The L1 and L-infinity norms of a gradient of either route: the sum and the largest of its magnitudes, in float64."""
    return list(generator_grad.grad_norms({"": grad.cpu().numpy() if hasattr(grad, "cpu") else grad}, ("",))[""])


# ---- the folder scoring
def discriminator_weights(ckpt: Optional[str], who: str) -> Dict[str, np.ndarray]:
    """The discriminators' weights of the latest checkpoint under `ckpt`, of init_discriminator_weights(1) without it."""
    if ckpt is None:
        from .weights import init_discriminator_weights
        return init_discriminator_weights(1)
    from .tf_bundle import latest_checkpoint, load_discriminator_weights
    prefix = latest_checkpoint(ckpt)
    if prefix is None:
        raise FileNotFoundError("%s: no checkpoint under %s" % (who, ckpt))
    return load_discriminator_weights(prefix)


def folder_steps(folder: str, ckpt: Optional[str], batch: int, device: int, who: str, with_generator: bool = False, with_mask22: bool = False):
    """The folder handling of the commands that score a generator on synthesised pairs: for every step of `batch` item folders
    `<folder>/<name>/` (the last one may hold fewer) yields (step, steps, img on the device, gt [b,S,S,3], mask_sv [b,S,S,3] (numpy), gs,
    con_rgb (the generator's outputs on the device)), with `with_generator` also the generator itself, whose last forward is the
    step's (Generator.last_f, Generator.probe), and with `with_mask22` after it the forward's mask22.  The generator's weights come from the latest checkpoint under `ckpt`, from init_weights
    without it."""
    import torch
    from . import Generator, init_weights
    from .dataset import Dataset
    from .fsrnet import SPLIT_FFHQ, Config
    from .pngio import read_rgb_u8
    cfg = Config(device)
    cfg.DATA_DIR_TEST = [os.path.join(folder, "*")]
    ds = Dataset(cfg, "test")
    if not ds.name_list:
        raise ValueError("%s: no item folder with a .npy under %s" % (who, folder))
    S = cfg.IMG_SIZE
    dev = torch.device("cuda", device)
    gen = Generator(device=device)
    if ckpt is not None:
        gen.restore(ckpt)
        gen._require_weights()
    else:
        gen.load_weights(init_weights(1))
    batch = max(1, int(batch))
    steps = (len(ds.name_list) + batch - 1) // batch
    try:
        for step in range(steps):
            names = ds.name_list[step * batch:(step + 1) * batch]
            rows, gts, masks = [], [], []
            for lm_path in names:
                element = next(ds.feed)[0]
                rows.append(torch.as_tensor(np.asarray(element)).reshape(-1, S, S, sum(SPLIT_FFHQ))[:1])
                stem = os.path.splitext(lm_path)[0]
                for path, dst in ((stem + "-gt.png", gts), (stem + "-mask.png", masks)):
                    a = read_rgb_u8(path)
                    if a.shape != (S, S, 3):
                        raise ValueError("%s: %s is %s, not %d x %d x 3" % (who, path, a.shape, S, S))
                    dst.append(a.astype(f32) / f32(255))
            im, _, uv, _, _ = torch.split(torch.cat(rows, 0).float(), list(SPLIT_FFHQ), dim=3)
            im_d = im.contiguous().to(dev)
            gs, con_rgb, mask22, _ = gen(im_d, uv.contiguous().to(dev), None, chuck=2, training=False)
            yield ((step, steps, im_d, np.stack(gts), np.stack(masks), gs, con_rgb) + ((gen,) if with_generator else ())
                   + ((mask22,) if with_mask22 else ()))
    finally:                    # also when the consumer stops early or raises: the handle is closed with the generator
        gen.close()


def score_steps(folder: str, ckpt: Optional[str], batch: int, device: int, who: str, step_fn: Callable, quiet: bool = False,
                with_generator: bool = False, nine_digits: bool = False, with_mask22: bool = False) -> Dict[str, float]:
    """The loop of the three commands: `step_fn(img, gt, mask_sv, gs, con_rgb[, generator])` on every step of folder_steps returns the
    step's record name -> value, and a list of (name, value) that is printed with it and not averaged -> the step-weighted means of the
    records.  Each step prints the running means as Logging.display does, with a blank line after the last; with `nine_digits` it
    prints "step/steps " and the step's own values as name:%.9g."""
    from .fsrnet import Logging
    acc: Dict[str, List[float]] = {}
    with contextlib.closing(folder_steps(folder, ckpt, batch, device, who, with_generator, with_mask22)) as batches:      # closes the generator handle on any way out
        for step, steps, *tensors in batches:
            record, extras = step_fn(*tensors)
            Logging.accumulate(acc, record)
            if quiet:
                continue
            if nine_digits:
                print("%d/%d " % (step + 1, steps) + ", ".join("%s:%.9g" % kv for kv in list(record.items()) + list(extras)), flush=True)
            else:
                print(Logging.format_line(acc, step, steps), end="", flush=True)
    if not quiet and not nine_digits:
        print("")
    return {k: s / max(c, 1) for k, (s, c) in acc.items()}


def score_folder(folder: str, vgg: str, ckpt: Optional[str] = None, batch: int = 8, host: bool = False, device: int = 0,
                 quiet: bool = False, grad: bool = False, grad_total: bool = False, tail: bool = False, decoder: bool = False,
                 nonlocal_: bool = False, bottleneck: bool = False, heads: bool = False) -> Dict[str, float]:
    """Every item folder `<folder>/<name>/` the shadow_synth command wrote -> the step-weighted means of ALL_NAMES.  `vgg`: the `.npz`
    of weights.load_vgg_weights; the other weights come from the latest checkpoint under `ckpt`, from init_weights and
    init_discriminator_weights without it.  `grad`, `grad_total` and BACKWARD's stages add to each batch's line what their flags do."""
    given = dict(tail=tail, decoder=decoder, nonlocal_=nonlocal_, bottleneck=bottleneck, heads=heads)
    wanted = tuple(s.name for s in BACKWARD if given[s.dest])
    refused = refusal(wanted, grad_total)
    if refused:
        raise ValueError("perceptual: " + refused)
    vgg_w = load_vgg_weights(vgg)
    gen_w = None
    if wanted:
        from .tf_bundle import latest_checkpoint, load_generator_weights
        from .weights import init_weights
        gen_w = init_weights(1) if ckpt is None else load_generator_weights(latest_checkpoint(ckpt))
    disc_w = discriminator_weights(ckpt, "perceptual")
    route = HostRoute(disc_w, vgg_w, gen_w, wanted) if host else DeviceRoute(disc_w, vgg_w, gen_w, device, wanted)

    def step(*tensors):
        arrays, kept = route.bring(*tensors)
        if not grad_total:
            three, gan, per, g = route.losses(*arrays, per_grad=grad)
            return loss_record(three, gan, per), list(zip(GRAD_NAMES, _norms(g))) if grad else []
        three, gan, per, grad_con, grad_gs = route.total_grad(*arrays)
        extras = list(zip(TOTAL_GRAD_NAMES, _norms(grad_con) + _norms(grad_gs)))
        context = dict(img=arrays[0], gs=arrays[3], mask22=kept.get("mask22"), grad_con=grad_con, grad_gs=grad_gs)
        for stage, norms in route.stage_norms(context, kept).items():
            extras += zip(stage_grad_names(stage), norms)
        return loss_record(three, gan, per), extras

    return score_steps(folder, ckpt, batch, device, "perceptual", step, quiet, with_generator=bool(wanted), nine_digits=True,
                       with_mask22=any("mask22" in _ROWS[name].takes for name in wanted))


def main(argv=None) -> int:
    import argparse
    ap = argparse.ArgumentParser(prog="python -m blindshadowremoval_amd.objective",
                                 description="Evaluate train_step's whole objective (six logged losses, per, g_total, d_total) on synthesised pairs.")
    ap.add_argument("folder")
    ap.add_argument("--vgg", required=True, help="the VGG19 variables as an .npz (weights.load_vgg_weights)")
    ap.add_argument("--ckpt", default=None, help="checkpoint directory; without it the weights come from init_weights / init_discriminator_weights")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--host", action="store_true", help="compute every term with the host statements instead of the device chains")
    ap.add_argument("--grad", action="store_true", help="per batch also the L1 and L-infinity norms of 0.005 d per / d con_rgb, this term's share of g_total_loss' gradient")
    ap.add_argument("--grad-total", action="store_true", help="per batch instead the norms of the whole d g_total_loss / d con_rgb and d g_total_loss / d gs")
    for s in BACKWARD:
        ap.add_argument("--" + s.name, dest=s.dest, action="store_true", help="with %s: %s" % (stage_goes_with(s.name), s.help))
    a = ap.parse_args(argv)
    stages = {s.dest: getattr(a, s.dest) for s in BACKWARD}
    refused = refusal([s.name for s in BACKWARD if stages[s.dest]], a.grad_total)
    if refused:
        ap.error(refused)
    means = score_folder(a.folder, a.vgg, ckpt=a.ckpt, batch=a.batch, host=a.host, grad=a.grad, grad_total=a.grad_total, **stages)
    print(", ".join("%s:%.9g" % (k, means[k]) for k in ALL_NAMES))
    return 0


if __name__ == "__main__":
    sys.exit(main())
