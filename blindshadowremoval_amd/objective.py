"""The objective of the reference's `train_step`: how its terms are weighted and added into g_total_loss, d_total_loss and one gradient
(train_test_GSC.py:301-336), and the folder scoring of the three commands that evaluate terms of it.  The terms themselves are stated in
train_losses.py (recon_gs, recon_c, grad), discriminator.py (gen, disc_real, disc_fake) and perceptual.py (per).

THE TOTALS, float32 in the reference's order:
  g_total_loss(recon_gs, recon_c, grad, gen, per) = ((recon * 400 + gen) + per * .005) + grad * 2,   recon = (recon_gs + recon_c) / 2
  d_total_loss(disc_real, disc_fake)              = disc_real + disc_fake

THE TOTAL GRADIENT, d g_total_loss / d (con_rgb, gs).  grad_gs is step_losses_grad's under train_losses.G_TOTAL_WEIGHTS: no other term reads
gs.  grad_con = (step_losses_grad's grad_con + gen_grad's grad) + per_loss_grad's grad under PER_WEIGHT, three float32 tensors added in
that order.  Through the generator's colour tail both become d / d f at clr_up3's output, the complete d / d gs and the gradients of the
tail's ten variables (generator_grad.tail_grad), and d / d f through the colour decoder becomes d / d x at res_stack/5's output and the
gradients of the decoder's twelve variables (generator_grad.decoder_grad).

THE ROUTES.  HostRoute states all of that over the three host statements, DeviceRoute over TrainLosses, Discriminators, Perceptual and
ColourTail, with the same methods; a command chooses one before its loop.  The methods take (img, gt, mask_sv, gs, con_rgb) as `bring`
returns them and return losses as float32 numpy arrays and gradients in the route's own type: numpy arrays or device tensors.

`python -m blindshadowremoval_amd.objective FOLDER --vgg FILE.npz [--ckpt DIR] [--batch N] [--host] [--grad] [--grad-total] [--tail] [--decoder]` evaluates
the whole objective on a folder written by `python -m blindshadowremoval_amd.shadow_synth` (folder_steps): ALL_NAMES per batch and as
step-weighted means, on the device route or with --host on the host route.  With --grad each batch's line also carries per_grad_l1 and
per_grad_linf, the L1 and L-infinity norms of the perceptual term's share of the total gradient; with --grad-total instead
TOTAL_GRAD_NAMES, the norms of the total gradient; with --tail beside it also tail_grad_names(), those of the total gradient taken
through the colour tail, and with --decoder beside both decoder_grad_names(), those of d_f taken on through the colour decoder.  `python -m blindshadowremoval_amd.perceptual` is the same command under its earlier name.
"""
from __future__ import annotations

import contextlib
import functools
import os
import sys
from typing import Callable, Dict, List, Optional

import numpy as np

from . import discriminator as disc
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


# the stages of the generator's backward pass from the output down: generator_grad's <STAGE>_NORM_NAMES and <stage>_norms, and here
# <stage>_grad_names() and the routes' <stage>_norms
STAGES = ("tail", "decoder", "nonlocal", "bottleneck")


def stage_grad_names(stage: str) -> List[str]:
    """`<name>_l1`, `<name>_linf` for generator_grad's <STAGE>_NORM_NAMES: the stage's data gradients (tail: d_f, d_gs; decoder: d_x;
    nonlocal: d_y3, d_skip; bottleneck: d_xin; heads: d_y), then its variables."""
    from . import generator_grad
    return [n + s for n in getattr(generator_grad, stage.upper() + "_NORM_NAMES") for s in ("_l1", "_linf")]


tail_grad_names, decoder_grad_names, nonlocal_grad_names, bottleneck_grad_names = (functools.partial(stage_grad_names, stage) for stage in STAGES)
heads_grad_names = functools.partial(stage_grad_names, "heads")      # the grey branch's first stage: its columns follow the colour branch's


def _stage_norms(stage: str, grads) -> List[float]:
    """stage_grad_names(stage)'s values of a stage's result on either route: name -> numpy array or device tensor."""
    from . import generator_grad
    arrays = {k: t.cpu().numpy() if hasattr(t, "cpu") else t for k, t in grads.items()}
    return [v for pair in getattr(generator_grad, stage + "_norms")(arrays).values() for v in pair]


# ---- the two routes
class HostRoute:
    """The objective over the three host statements, on numpy arrays."""

    def __init__(self, disc_w, vgg_w, gen_w=None, decoder: bool = False, nonlocal_: bool = False, bottleneck: bool = False, heads: bool = False):
        self.disc_w, self.vgg_w, self.gen_w = disc_w, vgg_w, gen_w
        self.decoder = decoder                 # --decoder: bring also copies the decoder's kept tensors
        self.nonlocal_ = nonlocal_             # --nonlocal: and res_stack/5's
        self.heads = heads                     # --heads: and the heads' input y and the forward's mask22

    def bring(self, im_d, gt_a, mask_a, gs, con_rgb, generator=None, mask22=None):
        """A step of folder_steps -> (img, gt, mask_sv, gs, con_rgb) as the methods take them, and f: a copy of the generator's, if one is given."""
        import torch
        torch.cuda.synchronize(im_d.device)
        f = None if generator is None else generator.probe("f").cpu().numpy()
        if self.heads:
            self.y, self.mask22 = generator.probe("y").cpu().numpy(), mask22.cpu().numpy()
        if self.decoder:
            self.acts = {k: generator.probe(k).cpu().numpy() for k in ("res5", "f1", "f2")}
            self.acts["f"] = f
        if self.nonlocal_:
            self.block5 = {k: generator.probe(k).cpu().numpy() for k in ("y3x5", "res4")}
        return (im_d.cpu().numpy(), gt_a, mask_a, gs.cpu().numpy(), con_rgb.cpu().numpy()), f

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

    def tail_norms(self, gs, f, grad_con, grad_gs) -> List[float]:
        """tail_grad_names() of the two gradients taken through the colour tail at f [B,H,W,64]."""
        from .generator_grad import tail_grad
        grads = tail_grad(self.gen_w, gs, f, grad_con, grad_gs)
        self.d_f, self.d_gs = grads["d_f"], grads["d_gs"]
        return _stage_norms("tail", grads)

    def decoder_norms(self) -> List[float]:
        """decoder_grad_names() of the last tail_norms' d_f taken through the colour decoder at the generator's kept res5, f1, f2, f."""
        from .generator_grad import decoder_grad
        grads = decoder_grad(self.gen_w, self.acts["res5"], self.d_f, acts=self.acts)
        self.d_x = grads["d_x"]
        return _stage_norms("decoder", grads)

    def nonlocal_norms(self) -> List[float]:
        """nonlocal_grad_names() of the last decoder_norms' d_x taken through res_stack/5's upper half at the generator's kept y3x5, res4
        and res5: y3 = y3x5 - pad(res4) in float32, as the device chain forms it."""
        from .generator_grad import nonlocal_grad
        xin = self.block5["res4"]
        y3 = (self.block5["y3x5"][..., :257] - xin[..., :257]).astype(f32)
        grads = nonlocal_grad(self.gen_w, y3, xin, self.d_x, acts={"out": self.acts["res5"]})
        self.d_y3, self.d_skip = grads["d_y3"], grads["d_skip"]
        return _stage_norms("nonlocal", grads)

    def bottleneck_norms(self) -> List[float]:
        """bottleneck_grad_names() of the last nonlocal_norms' d_y3 and d_skip taken through res_stack/5's lower half at the generator's
        kept res4."""
        from .generator_grad import bottleneck_grad
        return _stage_norms("bottleneck", bottleneck_grad(self.gen_w, self.block5["res4"], self.d_y3, self.d_skip))

    def heads_norms(self, img) -> List[float]:
        """heads_grad_names() of the last tail_norms' complete d_gs taken through the grey heads at the generator's kept y, with the mask
        the forward wrote (mask22[..., 0] - mask22[..., 2]), as the device chain reads it."""
        from .generator_grad import heads_grad
        mask = (self.mask22[..., 0:1] - self.mask22[..., 2:3]).astype(f32)
        return _stage_norms("heads", heads_grad(self.gen_w, img, self.y, self.d_gs.astype(f32), acts={"mask": mask}))


class DeviceRoute:
    """The objective over TrainLosses, Discriminators, Perceptual and ColourTail, on tensors of the device; f is read in the generator's workspace."""

    def __init__(self, disc_w, vgg_w, gen_w=None, device: int = 0, decoder: bool = False, nonlocal_: bool = False, bottleneck: bool = False,
                 heads: bool = False):
        import torch
        from . import BottleneckGrad, ColourDecoder, ColourTail, Discriminators, HeadsGrad, NonLocalGrad, Perceptual, TrainLosses
        self.dev = torch.device("cuda", device)
        self.three, self.gan, self.per = TrainLosses(device), Discriminators(device), Perceptual(device)
        self.gan.load_weights(disc_w)
        self.per.load_weights(vgg_w)
        if gen_w is not None:
            for name, stage, wanted in (("tail", ColourTail, True), ("dec", ColourDecoder, decoder), ("nl", NonLocalGrad, nonlocal_),
                                       ("bn", BottleneckGrad, bottleneck), ("hd", HeadsGrad, heads)):
                if wanted:
                    setattr(self, name, stage(device))
                    getattr(self, name).load_weights(gen_w)
        self.three_weights = torch.tensor(tl.G_TOTAL_WEIGHTS, dtype=torch.float32).to(self.dev)
        self.per_weight = torch.tensor([float(PER_WEIGHT)], dtype=torch.float32, device=self.dev)

    def bring(self, im_d, gt_a, mask_a, gs, con_rgb, generator=None, mask22=None):
        import torch
        self.mask22 = mask22
        return (im_d, torch.from_numpy(gt_a).to(self.dev), torch.from_numpy(mask_a).to(self.dev), gs, con_rgb), generator

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

    def tail_norms(self, gs, generator, grad_con, grad_gs) -> List[float]:
        res = self.tail.backward(generator, gs, grad_con, grad_gs)
        self.d_f, self.d_gs, self.generator = res["d_f"], res["d_gs"], generator
        return _stage_norms("tail", res)

    def decoder_norms(self) -> List[float]:
        res = self.dec.backward(self.generator, self.d_f)
        self.d_x = res["d_x"]
        return _stage_norms("decoder", res)

    def nonlocal_norms(self) -> List[float]:
        res = self.nl.backward(self.generator, self.d_x)
        self.d_y3, self.d_skip = res["d_y3"], res["d_skip"]
        return _stage_norms("nonlocal", res)

    def bottleneck_norms(self) -> List[float]:
        return _stage_norms("bottleneck", self.bn.backward(self.generator, self.d_y3, self.d_skip))

    def heads_norms(self, img) -> List[float]:
        return _stage_norms("heads", self.hd.backward(self.generator, img, self.mask22, self.d_gs))


def _norms(grad) -> List[float]:
    """The L1 and L-infinity norms of a gradient of either route: the sum and the largest of its magnitudes, in float64."""
    g = np.abs(np.asarray(grad.cpu().numpy() if hasattr(grad, "cpu") else grad, np.float64))
    return [float(g.sum()), float(g.max())]


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
    init_discriminator_weights without it.  `grad`, `grad_total`, `tail`, `decoder`, `nonlocal_` and `bottleneck` add to each batch's line what
    --grad, --grad-total, --tail, --decoder, --nonlocal and --bottleneck do; `heads` appends what --heads does after them."""
    if tail and not grad_total:
        raise ValueError("perceptual: --tail goes with --grad-total")
    if decoder and not tail:
        raise ValueError("perceptual: --decoder goes with --grad-total --tail")
    if nonlocal_ and not decoder:
        raise ValueError("perceptual: --nonlocal goes with --grad-total --tail --decoder")
    if bottleneck and not nonlocal_:
        raise ValueError("perceptual: --bottleneck goes with --grad-total --tail --decoder --nonlocal")
    if heads and not tail:
        raise ValueError("perceptual: --heads goes with --grad-total --tail")
    vgg_w = load_vgg_weights(vgg)
    gen_w = None
    if tail:
        from .tf_bundle import latest_checkpoint, load_generator_weights
        from .weights import init_weights
        gen_w = init_weights(1) if ckpt is None else load_generator_weights(latest_checkpoint(ckpt))
    disc_w = discriminator_weights(ckpt, "perceptual")
    route = (HostRoute(disc_w, vgg_w, gen_w, decoder=decoder, nonlocal_=nonlocal_, bottleneck=bottleneck, heads=heads) if host
             else DeviceRoute(disc_w, vgg_w, gen_w, device, decoder=decoder, nonlocal_=nonlocal_, bottleneck=bottleneck, heads=heads))

    def step(*tensors):
        arrays, f = route.bring(*tensors)
        if not grad_total:
            three, gan, per, g = route.losses(*arrays, per_grad=grad)
            return loss_record(three, gan, per), list(zip(GRAD_NAMES, _norms(g))) if grad else []
        three, gan, per, grad_con, grad_gs = route.total_grad(*arrays)
        extras = list(zip(TOTAL_GRAD_NAMES, _norms(grad_con) + _norms(grad_gs)))
        for stage, wanted, args in zip(STAGES, (tail, decoder, nonlocal_, bottleneck), ((arrays[3], f, grad_con, grad_gs), (), (), ())):
            if wanted:
                extras += zip(stage_grad_names(stage), getattr(route, stage + "_norms")(*args))
        if heads:
            extras += zip(heads_grad_names(), route.heads_norms(arrays[0]))
        return loss_record(three, gan, per), extras

    return score_steps(folder, ckpt, batch, device, "perceptual", step, quiet, with_generator=tail, nine_digits=True, with_mask22=heads)


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
    ap.add_argument("--tail", action="store_true", help="with --grad-total: also the norms of d g_total_loss / d f, the complete d / d gs and the colour tail's ten variable gradients")
    ap.add_argument("--decoder", action="store_true", help="with --grad-total --tail: also the norms of d g_total_loss / d x at res_stack/5's output and the colour decoder's twelve variable gradients")
    ap.add_argument("--nonlocal", dest="nonlocal_", action="store_true", help="with --grad-total --tail --decoder: also the norms of d g_total_loss / d y3 at res_stack/5's bnorm3 output, of what the block's skip carries to its input, and of the non-local block's ten variable gradients")
    ap.add_argument("--bottleneck", action="store_true", help="with --grad-total --tail --decoder --nonlocal: also the norms of d g_total_loss / d xin at res_stack/5's input and of the twelve variable gradients of the block's conv1, conv2, conv3 and their batch norms")
    ap.add_argument("--heads", action="store_true", help="with --grad-total --tail: after the other columns the norms of d g_total_loss / d y at up3's output and of the four variable gradients of the grey heads conv2 and conv3, from the tail's complete d / d gs")
    a = ap.parse_args(argv)
    if a.tail and not a.grad_total:
        ap.error("--tail goes with --grad-total")
    if a.decoder and not a.tail:
        ap.error("--decoder goes with --grad-total --tail")
    if a.nonlocal_ and not a.decoder:
        ap.error("--nonlocal goes with --grad-total --tail --decoder")
    if a.bottleneck and not a.nonlocal_:
        ap.error("--bottleneck goes with --grad-total --tail --decoder --nonlocal")
    if a.heads and not a.tail:
        ap.error("--heads goes with --grad-total --tail")
    means = score_folder(a.folder, a.vgg, ckpt=a.ckpt, batch=a.batch, host=a.host, grad=a.grad, grad_total=a.grad_total, tail=a.tail, decoder=a.decoder,
                         nonlocal_=a.nonlocal_, bottleneck=a.bottleneck, heads=a.heads)
    print(", ".join("%s:%.9g" % (k, means[k]) for k in ALL_NAMES))
    return 0


if __name__ == "__main__":
    sys.exit(main())
