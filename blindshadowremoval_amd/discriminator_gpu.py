"""The device binding of train_step's three discriminators and GAN losses, of the gen term's gradient with respect to con_rgb and of
d_total_loss's gradient with respect to the discriminators' variables: bsr_disc_losses (csrc/disc_kernels.h), bsr_disc_gen_grad
(csrc/disc_grad_kernels.h) and bsr_disc_wgrad (csrc/disc_wgrad_kernels.h), held to discriminator.py's host statement.  The checks, the
blobs, the calls and the differentiable scalar are post_gpu.WeightedTerm's; here are the names, what the discriminators leave in the
scratch, and the weight gradient's own call, which takes a third blob and returns a buffer of variables instead of an image."""
from __future__ import annotations

import ctypes
from typing import Dict, Optional

import torch

from . import _lib
from . import discriminator as host
from .pack import pack_discriminators, pack_discriminators_dgrad, pack_discriminators_wgrad
from .post_gpu import WeightedTerm
from .weights import N_LAYER_D, discriminator_trainable_names, discriminator_variable_shapes


class Discriminators(WeightedTerm):
    """`Discriminators(device).gan_losses(gt, con_rgb, mask_sv)` — gen, disc_real and disc_fake of the reference's train_step for a
    batch, on `device`, after `load_weights(dict)` (the three discriminators' variables, weights.discriminator_variable_shapes) or
    `restore(ckpt_dir)`.  `gen_grad(gt, con_rgb, mask_sv)` adds d gen / d con_rgb, and `gen_loss(gt, con_rgb, mask_sv)` is the gen term
    as a differentiable torch scalar; both need `load_weights` or `restore`, which also upload the gradient layers' blob
    (pack.pack_discriminators_dgrad) and the weight-gradient chain's (pack.pack_discriminators_wgrad).  `disc_grad(gt, con_rgb, mask_sv)`
    adds d (disc_real + disc_fake) / d each of the 54 trainable variables."""
    SYMBOL, GRAD_SYMBOL = "bsr_disc_losses", "bsr_disc_gen_grad"
    SCRATCH_QUERY, GRAD_SCRATCH_QUERY = "bsr_disc_losses_scratch_bytes", "bsr_disc_grad_scratch_bytes"
    BLOB_QUERY, DGRAD_BLOB_QUERY = "bsr_disc_blob_bytes", "bsr_disc_dgrad_blob_bytes"
    PACK, PACK_DGRAD = staticmethod(pack_discriminators), staticmethod(pack_discriminators_dgrad)
    IMAGES = ("gt", "con_rgb", "mask_sv")
    MAX_B, N_LOSSES, K = host.MAX_B, 3, host.K
    SIZE_TEXT = "discriminators take 1..32767 items of side 32, 64, 128 or 256, got B=%(b)d S=%(s)d"
    BLOB_TEXT = "a discriminator blob holds %d bytes, got %d"
    NO_WEIGHTS_TEXT = "the discriminators have no weights: call load_weights or restore first"
    NO_GRAD_WEIGHTS_TEXT = "the discriminators' gradient has no weights: call load_weights or restore first (load_blob brings the forward's alone)"

    WGRAD_SYMBOL, WGRAD_SCRATCH_QUERY, WGRAD_BLOB_QUERY = "bsr_disc_wgrad", "bsr_disc_wgrad_scratch_bytes", "bsr_disc_wgrad_blob_bytes"

    def __init__(self, device: int):
        super().__init__(device)
        self._wgrad_blob = None

    def load_weights(self, weights) -> None:
        """The three discriminators' variables -> the forward's blob, the gradient layers' and the weight-gradient chain's on the device."""
        super().load_weights(weights)
        wgrad = pack_discriminators_wgrad(weights)
        assert len(wgrad) == int(getattr(_lib.load(), self.WGRAD_BLOB_QUERY)())
        self._wgrad_blob = self._upload(wgrad)

    def load_blob(self, blob: bytes) -> None:
        """A blob of pack.pack_discriminators: the forward's weights alone; both gradient blobs loaded earlier are dropped."""
        super().load_blob(blob)
        self._wgrad_blob = None

    def restore(self, ckpt_dir: str) -> None:
        """The `discriminator_{1,2,3}/*` variables of the latest checkpoint under `ckpt_dir`."""
        from .tf_bundle import latest_checkpoint, load_discriminator_weights
        prefix = latest_checkpoint(ckpt_dir)
        if prefix is None:
            raise FileNotFoundError("no checkpoint under %s" % ckpt_dir)
        self.load_weights(load_discriminator_weights(prefix))

    def _scalar(self, losses):
        return losses[0]

    def _extra(self, b, s, logits=False):
        """The entry points' logits argument; with `logits` the three maps [2B,h_k,h_k] as a list of views of it."""
        if not logits:
            return (None,), ()
        sides = [host.final_side(s, k) for k in (1, 2, 3)]
        flat = self.empty((sum(2 * b * h * h for h in sides),), torch.float32)
        return (flat,), ([m.reshape(2 * b, h, h) for h, m in zip(sides, flat.split([2 * b * h * h for h in sides]))],)

    def activations(self, b: int, s: int) -> Dict[str, torch.Tensor]:
        """Copies of the activations the last call of these sizes left in the scratch: `d{k}/in` [2B,s,s,6], `d{k}/conv{i}`, `d{k}/out`
        [2B,h_k,h_k,1], as discriminator.forward names them."""
        lib = _lib.load()
        self.scratch(b, s)
        out = {}
        for k in (1, 2, 3):
            for layer, side in enumerate(host.map_sides(s, k)):
                c = 8 if layer == 0 else (host.DISC_CH[layer - 1] if layer <= N_LAYER_D else 1)
                a = self.view(int(lib.bsr_disc_act_offset(b, s, k, layer)), (2 * b, side, side, c))
                name = "in" if layer == 0 else ("conv%d" % (layer - 1) if layer <= N_LAYER_D else "out")
                out["d%d/%s" % (k, name)] = (a[..., :6] if layer == 0 else a).clone()
        return out

    def gan_losses(self, gt: torch.Tensor, con_rgb: torch.Tensor, mask_sv: torch.Tensor, logits: bool = False, keep: bool = False):
        """-> (losses float32 [3] = gen, disc_real, disc_fake (discriminator.LOSS_NAMES), sums float64 [B,9] (discriminator.DISC_SUM_NAMES))
        on the device, asynchronously on the current stream; with `logits` also the three maps [2B,h_k,h_k] as a list; with `keep` also
        the dict of activations (`activations`).  Everything is checked here, before any launch: TypeError / ValueError."""
        return self._forward((gt, con_rgb, mask_sv), keep, logits=logits)

    def gen_grad(self, gt: torch.Tensor, con_rgb: torch.Tensor, mask_sv: torch.Tensor, upstream: torch.Tensor = None, keep: bool = False):
        """-> (losses float32 [3], sums float64 [B,9], grad float32 [B,S,S,3] = d gen / d con_rgb * upstream) on the device, asynchronously
        on the current stream; losses, sums and the kept activations are gan_losses' bytes.  `upstream`: a float32 device tensor of one
        element, or None for 1.  With `keep` also the dict of activations.  Everything is checked here, before any launch: TypeError /
        ValueError."""
        return self._grad((gt, con_rgb, mask_sv), upstream, keep)

    def gradients(self, b: int, s: int) -> Dict[str, torch.Tensor]:
        """Copies of the gradient maps the last gen_grad / grad_stages call of these sizes left in the scratch, as discriminator.gen_grad
        names them: `d{k}/in` [B,s,s,3], `d{k}/conv{i}` [B,.,.,n_ch[i]]."""
        lib = _lib.load()
        self.scratch(b, s, grad=True)
        out = {}
        for k in (1, 2, 3):
            sides = host.map_sides(s, k)
            for layer in range(N_LAYER_D + 1):
                side, c = sides[layer], 4 if layer == 0 else host.DISC_CH[layer - 1]
                a = self.view(int(lib.bsr_disc_grad_offset(b, s, k, layer)), (b, side, side, c))
                out["d%d/%s" % (k, "in" if layer == 0 else "conv%d" % (layer - 1))] = (a[..., :3] if layer == 0 else a).clone()
        return out

    def grad_stages(self, gt: torch.Tensor, con_rgb: torch.Tensor, mask_sv: torch.Tensor, stop_after: int) -> Dict[str, torch.Tensor]:
        """For the stage-by-stage tests: the chain stopped after `stop_after` (0..6) of its backward launches (GRAD_LAUNCHES) ->
        `gradients`; the maps of launches that did not run hold whatever the scratch held."""
        b, s = self._check((gt, con_rgb, mask_sv), grad=True)
        if not 0 <= int(stop_after) <= len(GRAD_LAUNCHES):
            raise ValueError("stop_after must be 0..%d" % len(GRAD_LAUNCHES))
        self._run((gt, con_rgb, mask_sv), b, s, grad=True, stop_after=stop_after)
        return self.gradients(b, s)

    def gen_loss(self, gt: torch.Tensor, con_rgb: torch.Tensor, mask_sv: torch.Tensor) -> torch.Tensor:
        """gen as a differentiable scalar: float32 [] with a grad_fn whose backward hands d gen / d con_rgb * grad_output to con_rgb and
        None to gt and mask_sv.  When con_rgb requires a gradient, forward and backward run in one call here and the backward is one
        device multiply; nothing is synchronised."""
        return self._loss(gt, con_rgb, mask_sv)

    def _wgrad_run(self, images, b: int, s: int, stop_after: Optional[int] = None, logits: bool = False):
        """One checked weight-gradient call -> (losses, sums, the flat gradient buffer, with `logits` the three maps)."""
        lib = _lib.load()
        losses = self.empty((self.N_LOSSES,), torch.float32)
        sums = self.empty((b, self.K), torch.float64)
        extra, maps = self._extra(b, s, logits=logits)
        flat = self.empty((int(lib.bsr_disc_wgrad_floats()),), torch.float32)
        if stop_after is not None:
            flat.zero_()                       # a stopped chain leaves what it did not write at 0
        args = []
        for blob in (self._blob, self._dgrad_blob, self._wgrad_blob):
            args += [blob, ctypes.c_size_t(blob.numel())]
        args += [*images, b, s, sums, losses, *extra, flat, ctypes.c_void_p(self.scratch(b, s, self.WGRAD_SCRATCH_QUERY))]
        symbol = self.WGRAD_SYMBOL
        if stop_after is not None:
            args.append(int(stop_after))
            symbol = symbol.replace("bsr_", "bsr_debug_", 1)
        self.call(*args, symbol=symbol)
        return (losses, sums, flat) + maps

    def _wgrad_check(self, images):
        b, s = self._check(images, grad=True)
        if self._wgrad_blob is None:
            raise ValueError(self.NO_GRAD_WEIGHTS_TEXT)
        return b, s

    @staticmethod
    def split_grads(flat: torch.Tensor) -> Dict[str, torch.Tensor]:
        """The flat buffer of bsr_disc_wgrad -> name -> a view of it in the variable's shape, for weights.discriminator_trainable_names();
        the flat tensor itself under the key ""."""
        lib = _lib.load()
        shapes = discriminator_variable_shapes()
        out = {"": flat}
        for index, name in enumerate(discriminator_trainable_names()):
            off, n = int(lib.bsr_disc_wgrad_var_offset(index)), 1
            for d in shapes[name]:
                n *= d
            out[name] = flat[off:off + n].reshape(shapes[name])
        return out

    def disc_grad(self, gt: torch.Tensor, con_rgb: torch.Tensor, mask_sv: torch.Tensor, keep: bool = False, logits: bool = False):
        """-> (losses float32 [3], sums float64 [B,9], grads) on the device, asynchronously on the current stream; losses, sums and the kept
        activations are gan_losses' bytes.  grads: name -> float32 tensor in the variable's shape, d (disc_real + disc_fake) / d the
        variable, for the 54 names of weights.discriminator_trainable_names(); the tensors are views of one flat buffer, which is grads[""].
        With `logits` also the three maps [2B,h_k,h_k] as a list, with `keep` also the dict of activations, in that order.  Everything is
        checked here, before any launch: TypeError / ValueError."""
        images = (gt, con_rgb, mask_sv)
        b, s = self._wgrad_check(images)
        res = self._wgrad_run(images, b, s, logits=logits)
        out = res[:2] + (self.split_grads(res[2]),) + res[3:]
        return out + (self.activations(b, s),) if keep else out

    def wgrad_maps(self, b: int, s: int) -> Dict[str, torch.Tensor]:
        """Copies of the gradient maps the last disc_grad / wgrad_stages call of these sizes left in the scratch, as discriminator.disc_grad
        names them: `d{k}/conv{i}` [2B,.,.,n_ch[i]] and the seed `d{k}/out` [2B,h_k,h_k,1]."""
        lib = _lib.load()
        self.scratch(b, s, self.WGRAD_SCRATCH_QUERY)
        out = {}
        for k in (1, 2, 3):
            sides = host.map_sides(s, k)
            for layer in range(1, N_LAYER_D + 2):
                c = host.DISC_CH[layer - 1] if layer <= N_LAYER_D else 1
                a = self.view(int(lib.bsr_disc_wgrad_offset(b, s, k, layer)), (2 * b, sides[layer], sides[layer], c))
                out["d%d/%s" % (k, "conv%d" % (layer - 1) if layer <= N_LAYER_D else "out")] = a.clone()
        return out

    def wgrad_stages(self, gt: torch.Tensor, con_rgb: torch.Tensor, mask_sv: torch.Tensor, stop_after: int) -> Dict[str, torch.Tensor]:
        """For the stage-by-stage tests: the chain stopped after `stop_after` (0..11) of its backward launches (WGRAD_LAUNCHES) ->
        `wgrad_maps`, and under "" the flat gradient buffer, zero where no launch wrote; the maps of launches that did not run hold
        whatever the scratch held."""
        images = (gt, con_rgb, mask_sv)
        b, s = self._wgrad_check(images)
        if not 0 <= int(stop_after) <= len(WGRAD_LAUNCHES):
            raise ValueError("stop_after must be 0..%d" % len(WGRAD_LAUNCHES))
        flat = self._wgrad_run(images, b, s, stop_after=stop_after)[2]
        out = self.wgrad_maps(b, s)
        out[""] = flat
        return out


# the backward chain's launches in order and the gradient map each writes (the last writes grad)
GRAD_LAUNCHES = (("head", "conv3"), ("dgrad", "conv2"), ("dgrad", "conv1"), ("dgrad", "conv0"), ("dgrad_in", "in"), ("gather", "grad"))
# the weight-gradient chain's launches in order and what each writes
WGRAD_LAUNCHES = (("seed", "out, conv3"), ("head_wgrad", "head partials"), ("wgrad", "conv3 partials"), ("dgrad", "conv2"), ("wgrad", "conv2 partials"),
                  ("dgrad", "conv1"), ("wgrad", "conv1 partials"), ("dgrad", "conv0"), ("wgrad", "conv0 partials"), ("fold", "kernels"),
                  ("finish", "bias, gamma, beta, head"))
