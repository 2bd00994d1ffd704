"""Variable inventory of the GSC generator and a seeded synthetic initialiser.

The variable names and shapes are the ones ``tf.train.Checkpoint(generator=Generator())`` produces
for /root/reference/model.py:198-226 (layer table) — ``tests/golden/gsc_ckpt94_inventory.json`` holds
the same table parsed from the reference's own ``ckpt-94.index`` and the CPU test-suite checks the
two agree.  Kernel layouts are TensorFlow's: ``Conv2D`` HWIO ``[kh,kw,Cin,Cout]``
(/root/reference/model.py:119), ``Conv2DTranspose`` ``[kh,kw,Cout,Cin]`` (/root/reference/model.py:153).

The trained weights are not shipped with the reference (/root/reference/.MISSING_LARGE_BLOBS), so
benchmarks and parity tests use ``init_weights(seed)``.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Dict, List, Tuple  # noqa: F401 (Tuple: string annotations)

import numpy as np

N_RES = 6                       # /root/reference/model.py:199
N_CH = [32, 64, 64, 96, 128, 256, 256]   # /root/reference/model.py:201
RES_CH = N_CH[5] + 1            # 257, /root/reference/model.py:226
BN_EPS = 1e-3                   # Keras BatchNormalization default epsilon
LRELU_ALPHA = 0.3               # Keras LeakyReLU default alpha


def _conv(spec, stem, kh, cin, cout, bn, transpose=False):
    spec[stem + "/conv/kernel"] = (kh, kh, cout, cin) if transpose else (kh, kh, cin, cout)
    spec[stem + "/conv/bias"] = (cout,)
    if bn:
        for p in ("gamma", "beta", "moving_mean", "moving_variance"):
            spec[stem + "/bnorm/" + p] = (cout,)


RGB_CH = 2 * N_CH[5] + 1        # 513: ResBottleneck(n_ch[5]*2+1) of /root/reference/model_RGB.py:226


def rgb_variable_shapes() -> "OrderedDict[str, Tuple[int, ...]]":
    """name -> shape for the variables of the single-stage RGB baseline (/root/reference/model_RGB.py:198-266).  Keras creates variables
    only for layers that are called: ``call`` (:228-266) uses conv1-3, down1-3, up1-3 and res_stack[0:3]; clr_*, res_stack[3:6] and
    info_share are constructed but never called, so the checkpoint holds none of their variables (tests/golden/model_py_rgb_64.npz records
    the inventory the reference's own forward builds)."""
    s: "OrderedDict[str, Tuple[int, ...]]" = OrderedDict()
    c0 = N_CH[3] + 3                                        # cat[x, uv] = 99 (:237-238)
    _conv(s, "conv1", 7, 3, N_CH[0], True)                  # :203 'tconv1'
    _conv(s, "conv2", 7, N_CH[1] * 2, 3, False)             # :204 'tconv3': 7x7 on up3's 128 channels, no BN, no activation
    _conv(s, "conv3", 7, 3, 3, False)                       # :205 'tconv4': 7x7 on conv2's output
    _conv(s, "down1", 3, N_CH[0], N_CH[1], True)
    _conv(s, "down2", 3, N_CH[1], N_CH[2], True)
    _conv(s, "down3", 3, N_CH[2], N_CH[3], True)
    _conv(s, "up1", 3, RGB_CH, N_CH[3] * 2, True, transpose=True)                  # 513 -> 192 (:210,250)
    _conv(s, "up2", 3, N_CH[3] * 2 + N_CH[2], N_CH[2] * 2, True, transpose=True)   # cat[y, x3] = 256 -> 128 (:211,251)
    _conv(s, "up3", 3, N_CH[2] * 2 + N_CH[1], N_CH[1] * 2, True, transpose=True)   # cat[y, x2] = 192 -> 128 (:212,252)
    half = RGB_CH // 2                                      # 256
    for i in range(N_RES // 2):                             # :239-240
        cin = c0 if i == 0 else RGB_CH
        st = "res_stack/%d/" % i
        for name, shp in (("conv1", (1, 1, cin, half)), ("conv2", (3, 3, half, half)), ("conv3", (1, 1, half, RGB_CH))):
            s[st + name + "/kernel"] = shp
            s[st + name + "/bias"] = (shp[3],)
        for j, c in ((1, half), (2, half), (3, RGB_CH)):
            for p in ("gamma", "beta", "moving_mean", "moving_variance"):
                s[st + "bnorm%d/%s" % (j, p)] = (c,)
        for name in ("g", "phi", "theta"):
            s[st + "non_local/%s/kernel" % name] = (1, 1, RGB_CH, half)
            s[st + "non_local/%s/bias" % name] = (half,)
        s[st + "non_local/w/kernel"] = (1, 1, half, RGB_CH)
        s[st + "non_local/w/bias"] = (RGB_CH,)
        for p in ("gamma", "beta", "moving_mean", "moving_variance"):
            s[st + "non_local/bnorm/" + p] = (RGB_CH,)
    return s


def generator_variable_shapes(variant: str = "gsc") -> "OrderedDict[str, Tuple[int, ...]]":
    """name -> shape for the 258 float32 variables of the generator.  ``variant``: "gsc" (/root/reference/model.py),
    "tsm" (/root/reference/model_with_TSM.py: ShareLayer widens the bottleneck inputs to 291 / 877 channels) or "rgb"
    (/root/reference/model_RGB.py: the single-stage baseline, ``rgb_variable_shapes``)."""
    if variant not in ("gsc", "tsm", "rgb"):
        raise ValueError("variant must be 'gsc', 'tsm' or 'rgb'")
    if variant == "rgb":
        return rgb_variable_shapes()
    tsm = variant == "tsm"
    c0 = N_CH[3] + 3 + (2 * N_CH[3] if tsm else 0)            # cat[x, (x_share,) uv]: 99 | 291
    c12 = max(c0, RES_CH)                                       # output width of res blocks 0-2: 257 | 291
    c3 = c12 + 1 + 3 + (2 * c12 if tsm else 0)                  # cat[x_hole, bmask, (x_share,) uv]: 261 | 877
    s: "OrderedDict[str, Tuple[int, ...]]" = OrderedDict()
    _conv(s, "conv1", 7, 3, N_CH[0], True)                 # model.py:203
    _conv(s, "conv2", 7, N_CH[1], 1, False)                # model.py:204 (mask head)
    _conv(s, "conv3", 7, N_CH[1], 1, False)                # model.py:205 (con head)
    _conv(s, "down1", 3, N_CH[0], N_CH[1], True)           # model.py:207
    _conv(s, "down2", 3, N_CH[1], N_CH[2], True)
    _conv(s, "down3", 3, N_CH[2], N_CH[3], True)
    _conv(s, "up1", 3, c12, N_CH[3], True, transpose=True)               # model.py:210,243
    _conv(s, "up2", 3, N_CH[3] + N_CH[2], N_CH[2], True, transpose=True)  # cat[y,x3] model.py:244
    _conv(s, "up3", 3, N_CH[2] + N_CH[1], N_CH[1], True, transpose=True)  # cat[y,x2] model.py:245
    _conv(s, "clr_up1", 3, c3, N_CH[4], True, transpose=True)             # 261 -> 128 model.py:214,264
    _conv(s, "clr_up2", 3, N_CH[4], N_CH[3], True, transpose=True)
    _conv(s, "clr_up3", 3, N_CH[3], N_CH[2], True, transpose=True)
    _conv(s, "clr_conv1", 3, N_CH[2] + 1, 16, True)        # cat[gs,f] model.py:217,267
    _conv(s, "clr_conv2", 1, 16, 16, True)
    _conv(s, "clr_conv3", 1, 16, 3, False)
    half = RES_CH // 2                                      # 128
    for i in range(N_RES):
        cin = c0 if i == 0 else (c12 if i < N_RES // 2 else c3)   # GSC 99 / 257 / 261, TSM 291 / 291 / 877
        st = "res_stack/%d/" % i
        for name, shp in (("conv1", (1, 1, cin, half)), ("conv2", (3, 3, half, half)), ("conv3", (1, 1, half, RES_CH))):
            s[st + name + "/kernel"] = shp
            s[st + name + "/bias"] = (shp[3],)
        for j, c in ((1, half), (2, half), (3, RES_CH)):
            for p in ("gamma", "beta", "moving_mean", "moving_variance"):
                s[st + "bnorm%d/%s" % (j, p)] = (c,)
        for name in ("g", "phi", "theta"):                  # model.py:10-12
            s[st + "non_local/%s/kernel" % name] = (1, 1, RES_CH, half)
            s[st + "non_local/%s/bias" % name] = (half,)
        s[st + "non_local/w/kernel"] = (1, 1, half, RES_CH)  # model.py:13
        s[st + "non_local/w/bias"] = (RES_CH,)
        for p in ("gamma", "beta", "moving_mean", "moving_variance"):
            s[st + "non_local/bnorm/" + p] = (RES_CH,)
    return s


def generator_tail_trainable_names() -> List[str]:
    """The ten trainable variables of the generator's colour tail (clr_conv1, clr_conv2, clr_conv3) in generator_variable_shapes' order,
    9 763 floats in all: every kernel, bias, gamma and beta; moving_mean and moving_variance take no gradient."""
    return [n for n in generator_variable_shapes() if n.split("/", 1)[0] in ("clr_conv1", "clr_conv2", "clr_conv3")
            and not n.rsplit("/", 1)[1].startswith("moving_")]


def generator_decoder_trainable_names(variant: str = "gsc") -> List[str]:
    """The twelve trainable variables of the generator's colour decoder (clr_up1, clr_up2, clr_up3) in generator_variable_shapes' order,
    467 424 floats for GSC: every kernel [3,3,out,in], bias, gamma and beta; moving_mean and moving_variance take no gradient."""
    return [n for n in generator_variable_shapes(variant) if n.split("/", 1)[0] in ("clr_up1", "clr_up2", "clr_up3")
            and not n.rsplit("/", 1)[1].startswith("moving_")]


def generator_grey_decoder_trainable_names(variant: str = "gsc") -> List[str]:
    """The twelve trainable variables of the generator's grey decoder (up1, up2, up3) in generator_variable_shapes' order, 388 608 floats
    for GSC: every kernel [3,3,out,in] (in = 257, 160 = cat[up1, x3], 128 = cat[up2, x2]), bias, gamma and beta; moving_mean and
    moving_variance take no gradient."""
    return [n for n in generator_variable_shapes(variant) if n.split("/", 1)[0] in ("up1", "up2", "up3")
            and not n.rsplit("/", 1)[1].startswith("moving_")]


def generator_nonlocal_trainable_names(block: int = 5, variant: str = "gsc") -> List[str]:
    """The ten trainable variables of res_stack/<block>'s NonLocalBlock in generator_variable_shapes' order, 132 739 floats: the kernel
    and bias of g, phi, theta and w, and bnorm's gamma and beta; moving_mean and moving_variance take no gradient."""
    stem = "res_stack/%d/non_local/" % block
    return [n for n in generator_variable_shapes(variant) if n.startswith(stem) and not n.rsplit("/", 1)[1].startswith("moving_")]


def generator_bottleneck_trainable_names(block: int = 5, variant: str = "gsc") -> List[str]:
    """The twelve trainable variables of res_stack/<block>'s bottleneck convolutions in generator_variable_shapes' order, 215 299 floats
    for GSC: the kernel and bias of conv1, conv2, conv3 and the gamma and beta of bnorm1, bnorm2, bnorm3; the non-local block's are
    generator_nonlocal_trainable_names', and moving_mean and moving_variance take no gradient."""
    stem = "res_stack/%d/" % block
    return [n for n in generator_variable_shapes(variant)
            if n.startswith(stem) and not n.startswith(stem + "non_local/") and not n.rsplit("/", 1)[1].startswith("moving_")]


def generator_colour_trunk_trainable_names() -> List[str]:
    """The 44 trainable variables of res_stack/3 and res_stack/4 in generator_variable_shapes' order, 696 076 floats: per block the twelve
    of generator_bottleneck_trainable_names and the ten of generator_nonlocal_trainable_names; moving_mean and moving_variance take no
    gradient."""
    return [n for n in generator_variable_shapes() if n.startswith(("res_stack/3/", "res_stack/4/")) and not n.rsplit("/", 1)[1].startswith("moving_")]


def generator_lower_trunk_trainable_names() -> List[str]:
    """The 66 trainable variables of res_stack/0, res_stack/1 and res_stack/2, the blocks below the hole, block 0 first: per block the
    twelve of generator_bottleneck_trainable_names, then the ten of generator_nonlocal_trainable_names (block 0's conv1 is 99 -> 128, the
    others' 257 -> 128); moving_mean and moving_variance take no gradient."""
    return [n for b in (0, 1, 2) for names in (generator_bottleneck_trainable_names, generator_nonlocal_trainable_names) for n in names(b)]


def generator_heads_trainable_names(variant: str = "gsc") -> List[str]:
    """The four trainable variables of the generator's grey heads in generator_variable_shapes' order, 6 274 floats: the kernel
    [7,7,64,1] and bias of conv2 ('tconv3', the mask head) and of conv3 ('tconv4', the con head).  GSC and TSM share them; the RGB
    baseline's heads are 128 -> 3 and chained."""
    return [n for n in generator_variable_shapes(variant) if n in ("conv2/conv/kernel", "conv2/conv/bias", "conv3/conv/kernel", "conv3/conv/bias")]


N_LAYER_D = 4                   # Config.n_layer_D (/root/reference/train_test_GSC.py:121-123)
DISC_CH = [32, 32, 64, 64]      # the first n_layer_D entries of Discriminator's n_ch (/root/reference/model.py:295)
DISC_IN_CH = 6                  # cat[image 3 | mask_sv 3] (/root/reference/train_test_GSC.py:264-268)


def discriminator_variable_shapes(n_layer: int = N_LAYER_D) -> "OrderedDict[str, Tuple[int, ...]]":
    """name -> shape for the float32 variables of the three patch discriminators (/root/reference/model.py:292-312), named as
    ``tf.train.Checkpoint(discriminator_1=..., discriminator_2=..., discriminator_3=...)`` names them minus the variable suffix:
    ``discriminator_<k>/conv_stack/<i>/{conv/kernel, conv/bias, bnorm/*}`` and ``discriminator_<k>/conv2/conv/{kernel, bias}``.
    tests/golden/disc_ckpt_inventory.json holds the same table parsed from the reference's index files."""
    n_ch = [32, 32, 64, 64, 128, 256]
    if not 1 <= n_layer <= len(n_ch):
        raise ValueError("n_layer must be 1..%d" % len(n_ch))
    s: "OrderedDict[str, Tuple[int, ...]]" = OrderedDict()
    for k in (1, 2, 3):
        cin = DISC_IN_CH
        for i in range(n_layer):
            _conv(s, "discriminator_%d/conv_stack/%d" % (k, i), 4, cin, n_ch[i], True)      # Conv(n_ch[i], ksize=4, stride=2, norm='batch')
            cin = n_ch[i]
        _conv(s, "discriminator_%d/conv2" % k, 4, cin, 1, False)                            # Conv(1, ksize=4, norm=False, nl=False)
    return s


def discriminator_trainable_names(n_layer: int = N_LAYER_D) -> List[str]:
    """The trainable variables of the three discriminators in discriminator_variable_shapes' order: every kernel, bias, gamma and beta;
    moving_mean and moving_variance are BatchNormalization's statistics and take no gradient."""
    return [n for n in discriminator_variable_shapes(n_layer) if not n.rsplit("/", 1)[1].startswith("moving_")]


def _draw(rng, name: str, shp, fan_in: float, gain: float) -> np.ndarray:
    """One variable of the SURVEY.md §8d recipe, by the leaf of its name."""
    leaf = name.rsplit("/", 1)[1]
    if leaf == "kernel":
        w = rng.standard_normal(shp) * np.sqrt(gain / fan_in)
    elif leaf == "gamma":
        w = rng.uniform(0.8, 1.2, shp)
    elif leaf == "moving_variance":
        w = rng.uniform(0.75, 1.25, shp)
    else:                               # bias, beta, moving_mean
        w = rng.standard_normal(shp) * 0.05
    return w.astype(np.float32)


def init_discriminator_weights(seed: int = 1, n_layer: int = N_LAYER_D) -> Dict[str, np.ndarray]:
    """Seeded synthetic weights of the three discriminators in ``init_weights``' recipe: kernels N(0, 1.6/fan_in), biases / beta /
    moving_mean N(0, 0.05^2), gamma U[0.8,1.2], moving_variance U[0.75,1.25]."""
    rng = np.random.default_rng(seed)
    return {name: _draw(rng, name, shp, shp[0] * shp[1] * shp[2] if len(shp) == 4 else 1, 1.6)
            for name, shp in discriminator_variable_shapes(n_layer).items()}


def check_discriminator_weights(weights: Dict[str, np.ndarray], n_layer: int = N_LAYER_D) -> None:
    """Raise ValueError if ``weights`` is not exactly the three discriminators' variable set."""
    spec = discriminator_variable_shapes(n_layer)
    missing = [k for k in spec if k not in weights]
    if missing:
        raise ValueError("missing discriminator variables: %s%s" % (missing[:4], " ..." if len(missing) > 4 else ""))
    for k, shp in spec.items():
        if tuple(np.shape(weights[k])) != tuple(shp):
            raise ValueError("variable %s has shape %s, expected %s" % (k, tuple(np.shape(weights[k])), shp))


# ---- VGG19 up to block5_conv1: the perceptual term's feature extractor (train_test_GSC.py:128-139) ----
VGG_BLOCKS = ((64, 2), (128, 2), (256, 4), (512, 4), (512, 1))        # (channels, conv layers used) of block 1..5
VGG_LAYERS = tuple("block%d_conv%d" % (b + 1, i + 1) for b, (_, n) in enumerate(VGG_BLOCKS) for i in range(n))
VGG_TAPS = tuple("block%d_conv1" % b for b in range(1, 6))


def vgg_variable_shapes() -> "OrderedDict[str, Tuple[int, ...]]":
    """name -> shape for the 26 float32 variables of Keras' VGG19(include_top=False) up to block5_conv1, by Keras' layer names:
    `block<b>_conv<i>/kernel` (HWIO, 3 x 3) and `block<b>_conv<i>/bias`."""
    s: "OrderedDict[str, Tuple[int, ...]]" = OrderedDict()
    cin = 3
    for b, (ch, n) in enumerate(VGG_BLOCKS):
        for i in range(n):
            st = "block%d_conv%d" % (b + 1, i + 1)
            s[st + "/kernel"] = (3, 3, cin, ch)
            s[st + "/bias"] = (ch,)
            cin = ch
    return s


def init_vgg_weights(seed: int = 1) -> Dict[str, np.ndarray]:
    """Seeded synthetic VGG19 variables for tests and benchmarks (the ImageNet weights are in no checkpoint): He-normal kernels
    N(0, 2 / fan_in), biases N(0, 0.05^2)."""
    rng = np.random.default_rng(seed)
    out = {}
    for name, shp in vgg_variable_shapes().items():
        if name.endswith("/kernel"):
            out[name] = (rng.standard_normal(shp, dtype=np.float32) * np.float32(np.sqrt(2.0 / (shp[0] * shp[1] * shp[2])))).astype(np.float32)
        else:
            out[name] = (rng.standard_normal(shp) * 0.05).astype(np.float32)
    return out


def check_vgg_weights(weights: Dict[str, np.ndarray]) -> None:
    """Raise ValueError if ``weights`` is not exactly vgg_variable_shapes()' variable set."""
    spec = vgg_variable_shapes()
    missing = [k for k in spec if k not in weights]
    if missing:
        raise ValueError("missing VGG19 variables: %s%s" % (missing[:4], " ..." if len(missing) > 4 else ""))
    for k, shp in spec.items():
        if tuple(np.shape(weights[k])) != tuple(shp):
            raise ValueError("variable %s has shape %s, expected %s" % (k, tuple(np.shape(weights[k])), shp))


def load_vgg_weights(path: str) -> Dict[str, np.ndarray]:
    """An `.npz` with the keys of vgg_variable_shapes() (INTEGRATION.md shows how Keras' own weight file becomes one) -> the float32
    variables.  ValueError unless it holds exactly those shapes; further keys are ignored."""
    with np.load(path) as z:
        missing = [k for k in vgg_variable_shapes() if k not in z.files]
        if missing:
            raise ValueError("%s: missing VGG19 variables: %s%s" % (path, missing[:4], " ..." if len(missing) > 4 else ""))
        weights = {k: np.asarray(z[k], np.float32) for k in vgg_variable_shapes()}
    check_vgg_weights(weights)
    return weights


def save_vgg_weights(path: str, weights: Dict[str, np.ndarray]) -> None:
    """The inverse of load_vgg_weights."""
    check_vgg_weights(weights)
    np.savez(path, **{k: np.asarray(weights[k], np.float32) for k in vgg_variable_shapes()})


# Kernel variance gains (x 1/fan_in).  1.6 roughly preserves variance through LeakyReLU(0.3); the
# residual branches (``conv3``, ``non_local/w``) and the attention projections are damped so the six
# bottleneck blocks neither blow activations up nor saturate the 1024-wide softmax — a trained
# network keeps both O(1), and parity to 1e-3 absolute is only meaningful at that scale.
_GAINS = (("non_local/theta", 4.0), ("non_local/phi", 4.0), ("non_local/w", 0.15), ("/conv3/kernel", 0.45),
          ("clr_conv3", 0.25), ("clr_conv2", 1.0))


def _gain(name: str) -> float:
    if name.startswith("res_stack") or name.startswith("clr_conv"):
        for key, g in _GAINS:
            if key in name:
                return g
    return 1.6


def init_weights(seed: int = 1, con_bias_shift: float = 0.25, variant: str = "gsc") -> Dict[str, np.ndarray]:
    """Seeded synthetic weights (SURVEY.md §8d recipe): kernels N(0, 1.6/fan_in), biases / beta /
    moving_mean N(0, 0.05^2), gamma U[0.8,1.2], moving_variance U[0.75,1.25].

    ``con_bias_shift`` is added to the ``conv3`` (con head) bias; +0.1 pushes ``dif`` across the
    in-network 0.1 threshold (/root/reference/model.py:256) so ``bmask`` is non-degenerate."""
    rng = np.random.default_rng(seed)
    out: Dict[str, np.ndarray] = {}
    for name, shp in generator_variable_shapes(variant).items():
        fan_in = 1.0
        if name.endswith("/kernel"):
            transpose = name.split("/")[0] in ("up1", "up2", "up3", "clr_up1", "clr_up2", "clr_up3")
            fan_in = shp[0] * shp[1] * (shp[3] if transpose else shp[2])
            if transpose:
                fan_in = fan_in / 4.0       # stride-2 transposed conv: 9/4 taps reach one output on average
        out[name] = _draw(rng, name, shp, fan_in, _gain(name))
    if con_bias_shift and variant != "rgb":          # the RGB baseline has no threshold: its conv3 is the output layer
        out["conv3/conv/bias"] = (out["conv3/conv/bias"] + np.float32(con_bias_shift)).astype(np.float32)
    return out


def detect_variant(weights: Dict[str, np.ndarray]) -> str:
    """"gsc", "tsm" (291-channel res0 input) or "rgb" (256-wide bottleneck convs of the 513-channel blocks)."""
    k = weights.get("res_stack/0/conv1/kernel")
    if k is not None and k.shape[3] == RGB_CH // 2:
        return "rgb"
    return "tsm" if k is not None and k.shape[2] == 291 else "gsc"


def check_weights(weights: Dict[str, np.ndarray], variant: str = "gsc") -> None:
    """Raise ValueError if ``weights`` is not exactly the generator's variable set."""
    spec = generator_variable_shapes(variant)
    missing = [k for k in spec if k not in weights]
    if missing:
        raise ValueError("missing generator variables: %s%s" % (missing[:4], " ..." if len(missing) > 4 else ""))
    for k, shp in spec.items():
        if tuple(weights[k].shape) != tuple(shp):
            raise ValueError("variable %s has shape %s, expected %s" % (k, tuple(weights[k].shape), shp))
