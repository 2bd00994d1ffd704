"""Generate tests/golden/perceptual_32.npz (B = 2) and perceptual_64.npz (B = 1) — the reference's OWN `style_content_loss`
(utils.py:104-114), cut out of its file by its `def` line, its layer list and `vgg_feat_extractor` (train_test_GSC.py:129-133, 153-160)
and train_step's assignments to d_img, recon_loss, per_loss, g_total_loss and d_total_loss (train_test_GSC.py:264, 301, 303, 329, 336),
executed from their source over the TensorFlow stand-in of tools/make_discriminator_fixture.py (imported, unchanged), extended here by a
`keras.applications` stand-in.

Runs on the machine that holds the reference only; nothing of the reference's text is stored in the repository or read by a test —
only numbers are.  `train_step` is cut out by its `def` line and parsed; of its statements only the plain assignments to the names above
are executed, in their order, in a namespace that holds the stand-in, `self.feat_extractor` (built by the reference's own
vgg_feat_extractor from `self.vgg` and the reference's own `self.vgg_style_layers` assignment), style_content_loss and the inputs.  gt and
deshadow_img_c are perceptual.example_inputs(S, B, seed), the VGG19 variables init_vgg_weights(seed), assigned by Keras' layer names;
the other terms the two totals read (recon_loss_gs, recon_loss_c, gan_loss, grad_loss, d_loss_r, d_loss_s) are float32 draws of
`loss_terms(seed)`.  Only the seeds are stored.

THE `keras.applications` STAND-IN is ours, written from Keras' documentation of VGG19 and of preprocess_input, not from the reference:
  VGG19(include_top=False, weights='imagenet')    the layer table block1_conv1 .. block5_conv4 with block<b>_pool after each block:
                                                  Conv2D(3 x 3, 'same') + bias + ReLU in float64 loops (oracle/np_loops.py through the
                                                  imported stand-in's Conv2D), MaxPooling2D(2 x 2, stride 2) as a maximum of four slices
  .input, .get_layer(name).output, keras.Model([input], outputs)      symbolic handles; the model runs the table up to the last
                                                  requested layer and returns the requested activations in order
  vgg19.preprocess_input(x)                       'caffe' mode in float32: channels reversed, the BGR means subtracted, no scaling
  tf.abs, tf.reduce_mean, tf.split                numpy's float64 absolute value and mean over everything; np.split
The multiplication `inputs * 255` is the reference's own and runs on a float32 array.

The tool then runs the host statement on the same inputs and records `measured_mean_rel` — the five tap means and per, relative — and
`measured_total_rel`, the two totals (formed in float32 by the statement, in float64 by the stand-in), relative; each the worst over the
two cases.  tests/test_perceptual_fixture.py allows 4 x those, never above 1e-5.

Usage:  python tools/make_perceptual_fixture.py
"""
import ast
import importlib.util
import os
import sys
import textwrap
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from blindshadowremoval_amd import objective                                   # noqa: E402
from blindshadowremoval_amd import perceptual as host                          # noqa: E402
from blindshadowremoval_amd.weights import init_vgg_weights                    # noqa: E402

_spec = importlib.util.spec_from_file_location("make_discriminator_fixture", os.path.join(ROOT, "tools", "make_discriminator_fixture.py"))
md = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(md)
mm, t = md.mm, md.t
REF = mm.REF

WANTED = ("d_img", "recon_loss", "per_loss", "g_total_loss", "d_total_loss")
CASES = {32: 2, 64: 1}          # S: B
TERM_NAMES = ("recon_loss_gs", "recon_loss_c", "gan_loss", "grad_loss", "d_loss_r", "d_loss_s")


def loss_terms(seed):
    """The float32 terms the two totals read beside per_loss, on the scales train_step logs them at."""
    rng = np.random.default_rng(seed)
    scale = (0.05, 0.05, 1.0, 0.5, 1.0, 1.0)
    return {n: np.float32(rng.uniform(0.2, 1.0) * s * (-1 if n == "gan_loss" else 1)) for n, s in zip(TERM_NAMES, scale)}


def cut(path, head, indent=""):
    """make_discriminator_fixture.cut, but a comment line at any indent does not end the block (vgg_feat_extractor holds one that is
    indented with spaces between tab-indented statements)."""
    lines = open(os.path.join(REF, path)).read().split("\n")
    lo = next(i for i, l in enumerate(lines) if l.startswith(indent + head))
    hi = lo + 1
    while hi < len(lines) and (not lines[hi].strip() or lines[hi].lstrip().startswith("#") or lines[hi].startswith(indent + "\t")
                               or lines[hi].startswith(indent + " ")):
        hi += 1
    body = [l for l in lines[lo:hi] if not l.lstrip().startswith("#")]
    return "\n".join(l[len(indent):] for l in body)


# ---- the keras.applications stand-in
VGG19_TABLE = ((64, 2), (128, 2), (256, 4), (512, 4), (512, 4))        # (filters, conv layers) of block 1..5, each followed by block<b>_pool


class _Handle:
    def __init__(self, owner, name):
        self.owner, self.name = owner, name
        self.output = self


class VGG19:
    def __init__(self, include_top=True, weights="imagenet", **kw):
        assert include_top is False and weights == "imagenet" and not kw
        self.order, self.convs = [], {}
        for b, (filters, n) in enumerate(VGG19_TABLE):
            for i in range(n):
                name = "block%d_conv%d" % (b + 1, i + 1)
                self.convs[name] = mm.Conv2D(filters, (3, 3), padding="same")
                self.order.append(name)
            self.order.append("block%d_pool" % (b + 1))
        self.input = _Handle(self, "input")
        self.trainable = True

    def get_layer(self, name):
        assert name in self.order, name
        return _Handle(self, name)

    def run(self, x, wanted):
        acts, last = {"input": x}, max(self.order.index(n) for n in wanted)
        for name in self.order[:last + 1]:
            if name in self.convs:
                x = np.maximum(np.asarray(self.convs[name](t(x))), 0.0)
            else:
                x = np.maximum(np.maximum(x[:, 0::2, 0::2], x[:, 0::2, 1::2]), np.maximum(x[:, 1::2, 0::2], x[:, 1::2, 1::2]))
            acts[name] = x
        return [t(acts[n]) for n in wanted]


class Model:
    def __init__(self, inputs, outputs):
        assert len(inputs) == 1 and inputs[0].name == "input"
        self.owner, self.wanted = inputs[0].owner, [h.name for h in outputs]
        assert all(h.owner is self.owner for h in outputs)

    def __call__(self, x):
        return self.owner.run(np.asarray(x, np.float64), self.wanted)


def preprocess_input(x):
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.shape[-1] == 3
    out = x[..., ::-1].copy()
    for c, mean in enumerate((103.939, 116.779, 123.68)):
        out[..., c] -= np.float32(mean)
    return t(out)


def make_tf():
    tf, layers, tfa = md.make_tf()
    apps = types.ModuleType("tensorflow.keras.applications")
    apps.VGG19 = VGG19
    apps.vgg19 = types.ModuleType("tensorflow.keras.applications.vgg19")
    apps.vgg19.preprocess_input = preprocess_input
    tf.keras.applications = apps
    tf.keras.Model = Model
    tf.abs = lambda x: t(np.abs(np.asarray(x, np.float64)))
    return tf


def statements():
    """The assignments of train_step to the names in WANTED, in order, as a compiled module."""
    tree = ast.parse(textwrap.dedent(cut("train_test_GSC.py", "def train_step(", "\t")))
    picked = []

    def walk(body):
        for node in body:
            if isinstance(node, ast.With):
                walk(node.body)
            elif isinstance(node, ast.Assign) and len(node.targets) == 1 and isinstance(node.targets[0], ast.Name) and node.targets[0].id in WANTED:
                picked.append(node)
    walk(tree.body[0].body)
    assert [n.targets[0].id for n in picked] == list(WANTED), [n.targets[0].id for n in picked]
    return compile(ast.Module(body=picked, type_ignores=[]), "train_step", "exec")


def style_layers_statement():
    """The reference's assignment to self.vgg_style_layers, cut out of __init__ by its target."""
    tree = ast.parse(textwrap.dedent(cut("train_test_GSC.py", "def __init__(self, config", "\t")))
    picked = [n for n in ast.walk(tree) if isinstance(n, ast.Assign) and len(n.targets) == 1 and isinstance(n.targets[0], ast.Attribute)
              and n.targets[0].attr == "vgg_style_layers"]
    assert len(picked) == 1
    return compile(ast.Module(body=picked, type_ignores=[]), "__init__", "exec")


class _Self:
    pass


def run_case(S, B, seed, code, layers_code):
    tf = make_tf()
    ns = {"tf": tf, "np": np}
    exec(compile(cut("utils.py", "def style_content_loss("), "style_content_loss", "exec"), ns)
    exec(compile(textwrap.dedent(cut("train_test_GSC.py", "def vgg_feat_extractor(", "\t")), "vgg_feat_extractor", "exec"), ns)
    weights = init_vgg_weights(seed)
    me = _Self()
    me.vgg = tf.keras.applications.VGG19(include_top=False, weights="imagenet")          # train_test_GSC.py:128
    for name, conv in me.vgg.convs.items():
        if name + "/kernel" in weights:
            conv.kernel, conv.bias = weights[name + "/kernel"], weights[name + "/bias"]
    ns["self"] = me
    exec(layers_code, ns)
    assert tuple(me.vgg_style_layers) == host.VGG_TAPS
    me.feat_extractor = ns["vgg_feat_extractor"](me)
    assert me.vgg.trainable is False
    gt, con = host.example_inputs(S, B, seed)
    terms = loss_terms(seed)
    ns.update(gt=t(gt), deshadow_img_c=t(con), **terms)
    exec(code, ns)
    used = sorted(n for n, c in me.vgg.convs.items() if getattr(c, "_used", False))
    assert used == sorted(host.VGG_LAYERS), used
    feats = me.feat_extractor(tf.keras.applications.vgg19.preprocess_input(t(np.asarray(ns["d_img"]) * np.float32(255))))
    means = np.array([np.mean(np.abs(np.asarray(f[:B], np.float64) - np.asarray(f[B:], np.float64))) for f in feats])
    out = {"seed": np.int64(seed), "B": np.int64(B), "S": np.int64(S), "backend": np.array("numpy stand-in"), "tap_means": means,
           "per": np.float64(ns["per_loss"]), "g_total": np.float64(ns["g_total_loss"]), "d_total": np.float64(ns["d_total_loss"])}
    assert abs(float(means.sum()) - float(out["per"])) <= 1e-12 * float(out["per"]) and np.isfinite(list(map(float, (out["per"], out["g_total"], out["d_total"])))).all()
    return out


def host_values(case):
    """(the five tap means and per, the two totals) of the host statement on the case."""
    S, B, seed = int(case["S"]), int(case["B"]), int(case["seed"])
    r = host.per_loss(init_vgg_weights(seed), *host.example_inputs(S, B, seed))
    total = r["sums"].sum(axis=0)
    means = np.array([total[k] / (B * h * h * host.TAP_CH[k]) for k, h in enumerate(host.tap_sides(S))])
    tm = loss_terms(seed)
    g = objective.g_total_loss(tm["recon_loss_gs"], tm["recon_loss_c"], tm["grad_loss"], tm["gan_loss"], r["loss"][0])
    d = objective.d_total_loss(tm["d_loss_r"], tm["d_loss_s"])
    return np.append(means, float(r["loss"][0])), np.array([float(g), float(d)])


def differences(case):
    means, totals = host_values(case)
    want_m = np.append(case["tap_means"], float(case["per"]))
    want_t = np.array([float(case["g_total"]), float(case["d_total"])])
    return float((np.abs(means - want_m) / np.abs(want_m)).max()), float((np.abs(totals - want_t) / np.abs(want_t)).max())


def main():
    code, layers_code = statements(), style_layers_statement()
    done = []
    for S, B in CASES.items():
        case = run_case(S, B, 400 + S, code, layers_code)
        dm, dt = differences(case)
        print("S=%d B=%d seed %d: tap means %s per %.9g g_total %.9g d_total %.9g; |host - reference| means (relative) %.3g, totals %.3g"
              % (S, B, int(case["seed"]), case["tap_means"], case["per"], case["g_total"], case["d_total"], dm, dt))
        done.append((case, dm, dt))
    dm, dt = max(d[1] for d in done), max(d[2] for d in done)
    for case, _, _ in done:
        case["measured_mean_rel"], case["measured_total_rel"] = np.float64(dm), np.float64(dt)
        path = os.path.join(ROOT, "tests", "golden", "perceptual_%d.npz" % int(case["S"]))
        np.savez_compressed(path, **case)
        print("wrote %s (%d bytes), measured_mean_rel %.3g, measured_total_rel %.3g" % (path, os.path.getsize(path), dm, dt))
        assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
