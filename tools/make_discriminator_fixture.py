"""Generate tests/golden/discriminator_32.npz (B = 2) and discriminator_64.npz (B = 1) — the reference's OWN `Discriminator` and `Conv`
(model.py:115-147, 292-312) and `hinge_loss` (utils.py:100-102), cut out of their files by their `class` / `def` lines, and
train_step's assignments to d_img, d_mask, d_output_1..3, gan_loss, d_loss_r and d_loss_s (train_test_GSC.py:264-268, 302, 334-335),
executed from their source over the TensorFlow stand-in of tools/make_model_fixture.py (imported, unchanged).

Runs on the machine that holds the reference only; nothing of the reference's text is stored in the repository or read by a test —
only arrays are.  `train_step` is cut out by its `def` line and parsed; of its statements only the plain assignments to the names above
are executed, in their order, in a namespace that holds the stand-in, the three discriminators (`self.disc1..3`, constructed as
train_test_GSC.py:121-123 constructs them: downsize 1, 2, 4 and Config.n_layer_D = 4 layers), hinge_loss and the inputs.  gt,
deshadow_img_c and mask_sv are discriminator.example_inputs(S, B, seed), the variables init_discriminator_weights(seed), assigned by
their checkpoint names (every variable must land on a layer that the forward then uses); only the seeds are stored.  With that
initialiser the logits are small and every hinge term is active, so the second case multiplies the three head kernels by 8
(`head_gain`, stored) and moves to the next seed until hinge_loss's max(0, .) clips a real and a fake logit and leaves others
unclipped, no logit within 1e-3 of +-1: the clip is then pinned to the reference's own hinge_loss.

THE STAND-IN computes Conv2D, BatchNormalization and LeakyReLU in float64 loops (oracle/np_loops.py).  Operations added here, and ours:
  tf.image.resize(x, (h, w))          bilinear, half-pixel centres, no antialiasing, in ucb_post.resize_bilinear's float32 arithmetic,
                                      per item (the imported stand-in's resize is a float64 one)
  tf.reduce_mean / tf.math.reduce_mean(x), tf.math.maximum(a, b)        numpy's float64 mean over everything; the elementwise maximum
So the reference's logits and losses are float64 here; the six logit maps are stored as float32, TensorFlow's type for them.

The tool then runs the host statement on the same inputs and records `measured_logit_diff` — max |host - stored| / max |stored| over the
six maps, the float32 rounding of the stored maps included — and `measured_loss_rel`, the three losses, relative; each the worst over
the two cases.  tests/test_discriminator_fixture.py allows 4 x those, never above 1e-5.

Usage:  python tools/make_discriminator_fixture.py
"""
import ast
import importlib.util
import os
import sys
import textwrap

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from blindshadowremoval_amd import discriminator as host                       # noqa: E402
from blindshadowremoval_amd.ucb_post import resize_bilinear                    # noqa: E402
from blindshadowremoval_amd.weights import N_LAYER_D, init_discriminator_weights  # noqa: E402

_spec = importlib.util.spec_from_file_location("make_model_fixture", os.path.join(ROOT, "tools", "make_model_fixture.py"))
mm = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mm)
REF, t = mm.REF, mm.t

WANTED = ("d_img", "d_mask", "d_output_1", "d_output_2", "d_output_3", "gan_loss", "d_loss_r", "d_loss_s")
CASES = {32: (2, 1.0), 64: (1, 8.0)}          # S: (B, the gain on the three head kernels)


def cut(path, head, indent=""):
    """The source lines of the block that starts with `head` (e.g. "class Conv(") at `indent` in the reference's file `path`, up to the
    next line at that indent or less."""
    lines = open(os.path.join(REF, path)).read().split("\n")
    lo = next(i for i, l in enumerate(lines) if l.startswith(indent + head))
    hi = lo + 1
    while hi < len(lines) and (not lines[hi].strip() or lines[hi].startswith(indent + "\t") or lines[hi].startswith(indent + " ")):
        hi += 1
    return "\n".join(l[len(indent):] for l in lines[lo:hi])


def make_tf():
    mods = mm.make_tf_module()
    tf = mods["tensorflow"]
    tf.image.resize = lambda x, size: t(np.stack([resize_bilinear(item, int(size[0])) for item in np.asarray(x, np.float32)]))
    tf.reduce_mean = lambda x: t(np.mean(np.asarray(x, np.float64)))
    tf.math.reduce_mean = tf.reduce_mean
    tf.math.maximum = lambda a, b: t(np.maximum(np.asarray(a, np.float64), np.asarray(b, np.float64)))
    return tf, mods["tensorflow.keras.layers"], mods["tensorflow_addons"]


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


class _Self:
    pass


def case_weights(seed, gain):
    """init_discriminator_weights(seed) with the three head kernels multiplied by `gain` (float32)."""
    weights = init_discriminator_weights(seed)
    for k in (1, 2, 3):
        weights["discriminator_%d/conv2/conv/kernel" % k] = weights["discriminator_%d/conv2/conv/kernel" % k] * np.float32(gain)
    return weights


def run_case(S, B, seed, gain, code):
    tf, layers, tfa = make_tf()
    ns = {"tf": tf, "layers": layers, "tfa": tfa, "np": np}
    exec(compile(cut("model.py", "class Conv("), "Conv", "exec"), ns)
    exec(compile(cut("model.py", "class Discriminator("), "Discriminator", "exec"), ns)
    exec(compile(cut("utils.py", "def hinge_loss("), "hinge_loss", "exec"), ns)
    weights = case_weights(seed, gain)
    me = _Self()
    me.disc1 = ns["Discriminator"](1, N_LAYER_D)                      # train_test_GSC.py:121-123
    me.disc2 = ns["Discriminator"](2, N_LAYER_D)
    me.disc3 = ns["Discriminator"](4, N_LAYER_D)
    touched = []
    for k, disc in ((1, me.disc1), (2, me.disc2), (3, me.disc3)):
        pre = "discriminator_%d/" % k
        touched += mm.assign_weights(disc, {n[len(pre):]: v for n, v in weights.items() if n.startswith(pre)})
    gt, con, mask_sv = host.example_inputs(S, B, seed)
    ns.update(self=me, gt=t(gt), deshadow_img_c=t(con), mask_sv=t(mask_sv), training=False)
    exec(code, ns)
    unused = sorted({n for n, o in touched if not o._used})
    assert not unused, unused
    out = {"seed": np.int64(seed), "B": np.int64(B), "S": np.int64(S), "head_gain": np.float64(gain), "backend": np.array("numpy stand-in"),
           "losses": np.array([float(ns["gan_loss"]), float(ns["d_loss_r"]), float(ns["d_loss_s"])], np.float64)}
    for k in (1, 2, 3):
        real, fake = (np.asarray(a) for a in ns["d_output_%d" % k])
        h = host.final_side(S, k)
        assert real.shape == fake.shape == (B, h, h, 1) and real.dtype == np.float64
        out["real_%d" % k], out["fake_%d" % k] = real[..., 0].astype(np.float32), fake[..., 0].astype(np.float32)
    assert np.isfinite(out["losses"]).all()
    return out


def clipped(case):
    """Whether the reference's max(0, .) clips a real and a fake logit of the case (and leaves another of each unclipped)."""
    real = np.concatenate([case["real_%d" % k].reshape(-1) for k in (1, 2, 3)])
    fake = np.concatenate([case["fake_%d" % k].reshape(-1) for k in (1, 2, 3)])
    return bool((real > 1).any() and (real < 1).any() and (fake < -1).any() and (fake > -1).any())


def differences(case):
    """(max |host - stored| / max |stored| over the six maps, max relative difference of the three losses) of the host statement."""
    S, B, seed = int(case["S"]), int(case["B"]), int(case["seed"])
    ours = host.gan_losses(case_weights(seed, float(case["head_gain"])), *host.example_inputs(S, B, seed))
    worst = 0.0
    for k in (1, 2, 3):
        stored = np.concatenate([case["real_%d" % k], case["fake_%d" % k]]).astype(np.float64)
        worst = max(worst, float(np.abs(ours["logits"][k - 1] - stored).max() / np.abs(stored).max()))
    rel = float((np.abs(ours["losses"].astype(np.float64) - case["losses"]) / np.abs(case["losses"])).max())
    return worst, rel


def main():
    code = statements()
    done = []
    for S, (B, gain) in CASES.items():
        seed = 300 + S
        while True:
            case = run_case(S, B, seed, gain, code)
            logits = [case[n] for n in case if n.startswith(("real_", "fake_"))]
            if min(float(np.abs(np.abs(y) - 1).min()) for y in logits) > 1e-3 and (gain == 1.0 or clipped(case)):
                break
            seed += 1
        worst, rel = differences(case)
        print("S=%d B=%d seed %d: losses %s, |host - reference| logits (scaled) %.3g, losses (relative) %.3g" % (S, B, int(case["seed"]), case["losses"], worst, rel))
        done.append((case, worst, rel))
    worst, rel = max(d[1] for d in done), max(d[2] for d in done)
    for case, _, _ in done:
        case["measured_logit_diff"], case["measured_loss_rel"] = np.float64(worst), np.float64(rel)
        path = os.path.join(ROOT, "tests", "golden", "discriminator_%d.npz" % int(case["S"]))
        np.savez_compressed(path, **case)
        print("wrote %s (%d bytes), measured_logit_diff %.3g, measured_loss_rel %.3g" % (path, os.path.getsize(path), worst, rel))
        assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
