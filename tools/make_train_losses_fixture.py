"""Generate tests/golden/train_losses_32.npz (B = 3) and train_losses_64.npz (B = 2) — the reference's OWN `find_edge`, `l1_loss`,
`l1_loss_yuv` (utils.py:22-52, 116-125) and `get_img_grad` (train_test_GSC.py:107-115), cut out of their files by their `def` lines,
and the loss statements of `train_step` (train_test_GSC.py:253-258, 287-301, 307-328, 357), executed from their source over the numpy
TensorFlow stand-in of tools/make_shadow_synth_fixture.py (imported, unchanged), which gains the operations below.

Runs on the machine that holds the reference only; nothing of the reference's text is stored in the repository or read by a test —
only arrays are.  `train_step` is cut out by its `def` line and parsed; of its statements only the plain assignments to mask_bi,
mask_edge, dif, bmaskgt, recon_loss_gs, recon_loss_c, grad_gt_1..5, grad_rc_1..5, dif_grad_1..5, grad_loss and figs are executed, in
their order, in a namespace that holds the stand-in, the four functions and the inputs.  The generator's outputs (deshadow_img_gs,
deshadow_img_c) are supplied as arrays: train_losses.example_inputs(S, B, seed), of which only the seed is stored.

THE STAND-IN'S ADDED OPERATIONS (float32, and ours):
  tf.image.resize(x, [h, w])      bilinear, half-pixel centres, no antialiasing, in ucb_post.resize_bilinear's arithmetic, per item;
                                  method NEAREST goes to the imported stand-in's resize
  tf.image.image_gradients(x)     (dy, dx): dy[:, i] = x[:, i + 1] - x[:, i] with a zero last row, dx likewise along columns
  tf.image.rgb_to_grayscale(x)    (r * 0.2989 + g * 0.587) + b * 0.114, one channel kept
  tf.nn.dilation2d(x, k, SAME)    out[y, x, c] = max over the filter positions that fall inside the image of x[y + i - 2, x + j - 2, c]
                                  + k[i, j, c]: positions outside the image do not take part
  tf.split(x, n, axis)            n equal parts
  tf.reduce_mean / reduce_min / reduce_sum (also under tf.math), axis and keepdims: numpy's float32 reductions; the mean over the
                                  channel axis is ((a + b) + c) / 3
  tf.ones(shape), tf.ones_like(x) float32 ones
A Python scalar next to a stand-in tensor is converted to the tensor's float32, as TensorFlow converts a constant; so `+ 1e-6` is a
float32 addition here, and a float64 one in the host statement.

The tool moves to the next seed if any pixel of mean_c, min_c or dif lies within 1e-5 of .01, .3 or .04 (mask_sv's channels against
.01 too), so the binary planes are comparable exactly; the chosen seed is recorded.  It then runs the host statement on the same
inputs and records `measured_max_diff` (the dif_grad figure) and `measured_rel_diff` (the three losses, relative), each the worst over
the cases of the set; the tests allow 4 x those, never above 1e-4.

Usage:  python tools/make_train_losses_fixture.py
"""
import ast
import importlib.util
import math
import os
import sys
import textwrap

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from blindshadowremoval_amd import train_losses as host            # noqa: E402
from blindshadowremoval_amd.ucb_post import resize_bilinear        # noqa: E402

_spec = importlib.util.spec_from_file_location("make_shadow_synth_fixture", os.path.join(ROOT, "tools", "make_shadow_synth_fixture.py"))
sm = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(sm)
REF = sm.REF
t, _as, f32 = sm.t, sm._as, np.float32

WANTED = ({"mask_bi", "mask_edge", "dif", "bmaskgt", "recon_loss_gs", "recon_loss_c", "grad_loss", "figs"}
          | {"grad_%s_%d" % (k, i) for k in ("gt", "rc") for i in range(1, 6)} | {"dif_grad_%d" % i for i in range(1, 6)})
CASES = {32: 3, 64: 2}          # S: B


def _resize(x, size, method=None):
    if method == "nearest":
        return sm._resize(x, size, method)
    assert method is None and int(size[0]) == int(size[1])
    return t(np.stack([resize_bilinear(item, int(size[0])) for item in np.asarray(x, np.float32)]))


def _image_gradients(x):
    x = np.asarray(x, np.float32)
    dy, dx = np.zeros_like(x), np.zeros_like(x)
    dy[:, :-1] = x[:, 1:] - x[:, :-1]
    dx[:, :, :-1] = x[:, :, 1:] - x[:, :, :-1]
    return t(dy), t(dx)


def _rgb_to_grayscale(x):
    x = np.asarray(x, np.float32)
    return t(((x[..., 0] * f32(0.2989) + x[..., 1] * f32(0.587)) + x[..., 2] * f32(0.114))[..., None])


def _dilation2d(x, k, strides, padding, data_format, dilations, name=None):
    x, k = np.asarray(x, np.float32), np.asarray(k, np.float32)
    assert padding == "SAME" and data_format == "NHWC" and list(strides) == [1, 1, 1, 1] and list(dilations) == [1, 1, 1, 1]
    kh, kw = k.shape[:2]
    H, W = x.shape[1:3]
    pad = np.full((x.shape[0], H + kh - 1, W + kw - 1, x.shape[3]), -np.inf, np.float32)
    pad[:, kh // 2:kh // 2 + H, kw // 2:kw // 2 + W] = x
    out = np.full(x.shape, -np.inf, np.float32)
    for i in range(kh):
        for j in range(kw):
            out = np.maximum(out, pad[:, i:i + H, j:j + W] + k[i, j])
    return t(out)


def _reduce_mean(x, axis=None, keepdims=False):
    x = _as(x)
    if axis is None:
        return t(np.sum(x, dtype=np.float32) / f32(x.size))
    return t(np.add.reduce(x, axis=axis, keepdims=keepdims, dtype=np.float32) / f32(x.shape[axis]))


def make_tf():
    tf = sm.make_tf(sm.Tape(np.random.default_rng(0), []))
    tf.image.resize, tf.image.image_gradients, tf.image.rgb_to_grayscale = _resize, _image_gradients, _rgb_to_grayscale
    tf.nn.dilation2d = _dilation2d
    tf.split = lambda x, n, axis=0: [t(p) for p in np.split(_as(x), n, axis=axis)]
    tf.reduce_mean = _reduce_mean
    tf.reduce_min = lambda x, axis=None, keepdims=False: t(np.min(_as(x), axis=axis, keepdims=keepdims))
    tf.reduce_sum = lambda x, axis=None, keepdims=False: t(np.sum(_as(x), axis=axis, keepdims=keepdims))
    tf.math.reduce_mean, tf.math.reduce_sum = tf.reduce_mean, tf.reduce_sum
    tf.ones = lambda shape: t(np.ones([int(s) for s in shape], np.float32))
    tf.ones_like = lambda x: t(np.ones_like(_as(x)))
    return tf


def cut_def(path, name, indent=""):
    """The source lines of `def name(` at `indent` in the reference's file `path`, up to the next line at that indent or less."""
    lines = open(os.path.join(REF, path)).read().split("\n")
    lo = next(i for i, l in enumerate(lines) if l.startswith(indent + "def " + name + "("))
    hi = lo + 1
    while hi < len(lines) and (not lines[hi].strip() or lines[hi].startswith(indent + "\t") or lines[hi].startswith(indent + " ")):
        hi += 1
    return "\n".join(l[len(indent):] for l in lines[lo:hi])


def loss_statements():
    """The assignments of train_step to the names in WANTED, in order, as a compiled module."""
    tree = ast.parse(textwrap.dedent(cut_def("train_test_GSC.py", "train_step", "\t")))
    picked = []

    def walk(body):
        for node in body:
            if isinstance(node, ast.With):
                walk(node.body)
            elif isinstance(node, ast.Assign) and len(node.targets) == 1 and isinstance(node.targets[0], ast.Name) and node.targets[0].id in WANTED:
                picked.append(node)
    walk(tree.body[0].body)
    assert {n.targets[0].id for n in picked} == WANTED, WANTED - {n.targets[0].id for n in picked}
    return compile(ast.Module(body=picked, type_ignores=[]), "train_step", "exec")


def reference_namespace(tf):
    ns = {"tf": tf, "np": np, "m": math}
    for name in ("l1_loss", "l1_loss_yuv", "find_edge"):
        exec(compile(cut_def("utils.py", name), name, "exec"), ns)
    exec(compile(cut_def("train_test_GSC.py", "get_img_grad"), "get_img_grad", "exec"), ns)
    return ns


def near_a_threshold(img, gt, mask_sv):
    m = mask_sv.astype(np.float64)
    mean_c, min_c = m.mean(axis=3), m.min(axis=3)
    dif = host.gray(gt).astype(np.float64) - host.gray(img).astype(np.float64)
    return min(np.abs(mean_c - .01).min(), np.abs(m - .01).min(), np.abs(min_c - .3).min(), np.abs(dif - .04).min()) <= 1e-5


def run_case(S, B, seed, code):
    img, gt, mask_sv, gs, con = host.example_inputs(S, B, seed)
    if near_a_threshold(img, gt, mask_sv):
        return None
    ns = reference_namespace(make_tf())
    ns.update(img=t(img), gt=t(gt), mask_sv=t(mask_sv), deshadow_img_gs=t(gs), deshadow_img_c=t(con), bmask=t(np.zeros((B, S, S, 1), np.float32)))
    with np.errstate(all="ignore"):
        exec(code, ns)
    figs = ns["figs"]
    out = {"seed": np.int64(seed), "B": np.int64(B), "S": np.int64(S), "backend": np.array("numpy stand-in"),
           "mask_edge": np.asarray(figs[4]).astype(np.uint8), "bmaskgt": np.asarray(figs[5]).astype(np.uint8), "dif_grad": np.asarray(figs[7]),
           "losses": np.array([float(ns["recon_loss_gs"]), float(ns["recon_loss_c"]), float(ns["grad_loss"])], np.float64)}
    assert out["mask_edge"].shape == out["bmaskgt"].shape == (B, S, S, 1) and out["dif_grad"].shape == (B, S, S, 3) and out["dif_grad"].dtype == np.float32
    assert np.isfinite(out["dif_grad"]).all() and np.isfinite(out["losses"]).all()
    return out


def main():
    code = loss_statements()
    done = []
    for S, B in CASES.items():
        seed = 100 * S
        while True:
            case = run_case(S, B, seed, code)
            if case is not None:
                break
            seed += 1
        ours = host.step_losses(*host.example_inputs(S, B, seed))
        assert np.array_equal(ours["mask_edge"], case["mask_edge"]) and np.array_equal(ours["bmaskgt"], case["bmaskgt"])
        plane = float(np.abs(ours["dif_grad"].astype(np.float64) - case["dif_grad"].astype(np.float64)).max())
        rel = float((np.abs(ours["losses"].astype(np.float64) - case["losses"]) / np.abs(case["losses"])).max())
        print("S=%d B=%d seed %d: losses %s, |host - reference| dif_grad %.3g, losses (relative) %.3g" % (S, B, seed, case["losses"], plane, rel))
        done.append((case, plane, rel))
    # one pair of figures for the set, the worst over its cases, as make_shadow_synth_fixture.py records its own
    worst_plane, worst_rel = max(d[1] for d in done), max(d[2] for d in done)
    for case, _, _ in done:
        case["measured_max_diff"], case["measured_rel_diff"] = np.float64(worst_plane), np.float64(worst_rel)
        path = os.path.join(ROOT, "tests", "golden", "train_losses_%d.npz" % int(case["S"]))
        np.savez_compressed(path, **case)
        print("wrote %s (%d bytes), measured_max_diff %.3g, measured_rel_diff %.3g" % (path, os.path.getsize(path), worst_plane, worst_rel))
        assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
