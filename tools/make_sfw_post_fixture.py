"""Generate tests/golden/sfw_post_gsc.npz: outputs of the GSC model's OWN SFW scoring.

The body of `FSRNet.test_step_sfw` of /root/reference/train_test_GSC.py (:799-838) is taken from the reference file at run time
(ast -> compile; nothing of it is written to this repository) and executed over the TensorFlow stand-in of
tools/make_ucb_post_fixture.py (imported, not copied; `tf.equal` and `tf.constant`, which the UCB step does not call, are added here),
with `metrics` bound to the REAL sklearn.metrics — so the AUC is pinned to sklearn itself, not to a restatement — and `self.gen` a stub
that returns the case's outputs over the element's 10 rows.  SSIM / PSNR come from the stand-in's tf.image.ssim / psnr, i.e. from
blindshadowremoval_amd.metrics (see make_ucb_post_fixture.py for what that pins and what it does not).
Inputs are the cases of tests/sfw_post_cases.py (shared with the tests).  Stored per case:
  <case>_ssim, <case>_psnr       float32 losses
  <case>_auc                     float64: sklearn.metrics.roc_auc_score's own return value
  <case>_auc_f32                 float32: losses['auc'] as the reference stores it (tf.constant(auc, tf.float32))
  <case>_strip_sha256            SHA-256 of the uint8 strip [256, 1024, 3] of the four figures (Logging.save_img's pixels)

    python tools/make_sfw_post_fixture.py [--out PATH]       # needs /root/reference and sklearn
"""
import ast
import hashlib
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
REF = "/root/reference"

from make_ucb_post_fixture import _t, make_tf  # noqa: E402


def make_tf_sfw():
    tf = make_tf()
    tf.equal = lambda a, b: _t(np.asarray(a) == np.asarray(b))
    tf.constant = lambda x, dtype=None: _t(np.asarray(x, dtype=dtype))
    return tf


def reference_test_step_sfw(tf_mod, metrics_mod):
    """`FSRNet.test_step_sfw` compiled from train_test_GSC.py with tf / np / metrics bound to the given modules."""
    with open(os.path.join(REF, "train_test_GSC.py")) as fsrc:
        tree = ast.parse(fsrc.read())
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "FSRNet")
    fn = next(n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "test_step_sfw")
    ns = {"tf": tf_mod, "np": np, "metrics": metrics_mod, "print": lambda *a, **k: None}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), "<reference GSC test_step_sfw>", "exec"), ns)
    return ns["test_step_sfw"]


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    out_path = os.path.join(ROOT, "tests", "golden", "sfw_post_gsc.npz")
    while argv:
        a = argv.pop(0)
        if a == "--out" and argv:
            out_path = argv.pop(0)
        else:
            raise SystemExit(__doc__)
    import sklearn
    import sklearn.metrics
    from sfw_post_cases import cases, element
    seen = []
    metrics_mod = types.SimpleNamespace(roc_auc_score=lambda y, s: seen.append(sklearn.metrics.roc_auc_score(y, s)) or seen[-1])
    step = reference_test_step_sfw(make_tf_sfw(), metrics_mod)
    out = {"backend": np.array("standin-tf+sklearn-%s" % sklearn.__version__)}
    for key, img, con, mask, dif, face in cases():
        fake = types.SimpleNamespace(config=types.SimpleNamespace(IMG_SIZE=256))
        rep = lambda x: _t(np.repeat(x[None], 10, axis=0))
        fake.gen = lambda im, uv, reg, chuck, training, con=con, dif=dif: (rep(con[..., :1]), rep(con), rep(dif), rep(dif))
        seen.clear()
        losses, figs = step(fake, _t(element(img, con, mask, dif, face)), _t(np.array([0, 0, 256, 256], np.float32)), False)
        assert len(figs) == 4 and len(seen) == 1
        out[key + "_ssim"] = np.float32(losses["ssim"])
        out[key + "_psnr"] = np.float32(losses["psnr"])
        out[key + "_auc"] = np.float64(seen[0])
        out[key + "_auc_f32"] = np.float32(losses["auc"])
        cols = []
        for f in figs:
            c = np.clip(np.asarray(f, np.float32)[0], 0.0, 1.0) * np.float32(255)
            cols.append(np.repeat(c, 3, axis=2) if c.shape[2] == 1 else c[:, :, :3])
        strip = np.ascontiguousarray(np.rint(np.concatenate(cols, axis=1)).astype(np.uint8))
        assert strip.shape == (256, 1024, 3)
        out[key + "_strip_sha256"] = np.array(hashlib.sha256(strip.tobytes()).hexdigest())
        print(key, "ssim %.5f psnr %.3f auc %.17g" % (losses["ssim"], losses["psnr"], seen[0]))
    np.savez_compressed(out_path, **out)
    print(out_path, os.path.getsize(out_path), "bytes")
    return out


if __name__ == "__main__":
    main()
