"""Generate tests/golden/ucb_post_tsm_9156.npz: outputs of the TSM model's OWN UCB post-processing.

The body of `FSRNet.test_step` of /root/reference/train_with_TSM.py (:418-618) is taken from the reference file at run time (ast ->
compile; nothing of it is written to this repository) and executed over the TensorFlow / cv2 stand-ins of tools/make_ucb_post_fixture.py
(imported, not copied; see its docstring for what they pin), completed here with the ops only this step calls (tf.image.flip_left_right,
tf.random.uniform, tf.math.maximum).  `self.gen` is a stub that accepts `frame` and `share` and returns the case's pair
con[2,S,S,3] / dif[2,S,S,1], as the TSM generator does for one group of two frames.  Inputs are the cases of tests/ucb_tsm_cases.py.
Stored per case:
  <case>_ssim, <case>_psnr       float32 losses
  <case>_frac, <case>_mean       float64 frac_nose_in_shadow and mean_intensity
  <case>_strip_sha256           SHA-256 of the uint8 strip [256, 2048, 3] = rint(clip(fig, 0, 1) * 255) of the eight figures side by side
  <case>_out                     float16 composite, for the `...a` cases only

    python tools/make_ucb_post_tsm_fixture.py [--out PATH]       # needs /root/reference
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

from make_ucb_post_fixture import _t, make_cv2, make_tf  # noqa: E402


def make_tf_tsm():
    tf = make_tf()
    tf.image.flip_left_right = lambda x: _t(np.asarray(x)[..., :, ::-1, :])
    tf.random = types.SimpleNamespace(uniform=lambda shape: _t(np.float32(0.5)))       # any draw but exactly 0.0: `share` is True
    tf.math = types.SimpleNamespace(maximum=lambda a, b: _t(np.maximum(np.asarray(a), np.asarray(b))))
    return tf


def reference_test_step_tsm(tf_mod, cv2_mod):
    """`FSRNet.test_step` compiled from train_with_TSM.py with tf / cv2 / np bound to the given modules."""
    with open(os.path.join(REF, "train_with_TSM.py")) as fsrc:
        tree = ast.parse(fsrc.read())
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "FSRNet")
    fn = next(n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "test_step")
    ns = {"tf": tf_mod, "cv2": cv2_mod, "np": np, "print": lambda *a, **k: None}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), "<reference TSM test_step>", "exec"), ns)
    return ns["test_step"]


def run_case(step, row, box, m, con0, con1, dif0):
    """The reference's step on one case -> (losses, figs, frac, mean)."""
    fake = types.SimpleNamespace(config=types.SimpleNamespace(IMG_SIZE=row.shape[0]))
    con = _t(np.stack([con0, con1]))
    dif = _t(np.stack([dif0, dif0[:, ::-1]]))

    def gen(img, uv, reg, frame, share, chuck, training):
        assert np.asarray(img).shape[0] == 2 and chuck == 4
        return None, con, None, dif
    fake.gen = gen
    pair = np.stack([row, row[:, ::-1]])                 # row 1 is not read after the generator call
    w = _t
    return step(fake, w(pair), w(np.asarray(box, np.float32)), w(m["face_hair"]), w(m["face"]), w(m["mouth"]), w(m["nose"]),
                w(m["eyebrow"]), w(m["eye"]), w(m["glasses"]), False)


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    out_path = os.path.join(ROOT, "tests", "golden", "ucb_post_tsm_9156.npz")
    while argv:
        a = argv.pop(0)
        if a == "--out" and argv:
            out_path = argv.pop(0)
        else:
            raise SystemExit(__doc__)
    from ucb_tsm_cases import cases
    step = reference_test_step_tsm(make_tf_tsm(), make_cv2())
    out = {"backend": np.array("standin")}
    for key, row, box, m, con0, con1, dif0 in cases():
        losses, figs, frac, mean = run_case(step, row, box, m, con0, con1, dif0)
        assert len(figs) == 8
        out[key + "_ssim"] = np.float32(losses["ssim"])
        out[key + "_psnr"] = np.float32(losses["psnr"])
        out[key + "_frac"] = np.float64(frac)
        out[key + "_mean"] = np.float64(mean)
        cols = [np.clip(np.asarray(f, np.float32)[0], 0.0, 1.0) * np.float32(255) for f in figs]
        strip = np.ascontiguousarray(np.rint(np.concatenate(cols, axis=1)).astype(np.uint8))
        out[key + "_strip_sha256"] = np.array(hashlib.sha256(strip.tobytes()).hexdigest())
        if key.endswith("a"):
            out[key + "_out"] = np.asarray(figs[1])[0].astype(np.float16)
        print(key, "ssim %.4f psnr %.2f frac %.4f mean %.4f" % (losses["ssim"], losses["psnr"], frac, mean))
    np.savez_compressed(out_path, **out)
    print(out_path, os.path.getsize(out_path), "bytes")
    return out


if __name__ == "__main__":
    main()
