"""Generate tests/golden/ucb_post_rgb_9156.npz: outputs of the RGB baseline's OWN UCB post-processing.

The body of `FSRNet.test_step` of /root/reference/train_RGB_test.py (:403-505) is taken from the reference file at run time (ast ->
compile; nothing of it is written to this repository) and executed over the TensorFlow / cv2 stand-ins of
tools/make_ucb_post_fixture.py (imported, not copied: see its docstring for what they pin and what they do not), with `self.gen` a
stub that returns the case's `con` repeated over the element's 10 rows as ONE tensor, as model_RGB.Generator returns it.
Inputs are the ten cases of tests/ucb_cases.py (shared with the GSC fixture and with the tests).  Stored per case:
  <case>_ssim, <case>_psnr       float32 losses
  <case>_strip_sha256           SHA-256 of the uint8 strip [256, 768, 3] = rint(clip(fig, 0, 1) * 255) of the three figures side by
                                 side (Logging.save_img): byte equality is checked through the digest, because the ten strips
                                 themselves are 3.6 MB compressed (noisy predictions) and the file is kept well under 1 MB
  <case>_out                     float16 composite, for the `...a` cases only (as the GSC fixture)

    python tools/make_ucb_post_rgb_fixture.py [--backend standin|tf] [--out PATH]       # needs /root/reference
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

from make_ucb_post_fixture import _t, load_backend  # noqa: E402  (the stand-ins: make_tf / make_cv2 behind load_backend)


def reference_test_step_rgb(tf_mod, cv2_mod):
    """`FSRNet.test_step` compiled from train_RGB_test.py with tf / cv2 / np bound to the given modules."""
    with open(os.path.join(REF, "train_RGB_test.py")) as fsrc:
        tree = ast.parse(fsrc.read())
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "FSRNet")
    fn = next(n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "test_step")
    ns = {"tf": tf_mod, "cv2": cv2_mod, "np": np, "print": lambda *a, **k: None}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), "<reference RGB test_step>", "exec"), ns)
    return ns["test_step"]


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    backend, out_path = "standin", os.path.join(ROOT, "tests", "golden", "ucb_post_rgb_9156.npz")
    while argv:
        a = argv.pop(0)
        if a == "--backend" and argv:
            backend = argv.pop(0)
            if backend not in ("standin", "tf"):
                raise SystemExit("--backend must be standin or tf")
        elif a == "--out" and argv:
            out_path = argv.pop(0)
        else:
            raise SystemExit(__doc__)
    from ucb_cases import cases
    tf_mod, cv2_mod, label = load_backend(backend)
    step = reference_test_step_rgb(tf_mod, cv2_mod)
    real_tf = label.startswith("tf-") and label != "tf-mock"
    wrap = (lambda x, dtype=None: tf_mod.convert_to_tensor(np.asarray(x, dtype=dtype))) if real_tf else _t
    out = {"backend": np.array(label)}
    for key, row, box, m, con, _ in cases():
        fake = types.SimpleNamespace(config=types.SimpleNamespace(IMG_SIZE=256))
        fake.gen = lambda im, uv, reg, chuck, training, con=con: wrap(np.repeat(con[None], 10, 0))
        stack = np.repeat(row[None], 10, axis=0)
        losses, figs = step(fake, wrap(stack), wrap(np.asarray(box, np.int32)), wrap(m["face_hair"]), wrap(m["face"]), wrap(m["mouth"]), wrap(m["nose"]),
                            wrap(m["eyebrow"]), wrap(m["eye"]), wrap(m["glasses"]), False)
        assert len(figs) == 3
        out[key + "_ssim"] = np.float32(losses["ssim"])
        out[key + "_psnr"] = np.float32(losses["psnr"])
        cols = [np.clip(np.asarray(f, np.float32)[0], 0.0, 1.0) * np.float32(255) for f in figs]
        strip = np.ascontiguousarray(np.rint(np.concatenate(cols, axis=1)).astype(np.uint8))
        out[key + "_strip_sha256"] = np.array(hashlib.sha256(strip.tobytes()).hexdigest())
        if key.endswith("a"):
            out[key + "_out"] = np.asarray(figs[1])[0].astype(np.float16)
        print(key, "size", int(box[3] - box[1]), "ssim %.4f psnr %.2f" % (losses["ssim"], losses["psnr"]))
    np.savez_compressed(out_path, **out)
    print(out_path, os.path.getsize(out_path), "bytes")
    return out


if __name__ == "__main__":
    main()
