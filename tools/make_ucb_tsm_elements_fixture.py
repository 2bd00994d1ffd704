"""Generate tests/golden/ucb_tsm_elements.npz — what the TSM script's OWN UCB loader makes of two items of tests/golden/UCB.

Runs IN THE BUILD CONTAINER ONLY: imports /root/reference/dataset_with_TSM.py (with utils.py / warp.py) over the stand-ins of
tools/make_sample_fixture.py (TensorFlow etc. stubbed; cv2.imread / cvtColor / resize / GaussianBlur restated with OpenCV's documented
semantics, cv2.flip as in tools/make_sfw_fixture.py; tf.numpy_function simply calls the function) and calls `Dataset.parse_fn_test`
(dataset_with_TSM.py:153-189) on the items' landmark files.  The reference builds the ground-truth path from `_lm_part[0:7]` (:159), so
the items are copied under a temporary folder of exactly that depth: <5 folders>/train/{input,gt}/9156/.  Elements are [2,256,256,16]
float32; the fixture stores every 8th pixel (in both directions) plus per-channel sums, like tools/make_sfw_gsc_fixture.py, and the box.
tests/test_ucb_tsm_dataset.py rebuilds them with blindshadowremoval_amd.dataset (dset='ucb_tsm')."""
import contextlib
import io
import os
import shutil
import sys
import tempfile
import types

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
GOLDEN_UCB = os.path.join(ROOT, "tests", "golden", "UCB", "train")
ITEMS = ("9156-004", "9156-005")


def staged_tree(tmp):
    """Copy the items to <tmp>/x.../train/{input,gt}/9156 with `train` at index 6 of path.split('/') -> the input folder."""
    depth = len(os.path.abspath(tmp).split("/"))
    if depth > 6:
        raise SystemExit("temporary folder %s is too deep for the reference's _lm_part[0:7]" % tmp)
    base = os.path.join(tmp, *["d%d" % i for i in range(6 - depth)], "train")
    for kind in ("input", "gt"):
        os.makedirs(os.path.join(base, kind, "9156"))
    for item in ITEMS:
        for ext in (".png", ".npy"):
            shutil.copy(os.path.join(GOLDEN_UCB, "input", "9156", item + ext), os.path.join(base, "input", "9156"))
        shutil.copy(os.path.join(GOLDEN_UCB, "gt", "9156", item + ".png"), os.path.join(base, "gt", "9156"))
    assert base.split("/")[6] == "train", base
    return os.path.join(base, "input", "9156")


def main():
    import make_sample_fixture as msf
    msf._install_stubs()
    import cv2
    cv2.flip = lambda img, code: np.ascontiguousarray(img[:, ::-1]) if code == 1 else (_ for _ in ()).throw(NotImplementedError())
    rgb = cv2.imread

    def imread(path, flag=1):
        if not os.path.isfile(path):
            return None
        if flag == 0:
            return np.asarray(Image.open(path).convert("L")).copy()
        return rgb(path)
    cv2.imread = imread
    tf = sys.modules["tensorflow"]
    tf.numpy_function = lambda fn, inp, Tout: fn(*inp)
    tf.ensure_shape = lambda x, shape: x
    tf.float32, tf.string = "float32", "string"
    tf.data = types.SimpleNamespace(experimental=types.SimpleNamespace(AUTOTUNE=-1))
    sys.path.insert(0, REF)
    import dataset_with_TSM as ref
    me = types.SimpleNamespace(config=types.SimpleNamespace(IMG_SIZE=256))
    small = {}
    tmp = tempfile.mkdtemp()
    try:
        folder = staged_tree(tmp)
        with contextlib.redirect_stdout(io.StringIO()):
            for item in ITEMS:
                img, box, name = ref.Dataset.parse_fn_test(me, os.path.join(folder, item + ".npy").encode())
                img = np.asarray(img, np.float32)
                assert img.shape == (2, 256, 256, 16), img.shape
                assert name.endswith("/train/gt/9156/%s.png" % item), name
                key = item.replace("-", "_")
                small[key] = img[:, ::8, ::8, :].copy()
                small[key + "_sum"] = img.astype(np.float64).sum(axis=(1, 2))
                small[key + "_box"] = np.asarray(box, np.float32)
    finally:
        shutil.rmtree(tmp)
    dst = os.path.join(ROOT, "tests", "golden", "ucb_tsm_elements.npz")
    np.savez_compressed(dst, **small)
    print(dst, os.path.getsize(dst))


if __name__ == "__main__":
    main()
