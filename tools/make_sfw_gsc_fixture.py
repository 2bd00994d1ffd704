"""Generate tests/golden/sfw_gsc_elements.npz — what the GSC script's OWN SFW loader makes of tests/golden/sfw_synth.

Runs IN THE BUILD CONTAINER ONLY: imports /root/reference/dataset.py (with utils.py / warp.py) over the stand-ins of
tools/make_sample_fixture.py and tools/make_sfw_fixture.py (TensorFlow etc. stubbed; cv2.imread / cvtColor / resize / GaussianBlur
restated with OpenCV's documented semantics; tf.numpy_function simply calls the function) and calls `Dataset.parse_fn_test_sfw`
(dataset.py:338-612) on the two labelled frames of the synthetic folder, whose frames 1-19 cover both frames' nine neighbours.  One
more cv2 behaviour matters on this path and is restated here: cv2.resize of an HxWx1 array returns HxW of the input's dtype (the
8-bit mask of the neighbour chain).  Elements are [10,256,256,17] float32, so the fixture stores every 8th pixel of each (in both directions) plus
per-channel sums, like tools/make_sfw_fixture.py; tests/test_sfw_gsc_dataset.py rebuilds them with blindshadowremoval_amd.dataset."""
import contextlib
import io
import os
import sys
import types

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
SYNTH = os.path.join(ROOT, "tests", "golden", "sfw_synth", "vid0")


def main():
    import make_sample_fixture as msf
    msf._install_stubs()
    import cv2
    rgb = cv2.imread

    def imread(path, flag=1):
        if not os.path.isfile(path):
            return None
        if flag == 0:
            return np.asarray(Image.open(path).convert("L")).copy()
        return rgb(path)

    def resize(img, dsize, **k):
        a = np.asarray(img)
        if a.ndim == 3 and a.shape[2] == 1:
            a = a[:, :, 0]
        if (a.shape[1], a.shape[0]) == tuple(dsize):
            return a.copy()                                    # cv2 copies when the size does not change
        out = msf._resize_linear(a, dsize)
        if a.dtype == np.uint8:
            raise NotImplementedError("8-bit resize across sizes is not restated (all frames of the synthetic folder share their size)")
        return out
    cv2.imread = imread
    cv2.resize = resize
    tf = sys.modules["tensorflow"]
    tf.numpy_function = lambda fn, inp, Tout: fn(*inp)
    tf.ensure_shape = lambda x, shape: x
    tf.float32, tf.string = "float32", "string"
    tf.data = types.SimpleNamespace(experimental=types.SimpleNamespace(AUTOTUNE=-1))
    sys.path.insert(0, REF)
    import dataset as ref
    me = types.SimpleNamespace(config=types.SimpleNamespace(IMG_SIZE=256))
    out = {}
    with contextlib.redirect_stdout(io.StringIO()):
        for n in (1, 10):
            label = os.path.join(SYNTH, "%d_label.png" % n)
            img, box, name = ref.Dataset.parse_fn_test_sfw(me, label.encode())
            out["gsc%d" % n], out["gsc%d_box" % n] = np.asarray(img, np.float32), np.asarray(box, np.float32)
    small = {}
    for k, v in out.items():
        if v.ndim == 4:
            assert v.shape == (10, 256, 256, 17), v.shape
            small[k] = v[:, ::8, ::8, :].copy()
            small[k + "_sum"] = v.astype(np.float64).sum(axis=(1, 2))
        else:
            small[k] = v
    dst = os.path.join(ROOT, "tests", "golden", "sfw_gsc_elements.npz")
    np.savez_compressed(dst, **small)
    print(dst, os.path.getsize(dst), {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
