"""Generate tests/golden/wild_crop.npz — what the reference's OWN `dataprocess.py` ("Preprocessing New Images") makes of the cases of
tests/wild_cases.py.

Runs IN THE BUILD CONTAINER ONLY: it executes the text of /root/reference/dataprocess.py, once per case, in a scratch folder that holds
the case as `sample_uncropped_images/<name>.png` + `.npy`, over stand-ins for the two modules that are not installed here:
  cv2.imread   -> PIL's RGB decode, channels reversed (BGR)
  cv2.resize   -> blindshadowremoval_amd.wild_crop.resize_u8 for an 8-bit image, resize_f64 for a float64 one: the host statement's two
                  restatements of OpenCV's INTER_LINEAR — the RESIZE ARITHMETIC IS THEREFORE NOT PINNED HERE, only the script's wiring
                  (box, skip rule, padding, which resize runs on what, landmark shift and scale)
  cv2.imwrite  -> wild_crop.to_u8 for a float64 image (cvRound + saturation), channels reversed back, kept in memory
  skimage.io   -> an empty module (imported, never used)
The script's `box` is read from its namespace after the run.  Per case the fixture stores the input landmarks, the box, the landmarks
and the crop the script wrote (kept = 0 and zeros where it wrote nothing).  The synthetic photographs are rebuilt from their seeds by
tests/wild_cases.py; "01001" is tests/golden/wild/01001 (the reference's photograph trimmed to the window around its box, see
wild_cases.py), and this tool also runs the reference's whole 1024 x 1024 file and requires the same crop, the same landmarks and
the box shifted by the window's corner.  tests/test_wild_crop.py reads only the fixture and tests/golden/wild/."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _install_stubs(written: dict):
    from blindshadowremoval_amd import wild_crop as W
    cv2 = types.ModuleType("cv2")
    cv2.IMWRITE_PNG_COMPRESSION = 16
    cv2.imread = lambda path: np.asarray(Image.open(path).convert("RGB"))[:, :, ::-1].copy()

    def resize(img, dsize, **k):
        assert tuple(dsize) == (256, 256) and not k
        a = np.ascontiguousarray(img)
        return W.resize_u8(a, 256) if a.dtype == np.uint8 else W.resize_f64(a, 256)

    def imwrite(path, img, params=None):
        a = np.asarray(img)
        written[path] = (a if a.dtype == np.uint8 else W.to_u8(a))[:, :, ::-1].copy()
        return True
    cv2.resize, cv2.imwrite = resize, imwrite
    sys.modules["cv2"] = cv2
    sk = types.ModuleType("skimage")
    sk.io = types.ModuleType("skimage.io")
    sys.modules["skimage"], sys.modules["skimage.io"] = sk, sk.io


def run_script(img: np.ndarray, lm: np.ndarray, name: str, text: str, written: dict):
    """dataprocess.py over one photograph -> (box, lm256 | None, crop | None)"""
    work = tempfile.mkdtemp(prefix="wild_fixture_")
    cwd = os.getcwd()
    try:
        os.makedirs(os.path.join(work, "sample_uncropped_images"))
        os.makedirs(os.path.join(work, "sample_uncropped_images_cropped"))
        Image.fromarray(img).save(os.path.join(work, "sample_uncropped_images", name + ".png"))
        np.save(os.path.join(work, "sample_uncropped_images", name + ".npy"), lm)
        os.chdir(work)
        written.clear()
        ns = {"__name__": "dataprocess"}
        with contextlib.redirect_stdout(io.StringIO()):
            exec(compile(text, os.path.join(REF, "dataprocess.py"), "exec"), ns)
        box = [int(v) for v in ns["box"]]
        out = os.path.join("sample_uncropped_images_cropped", name, name)
        if not written:
            assert not os.path.exists(out + ".npy")
            return box, None, None
        (path, crop), = written.items()
        assert path == out + ".png", path
        return box, np.load(out + ".npy"), crop
    finally:
        os.chdir(cwd)
        shutil.rmtree(work, ignore_errors=True)


def main():
    import wild_cases as C
    from blindshadowremoval_amd.pngio import read_rgb_u8
    written = {}
    _install_stubs(written)
    with open(os.path.join(REF, "dataprocess.py")) as f:
        text = f.read()
    cases = {name: C.case_inputs(name) for name in sorted(C.CASES)}
    cases["01001"] = (read_rgb_u8(os.path.join(C.WILD, "01001.png")), np.load(os.path.join(C.WILD, "01001.npy")))
    out = {"names": np.array(sorted(cases))}
    for name, (img, lm) in sorted(cases.items()):
        box, lm256, crop = run_script(img, lm, name, text, written)
        kept = crop is not None
        out[name + "_lm_in"], out[name + "_box"], out[name + "_kept"] = lm, np.asarray(box, np.int32), np.int32(kept)
        out[name + "_lm"] = lm256 if kept else np.zeros((68, 2), np.float32)
        out[name + "_crop"] = crop if kept else np.zeros((1, 1, 3), np.uint8)
        assert not kept or (lm256.dtype == np.float32 and crop.dtype == np.uint8 and crop.shape == (256, 256, 3))
        print(name, "kept" if kept else "skipped", box)
    # the trimmed 01001 against the reference's whole photograph
    whole = os.path.join(REF, "sample_uncropped_images", "01001")
    box, lm256, crop = run_script(read_rgb_u8(whole + ".png"), np.load(whole + ".npy"), "01001", text, written)
    assert np.array_equal(crop, out["01001_crop"]) and np.array_equal(lm256, out["01001_lm"])
    assert [box[0] - C.TRIM[0], box[1] - C.TRIM[1], box[2] - C.TRIM[0], box[3] - C.TRIM[1]] == out["01001_box"].tolist()
    dst = C.FIXTURE
    np.savez_compressed(dst, **out)
    print(dst, os.path.getsize(dst))


if __name__ == "__main__":
    main()
