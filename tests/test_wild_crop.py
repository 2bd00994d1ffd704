"""blindshadowremoval_amd/wild_crop.py — the reference's "Preprocessing New Images" procedure (dataprocess.py) restated — on the host:
its wiring against the reference's own text (tests/golden/wild_crop.npz, tools/make_wild_crop_fixture.py), its 8-bit resize against
the float64 bilinear it approximates, the folder it writes against the loader that reads uncropped photographs directly, the command
line's rules, and the host reconstruction of tall PNG files against PIL."""
import io
import os

import numpy as np
import pytest

import wild_cases as C


@pytest.fixture(scope="module")
def fixture():
    return np.load(C.FIXTURE)


def _inputs(name):
    from blindshadowremoval_amd.pngio import read_rgb_u8
    if name == "01001":
        return read_rgb_u8(os.path.join(C.WILD, "01001.png")), np.load(os.path.join(C.WILD, "01001.npy"))
    return C.case_inputs(name)


@pytest.mark.parametrize("name", sorted(C.CASES) + ["01001"])
def test_crop_face_reproduces_the_reference_script(fixture, name):
    from blindshadowremoval_amd.wild_crop import crop_face, crop_geometry
    img, lm = _inputs(name)
    np.testing.assert_array_equal(lm, fixture[name + "_lm_in"])          # the case is the one the fixture was made from
    res = crop_face(img, lm)
    if not int(fixture[name + "_kept"]):
        assert res is None and crop_geometry(lm, img.shape[0], img.shape[1]) is None
        return
    face, lm256, box = res
    assert list(box) == fixture[name + "_box"].tolist()
    assert lm256.dtype == np.float32 and face.dtype == np.uint8 and face.shape == (256, 256, 3)
    np.testing.assert_array_equal(lm256, fixture[name + "_lm"])
    np.testing.assert_array_equal(face, fixture[name + "_crop"])


def test_the_fixture_reaches_every_branch(fixture):
    """The padded branch on each side, the exact edge without padding, the skip rule."""
    from blindshadowremoval_amd.wild_crop import crop_geometry
    padded = {}
    for name in sorted(C.CASES):
        img, lm = C.case_inputs(name)
        geo = crop_geometry(lm, img.shape[0], img.shape[1])
        padded[name] = None if geo is None else (geo[1] > 0, geo[2] > 0)
    assert padded["skip"] is None and padded["just_kept"] == (False, False)
    assert padded["inside"] == padded["edge_exact"] == (False, False)
    assert padded["left"] == padded["right"] == (True, False) and padded["top"] == padded["bottom"] == (False, True)
    assert padded["left_top"] == padded["right_bottom_frac"] == (True, True)
    box = fixture["edge_exact_box"].tolist()
    assert box[2] == C.PHOTO_W and box[3] == C.PHOTO_H


def _bilinear_f64(img, size):
    """float64 half-pixel bilinear with an edge clamp, rounded half to even: what the 8-bit fixed-point resize approximates."""
    f = img.astype(np.float64)

    def axis(n):
        src = np.maximum((np.arange(size) + 0.5) * (n / size) - 0.5, 0.0)
        i0 = np.minimum(np.floor(src).astype(np.int64), n - 1)
        return i0, np.minimum(i0 + 1, n - 1), src - i0
    y0, y1, wy = axis(f.shape[0])
    x0, x1, wx = axis(f.shape[1])
    wx, wy = wx[None, :, None], wy[:, None, None]
    top = f[y0][:, x0] * (1 - wx) + f[y0][:, x1] * wx
    bot = f[y1][:, x0] * (1 - wx) + f[y1][:, x1] * wx
    return np.rint(top * (1 - wy) + bot * wy)


def test_the_8bit_resize_stays_within_one_grey_level_of_float_bilinear(fixture):
    """The 11-bit coefficients and the truncating shifts of the fixed-point form cost at most one grey level."""
    from blindshadowremoval_amd.wild_crop import resize_u8
    img, _ = _inputs("01001")
    box = fixture["01001_box"].tolist()
    for a in (C.noise(600, 560, 7), img[box[1]:box[3], box[0]:box[2]]):
        d = np.abs(resize_u8(a, 256).astype(np.int64) - _bilinear_f64(a, 256))
        print("8-bit resize vs float64 bilinear: max %d, differing %.3f" % (d.max(), (d > 0).mean()))
        assert d.max() <= 1


def test_the_padded_resize_is_float_bilinear_with_float32_weights():
    """resize_f64 against the same float64 bilinear: only the float32 rounding of the source coordinate separates them.  A coordinate
    below 512 is within 2^-24 * 512 of its double; that error enters each of the four weights once, on values of at most 255."""
    from blindshadowremoval_amd.wild_crop import resize_f64
    a = C.noise(300, 280, 3).astype(np.float64)
    f = a

    def axis(n):
        src = np.maximum((np.arange(64) + 0.5) * (n / 64) - 0.5, 0.0)
        i0 = np.minimum(np.floor(src).astype(np.int64), n - 1)
        return i0, np.minimum(i0 + 1, n - 1), src - i0
    y0, y1, wy = axis(300)
    x0, x1, wx = axis(280)
    wx, wy = wx[None, :, None], wy[:, None, None]
    want = (f[y0][:, x0] * (1 - wx) + f[y0][:, x1] * wx) * (1 - wy) + (f[y1][:, x0] * (1 - wx) + f[y1][:, x1] * wx) * wy
    assert np.abs(resize_f64(a, 64) - want).max() <= 255 * 4 * 2.0 ** -24 * 512


def _wild_folder(tmp_path):
    """01001 and a photograph the size rule drops, side by side as in sample_uncropped_images/."""
    import shutil
    from blindshadowremoval_amd.pngio import write_png
    src = tmp_path / "uncropped"
    src.mkdir()
    for ext in (".png", ".npy"):
        shutil.copy(os.path.join(C.WILD, "01001" + ext), str(src / ("01001" + ext)))
    img, lm = C.case_inputs("skip")
    write_png(str(src / "00002.png"), img)
    np.save(str(src / "00002.npy"), lm)
    return src


def test_the_uncropped_loader_equals_the_folder_route(tmp_path):
    from blindshadowremoval_amd.dataset import Dataset
    from blindshadowremoval_amd.fsrnet import Config
    from blindshadowremoval_amd.wild_crop import main, preprocess_folder
    src = _wild_folder(tmp_path)
    dst = tmp_path / "cropped"
    assert preprocess_folder(str(src / "*.png"), str(dst)) == ["01001"]
    assert sorted(os.listdir(str(dst))) == ["01001"] and sorted(os.listdir(str(dst / "01001"))) == ["01001.npy", "01001.png"]
    cfg = Config(0)
    cfg.DATA_DIR_TEST = [str(dst / "*")]
    folder = Dataset(cfg, "test")
    cfg2 = Config(0)
    cfg2.DATA_DIR_TEST = [str(src / "*.png")]
    wild = Dataset(cfg2, "test", uncropped=True)
    assert wild.name_list == [str(src / "01001.png")]                      # 00002 fails `length > 250`
    a, b = next(folder.feed), next(wild.feed)
    assert a[0].shape == b[0].shape == (1, 1, 256, 256, 16) and a[0].dtype == b[0].dtype == np.float32
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert next(wild.feed, None) is None
    # the command is preprocess_folder
    dst2 = tmp_path / "cropped2"
    assert main([str(src / "*.png"), str(dst2)]) == 0
    for f in ("01001.png", "01001.npy"):
        with open(str(dst / "01001" / f), "rb") as fa, open(str(dst2 / "01001" / f), "rb") as fb:
            assert fa.read() == fb.read()
    assert main([str(src / "*.png")]) == 2


def test_uncropped_is_the_ffhq_loader_only():
    from blindshadowremoval_amd.dataset import Dataset
    from blindshadowremoval_amd.fsrnet import Config
    cfg = Config(0)
    cfg.DATA_DIR_TEST = []
    for kw in (dict(ucb=True), dict(rows=10), dict(dset="sfw"), dict(dset="ucb_tsm", ucb=True, device_groups=0)):
        with pytest.raises(ValueError):
            Dataset(cfg, "test", uncropped=True, **kw)


@pytest.mark.parametrize("extra", [["--loop", "ucb"], ["--loop", "sfw"], ["--loop", "sfw_video"], ["--model", "tsm", "--loop", "ucb"],
                                   ["--model", "rgb", "--loop", "ucb"]])
def test_run_loop_refuses_uncropped_outside_the_ffhq_loop(extra, tmp_path, capsys):
    from blindshadowremoval_amd import run_loop
    rc = run_loop.main(["--uncropped", "--data", str(tmp_path / "*.png"), "--checkpoint-dir", str(tmp_path)] + extra)
    assert rc == 2
    assert "--uncropped" in capsys.readouterr().err


def test_run_loop_knows_the_flags(monkeypatch):
    """--uncropped and --host-prep parse together with --loop ffhq (the loop itself needs a GPU: tests/test_wild_crop_gpu.py)."""
    import argparse
    from blindshadowremoval_amd import run_loop
    seen = {}
    real = argparse.ArgumentParser.parse_args

    def spy(self, argv=None):
        seen.update(vars(real(self, argv)))
        raise SystemExit(0)                     # stop before the device probe
    monkeypatch.setattr(argparse.ArgumentParser, "parse_args", spy)
    with pytest.raises(SystemExit):
        run_loop.main(["--loop", "ffhq", "--uncropped", "--host-prep", "--data", "x/*.png", "--checkpoint-dir", "y"])
    assert seen["uncropped"] is True and seen["host_prep"] is True and seen["loop"] == "ffhq"


@pytest.mark.parametrize("h", [257, 513, 1024])
def test_tall_host_reconstruction_equals_pil(h):
    """Files taller than the short device kernel's 256 rows, written by PIL's encoder (adaptive filters), reconstructed by the host
    statement bsr_png_unfilter_tall is held to."""
    from PIL import Image
    from blindshadowremoval_amd import pngio
    from blindshadowremoval_amd.wild_crop import unfilter_tall_host
    rng = np.random.RandomState(h)
    img = np.cumsum(rng.randint(-3, 4, (h, 37, 3)), axis=0).astype(np.uint8)      # smooth down the columns: the encoder picks Up / Paeth / Average rows
    b = io.BytesIO()
    Image.fromarray(img).save(b, "PNG")
    w, hh, c, raw = pngio._parse_8bit(b.getvalue())
    assert (w, hh, c) == (37, h, 3)
    out = unfilter_tall_host(raw, hh, w, c)
    np.testing.assert_array_equal(out, np.asarray(Image.open(io.BytesIO(b.getvalue())).convert("RGB")))
    np.testing.assert_array_equal(out, img)
