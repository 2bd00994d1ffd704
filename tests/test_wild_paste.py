"""The host statement of the way back for in-the-wild photographs (blindshadowremoval_amd/wild_paste.py): properties that follow from
its arithmetic, on the constructed cases of tests/wild_paste_cases.py, the refusals, and Dataset(keep_photo=True) on the host route.
The reference has no counterpart of this step: the statement is pinned by these properties, and the device kernel to the statement
(tests/test_wild_paste_gpu.py)."""
import os

import numpy as np
import pytest

import wild_cases as W
import wild_paste_cases as C
from blindshadowremoval_amd.wild_paste import MODES, paste_face, paste_region


def _run(c, mode, **over):
    a = dict(c, **over)
    return paste_face(a["photo"], a["box"], a["preset_x"], a["preset_y"], a["im"], a["con"], a["face"], mode)


def _region(c):
    h, w = c["photo"].shape[:2]
    return paste_region(c["box"], c["preset_x"], c["preset_y"], h, w)


def test_the_cases_cover_what_they_claim():
    cs = C.cases()
    assert {c["S"] for c in cs} == set(C.SIZES)
    for S in C.SIZES:
        assert {c["n"] for c in cs if c["S"] == S} == set(C.sides(S))
    pos = {c["position"] for c in cs}
    assert {"inside", "flush_left", "flush_top", "flush_right", "flush_bottom", "out_left", "out_right", "out_top", "out_bottom", "out_left_top",
            "out_right_bottom", "over_centred", "over_corner"} <= pos
    assert {c["face_kind"] for c in cs} == {"ones", "zeros", "ramp"}
    assert any(c["preset_x"] > 0 and c["preset_y"] > 0 for c in cs) and any(c["preset_x"] > 0 and c["preset_y"] == 0 for c in cs)
    whole = [c for c in cs if _region(c) == (0, 0, c["photo"].shape[1], c["photo"].shape[0])]
    assert whole, "no box larger than its whole photograph"
    assert any((c["con"] < 0).any() and (c["con"] > 1).any() for c in cs)
    assert {c["photo"].shape[:2] for c in cs} == set(C.PHOTOS)
    # the same bytes on every call and in every process
    first = cs[0]["photo"].copy()
    C._CASES = None
    assert np.array_equal(C.cases()[0]["photo"], first)


@pytest.mark.parametrize("mode", MODES)
def test_pixels_outside_the_box_are_the_photographs(mode):
    for c in C.cases():
        out = _run(c, mode)
        assert out.dtype == np.uint8 and out.shape == c["photo"].shape
        x_lo, y_lo, x_hi, y_hi = _region(c)
        keep = np.ones(c["photo"].shape[:2], bool)
        if x_hi > x_lo and y_hi > y_lo:
            keep[y_lo:y_hi, x_lo:x_hi] = False
        assert np.array_equal(out[keep], c["photo"][keep]), c["name"]


def test_residual_without_a_change_or_without_a_face_returns_the_photograph():
    for c in C.cases():
        assert np.array_equal(_run(c, "residual", con=np.clip(c["im"], 0, 1), im=np.clip(c["im"], 0, 1)), c["photo"]), c["name"]
        assert np.array_equal(_run(c, "residual", face=np.zeros_like(c["face"])), c["photo"]), c["name"]
    zeros = [c for c in C.cases() if c["face_kind"] == "zeros"]
    assert zeros and all(np.array_equal(_run(c, "residual"), c["photo"]) for c in zeros)


def test_residual_changes_something_where_there_is_a_face():
    hit = [c for c in C.cases() if c["face_kind"] == "ones" and c["want"] is None]
    assert hit and all(not np.array_equal(_run(c, "residual"), c["photo"]) for c in hit)


def test_replace_at_the_networks_own_size_is_the_prediction():
    seen = 0
    for c in C.cases():
        if c["n"] != c["S"] or c["position"] != "inside":
            continue
        seen += 1
        out = _run(c, "replace", face=np.ones_like(c["face"]))
        x0, y0, x1, y1 = c["box"]
        want = np.clip(np.rint(np.clip(c["con"], 0, 1) * np.float32(255)), 0, 255).astype(np.uint8)
        assert np.array_equal(out[y0:y1, x0:x1], want), c["name"]
    assert seen >= len(C.SIZES)


@pytest.mark.parametrize("d", [0.1, -0.2, 37 / 255.0])
def test_a_constant_residual_shifts_the_box_by_its_grey_levels(d):
    """The interpolation weights sum to one in float32: a constant plane comes back as that constant, within one grey level."""
    for c in C.cases():
        S = c["S"]
        im = np.full((S, S, 3), 0.5, np.float32)
        out = _run(c, "residual", im=im, con=(im + np.float32(d)).astype(np.float32), face=np.ones((S, S, 1), np.float32))
        x_lo, y_lo, x_hi, y_hi = _region(c)
        if x_hi <= x_lo or y_hi <= y_lo:
            continue
        want = np.clip(c["photo"][y_lo:y_hi, x_lo:x_hi].astype(np.int64) + int(np.rint(255 * d)), 0, 255)
        assert np.abs(out[y_lo:y_hi, x_lo:x_hi].astype(np.int64) - want).max() <= 1, c["name"]


def test_ties_round_half_to_even_and_saturate():
    half = [c for c in C.cases() if c["want"] is not None]
    assert len(half) == len(C.SIZES)
    for c in half:
        x0, y0, x1, y1 = c["box"]
        got = _run(c, "residual")[y0:y1, x0:x1]
        assert np.array_equal(got, c["want"]), c["name"]
        assert (c["want"] == 0).any() and (c["want"] == 255).any()


@pytest.mark.parametrize("mode", MODES)
def test_a_padded_box_equals_the_materialised_canvas(mode):
    """Only pixels of the photograph are produced; they are the ones the same case gives on the explicit zero canvas, cropped back."""
    seen = 0
    for c in C.cases():
        px, py = c["preset_x"], c["preset_y"]
        if px == 0 and py == 0:
            continue
        seen += 1
        h, w = c["photo"].shape[:2]
        canvas = np.zeros((h + 2 * py + 2, w + 2 * px + 2, 3), np.uint8)
        canvas[py:py + h, px:px + w] = c["photo"]
        big = paste_face(canvas, c["box"], 0, 0, c["im"], c["con"], c["face"], mode)
        assert np.array_equal(_run(c, mode), big[py:py + h, px:px + w]), c["name"]
    assert seen > 20


def test_refusals():
    c = C.cases()[0]
    with pytest.raises(ValueError, match="uint8"):
        _run(c, "residual", photo=c["photo"].astype(np.float32))
    with pytest.raises(ValueError, match="uint8"):
        _run(c, "residual", photo=c["photo"][:, :, 0])
    with pytest.raises(ValueError, match="at least 2"):
        _run(c, "residual", box=[3, 3, 4, 4])
    with pytest.raises(ValueError, match="mode"):
        _run(c, "gain")
    with pytest.raises(ValueError, match=r"\[S,S,3\]"):
        _run(c, "residual", face=c["face"][:, :, 0])


@pytest.mark.parametrize("argv", [["--loop", "ffhq", "--paste-back"], ["--loop", "ffhq", "--paste-back", "replace"],
                                  ["--loop", "ucb", "--paste-back"], ["--model", "rgb", "--loop", "ucb", "--paste-back"],
                                  ["--model", "tsm", "--loop", "sfw", "--paste-back", "residual"], ["--loop", "sfw", "--paste-back"]])
def test_run_loop_refuses_paste_back_without_uncropped_photographs(argv, capsys, tmp_path):
    from blindshadowremoval_amd import run_loop
    assert run_loop.main(argv + ["--data", "x", "--checkpoint-dir", str(tmp_path)]) == 2
    assert "--paste-back" in capsys.readouterr().err


def test_run_loop_refuses_an_unknown_mode(tmp_path):
    from blindshadowremoval_amd import run_loop
    with pytest.raises(SystemExit) as e:
        run_loop.main(["--loop", "ffhq", "--uncropped", "--paste-back", "gain", "--data", "x", "--checkpoint-dir", str(tmp_path)])
    assert e.value.code == 2


def test_keep_photo_leaves_the_row_as_it_is_and_adds_the_photograph():
    from blindshadowremoval_amd.dataset import Dataset
    from blindshadowremoval_amd.fsrnet import Config
    from blindshadowremoval_amd.pngio import read_rgb_u8
    from blindshadowremoval_amd.wild_crop import crop_geometry
    src = os.path.join(W.WILD, "*.png")
    got = []
    for keep in (False, True):
        cfg = Config(0)
        cfg.DATA_DIR_TEST = [src]
        ds = Dataset(cfg, "test", uncropped=True, keep_photo=keep)
        got.append(list(ds.feed))
        ds.close()
    (plain,), (kept,) = got
    assert len(plain) == 3 and len(kept) == 4
    assert plain[0].tobytes() == kept[0].tobytes() and plain[1].tobytes() == kept[1].tobytes() and plain[2] == kept[2]
    photo = read_rgb_u8(os.path.join(W.WILD, "01001.png"))
    ph = kept[3]
    assert np.array_equal(ph.array, photo) and (ph.h, ph.w) == photo.shape[:2] and ph.blob is None
    box, px, py, _ = crop_geometry(np.load(os.path.join(W.WILD, "01001.npy")), photo.shape[0], photo.shape[1])
    assert (ph.box, ph.preset_x, ph.preset_y) == (list(box), px, py)


def test_keep_photo_needs_uncropped():
    from blindshadowremoval_amd.dataset import Dataset
    from blindshadowremoval_amd.fsrnet import Config
    with pytest.raises(ValueError, match="keep_photo"):
        Dataset(Config(0), "test", keep_photo=True)


def test_paste_record_is_the_kernels():
    from blindshadowremoval_amd import prep
    assert prep.PASTE_DTYPE.itemsize == 48
    assert [prep.PASTE_DTYPE.fields[k][1] for k in ("photo_off", "h", "w", "box", "preset_x", "preset_y", "row")] == [0, 8, 12, 16, 32, 36, 40]
