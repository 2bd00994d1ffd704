"""The device half of the in-the-wild route (csrc/wild_crop_kernels.h): bsr_png_unfilter_tall against the host reconstruction,
bsr_crop_faces against wild_crop.crop_pixels — both bit for bit, it is integer and unfused float64 arithmetic — and the whole route on
tests/golden/wild/01001 against the folder the host statement writes.  Bad records are refused before anything is launched."""
import os

import numpy as np
import pytest

import wild_cases as C
from unfilter_cases import filter_rows

pytestmark = pytest.mark.gpu

ERR_ARG = 1          # include/bsr_hip.h BSR_ERR_ARG


def run_tall(items, fill=0xA5):
    """items: [(raw uint8 [h, 1 + w c], h, w, c, grey_out, rows_needed)] -> what the kernel left in each output area, [h,w,3 | 1], in ONE
    launch.  The blob keeps 16 bytes around every filtered image and behind every output area; untouched bytes keep `fill`."""
    import torch
    from blindshadowremoval_amd import _lib, prep
    lib = _lib.load()
    tab = np.zeros(len(items), prep.UNFILTER_TALL_DTYPE)
    off = ((tab.nbytes + 7) & ~7) + 16
    for k, (raw, h, w, c, grey, need) in enumerate(items):
        assert raw.size == h * (1 + w * c) and 1 <= h <= 65535 and w * c >= 4 and c in (1, 3, 4) and (c == 1 or not grey)
        tab[k] = (off, 0, h, w, c, 1 if grey else 0, need, 0)
        off = ((off + raw.size + 7) & ~7) + 16
    for k, (raw, h, w, c, grey, need) in enumerate(items):
        tab[k]["out_off"] = off
        off = ((off + h * w * (1 if grey else 3) + 7) & ~7) + 16
    blob = np.full(off, fill, np.uint8)
    blob[:tab.nbytes] = tab.view(np.uint8)
    for k, (raw, h, w, c, grey, need) in enumerate(items):
        blob[tab[k]["raw_off"]:tab[k]["raw_off"] + raw.size] = raw.reshape(-1)
    d = torch.from_numpy(blob).cuda()
    _lib.check(lib.bsr_png_unfilter_tall(0, d.data_ptr(), d.numel(), 0, len(items), torch.cuda.current_stream().cuda_stream), "bsr_png_unfilter_tall")
    torch.cuda.synchronize()
    res = d.cpu().numpy()
    return [res[t["out_off"]:t["out_off"] + t["h"] * t["w"] * (1 if t["grey_out"] else 3)].reshape(t["h"], t["w"], -1) for t in tab]


def _want(img, grey):
    c = img.shape[2]
    return img if (c == 3 or grey) else (np.repeat(img, 3, axis=2) if c == 1 else img[:, :, :3])


# (w, c, grey_out): scanlines of 4, 5, 12 and 96 bytes with 1, 3 and 4 channels, grey output on and off
GEOMETRIES = [(4, 1, False), (4, 1, True), (1, 4, False), (5, 1, False), (5, 1, True), (4, 3, False), (3, 4, False), (12, 1, True),
              (32, 3, False), (24, 4, False), (96, 1, False)]
_HOST_CHECKED = set()


def _image(rng, h, w, c):
    img = rng.randint(0, 256, (h, w, c)).astype(np.uint8)
    img[h // 3:h // 2] = img[h // 3]                            # flat stretches: ties in the Paeth predictor
    return img


@pytest.mark.parametrize("h", [1, 255, 256, 257, 300, 512, 513, 1024])
def test_tall_reconstruction_equals_the_host(h):
    """Every geometry at this height in one launch, each row's filter type drawn from 0-4."""
    from blindshadowremoval_amd.wild_crop import unfilter_tall_host
    rng = np.random.RandomState(1000 + h)
    items, want = [], []
    for w, c, grey in GEOMETRIES:
        img = _image(rng, h, w, c)
        raw = filter_rows(img, rng.randint(0, 5, h))
        np.testing.assert_array_equal(unfilter_tall_host(raw, h, w, c), img)          # the host reconstruction is the reference
        items.append((raw, h, w, c, grey, 0))
        want.append(_want(img, grey))
    for (w, c, grey), o, wv in zip(GEOMETRIES, run_tall(items), want):
        np.testing.assert_array_equal(o, wv, err_msg="h=%d w=%d c=%d grey=%d" % (h, w, c, grey))


def test_one_filter_type_across_the_band_seams_and_mixed_sizes_in_one_launch():
    """All-Paeth, all-Up and all-Average files of three and five bands, next to short and odd ones, in one launch."""
    rng = np.random.RandomState(77)
    items, want = [], []
    for h, w, c, grey, ft in [(600, 32, 3, False, 4), (600, 32, 3, False, 2), (1100, 5, 1, True, 4), (1100, 24, 4, False, 2), (513, 4, 3, False, 3),
                              (7, 96, 1, False, None), (257, 33, 3, False, None), (1, 4, 1, False, 1), (300, 129, 1, False, None)]:
        img = _image(rng, h, w, c)
        items.append((filter_rows(img, np.full(h, ft) if ft is not None else rng.randint(0, 5, h)), h, w, c, grey, 0))
        want.append(_want(img, grey))
    for k, (o, wv) in enumerate(zip(run_tall(items), want)):
        np.testing.assert_array_equal(o, wv, err_msg="item %d" % k)


def test_rows_needed_stops_the_walk():
    """rows_needed of 1, 256, 257 and h: the rows above it are the image's, the rows below it are never written."""
    rng = np.random.RandomState(5)
    h, w, c = 300, 32, 3
    img = _image(rng, h, w, c)
    raw = filter_rows(img, rng.randint(0, 5, h))
    needs = [1, 256, 257, h]
    for need, o in zip(needs, run_tall([(raw, h, w, c, False, n) for n in needs])):
        np.testing.assert_array_equal(o[:need], img[:need], err_msg="rows_needed=%d" % need)
        assert (o[need:] == 0xA5).all(), "rows_needed=%d: a row below it was written" % need


def test_tall_refuses_bad_records_before_launching():
    import torch
    from blindshadowremoval_amd import _lib, prep
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    n = 4096
    # (a sound record here: 8 x 25 scanlines at 64, the 8 x 8 x 3 output at 2048)
    for rec in [(8, 2048, 8, 8, 3, 0, 0, 0),                                             # no 16 bytes in front of the scanlines
                (n - 100, 2048, 8, 8, 3, 0, 0, 0),                                       # scanlines leave the blob
                (64, n - 100, 8, 8, 3, 0, 0, 0),                                         # output leaves the blob
                (64, -8, 8, 8, 3, 0, 0, 0), (64, 2048, 0, 8, 3, 0, 0, 0), (64, 2048, 8, 1, 3, 0, 0, 0), (64, 2048, 8, 8, 2, 0, 0, 0),
                (64, 2048, 8, 8, 3, 1, 0, 0), (64, 2048, 8, 8, 3, 0, -1, 0), (64, 2048, 70000, 8, 3, 0, 0, 0)]:
        blob = np.full(n, 0xA5, np.uint8)
        tab = np.zeros(1, prep.UNFILTER_TALL_DTYPE)
        tab[0] = rec
        blob[:40] = tab.view(np.uint8)
        d = torch.from_numpy(blob).cuda()
        assert lib.bsr_png_unfilter_tall(0, d.data_ptr(), n, 0, 1, stream) == ERR_ARG, rec
        torch.cuda.synchronize()
        assert (d.cpu().numpy()[40:] == 0xA5).all(), rec                                 # nothing ran
    d = torch.zeros(n, dtype=torch.uint8, device="cuda")
    assert lib.bsr_png_unfilter_tall(0, d.data_ptr(), n, 4, 1, stream) == ERR_ARG        # unaligned table
    assert lib.bsr_png_unfilter_tall(0, d.data_ptr(), n, n - 8, 1, stream) == ERR_ARG    # the table leaves the blob
    assert lib.bsr_png_unfilter_tall(0, None, n, 0, 1, stream) == ERR_ARG


# ---- bsr_crop_faces ----

def canvas_box(box, h, w):
    """dataprocess.py:49-62 for a box in photograph coordinates: -> (box in canvas coordinates, preset_x, preset_y)."""
    px = max(-box[0], box[2] - w) if (box[0] < 0 or box[2] > w) else 0
    py = max(-box[1], box[3] - h) if (box[1] < 0 or box[3] > h) else 0
    return [box[0] + px, box[1] + py, box[2] + px, box[3] + py], px, py


def crop_blob(items, S):
    """items: [(img uint8 [h,w,3], canvas box, preset_x, preset_y)] -> (blob, records) with the crops' areas filled with 0xA5."""
    from blindshadowremoval_amd import prep
    tab = np.zeros(len(items), prep.CROP_DTYPE)
    off = (tab.nbytes + 7) & ~7
    for k, (img, box, px, py) in enumerate(items):
        tab[k] = (off, 0, img.shape[0], img.shape[1], box, px, py)
        off = (off + img.nbytes + 7) & ~7
    for k in range(len(items)):
        tab[k]["out_off"] = off
        off += S * S * 3
    blob = np.full(off, 0xA5, np.uint8)
    for k, (img, _, _, _) in enumerate(items):
        blob[tab[k]["src_off"]:tab[k]["src_off"] + img.nbytes] = img.reshape(-1)
    return blob, tab


def run_crop(items, S):
    import torch
    from blindshadowremoval_amd import _lib
    lib = _lib.load()
    blob, tab = crop_blob(items, S)
    blob[:tab.nbytes] = tab.view(np.uint8)
    d = torch.from_numpy(blob).cuda()
    _lib.check(lib.bsr_crop_faces(0, d.data_ptr(), d.numel(), 0, len(items), S, torch.cuda.current_stream().cuda_stream), "bsr_crop_faces")
    torch.cuda.synchronize()
    res = d.cpu().numpy()
    return [res[t["out_off"]:t["out_off"] + S * S * 3].reshape(S, S, 3) for t in tab]


def _crop_items():
    big, small, other = C.noise(600, 560, 11), C.noise(300, 280, 12), C.noise(300, 280, 13)
    items = [(big, [40, 30, 540, 530], 0, 0),                            # inside
             (big, [60, 100, 560, 600], 0, 0),                           # right and bottom edges ARE w and h: no padding
             (big, [33, 21, 290, 277], 0, 0)]                            # 257 pixels to 256: weights near 0 and 1
    for box in ([-30, 20, 230, 280], [10, -25, 270, 235], [40, 20, 300, 280], [10, 60, 270, 320], [-30, -25, 230, 235], [40, 60, 300, 320],
                [-100, -120, 380, 360]):                                 # left, top, right, bottom, left + top, right + bottom, all four
        items.append((small if len(items) % 2 else other,) + tuple(canvas_box(box, 300, 280)))
    return items


@pytest.mark.parametrize("S", [32, 256])
def test_crop_equals_the_host_statement(S):
    """Every case in ONE launch: three sizes of photograph, both branches."""
    from blindshadowremoval_amd.wild_crop import crop_pixels
    items = _crop_items()
    assert sum(1 for it in items if it[2] or it[3]) == 7 and sum(1 for it in items if it[2] and it[3]) == 3
    for k, (o, (img, box, px, py)) in enumerate(zip(run_crop(items, S), items)):
        np.testing.assert_array_equal(o, crop_pixels(img, box, px, py, S), err_msg="item %d box %s presets %d %d" % (k, box, px, py))


def test_crop_of_the_fixture_cases_equals_the_reference_script():
    """The records crop_geometry makes for the fixture's cases: the kernel writes the bytes the reference's script wrote."""
    from blindshadowremoval_amd.wild_crop import crop_geometry
    fx = np.load(C.FIXTURE)
    names = [n for n in sorted(C.CASES) if int(fx[n + "_kept"])]
    items = []
    for n in names:
        img, lm = C.case_inputs(n)
        box, px, py, _ = crop_geometry(lm, img.shape[0], img.shape[1])
        items.append((img, box, px, py))
    for n, o in zip(names, run_crop(items, 256)):
        np.testing.assert_array_equal(o, fx[n + "_crop"], err_msg=n)


def test_crop_refuses_bad_records_before_launching():
    import torch
    from blindshadowremoval_amd import _lib
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    img = C.noise(64, 48, 1)
    blob0, tab0 = crop_blob([(img, [4, 4, 44, 44], 0, 0)], 32)

    def rc_of(change, S=32, nbytes=None):
        tab = tab0.copy()
        change(tab[0])
        blob = blob0.copy()
        blob[:tab.nbytes] = tab.view(np.uint8)
        d = torch.from_numpy(blob).cuda()
        rc = lib.bsr_crop_faces(0, d.data_ptr(), d.numel() if nbytes is None else nbytes, 0, 1, S, stream)
        torch.cuda.synchronize()
        out = d.cpu().numpy()[int(tab0[0]["out_off"]):]
        return rc, bool((out == 0xA5).all())
    assert rc_of(lambda t: None) == (0, False)                               # the record as built is fine and the crop is written

    def put(field, value):
        def change(t):
            t[field] = value
        return change
    for change in [put("src_off", blob0.size - 100), put("src_off", -8), put("out_off", blob0.size - 8), put("out_off", -1),
                   put("h", 6400), put("w", 4800), put("h", 0), put("box", [4, 4, 49, 44]), put("box", [4, 4, 44, 65]), put("box", [-1, 4, 39, 44]),
                   put("box", [10, 4, 10, 44]), put("preset_x", -1)]:
        assert rc_of(change) == (ERR_ARG, True)                              # refused, nothing written
    # a padded record's box is held to the canvas, h + 2 preset_y + 2 by w + 2 preset_x + 2
    assert rc_of(lambda t: (t.__setitem__("preset_x", 3), t.__setitem__("box", [0, 0, 56, 64])))[0] == 0
    assert rc_of(lambda t: (t.__setitem__("preset_x", 3), t.__setitem__("box", [0, 0, 57, 64]))) == (ERR_ARG, True)
    assert rc_of(lambda t: None, S=48) == (ERR_ARG, True)
    assert rc_of(lambda t: None, nbytes=int(tab0[0]["out_off"]) + 100) == (ERR_ARG, True)      # the crop's area leaves blob_bytes


# ---- the whole route on tests/golden/wild/01001 ----

@pytest.fixture(scope="module")
def wild_folder(tmp_path_factory):
    """(glob of the uncropped photographs, glob of the item folders preprocess_folder wrote for them)"""
    from blindshadowremoval_amd.wild_crop import preprocess_folder
    dst = tmp_path_factory.mktemp("wild_cropped")
    src = os.path.join(C.WILD, "*.png")
    assert preprocess_folder(src, str(dst)) == ["01001"]
    return src, os.path.join(str(dst), "*")


@pytest.mark.parametrize("workers", [0, 1])
def test_device_route_equals_the_existing_route_on_the_written_folder(wild_folder, workers):
    """Dataset(uncropped=True, device_prep=0) — inflated scanlines in, bsr_png_unfilter_tall, bsr_crop_faces, bsr_prep_rows — against the
    existing device route over the folder the host statement wrote: the same element, bit for bit.  workers=1: through a worker's pipe."""
    import torch
    from blindshadowremoval_amd.dataset import Dataset
    from blindshadowremoval_amd.fsrnet import Config
    src, folders = wild_folder
    cfg = Config(0)
    cfg.DATA_DIR_TEST = [folders]
    ds = Dataset(cfg, "test", device_prep=0)
    a = next(ds.feed)
    cfg2 = Config(0)
    cfg2.DATA_DIR_TEST = [src, src]
    wild = Dataset(cfg2, "test", uncropped=True, device_prep=0, workers=workers)
    assert len(wild.name_list) == 2
    try:
        got = list(wild.feed)
    finally:
        wild.close()
        ds.close()
    assert len(got) == 2
    for b in got:
        assert b[0].is_cuda and tuple(b[0].shape) == tuple(a[0].shape) == (1, 1, 256, 256, 16)
        assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))
        assert a[1].tobytes() == b[1].tobytes()


def test_testFFHQ_writes_the_same_png_for_the_uncropped_item(wild_folder, tmp_path):
    from blindshadowremoval_amd.dataset import Dataset
    from blindshadowremoval_amd.fsrnet import Config, FSRNet
    from blindshadowremoval_amd.weights import init_weights
    src, folders = wild_folder
    w = init_weights(1)
    files = []
    for k, (data, kw) in enumerate((([folders, folders], {}), ([src, src], dict(uncropped=True)))):
        cfg = Config(0)
        cfg.DATA_DIR_TEST = data
        cfg.CHECKPOINT_DIR = str(tmp_path / ("run%d" % k))
        ds = Dataset(cfg, "test", device_prep=0, device_batch=2, **kw)
        assert len(ds.name_list) == 2
        fsr = FSRNet(cfg, weights=w)
        fsr.return_figs = False
        try:
            res = fsr.testFFHQ(ds, batch=2)
        finally:
            ds.close()
            fsr.close()
        assert len(res) == 2
        saved = sorted(set(fsr.log.saved))
        assert len(saved) == 1 and os.path.isfile(saved[0])            # the item twice: one name, written twice with the same bytes
        with open(saved[0], "rb") as f:
            files.append(f.read())
    assert len(files[0]) > 256 * 256 * 3 and files[0] == files[1]
