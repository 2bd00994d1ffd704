"""The device half of the way back for in-the-wild photographs (csrc/wild_paste_kernels.h): bsr_paste_faces against the host statement
wild_paste.paste_face, byte for byte, over the constructed cases of tests/wild_paste_cases.py; its refusals; and the whole route —
FSRNet.testFFHQ(paste_back=...) on tests/golden/wild/01001 — device against host."""
import os

import numpy as np
import pytest

import wild_cases as W
import wild_paste_cases as C

pytestmark = pytest.mark.gpu

ERR_ARG = 1          # include/bsr_hip.h BSR_ERR_ARG
GUARD = 16           # bytes of 0xA5 in front of and behind every photograph area
MODES = ("residual", "replace")


def paste_blob(cs):
    """-> (blob, records): [records | per case: guard, photograph, guard], everything that is no record or photograph 0xA5."""
    from blindshadowremoval_amd import prep
    tab = np.zeros(len(cs), prep.PASTE_DTYPE)
    off = (tab.nbytes + 7) & ~7
    for k, c in enumerate(cs):
        off += GUARD
        h, w = c["photo"].shape[:2]
        tab[k] = (off, h, w, c["box"], c["preset_x"], c["preset_y"], k, 0)
        off = (off + c["photo"].nbytes + GUARD + 7) & ~7
    blob = np.full(off, 0xA5, np.uint8)
    blob[:tab.nbytes] = tab.view(np.uint8)
    for k, c in enumerate(cs):
        blob[tab[k]["photo_off"]:tab[k]["photo_off"] + c["photo"].nbytes] = c["photo"].reshape(-1)
    return blob, tab


def planes(cs):
    """The cases' im | con | face as ONE packed [n,S,S,8] device tensor, im at channel 0, con at 3, face at 6: pixel strides of 8."""
    import torch
    p = np.full((len(cs), cs[0]["S"], cs[0]["S"], 8), np.nan, np.float32)
    for k, c in enumerate(cs):
        p[k, ..., 0:3], p[k, ..., 3:6], p[k, ..., 6:7] = c["im"], c["con"], c["face"]
    return torch.from_numpy(p).cuda()


def launch(d_blob, n, S, d_planes, mode, items_off=0, nbytes=None, null=None):
    import torch
    from blindshadowremoval_amd import _lib
    lib = _lib.load()
    ptr = [d_planes[..., 0:3].data_ptr(), d_planes[..., 3:6].data_ptr(), d_planes[..., 6:7].data_ptr()]
    blob_ptr = d_blob.data_ptr()
    if null == "blob":
        blob_ptr = None
    elif null is not None:
        ptr[null] = None
    rc = lib.bsr_paste_faces(0, blob_ptr, d_blob.numel() if nbytes is None else nbytes, items_off, n, S, ptr[0], 8, ptr[1], 8, ptr[2], 8, mode,
                             torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


@pytest.fixture(scope="module")
def host_results():
    """paste_face of every case in both modes, computed once."""
    from blindshadowremoval_amd.wild_paste import paste_face
    return {(c["name"], m): paste_face(c["photo"], c["box"], c["preset_x"], c["preset_y"], c["im"], c["con"], c["face"], m)
            for c in C.cases() for m in MODES}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("S", C.SIZES)
def test_paste_equals_the_host_statement(S, mode, host_results):
    """Every case of this S — both photograph sizes, every side and position — in ONE launch, and again on a fresh copy."""
    import torch
    from blindshadowremoval_amd import _lib
    cs = [c for c in C.cases() if c["S"] == S]
    assert len(cs) > 40 and len({c["photo"].shape for c in cs}) == 2
    blob, tab = paste_blob(cs)
    d_planes = planes(cs)
    runs = []
    for _ in range(2):
        d = torch.from_numpy(blob).cuda()
        _lib.check(launch(d, len(cs), S, d_planes, MODES.index(mode)), "bsr_paste_faces")
        runs.append(d.cpu().numpy())
    res = runs[0]
    assert np.array_equal(runs[0], runs[1]), "two launches on fresh copies differ"
    assert np.array_equal(res[:tab.nbytes], blob[:tab.nbytes]), "the records were written to"
    changed = 0
    for k, c in enumerate(cs):
        o, nb = int(tab[k]["photo_off"]), c["photo"].nbytes
        got = res[o:o + nb].reshape(c["photo"].shape)
        np.testing.assert_array_equal(got, host_results[(c["name"], mode)], err_msg="%s %s" % (c["name"], mode))
        assert (res[o - GUARD:o] == 0xA5).all() and (res[o + nb:o + nb + GUARD] == 0xA5).all(), "%s: guard bytes changed" % c["name"]
        changed += int(not np.array_equal(got, c["photo"]))
        if mode == "residual" and c["want"] is not None:
            x0, y0, x1, y1 = c["box"]
            np.testing.assert_array_equal(got[y0:y1, x0:x1], c["want"], err_msg=c["name"])
    assert changed > len(cs) // 2                                    # the kernel did write


def test_paste_refuses_bad_records_before_launching():
    import torch
    S = 32
    cs = [c for c in C.cases() if c["S"] == S and c["position"] == "inside" and c["face_kind"] == "ones"][:2]
    assert len(cs) == 2
    blob0, tab0 = paste_blob(cs)
    d_planes = planes(cs)

    def rc_of(change, **kw):
        tab = tab0.copy()
        change(tab)
        blob = blob0.copy()
        blob[:tab.nbytes] = tab.view(np.uint8)
        d = torch.from_numpy(blob).cuda()
        rc = launch(d, kw.pop("n", 2), kw.pop("S", S), d_planes, kw.pop("mode", 0), **kw)
        return rc, bool(np.array_equal(d.cpu().numpy()[tab.nbytes:], blob0[tab.nbytes:]))
    assert rc_of(lambda t: None) == (0, False)                               # the records as built are fine and the photographs are rewritten

    def put(k, field, value):
        def change(t):
            t[k][field] = value
        return change
    h, w = cs[1]["photo"].shape[:2]
    for change in [put(1, "photo_off", blob0.size - 100), put(0, "photo_off", blob0.size + 8), put(0, "photo_off", -8), put(1, "photo_off", 8),
                   put(0, "box", [5, 5, 5, 22]), put(0, "box", [9, 5, 5, 22]), put(1, "box", [3, 5, 4, 22]), put(1, "box", [3, 5, 20, 6]),
                   put(0, "box", [-1, 5, 16, 22]), put(1, "box", [3, 5, w + 1, 22]), put(1, "box", [3, h - 4, 20, h + 1]),
                   put(0, "h", -1), put(0, "h", 0), put(1, "w", 70000), put(1, "h", 6400), put(0, "preset_x", -1), put(1, "preset_y", (1 << 20) + 1),
                   put(0, "row", 2), put(1, "row", -1), put(1, "row", 1 << 30)]:
        assert rc_of(change) == (ERR_ARG, True)                              # refused, nothing written
    assert rc_of(lambda t: None, mode=7) == (ERR_ARG, True)
    assert rc_of(lambda t: None, mode=-1) == (ERR_ARG, True)
    assert rc_of(lambda t: None, S=48) == (ERR_ARG, True)
    assert rc_of(lambda t: None, n=0) == (ERR_ARG, True)
    assert rc_of(lambda t: None, items_off=4) == (ERR_ARG, True)             # unaligned table
    assert rc_of(lambda t: None, items_off=blob0.size - 8) == (ERR_ARG, True)
    assert rc_of(lambda t: None, nbytes=int(tab0[1]["photo_off"]) + 100) == (ERR_ARG, True)       # the second photograph leaves blob_bytes
    for null in ("blob", 0, 1, 2):
        assert rc_of(lambda t: None, null=null) == (ERR_ARG, True)
    from blindshadowremoval_amd import _lib
    assert b"bsr_paste_faces" in _lib.load().bsr_last_error()
    # a padded record's box is held to its canvas, (h + 2 preset_y + 2) x (w + 2 preset_x + 2)
    h0, w0 = cs[0]["photo"].shape[:2]
    assert rc_of(lambda t: (t[0].__setitem__("preset_x", 3), t[0].__setitem__("box", [w0 - 10, 0, w0 + 8, 18])))[0] == 0
    assert rc_of(lambda t: (t[0].__setitem__("preset_x", 3), t[0].__setitem__("box", [w0 - 9, 0, w0 + 9, 18]))) == (ERR_ARG, True)


# ---- the whole route on tests/golden/wild/01001 ----

def _run_loop(tmp, data, paste_back, device_prep=True, batch=2):
    """FSRNet.testFFHQ over `data` with synthetic weights -> (results, log.saved, log.pasted)"""
    from blindshadowremoval_amd.dataset import Dataset
    from blindshadowremoval_amd.fsrnet import Config, FSRNet
    from blindshadowremoval_amd.weights import init_weights
    cfg = Config(0)
    cfg.DATA_DIR_TEST = data
    cfg.CHECKPOINT_DIR = str(tmp)
    kw = dict(device_prep=0, device_batch=batch) if device_prep else {}
    ds = Dataset(cfg, "test", uncropped=True, keep_photo=paste_back is not None, **kw)
    fsr = FSRNet(cfg, weights=init_weights(1))
    try:
        res = fsr.testFFHQ(ds, batch=batch, **({"paste_back": paste_back} if paste_back else {}))
        res = [(r[0], [f.cpu().numpy() for f in r[1]]) for r in res]
    finally:
        ds.close()
        fsr.close()
    return res, list(fsr.log.saved), list(fsr.log.pasted)


def _face_of(data, device_prep=True):
    """channel 15 of every element's row (the blurred face hull the paste multiplies by), from a loader of its own"""
    from blindshadowremoval_amd.dataset import Dataset
    from blindshadowremoval_amd.fsrnet import Config
    cfg = Config(0)
    cfg.DATA_DIR_TEST = data
    ds = Dataset(cfg, "test", uncropped=True, **(dict(device_prep=0, device_batch=2) if device_prep else {}))
    try:
        return [np.asarray(e[0].cpu() if hasattr(e[0], "cpu") else e[0]).reshape(256, 256, 16)[..., 15:16].copy() for e in ds.feed]
    finally:
        ds.close()


def _host_paste(png, figs, face, mode):
    from blindshadowremoval_amd.pngio import read_rgb_u8
    from blindshadowremoval_amd.wild_crop import crop_geometry
    from blindshadowremoval_amd.wild_paste import paste_face
    photo = read_rgb_u8(png)
    box, px, py, _ = crop_geometry(np.load(os.path.splitext(png)[0] + ".npy"), photo.shape[0], photo.shape[1])
    return photo, paste_face(photo, box, px, py, figs[0][0], figs[1][0], face, mode)


@pytest.fixture(scope="module")
def routes(tmp_path_factory):
    src = [os.path.join(W.WILD, "*.png")]
    tmp = tmp_path_factory.mktemp("paste")
    return {"src": src, "dev": _run_loop(tmp / "dev", src, "residual"), "plain": _run_loop(tmp / "plain", src, None),
            "host": _run_loop(tmp / "host", src, "residual", device_prep=False)}


def test_testFFHQ_pastes_the_face_back_on_the_device(routes):
    """The -pasted.png of the device route decodes to paste_face of that item's own im / con_rgb / face, fetched from the same forward."""
    from blindshadowremoval_amd.pngio import read_rgb_u8
    res, saved, pasted = routes["dev"]
    assert len(res) == 1 and len(pasted) == 1 and pasted[0].endswith("-pasted.png") and os.path.dirname(pasted[0]) == os.path.dirname(saved[0])
    face = _face_of(routes["src"])[0]
    photo, want = _host_paste(os.path.join(W.WILD, "01001.png"), res[0][1], face, "residual")
    got = read_rgb_u8(pasted[0])
    assert got.shape == photo.shape == (840, 840, 3)
    diff = got != want
    print("device file vs paste_face of the same forward: %d of %d bytes differ" % (diff.sum(), diff.size))
    assert not diff.any()
    assert (got != photo).any()                                             # synthetic weights: the face region did change


def test_the_strip_is_the_one_written_without_paste_back(routes):
    (_, saved, _), (_, plain, pasted) = routes["dev"], routes["plain"]
    assert pasted == [] and len(saved) == len(plain) == 1 and os.path.basename(saved[0]) == os.path.basename(plain[0])
    with open(saved[0], "rb") as a, open(plain[0], "rb") as b:
        assert a.read() == b.read()


def test_host_and_device_routes_decode_to_the_same_pixels(routes):
    from blindshadowremoval_amd.pngio import read_rgb_u8
    a, b = read_rgb_u8(routes["dev"][2][0]), read_rgb_u8(routes["host"][2][0])
    diff = a != b
    print("device route vs --host-prep route: %d of %d bytes differ, largest step %d" % (diff.sum(), diff.size, np.abs(a.astype(int) - b).max()))
    assert a.shape == b.shape and not diff.any()


def test_the_host_route_is_paste_face_of_its_own_forward(routes):
    from blindshadowremoval_amd.pngio import read_rgb_u8
    res, _, pasted = routes["host"]
    face = _face_of(routes["src"], device_prep=False)[0]
    _, want = _host_paste(os.path.join(W.WILD, "01001.png"), res[0][1], face, "residual")
    assert np.array_equal(read_rgb_u8(pasted[0]), want)


def test_a_batch_of_two_photograph_sizes(tmp_path):
    """The fixture and a trimmed copy of it — its box then leaves the photograph on the left and at the top — in one batch, mode replace."""
    from blindshadowremoval_amd.pngio import read_rgb_u8, write_png
    from blindshadowremoval_amd.wild_crop import crop_geometry
    photo = read_rgb_u8(os.path.join(W.WILD, "01001.png"))
    lm = np.load(os.path.join(W.WILD, "01001.npy"))
    box, px, py, _ = crop_geometry(lm, photo.shape[0], photo.shape[1])
    assert px == 0 and py == 0
    tx, ty = box[0] + 9, box[1] + 14                                         # the trimmed photograph starts inside the box
    folder = tmp_path / "photos"
    os.makedirs(str(folder))
    write_png(str(folder / "a.png"), photo)
    np.save(str(folder / "a.npy"), lm)
    small = np.ascontiguousarray(photo[ty:, tx:])
    write_png(str(folder / "b.png"), small)
    np.save(str(folder / "b.npy"), (lm - np.array([tx, ty], lm.dtype)).astype(lm.dtype))
    geo = crop_geometry(np.load(str(folder / "b.npy")), small.shape[0], small.shape[1])
    assert geo is not None and geo[1] > 0 and geo[2] > 0 and small.shape != photo.shape
    data = [str(folder / "*.png")]
    res, saved, pasted = _run_loop(tmp_path / "run", data, "replace")
    assert len(res) == 2 and len(pasted) == 2 and len(set(pasted)) == 2
    faces = _face_of(data)
    for k, name in enumerate(("a", "b")):
        assert os.path.basename(pasted[k]) == "photos_%s-pasted.png" % name
        src, want = _host_paste(str(folder / (name + ".png")), res[k][1], faces[k], "replace")
        got = read_rgb_u8(pasted[k])
        assert got.shape == src.shape
        np.testing.assert_array_equal(got, want, err_msg=name)
        assert (got != src).any()
