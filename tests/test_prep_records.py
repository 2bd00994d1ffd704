"""The records prep.py passes between the loaders' workers and the loop's thread (HostPart, UncroppedPart, RingPart) through the
pickle the workers' pipes use, and the blob of a batch of uncropped photographs (prep._layout_uncropped) as plain arithmetic: alignment,
no overlap, every record inside the blob.  CPU only, on the golden UCB / SFW / wild items of the neighbouring tests."""
import os
import pickle

import numpy as np
import pytest

import wild_cases as W
from blindshadowremoval_amd import prep
from tsm_group_cases import sfw_labels, ucb_items

SIZE = 256


@pytest.fixture(scope="module")
def records(tmp_path_factory, golden_dir):
    """One record of every kind, made once: name -> record."""
    from blindshadowremoval_amd.fsrnet import Config, _ucb_mask_files
    cfg = Config(0)
    cfg.DATA_DIR_TEST = [os.path.join(golden_dir, "UCB", "train", "input", "*")]
    cfg.UCB_MASK_ROOT = os.path.join(golden_dir, "UCB_masks")
    lm_path, gt = ucb_items()[4]
    masks = _ucb_mask_files(cfg)[4]
    cap = 3 * prep.RING_CAP // 2
    path = str(tmp_path_factory.mktemp("ring") / "ring")
    with open(path, "wb") as f:
        f.truncate(4 * cap)
    photo = os.path.join(W.WILD, "01001.png")
    return {
        "row": prep.host_part((lm_path, None, SIZE)),
        "row_masks": prep.host_part((lm_path, gt, SIZE, masks)),
        "row_raw": prep.host_part((lm_path, gt, SIZE, masks), raw=True),
        "group": prep.host_part_group((lm_path, gt, SIZE)),
        "sfw": prep.host_part_group((sfw_labels()[0], "<sfw>", SIZE)),
        "wild_raw": prep.host_part_uncropped((photo, SIZE)),
        "wild_decoded": prep.host_part_uncropped((photo, SIZE), raw=False),
        "ring": prep.host_part_ring((lm_path, gt, SIZE, masks), (path, 0, cap)),
        "ring_raw": prep.host_part_ring((lm_path, gt, SIZE, masks), (path, 1, cap, True)),
        "ring_group": prep.host_part_ring((lm_path, gt, SIZE), (path, 2, cap, True), group=True),
        "ring_overflow": prep.host_part_ring((lm_path, gt, SIZE, masks), (path, 3, 1 << 16, True)),
    }


KINDS = {"row": prep.HostPart, "row_masks": prep.HostPart, "row_raw": prep.HostPart, "group": prep.HostPart, "sfw": prep.HostPart,
         "wild_raw": prep.UncroppedPart, "wild_decoded": prep.UncroppedPart, "ring": prep.RingPart, "ring_raw": prep.RingPart,
         "ring_group": prep.RingPart, "ring_overflow": prep.HostPart}


def _same(a, b) -> bool:
    """Equal types and contents, through tuples, lists, arrays and pngio.RawScanlines."""
    if type(a) is not type(b):
        return False
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)
    if hasattr(a, "raw"):
        return (a.h, a.w, a.c) == (b.h, b.w, b.c) and _same(a.raw, b.raw)
    return a == b


@pytest.mark.parametrize("name", sorted(KINDS))
def test_record_survives_the_workers_pickle(records, name):
    rec = records[name]
    assert type(rec) is KINDS[name] and rec._fields == KINDS[name]._fields
    back = pickle.loads(pickle.dumps(rec, protocol=pickle.HIGHEST_PROTOCOL))
    assert _same(back, rec)
    assert not _same(back, rec._replace(name=b"another"))                     # (_same does look)
    if name.startswith("wild"):
        assert type(back.crop) is prep.CropGeometry and back.gt is None
    if isinstance(rec, prep.RingPart):
        assert prep._is_ring(back) and back.tag == "ring" and len(back.rawc) == 2
        assert back.masks is None if name == "ring_group" else type(back.masks) is prep.RingMasks
        assert len(pickle.dumps(rec, protocol=pickle.HIGHEST_PROTOCOL)) < 1000
    else:
        assert not prep._is_ring(back)


def test_the_records_are_what_their_names_say(records):
    r = records
    assert r["row"].gt is None and r["row"].masks is None and r["row"].label is None and len(r["row"].tabs) == 4
    assert r["row_masks"].masks[0] == "bits" and r["row_raw"].masks[0] == "raw8" and hasattr(r["row_raw"].img, "raw")
    assert len(r["group"].tabs) == 8 and r["group"].masks is None and r["group"].label is None
    assert r["sfw"].masks is None and r["sfw"].label.shape == r["sfw"].img.shape[:2]
    assert hasattr(r["wild_raw"].img, "raw") and isinstance(r["wild_decoded"].img, np.ndarray)
    assert r["ring"].rawc == (0, 0) and r["ring"].masks.kind == "bits" and r["ring_raw"].rawc == (3, 3) and r["ring_raw"].masks.kind == "raw8"
    assert len(r["ring_group"].tab_offs) == len(r["ring_group"].ntri) == 8
    over = r["ring_overflow"]                                                  # through the pipe after all: decoded, bit-packed
    assert _same(over, r["row_masks"])


def test_a_group_without_ground_truth_is_refused():
    with pytest.raises(ValueError, match="needs the ground truth"):
        prep.host_part_group((ucb_items()[4][0], None, SIZE))


def _spans_are_disjoint(spans) -> bool:
    spans = sorted(spans)
    return all(a1 <= b0 for (_, a1), (b0, _) in zip(spans, spans[1:]))


@pytest.mark.parametrize("keep_photo", [False, True])
@pytest.mark.parametrize("which", [("wild_raw",), ("wild_decoded",), ("wild_raw", "wild_decoded"), ("wild_decoded", "wild_raw", "wild_raw")])
def test_uncropped_blob_layout(records, which, keep_photo):
    parts = [records[k] for k in which]
    B, S3 = len(parts), SIZE * SIZE * 3
    lay = prep._layout_uncropped(parts, SIZE, keep_photo)
    assert type(lay) is prep.UncroppedLayout and len(lay) == 10
    n_tall = sum(k == "wild_raw" for k in which)
    assert lay.n_tall == n_tall and 0 < lay.head <= lay.total
    by_off = dict(lay.pieces)
    rows, crops = by_off[lay.rows_off], by_off[lay.crop_off]
    talls = by_off[lay.tall_off] if n_tall else np.zeros(0, prep.UNFILTER_TALL_DTYPE)
    assert (rows.dtype, crops.dtype, talls.dtype) == (prep.ROW_DTYPE, prep.CROP_DTYPE, prep.UNFILTER_TALL_DTYPE)
    assert (len(rows), len(crops), len(talls)) == (B, B, n_tall)
    offsets = [lay.total, lay.head, lay.rows_off, lay.grid_off, lay.crop_off, lay.tall_off] + [o for o, _ in lay.pieces]
    for name in ("img_off", "gt_off", "tri_off"):
        offsets += rows[name].reshape(-1).tolist()
    offsets += crops["src_off"].tolist() + crops["out_off"].tolist() + talls["raw_off"].tolist() + talls["out_off"].tolist()
    if keep_photo:
        assert lay.photo_offs == crops["src_off"].tolist()
        offsets += [lay.paste_off] + lay.photo_offs
    else:
        assert lay.paste_off is None and lay.photo_offs is None
    assert all(int(o) % 8 == 0 and o >= 0 for o in offsets)
    # the head: every piece the host stages, none on another, the tall table's room kept even when it is empty
    # (filtered scanlines with their slack: the tall kernel reads a few bytes around them)
    slack = {int(o): prep.UNFILTER_SLACK for o in talls["raw_off"]}
    staged = [(o - slack.get(o, 0), o + np.asarray(a).nbytes + slack.get(o, 0)) for o, a in lay.pieces]
    assert _spans_are_disjoint(staged + ([] if n_tall else [(lay.tall_off, lay.tall_off + prep.UNFILTER_TALL_DTYPE.itemsize)]))
    assert max(e for _, e in staged) <= lay.head
    # device only, behind the head: the reconstructed photographs, the crops, the paste records
    device = [(int(c["out_off"]), int(c["out_off"]) + S3) for c in crops]
    device += [(int(t["out_off"]), int(t["out_off"]) + int(t["h"]) * int(t["w"]) * 3 + prep.UNFILTER_SLACK) for t in talls]
    if keep_photo:
        device.append((lay.paste_off, lay.paste_off + B * prep.PASTE_DTYPE.itemsize))
    assert _spans_are_disjoint(device) and min(s for s, _ in device) >= lay.head and max(e for _, e in device) <= lay.total
    k = 0
    for i, (part, key) in enumerate(zip(parts, which)):
        r, c = rows[i], crops[i]
        h, w = part.img.shape[:2]
        assert (int(c["h"]), int(c["w"]), int(c["preset_x"]), int(c["preset_y"])) == (h, w, part.crop.preset_x, part.crop.preset_y)
        assert np.array_equal(c["box"], part.crop.box) and np.array_equal(r["box"], part.box) and (r["h"], r["w"]) == (SIZE, SIZE)
        assert r["img_off"] == r["gt_off"] == c["out_off"]                     # the crop's output is the row's image
        assert 0 <= c["src_off"] and c["src_off"] + h * w * 3 <= lay.total
        for m in range(4):
            o, n = int(r["tri_off"][m]), int(r["ntri"][m])
            assert n == part.tabs[m].shape[0] <= prep.MAX_TRI and o + n * prep.TRI_DOUBLES * 8 <= lay.head and by_off[o] is part.tabs[m]
        if key == "wild_raw":
            t = talls[k]
            k += 1
            n = part.img.h * (1 + part.img.w * part.img.c)
            assert (int(t["h"]), int(t["w"]), int(t["c"]), int(t["grey_out"])) == (part.img.h, part.img.w, part.img.c, 0)
            assert by_off[int(t["raw_off"])] is part.img.raw and part.img.raw.nbytes == n
            assert t["raw_off"] - prep.UNFILTER_SLACK >= lay.tall_off and t["raw_off"] + n + prep.UNFILTER_SLACK <= lay.head
            assert t["out_off"] == c["src_off"] >= lay.head                    # reconstructed on the device, cropped from there
            want = min(max(int(part.crop.box[3]) - part.crop.preset_y, 1), part.img.h)
            assert int(t["rows_needed"]) == (0 if keep_photo else want) and (keep_photo or 0 < want <= part.img.h)
        else:
            assert by_off[int(c["src_off"])] is part.img and c["src_off"] + h * w * 3 <= lay.head
