"""The host half of the device-prepared TSM groups (prep.host_part_group, the group records of prep._layout_ex) and the
Dataset(device_groups=...) keyword, without a GPU: landmarks, mirror landmarks and box against face_crop_and_resize(with_mirror=True)
bit for bit, the tables of row 0 against prep.meshes, the blob's layout, and a numpy statement of the group kernel against the host
pair builders."""
import os

import numpy as np
import pytest

from blindshadowremoval_amd import dataset as D
from blindshadowremoval_amd import prep
from prep_cases import emulate
from tsm_group_cases import make_edges, sfw_labels, ucb_items


class _Cfg:
    IMG_SIZE = 256

    def __init__(self, data):
        self.DATA_DIR_TEST = data


def test_device_groups_keyword_and_its_refusals(golden_dir):
    ucb = _Cfg([os.path.join(golden_dir, "UCB", "train", "input", "*")])
    sfw = _Cfg([os.path.join(golden_dir, "sfw_synth", "*")])
    ds = D.Dataset(ucb, "test", dset="ucb_tsm", ucb=True, device_groups=0)
    assert ds.device_groups == 0 and ds.device_prep is None and len(ds.name_list) == 100
    assert D.Dataset(sfw, "test", dset="sfw", device_groups=0).device_groups == 0
    assert D.Dataset(ucb, "test", dset="ucb_tsm", ucb=True).device_groups is None          # the host path stays the default
    with pytest.raises(NotImplementedError, match="device_prep"):
        D.Dataset(ucb, "test", ucb=True, device_groups=0)                                  # the GSC rows are device_prep's
    with pytest.raises(NotImplementedError, match="sfw_gsc"):
        D.Dataset(sfw, "test", dset="sfw_gsc", device_groups=0)
    with pytest.raises(NotImplementedError, match="sfw_video"):
        D.Dataset(sfw, "test", dset="sfw_video", device_groups=0)
    for dset in ("ucb_tsm", "sfw"):                                                        # device_prep is not widened
        with pytest.raises(NotImplementedError, match="device_prep prepares row 0"):
            D.Dataset(ucb, "test", dset=dset, ucb=dset == "ucb_tsm", device_prep=0)
    with pytest.raises(ValueError):
        prep.DevicePrep.__init__(object.__new__(prep.DevicePrep), 0, 256, planes=5)


def test_sfw_groups_are_refused_a_ring_record(tmp_path):
    """A ring record carries no label plane (its aux_off points at the photograph): DevicePrep(planes=7) refuses one before any device work."""
    lm_path, gt = ucb_items()[2]
    cap = 3 * prep.RING_CAP // 2
    path = str(tmp_path / "ring")
    with open(path, "wb") as f:
        f.truncate(cap)
    rec = prep.host_part_ring((lm_path, gt, 256), (path, 0, cap, False), group=True)

    class _Ring:
        pass
    dp = object.__new__(prep.DevicePrep)
    dp._torch, dp.device, dp.size, dp.planes, dp.ring = None, 0, 256, 7, _Ring()
    dp.ring.cap = cap
    with pytest.raises(ValueError, match="planes=7"):
        dp.rows_ex([rec])


def test_jobs_of_a_device_groups_dataset(golden_dir):
    ucb = _Cfg([os.path.join(golden_dir, "UCB", "train", "input", "*")])
    ds = D.Dataset(ucb, "test", dset="ucb_tsm", ucb=True, device_groups=0)
    ds.ucb_mask_files = [{"face_hair": "m%d" % i} for i in range(100)]
    jobs = list(ds._jobs())
    lm_path, gt = ucb_items()[3]
    assert jobs[3] == (lm_path, ("<device_group>", gt, {"face_hair": "m3"}), [], 256)
    ds = D.Dataset(_Cfg([os.path.join(golden_dir, "sfw_synth", "*")]), "test", dset="sfw", device_groups=0)
    assert [j[1] for j in ds._jobs()] == [("<device_group>", "<sfw>")] * 2


@pytest.mark.parametrize("k", [0, 37, 99])
def test_host_part_group_is_face_crop_and_resize_with_mirror(k):
    lm_path, gt = ucb_items()[k]
    img = D.imread_rgb(os.path.splitext(lm_path)[0] + ".png")
    _, lm, lm_m, box = D.face_crop_and_resize(img, np.load(lm_path), 256, with_mirror=True)
    b, l, m = prep.crop_box_pair(np.load(lm_path), img.shape[1])
    assert b == box and l.dtype == lm.dtype == np.float32 and m.dtype == np.float32
    assert np.array_equal(l, lm) and np.array_equal(m, lm_m)
    part = prep.host_part_group((lm_path, gt, 256))
    assert np.array_equal(part[2], np.asarray(box, np.int32)) and part[4] == gt.encode() and len(part[3]) == 8
    for got, want in zip(part[3], prep.meshes(lm) + prep.meshes(lm_m)):
        assert got.dtype == np.float64 and np.array_equal(got, want)
    row = prep.host_part((lm_path, gt, 256))                     # row 0 of the group is the GSC row of the item
    assert np.array_equal(part[0], row[0]) and np.array_equal(part[1], row[1]) and np.array_equal(part[2], row[2])
    assert all(np.array_equal(a, b) for a, b in zip(part[3][:4], row[3]))


def test_group_blob_layout_round_trips():
    ucb = prep.host_part_group(ucb_items()[5] + (256,))
    sfw = prep.host_part_group((sfw_labels()[0], "<sfw>", 256))
    assert len(sfw) == 7 and sfw[5] is None and sfw[6].dtype == np.uint8 and sfw[6].shape == sfw[0].shape[:2]
    for parts in ([ucb, ucb], [sfw, sfw]):
        blob, goff, grid_off = prep.pack_group_batch(parts, 256)
        recs = np.frombuffer(blob, prep.GROUP_DTYPE, count=2, offset=goff)
        assert goff % 8 == 0 and grid_off % 8 == 0
        assert np.array_equal(np.frombuffer(blob, "<f8", count=256, offset=grid_off), np.linspace(0, 1, 256))
        r, part = recs[1], parts[1]
        h, w = int(r["h"]), int(r["w"])
        assert (h, w) == part[0].shape[:2] and np.array_equal(r["box"], part[2])
        for off, a in ((r["img_off"], part[0]), (r["gt_off"], part[1])):
            assert int(off) % 8 == 0 and np.array_equal(np.frombuffer(blob, np.uint8, count=h * w * 3, offset=int(off)).reshape(h, w, 3), a)
        if part[6] is not None:
            assert np.array_equal(np.frombuffer(blob, np.uint8, count=h * w, offset=int(r["aux_off"])).reshape(h, w), part[6])
        for m in range(8):
            t = np.frombuffer(blob, "<f8", count=int(r["ntri"][m]) * prep.TRI_DOUBLES, offset=int(r["tri_off"][m])).reshape(-1, prep.TRI_DOUBLES)
            assert int(r["tri_off"][m]) % 8 == 0 and np.array_equal(t, part[3][m])
    with pytest.raises(ValueError, match="triangle tables"):
        prep.pack_group_batch([prep.host_part(ucb_items()[5] + (256,))], 256)             # a row's part in a group blob


def _emulate_group(part, size):
    """numpy statement of csrc/prep_group_kernels.h for one group, on prep_cases.emulate (the row kernel's statement)."""
    img, gt, box, tabs = part[:4]
    r0 = emulate((img, gt, box, tabs[:4], b""), size)
    r1 = emulate((img, gt, box, tabs[4:], b""), size)
    planes = [r0[..., :6]]
    if part[6] is not None:                                      # the label plane: the zero-extended crop of its grey levels (not / 255), resized
        n = int(box[2] - box[0])
        c = np.zeros((n, n, 1), np.float64)
        ys, xs = np.arange(n) + box[1], np.arange(n) + box[0]
        oky, okx = (ys >= 0) & (ys < part[6].shape[0]), (xs >= 0) & (xs < part[6].shape[1])
        c[np.ix_(oky, okx)] = part[6][np.ix_(ys[oky], xs[okx])].astype(np.float64)[:, :, None]
        planes.append(D.resize_linear(c, size))
    crop = np.concatenate(planes, axis=2)
    return np.stack([np.concatenate([crop, r0[..., 6:]], axis=2), np.concatenate([crop[:, ::-1], r1[..., 6:]], axis=2)]).astype(np.float32)


def test_group_arithmetic_reproduces_the_host_pairs(tmp_path):
    lm_path, gt = ucb_items()[11]
    want = D.build_ucb_tsm_pair(lm_path, gt, 256)[0][0]
    got = _emulate_group(prep.host_part_group((lm_path, gt, 256)), 256)
    assert got.shape == want.shape == (2, 256, 256, 16)
    err = np.abs(got - want).max(axis=(1, 2))
    assert err.max() <= 1e-6, err
    for label in sfw_labels():                                   # the 17-channel layout
        want = D.build_sfw_pair(label, 256)[0][0]
        got = _emulate_group(prep.host_part_group((label, "<sfw>", 256)), 256)
        assert got.shape == want.shape == (2, 256, 256, 17) and want[0, :, :, 6].max() > 1.0
        err = np.abs(got - want).max(axis=(1, 2))
        assert err.max() <= 1e-6, (label, err)
    edges = make_edges(str(tmp_path))
    for name in ("leaves", "empty"):
        part = prep.host_part_group(edges[name] + (256,))
        want = D.build_ucb_tsm_pair(*edges[name], 256)[0][0]
        box = part[2]
        if name == "leaves":
            assert box[2] > part[0].shape[1] and box[3] > part[0].shape[0]
        else:                                                   # (emulate's resize has no statement for a crop without pixels: the kernel is
            assert box[2] == box[0] and box[3] == box[1] and not want[..., :6].any()      # held to this item in test_prep_groups_gpu.py)
            continue
        err = np.abs(_emulate_group(part, 256) - want).max(axis=(1, 2))
        assert err.max() <= 1e-6, (name, err)


def test_ring_record_of_a_group_round_trips(tmp_path):
    """host_part_ring(group=True) writes the eight tables into the slot, and _layout_ex turns the record into a group record that points at them."""
    lm_path, gt = ucb_items()[2]
    cap = 3 * prep.RING_CAP // 2
    path = str(tmp_path / "ring")
    with open(path, "wb") as f:
        f.truncate(2 * cap)
    rec = prep.host_part_ring((lm_path, gt, 256), (path, 1, cap, False), group=True)
    part = prep.host_part_group((lm_path, gt, 256))
    assert rec[0] == "ring" and rec[1] == 1 and len(rec[5]) == 8 and rec[6] == tuple(t.shape[0] for t in part[3])
    total, goff, _, pieces, head, cells, _ = prep._layout_ex([rec], 256, cap, group=True)
    assert cells == [(0, 1, head)] and total == head + cap
    blob = np.zeros(total, np.uint8)
    prep.pack_into(blob, pieces)
    blob[head:head + cap] = np.fromfile(path, np.uint8)[cap:2 * cap]
    r = np.frombuffer(blob.tobytes(), prep.GROUP_DTYPE, count=1, offset=goff)[0]
    h, w = int(r["h"]), int(r["w"])
    assert np.array_equal(blob[int(r["img_off"]):int(r["img_off"]) + h * w * 3].reshape(h, w, 3), part[0])
    assert np.array_equal(blob[int(r["gt_off"]):int(r["gt_off"]) + h * w * 3].reshape(h, w, 3), part[1])
    for m in range(8):
        o = int(r["tri_off"][m])
        assert np.array_equal(blob[o:o + part[3][m].nbytes].view("<f8").reshape(-1, prep.TRI_DOUBLES), part[3][m])
