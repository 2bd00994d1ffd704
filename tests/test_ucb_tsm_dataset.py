"""Dataset(dset='ucb_tsm', ucb=True) — the TSM script's UCB loader (parse_fn_test, dataset_with_TSM.py:153-189) — against what the
reference's own parser makes of two golden UCB items (tests/golden/ucb_tsm_elements.npz, tools/make_ucb_tsm_elements_fixture.py); row 0
is bit-equal to the GSC UCB loader's row."""
import os

import numpy as np
import pytest

from blindshadowremoval_amd import dataset as D
from blindshadowremoval_amd.fsrnet import Config

FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ucb_tsm_elements.npz")


def _cfg(golden_dir):
    cfg = Config(0)
    cfg.DATA_DIR_TEST = [os.path.join(golden_dir, "UCB", "train", "input", "9156")]
    return cfg


def test_elements_match_the_reference_parser(golden_dir):
    fx = np.load(FIX)
    ds = D.Dataset(_cfg(golden_dir), "test", dset="ucb_tsm", ucb=True)
    gsc = D.Dataset(_cfg(golden_dir), "test", ucb=True)
    assert ds.name_list == gsc.name_list and all(n.endswith(".npy") for n in ds.name_list)
    for item in ("9156-004", "9156-005"):
        img, box, name = next(ds.feed)
        g_img, g_box, g_name = next(gsc.feed)
        assert os.path.basename(ds.name_list[0 if item.endswith("4") else 1]) == item + ".npy"
        key = item.replace("-", "_")
        assert img.shape == (1, 2, 256, 256, 16) and img.dtype == np.float32 and box.shape == (1, 4)
        np.testing.assert_array_equal(img[0][:, ::8, ::8, :], fx[key])
        np.testing.assert_array_equal(img[0].astype(np.float64).sum(axis=(1, 2)), fx[key + "_sum"])
        np.testing.assert_array_equal(box[0], fx[key + "_box"])
        np.testing.assert_array_equal(img[0, 0], g_img[0, 0])                   # row 0 = the GSC UCB row, bit for bit
        np.testing.assert_array_equal(box, g_box)
        assert name[0] == g_name[0] and name[0].decode().endswith("/gt/9156/%s.png" % item)
        np.testing.assert_array_equal(img[0, 1, :, :, :6], img[0, 0, :, ::-1, :6])       # the mirror row's pixels: the flipped crop


def test_workers_and_shard_give_the_serial_elements(golden_dir):
    serial = D.Dataset(_cfg(golden_dir), "test", dset="ucb_tsm", ucb=True)
    want = [next(serial.feed) for _ in range(len(serial.name_list))]
    par = D.Dataset(_cfg(golden_dir), "test", dset="ucb_tsm", ucb=True, workers=2)
    par.shard(1, len(par.name_list))
    try:
        got = list(par.feed)
    finally:
        par.close()
    assert len(got) == len(want) - 1
    for a, b in zip(got, want[1:]):
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(a[1], b[1])
        assert a[2][0] == b[2][0]


def test_refusals(golden_dir):
    with pytest.raises(ValueError, match="ucb=True"):
        D.Dataset(_cfg(golden_dir), "test", dset="ucb_tsm")
    with pytest.raises(NotImplementedError, match="device_prep"):
        D.Dataset(_cfg(golden_dir), "test", dset="ucb_tsm", ucb=True, device_prep=0)
