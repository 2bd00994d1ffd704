"""Dataset(config, 'test', dset='sfw_gsc', rows=R) — the GSC script's SFW loader (`parse_fn_test_sfw`, /root/reference/dataset.py:338-612) —
against tests/golden/sfw_gsc_elements.npz, the output of the reference's OWN parser on tests/golden/sfw_synth
(tools/make_sfw_gsc_fixture.py; every 8th pixel + per-channel sums are stored).  Also: row 0 of the GSC element is the TSM pair's row 0,
and the argument checks."""
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _cfg():
    return type("C", (), {"DATA_DIR_TEST": [os.path.join(GOLDEN, "sfw_synth", "*")], "IMG_SIZE": 256})()


def test_sfw_gsc_elements_match_the_reference_parser():
    from blindshadowremoval_amd import dataset as D
    z = np.load(os.path.join(GOLDEN, "sfw_gsc_elements.npz"))
    ds = D.Dataset(_cfg(), "test", dset="sfw_gsc", rows=10)
    assert [os.path.basename(n) for n in ds.name_list] == ["1_label.png", "10_label.png"]
    for n in (1, 10):
        img, box, name = next(ds.feed)
        assert img.shape == (1, 10, 256, 256, 17) and img.dtype == np.float32
        np.testing.assert_allclose(img[0, :, ::8, ::8, :], z["gsc%d" % n], rtol=0, atol=1e-6)
        np.testing.assert_allclose(img[0].astype(np.float64).sum(axis=(1, 2)), z["gsc%d_sum" % n], rtol=1e-6, atol=1e-3)
        np.testing.assert_array_equal(box[0], z["gsc%d_box" % n])                 # the LAST row's box, as the reference leaves it
        assert os.path.basename(name[0].decode()) == "%d.png" % n


def test_sfw_gsc_rows_are_a_prefix_and_workers_agree():
    from blindshadowremoval_amd import dataset as D
    full = [e[0] for e in D.Dataset(_cfg(), "test", dset="sfw_gsc", rows=10).feed]
    one = [e for e in D.Dataset(_cfg(), "test", dset="sfw_gsc").feed]          # rows=1 is the default
    three = [e[0] for e in D.Dataset(_cfg(), "test", dset="sfw_gsc", rows=3, workers=2).feed]
    for f, o, t in zip(full, one, three):
        assert o[0].shape == (1, 1, 256, 256, 17)
        np.testing.assert_array_equal(o[0][0, 0], f[0, 0])
        np.testing.assert_array_equal(t[0], f[0, :3])


def test_sfw_gsc_row0_equals_the_tsm_pair_row0():
    """dataset_with_TSM.py:225-262 and dataset.py:338-366 build row 0 the same way: FSRNet.testsfw accepts either element."""
    from blindshadowremoval_amd import dataset as D
    gsc = [e[0] for e in D.Dataset(_cfg(), "test", dset="sfw_gsc").feed]
    pair = [e[0] for e in D.Dataset(_cfg(), "test", dset="sfw").feed]
    z_gsc, z_pair = np.load(os.path.join(GOLDEN, "sfw_gsc_elements.npz")), np.load(os.path.join(GOLDEN, "sfw_elements.npz"))
    for k, (g, p) in enumerate(zip(gsc, pair)):
        assert p.shape == (1, 2, 256, 256, 17)
        np.testing.assert_array_equal(g[0, 0], p[0, 0])
        n = (1, 10)[k]                                                              # and the two reference parsers agree on it too
        np.testing.assert_allclose(z_gsc["gsc%d" % n][0, :, :, :], z_pair["pair%d" % n][0, ::2, ::2, :], rtol=0, atol=1e-6)


def test_sfw_gsc_argument_checks():
    from blindshadowremoval_amd import dataset as D
    with pytest.raises(ValueError):
        D.Dataset(_cfg(), "test", dset="sfw_gsc", rows=11)
    with pytest.raises(ValueError):
        D.Dataset(_cfg(), "test", dset="sfw_gsc", rows=0)
    with pytest.raises(NotImplementedError):
        D.Dataset(_cfg(), "test", dset="sfw_gsc", device_prep=0)


def test_resize_chain_keeps_8bit_levels_across_sizes():
    from blindshadowremoval_amd.dataset import _resize_to
    m = (np.arange(64, dtype=np.uint8).reshape(8, 8) % 3)
    same = _resize_to(m, 8, 8)
    assert same.dtype == np.uint8 and np.array_equal(same, m)
    big = _resize_to(np.ones((4, 6, 3)), 8, 12)
    assert big.shape == (8, 12, 3) and np.allclose(big, 1.0)
