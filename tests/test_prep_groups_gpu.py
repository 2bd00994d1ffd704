"""bsr_prep_groups (csrc/prep_group_kernels.h) on the GPU: the device-prepared groups of the TSM loaders against the host statements
build_ucb_tsm_pair / build_sfw_pair on every golden UCB item and every labelled frame of sfw_synth/vid0, to the tolerance
tests/test_prep_gpu.py holds the GSC rows to (1e-6, every pixel of every channel; the face channel is a blurred 0 / 1 mask whose
smallest weight is 1/256, so a hull pixel decided differently cannot hide under it); row 1's crop planes against row 0's, and row 0
against bsr_prep_rows, bit for bit; the zero-extended and the empty crop; the loader's ring path; the entry point's refusals."""
import os

import numpy as np
import pytest
import torch

from blindshadowremoval_amd import dataset as D
from blindshadowremoval_amd import prep
from tsm_group_cases import make_edges, sfw_labels, ucb_items

pytestmark = pytest.mark.gpu
TOL = 1e-6            # tests/test_prep_gpu.py: device rows against build_row


def _groups(parts, planes):
    out, boxes = prep.DevicePrep(0, 256, planes=planes).rows(parts)
    torch.cuda.synchronize()
    return out.cpu().numpy(), boxes


def _check_pair(got, want, what, planes):
    assert got.shape == want.shape == (2, 256, 256, planes + 10), what
    assert np.isfinite(got).all(), what
    err = np.abs(got - want).max(axis=(1, 2))
    print(what, "max |device - host| per row:", err.max(axis=1))
    assert err.max() <= TOL, (what, err)
    assert np.array_equal(got[1, :, :, :planes], got[0, :, ::-1, :planes]), what          # the mirror's crop planes: row 0's, flipped


def test_ucb_groups_match_the_host_pair_and_the_row_kernel():
    items = ucb_items()
    for lo in range(0, 100, 25):
        chunk = items[lo:lo + 25]
        got, boxes = _groups([prep.host_part_group(it + (256,)) for it in chunk], 6)
        rows, _ = prep.DevicePrep(0, 256).rows([prep.host_part(it + (256,)) for it in chunk])
        torch.cuda.synchronize()
        rows = rows.cpu().numpy()
        for j, (lm_path, gt) in enumerate(chunk):
            want, box, _ = D.build_ucb_tsm_pair(lm_path, gt, 256)
            assert np.array_equal(boxes[j], box[0])
            _check_pair(got[j], want[0], os.path.basename(lm_path), 6)
            assert np.array_equal(got[j, 0].view(np.uint32), rows[j].view(np.uint32)), lm_path      # row 0: bsr_prep_rows' bits


def test_sfw_groups_match_the_host_pair():
    labels = sfw_labels()
    got, boxes = _groups([prep.host_part_group((p, "<sfw>", 256)) for p in labels], 7)
    for j, p in enumerate(labels):
        want, box, _ = D.build_sfw_pair(p, 256)
        assert np.array_equal(boxes[j], box[0])
        _check_pair(got[j], want[0], os.path.basename(p), 7)
        assert got[j, 0, :, :, 6].max() > 1.0                                         # the label plane kept its grey levels


def test_edge_groups_match_the_host_pair(tmp_path):
    edges = make_edges(str(tmp_path))
    parts = [prep.host_part_group(edges[n] + (256,)) for n in ("leaves", "empty")]
    assert parts[0][2][2] > parts[0][0].shape[1] and parts[0][2][3] > parts[0][0].shape[0]      # the box leaves the cut photograph
    assert parts[1][2][2] == parts[1][2][0]                                                       # the box without pixels
    got, _ = _groups(parts, 6)
    for j, n in enumerate(("leaves", "empty")):
        want = D.build_ucb_tsm_pair(*edges[n], 256)[0][0]
        _check_pair(got[j], want, n, 6)
    assert not got[1, :, :, :, :6].any() and got[0, 0, :, :, :3].any()


def test_loader_ring_path_gives_the_same_groups(golden_dir):
    """Dataset(device_groups=0) with worker processes (the page-locked ring, filtered scanlines reconstructed on the device, the masks
    next to the photographs) yields the bits DevicePrep gives the same items decoded in this process."""
    from blindshadowremoval_amd.fsrnet import Config, _ucb_mask_files
    cfg = Config(0)
    cfg.DATA_DIR_TEST = [os.path.join(golden_dir, "UCB", "train", "input", "*")]
    cfg.UCB_MASK_ROOT = os.path.join(golden_dir, "UCB_masks")
    n = 24
    masks = _ucb_mask_files(cfg)
    ds = D.Dataset(cfg, "test", dset="ucb_tsm", ucb=True, workers=4, device_groups=0, device_batch=16)
    ds.ucb_mask_files = masks
    ds.name_list = ds.name_list[:n]
    try:
        ds.warm()
        if getattr(ds, "_ring", None) is None and getattr(ds, "ring_error", None):
            pytest.skip("no loader ring on this machine: %s" % ds.ring_error)
        assert getattr(ds, "_ring", None) is not None and ds._ring.cap == 3 * prep.RING_CAP // 2
        seen, rows_ex = [], ds._dp.rows_ex

        def spy(parts):                                  # what the workers handed over
            seen.extend(parts)
            return rows_ex(parts)
        ds._dp.rows_ex = spy
        els = [next(ds.feed) for _ in range(n)]
        ring = [p for p in seen if p[0] == "ring"]
        assert len(seen) == n and len(ring) == n, [p[0] if isinstance(p[0], str) else "pipe" for p in seen]
        # filtered scanlines in the slots (two RGB photographs, seven grey masks per item), eight tables: bsr_png_unfilter reconstructs them
        assert all(tuple(p[11]) == (3, 3) and p[9][0] == "raw8" and len(p[5]) == 8 for p in ring), [(p[11], p[9][0]) for p in ring]
        torch.cuda.synchronize()
        want, boxes = _groups([prep.host_part_group(it + (256,)) for it in ucb_items()[:n]], 6)
        for j, el in enumerate(els):
            assert el[0].is_cuda and tuple(el[0].shape) == (1, 2, 256, 256, 16)
            assert np.array_equal(el[0][0].cpu().numpy().view(np.uint32), want[j].view(np.uint32)), j
            assert np.array_equal(el[1][0], boxes[j]) and el[2][0] == ucb_items()[j][1].encode()
            got_m = prep.unpack_masks([el[3]], "cuda:0")[0].cpu().numpy()
            assert np.array_equal(got_m, prep.read_masks_u8(masks[j])), j
    finally:
        ds.close()


def test_entry_point_refusals():
    from blindshadowremoval_amd import _lib
    lib = _lib.load()
    blob, goff, grid_off = prep.pack_group_batch([prep.host_part_group(ucb_items()[0] + (256,))], 256)
    d = torch.frombuffer(bytearray(blob), dtype=torch.uint8).cuda()
    out = torch.empty((1, 2, 256, 256, 17), dtype=torch.float32, device="cuda")
    tmp = torch.empty((2, 256, 256), dtype=torch.float32, device="cuda")
    n = d.numel()

    def call(blob_ptr=d.data_ptr(), nbytes=n, go=goff, gr=grid_off, B=1, S=256, planes=6, o=out.data_ptr(), t=tmp.data_ptr()):
        return lib.bsr_prep_groups(0, blob_ptr, nbytes, go, gr, B, S, planes, o, t, None)
    assert call() == 0
    torch.cuda.synchronize()
    for kw in (dict(blob_ptr=None), dict(o=None), dict(t=None), dict(B=0), dict(S=0), dict(S=100), dict(planes=5), dict(planes=8), dict(planes=16),
               dict(go=goff + 4), dict(gr=grid_off + 4), dict(go=n + 8), dict(go=n - 8), dict(gr=n - 8), dict(B=1 << 20), dict(nbytes=goff + 8)):
        assert call(**kw) != 0, kw
        assert b"bsr_prep_groups" in lib.bsr_last_error(), kw
    torch.cuda.synchronize()
