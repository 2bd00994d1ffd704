"""bsr_ucb_post_tsm (csrc/ucb_tsm_kernels.h) against its host statement (blindshadowremoval_amd/ucb_post_tsm.py, itself pinned to the
reference's own train_with_TSM.py test_step by tests/golden/ucb_post_tsm_9156.npz): every figure bit for bit, the strips byte for
byte, frac_nose_in_shadow and mean_intensity exactly, SSIM / PSNR to 1e-4; over the fixture cases, the edge cases and S = 128, 64."""
import hashlib
import os

import numpy as np
import pytest

from ucb_cases import GOLDEN
from ucb_tsm_cases import cases, edge_cases

pytestmark = pytest.mark.gpu
FIX = np.load(os.path.join(GOLDEN, "ucb_post_tsm_9156.npz"))
MASKS = ("face_hair", "face", "nose")


def _run(batch, times=2):
    import torch
    from blindshadowremoval_amd.ucb_post_tsm_gpu import UcbPostTsmDevice
    rows = torch.from_numpy(np.stack([np.concatenate([row[..., 0:3], row[..., 3:6], c0, c1, d0], axis=2) for _, row, _, _, c0, c1, d0 in batch])).cuda()
    masks = torch.from_numpy(np.stack([np.stack([np.rint(m[k][:, :, 0] * 255.0).astype(np.uint8) for k in MASKS]) for _, _, _, m, _, _, _ in batch])).cuda()
    boxes = torch.from_numpy(np.stack([np.asarray(b, np.float32).reshape(4) for _, _, b, _, _, _, _ in batch])).cuda()
    post = UcbPostTsmDevice(0)
    outs = []
    for _ in range(times):                                  # nothing may depend on what the scratch held before
        res = post.run(rows, masks, boxes, want_figs=True)
        torch.cuda.synchronize()
        outs.append(tuple(t.cpu().numpy() for t in res))
    return outs


def _same(a, b):
    return a == b or (np.isnan(a) and np.isnan(b))


def _check_against_host(batch, outs, fixture=False):
    from blindshadowremoval_amd.ucb_post_tsm import strip_of, ucb_postprocess_tsm
    for losses, stats, strips, figs, status in outs:
        assert (status == 0).all(), status
        for j, (key, row, box, m, c0, c1, d0) in enumerate(batch):
            l_ref, f_ref, frac, mean = ucb_postprocess_tsm(row[..., 0:3], row[..., 3:6], c0, c1, d0, box, m)
            for k in range(8):
                np.testing.assert_array_equal(figs[j, k], f_ref[k][0], err_msg="%s fig %d" % (key, k))
            np.testing.assert_array_equal(strips[j], strip_of(f_ref))
            assert _same(float(stats[j, 0]), frac) and _same(float(stats[j, 1]), mean), (key, stats[j], frac, mean)
            assert abs(float(losses[j, 0]) - l_ref["ssim"]) < 1e-4 and abs(float(losses[j, 1]) - l_ref["psnr"]) < 1e-4, (key, losses[j], l_ref)
            if fixture:
                assert hashlib.sha256(np.ascontiguousarray(strips[j]).tobytes()).hexdigest() == str(FIX[key + "_strip_sha256"]), key
                assert float(stats[j, 0]) == float(FIX[key + "_frac"]) and float(stats[j, 1]) == float(FIX[key + "_mean"]), key


def test_device_post_matches_the_host_statement_and_the_reference_fixture():
    batch = list(cases())
    outs = _run(batch)
    _check_against_host(batch, outs, fixture=True)
    for a, b in zip(outs[0], outs[1]):                      # the second run on the same scratch: the same bytes
        np.testing.assert_array_equal(a, b)


def test_edge_cases():
    """No component and an all-hair kept set: nothing kept, mean_intensity NaN (as the host statement); an empty nose mask: status 1."""
    from blindshadowremoval_amd.ucb_post_tsm_gpu import raise_for_status
    ok = [e[:7] for e in edge_cases() if e[7] != "empty_nose"]
    _check_against_host(ok, _run(ok, times=1))
    bad = [e[:7] for e in edge_cases()]
    losses, stats, strips, figs, status = _run(bad, times=1)[0]
    assert list(status) == [0, 0, 1]
    assert np.isnan(stats[2]).all() and np.isnan(losses[2]).all() and (strips[2] == 0).all() and (figs[2] == 0).all()
    assert np.isnan(stats[0, 1]) and stats[0, 0] == 0.0
    with pytest.raises(ValueError, match="item c"):
        raise_for_status(status, ["a", "b", "c"])


def test_other_image_sizes_and_bad_boxes():
    base = list(cases())
    for step in (2, 4):
        small = []
        for i, (key, row, box, m, c0, c1, d0) in enumerate(base):
            S = row.shape[0] // step
            b = np.asarray(box, np.float32).reshape(4).copy()
            b[3] = b[1] + (S if i % 2 == 0 else S - 1 - i)
            sub = lambda a: np.ascontiguousarray(a[::step, ::step])
            small.append(("%s_S%d" % (key, S), sub(row), b, {k: sub(v) for k, v in m.items()}, sub(c0), sub(c1), sub(d0)))
        _check_against_host(small, _run(small, times=1))          # the nose windows of the subsampled cases fall anywhere: both must agree
    key, row, box, m, c0, c1, d0 = base[0]
    b = np.asarray(box, np.float32).reshape(4).copy()
    b[3] = b[1] + 300
    losses, stats, strips, figs, status = _run([(key, row, b, m, c0, c1, d0)], times=1)[0]
    assert list(status) == [2] and np.isnan(losses).all() and (strips == 0).all()
