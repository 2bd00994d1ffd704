"""bsr_ucb_post_rgb (csrc/ucb_rgb_kernels.h) against its host statement (blindshadowremoval_amd/ucb_post_rgb.py, itself pinned to the
reference's own train_RGB_test.py test_step by tests/golden/ucb_post_rgb_9156.npz): every figure bit for bit, the strips byte for byte,
SSIM / PSNR to 1e-4."""
import hashlib
import os

import numpy as np
import pytest

from ucb_cases import GOLDEN, cases

pytestmark = pytest.mark.gpu
FIX = np.load(os.path.join(GOLDEN, "ucb_post_rgb_9156.npz"))


def _run(batch, want_figs=True, times=2):
    import torch
    from blindshadowremoval_amd.ucb_post_rgb_gpu import UcbPostRgbDevice
    rows9 = torch.from_numpy(np.stack([np.concatenate([row[..., 0:3], row[..., 3:6], con], axis=2) for _, row, _, _, con in batch])).cuda()
    masks = torch.from_numpy(np.stack([np.rint(m[:, :, 0] * 255.0).astype(np.uint8) for _, _, _, m, _ in batch])).cuda()
    boxes = torch.from_numpy(np.stack([np.asarray(b, np.float32).reshape(4) for _, _, b, _, _ in batch])).cuda()
    post = UcbPostRgbDevice(0)
    outs = []
    for _ in range(times):                                  # nothing may depend on what the scratch held before
        losses, strips, figs, status = post.run(rows9, masks, boxes, want_figs=want_figs)
        torch.cuda.synchronize()
        outs.append((losses.cpu().numpy(), strips.cpu().numpy(), (figs.cpu().numpy() if figs is not None else None), status.cpu().numpy()))
    return outs


def _check_against_host(batch, outs, fixture=False):
    from blindshadowremoval_amd.ucb_post_rgb import strip_of, ucb_postprocess_rgb
    for losses, strips, figs, status in outs:
        assert (status == 0).all()
        for j, (key, row, box, fh, con) in enumerate(batch):
            l_ref, f_ref = ucb_postprocess_rgb(row[..., 0:3], row[..., 3:6], con, box, fh)
            for k in range(3):
                np.testing.assert_array_equal(figs[j, k], f_ref[k][0], err_msg="%s fig %d" % (key, k))
            np.testing.assert_array_equal(strips[j], strip_of(f_ref))
            assert abs(float(losses[j, 0]) - l_ref["ssim"]) < 1e-4 and abs(float(losses[j, 1]) - l_ref["psnr"]) < 1e-4, (key, losses[j], l_ref)
            if fixture:
                assert hashlib.sha256(np.ascontiguousarray(strips[j]).tobytes()).hexdigest() == str(FIX[key + "_strip_sha256"]), key
                assert abs(float(losses[j, 0]) - float(FIX[key + "_ssim"])) < 1e-4 and abs(float(losses[j, 1]) - float(FIX[key + "_psnr"])) < 1e-4


def test_device_post_matches_the_host_statement_and_the_reference_fixture():
    batch = [(key, row, box, m["face_hair"], con) for key, row, box, m, con, _ in cases()]
    outs = _run(batch)
    _check_against_host(batch, outs, fixture=True)
    for a, b in zip(outs[0], outs[1]):                      # the second run on the same scratch: the same bytes
        np.testing.assert_array_equal(a, b)


def test_other_crop_sizes_and_image_sizes():
    """Crop boxes of other sizes (odd scales put the rounded mask on .5 ties; size == S is the identity resize) and S = 32, 64, 128."""
    base = list(cases())
    batch = []
    for i, size in enumerate((256, 255, 192, 200, 171, 129, 128, 233, 250, 96)):
        key, row, box, m, con, _ = base[i % len(base)]
        b = np.asarray(box, np.float32).reshape(4).copy()
        b[3] = b[1] + size
        batch.append(("%s_s%d" % (key, size), row, b, m["face_hair"], (con * np.float32(1 + 0.2 * i) - np.float32(0.1 * i)).astype(np.float32)))
    _check_against_host(batch, _run(batch, times=1))
    for step in (2, 4, 8):
        small = []
        for i, (key, row, box, m, con, _) in enumerate(base):
            S = row.shape[0] // step
            b = np.asarray(box, np.float32).reshape(4).copy()
            b[3] = b[1] + (S if i % 2 == 0 else S - 1 - i)
            sub = lambda a: np.ascontiguousarray(a[::step, ::step])
            small.append(("%s_S%d" % (key, S), sub(row), b, sub(m["face_hair"]), sub(con)))
        _check_against_host(small, _run(small, times=1))


def test_bad_box_is_reported():
    import torch
    from blindshadowremoval_amd.ucb_post_rgb_gpu import UcbPostRgbDevice, raise_for_status
    key, row, box, m, con, _ = next(iter(cases()))
    rows9 = torch.from_numpy(np.concatenate([row[..., 0:3], row[..., 3:6], con], axis=2)[None].repeat(3, 0)).cuda()
    masks = torch.from_numpy(np.rint(m["face_hair"][:, :, 0] * 255.0).astype(np.uint8)[None].repeat(3, 0)).cuda()
    boxes = np.asarray(box, np.float32).reshape(1, 4).repeat(3, 0)
    boxes[1, 3] = boxes[1, 1] + 300                         # item 1: a 300-pixel box in a 256-pixel image
    boxes[2, 3] = boxes[2, 1]                               # item 2: an empty box
    losses, strips, figs, status = UcbPostRgbDevice(0).run(rows9, masks, torch.from_numpy(boxes).cuda(), want_figs=True)
    st = status.cpu().numpy()
    assert list(st) == [0, 2, 2]
    assert np.isfinite(losses[0].cpu().numpy()).all() and np.isnan(losses[1:].cpu().numpy()).all()
    assert (strips[1:].cpu().numpy() == 0).all() and (figs[1:].cpu().numpy() == 0).all()
    with pytest.raises(ValueError, match="item b: the crop box is larger than the image or empty"):
        raise_for_status(st, ["a", "b", "c"])
    with pytest.raises(TypeError):
        UcbPostRgbDevice(0).run(rows9.cpu(), masks, torch.from_numpy(boxes).cuda())
    with pytest.raises(ValueError, match="S in"):
        UcbPostRgbDevice(0).run(rows9[:, :200, :200].contiguous(), masks[:, :200, :200].contiguous(), torch.from_numpy(boxes).cuda())
