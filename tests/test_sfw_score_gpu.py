"""bsr_sfw_score (csrc/sfw_kernels.h) against its host statement (blindshadowremoval_amd/sfw_post.py, itself pinned to the reference's own
test_step_sfw and sklearn by tests/golden/sfw_post_gsc.npz): the AUC EQUAL to fsrnet.roc_auc_score (no tolerance) over 16 items that
cover the ways an exact rank count can go wrong, mask_pred and the label plane bit for bit, SSIM / PSNR to 1e-4, the status word of a
NaN score, and the PNG strips byte for byte."""
import io
import os

import numpy as np
import pytest

from sfw_post_cases import S, cases

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _items():
    """16 (key, img, con, mask, dif, face): the six fixture cases, then edges of the rank count; the last has a NaN score."""
    rng = np.random.default_rng(7)
    items = list(cases())
    img, con = rng.random((S, S, 3), dtype=np.float32), rng.random((S, S, 3), dtype=np.float32)
    one = np.ones((S, S, 1), np.float32)
    lab = lambda p: np.where(rng.random((S, S, 1)) < p, 2, rng.integers(0, 2, (S, S, 1))).astype(np.float32)
    items.append(("allties", img, con, lab(0.3), np.full((S, S, 1), 0.5, np.float32), one))
    pm0 = np.where(rng.random((S, S, 1)) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    pm0[:8] = rng.random((8, S, 1))                                                  # a few non-zero scores above the +-0 ties
    items.append(("pm0", img, con, lab(0.4), pm0, one))
    bits = rng.integers(1, 1 << 23, (S, S, 1)).astype(np.uint32) | (rng.integers(0, 2, (S, S, 1)).astype(np.uint32) << 31)
    items.append(("subnormal_bits", img, con, lab(0.5), bits.view(np.float32), one))          # every score subnormal, either sign
    distinct = np.arange(S * S, dtype=np.float32)[rng.permutation(S * S)].reshape(S, S, 1) / np.float32(S * S) - np.float32(0.3)
    items.append(("distinct", img, con, lab(0.5), distinct, one))                             # 65 536 distinct scores
    single = np.zeros((S, S, 1), np.float32)
    single[200, 17] = 2
    items.append(("single_pos", img, con, single, rng.random((S, S, 1), dtype=np.float32), one))
    levels = np.array([0.1, 0.2, 0.3, 0.7], np.float32)
    items.append(("cross_tile_eq", img, con, lab(0.5), levels[rng.integers(0, 4, (S, S, 1))], one))   # positives equal keys in every tile
    items.append(("no_label", img, con, np.zeros((S, S, 1), np.float32), np.zeros((S, S, 1), np.float32), np.zeros((S, S, 1), np.float32)))
    items.append(("all_label", img, con, np.full((S, S, 1), 2, np.float32), rng.normal(0, 1, (S, S, 1)).astype(np.float32), one))
    items.append(("wide", img, con, lab(0.2), (rng.normal(0, 1, (S, S, 1)) * 1e3).astype(np.float32), one))
    nan = rng.random((S, S, 1), dtype=np.float32)
    nan[100, 100] = np.nan
    items.append(("nan", img, con, lab(0.3), nan, one))
    assert len(items) == 16
    return items


def _run(items, times=2):
    import torch
    from blindshadowremoval_amd.sfw_post_gpu import SfwScoreDevice
    rows3 = torch.from_numpy(np.stack([np.concatenate([m, d, f], axis=2) for _, _, _, m, d, f in items])).cuda()
    dev = SfwScoreDevice(0)
    outs = []
    for _ in range(times):                                   # nothing may depend on what the scratch held before
        losses, auc, pred, label, status = dev.run(rows3)
        torch.cuda.synchronize()
        outs.append(tuple(t.cpu().numpy() for t in (losses, auc, pred, label, status)))
    return outs


def test_device_auc_equals_the_exact_host_form():
    from blindshadowremoval_amd.fsrnet import roc_auc_score
    from blindshadowremoval_amd.sfw_post import sfw_score
    items = _items()
    outs = _run(items)
    for losses, auc, pred, label, status in outs:
        for j, (key, _, _, mask, dif, face) in enumerate(items):
            want_pred = (dif * face).astype(np.float32)
            np.testing.assert_array_equal(pred[j].view(np.uint32), want_pred.view(np.uint32), err_msg=key)      # bit for bit, -0.0 included
            np.testing.assert_array_equal(label[j], (mask == 2).astype(np.float32), err_msg=key)
            if key == "nan":
                assert status[j] == 3 and np.isnan(auc[j])
                continue
            assert status[j] == 0, key
            extr = np.array([1, 0])
            exact = roc_auc_score(np.concatenate([extr, (mask == 2).reshape(-1)]), np.concatenate([extr, want_pred.reshape(-1)]))
            assert float(auc[j]) == exact, (key, float(auc[j]), exact)
            want, _, _ = sfw_score(mask, dif, face)
            assert float(auc[j]) == want["auc"]
            for i, k in enumerate(("ssim", "psnr")):                # identical planes: PSNR is +inf on both sides
                assert float(losses[j, i]) == want[k] or abs(float(losses[j, i]) - want[k]) <= 1e-4, (key, losses[j], want)
    for a, b in zip(outs[0], outs[1]):
        np.testing.assert_array_equal(a, b)                  # deterministic


def test_device_auc_against_sklearn_fixture():
    z = np.load(os.path.join(GOLDEN, "sfw_post_gsc.npz"))
    items = cases()
    losses, auc, _, _, status = _run(items, times=1)[0]
    for j, (key, *_) in enumerate(items):
        assert status[j] == 0
        assert abs(float(auc[j]) - float(z[key + "_auc"])) <= 1e-12, key
        assert abs(float(losses[j, 0]) - float(z[key + "_ssim"])) <= 1e-4 and abs(float(losses[j, 1]) - float(z[key + "_psnr"])) <= 1e-4, key


def test_nan_status_raises_in_the_loop_helper():
    from blindshadowremoval_amd.sfw_post_gpu import raise_for_status
    raise_for_status(np.zeros(3, np.int32), ["a", "b", "c"])
    with pytest.raises(ValueError, match="b"):
        raise_for_status(np.array([0, 3, 0], np.int32), ["a", "b", "c"])


def test_strips_and_files_equal_the_host_figures(tmp_path):
    import torch
    from PIL import Image
    from blindshadowremoval_amd import pngio
    from blindshadowremoval_amd.fsrnet import Config, Logging
    from blindshadowremoval_amd.sfw_post import sfw_postprocess, strip_of
    from blindshadowremoval_amd.sfw_post_gpu import SfwScoreDevice
    items = _items()[:15]
    t = lambda a: torch.from_numpy(np.stack(a)).cuda()
    im, con = t([it[1] for it in items]), t([it[2] for it in items])
    mask, dif, face = t([it[3] for it in items]), t([it[4] for it in items]), t([it[5] for it in items])
    _, _, pred, label, _ = SfwScoreDevice(0).run(torch.cat([mask, dif, face], dim=3))
    cfg = Config(0)
    cfg.CHECKPOINT_DIR = str(tmp_path)
    log = Logging(cfg)
    files = log.files_on_device([im, con, (dif, face, 2.0), label]).cpu().numpy()           # the loop's call: the encoder multiplies
    strips = Logging.strips_on_device([im, torch.clamp(con, 0, 1), pred * 2, label]).cpu().numpy()
    for j, (key, img, c, m, d, f) in enumerate(items):
        _, figs = sfw_postprocess(img, c, m, d, f)
        host = strip_of(figs)
        np.testing.assert_array_equal(strips[j], host, err_msg=key)
        np.testing.assert_array_equal(host, Logging.get_imgs([torch.from_numpy(x) for x in figs]))
        data = files[j].tobytes()
        assert data == pngio.encode_png_stored(host), key
        path = log.save_img([torch.from_numpy(x) for x in figs], "%s.png" % key)             # what Logging.save_img writes for the host figures
        np.testing.assert_array_equal(np.asarray(Image.open(path).convert("RGB")), np.asarray(Image.open(io.BytesIO(data)).convert("RGB")))
    log.close()
