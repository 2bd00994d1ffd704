"""FSRNetTSM.test and FSRNetTSM.testsfw over Dataset(device_groups=0) against the same loops over the host loader: the device-prepared
groups differ from the host's by at most 1e-6 (tests/test_prep_groups_gpu.py), so per item SSIM, PSNR, frac_nose_in_shadow and
mean_intensity agree to the tolerance tests/test_dataset.py::test_ucb_full_set_100_items holds the GSC device path to (1e-3 of
max(1, |value|)), the status words of bsr_ucb_post_tsm are equal, and the number of byte-identical strips is reported.  FSRNetTSM.testsfw
itself reports PSNR and AUC only (both of the mask head): the SFW test takes the SSIM of the restored image per item and run itself, and
compares the restored images and the shown masks of the two runs directly."""
import os
import shutil

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
REL = 1e-3            # tests/test_dataset.py::test_ucb_full_set_100_items

# Items whose decision bits may differ because an input difference of 1e-6 straddles a post-processing threshold: name -> the two values
# on either side.  At most 2 of the 100; none has been needed.
EXCEPTED = {}


def _close(a, b):
    if np.isnan(a) or np.isnan(b):
        return bool(np.isnan(a) and np.isnan(b))
    return abs(a - b) / max(1.0, abs(b)) < REL


def test_ucb_loop_with_device_groups_equals_the_host_loader(golden_dir, tmp_path):
    from blindshadowremoval_amd import dataset as D
    from blindshadowremoval_amd.fsrnet import Config, FSRNetTSM
    from blindshadowremoval_amd.weights import init_weights
    w = init_weights(1, variant="tsm")
    runs = {}
    for mode in ("host", "device"):
        cfg = Config(0)
        cfg.DATA_DIR_TEST = [os.path.join(golden_dir, "UCB", "train", "input", "*")]
        cfg.UCB_MASK_ROOT = os.path.join(golden_dir, "UCB_masks")
        cfg.CHECKPOINT_DIR = str(tmp_path / mode)
        kw = dict(device_groups=0, device_batch=16) if mode == "device" else {}
        ds = D.Dataset(cfg, "test", dset="ucb_tsm", ucb=True, workers=6, **kw)
        fsr = FSRNetTSM(cfg, weights=w)
        fsr.return_figs = False
        try:
            res = fsr.test(ds, batch=16, mat_path=os.path.join(cfg.CHECKPOINT_DIR, "frac_in_nose.mat"))
            runs[mode] = (res, list(fsr.log.saved), list(fsr.statuses), ds.ucb_mask_files is not None)
        finally:
            ds.close()
            fsr.log.close()
    (host, host_png, host_st, host_m), (dev, dev_png, dev_st, dev_m) = runs["host"], runs["device"]
    assert len(host) == len(dev) == 100 and [r[0] for r in host] == [r[0] for r in dev]
    assert dev_m and not host_m                     # the device loader carried the masks, the host loop read them itself
    assert len(host_st) == len(dev_st) == 100
    flips = [(r[0], a, b) for r, a, b in zip(host, host_st, dev_st) if a != b and r[0] not in EXCEPTED]
    assert not flips, "status words differ (item, host loader, device groups): %s" % flips
    assert len(EXCEPTED) <= 2
    worst, same = {"ssim": 0.0, "psnr": 0.0, "frac": 0.0, "mean": 0.0}, 0
    bad = []
    for a, b, pa, pb in zip(dev, host, dev_png, host_png):
        vals = (("ssim", a[1]["ssim"], b[1]["ssim"]), ("psnr", a[1]["psnr"], b[1]["psnr"]), ("frac", a[2], b[2]), ("mean", a[3], b[3]))
        for key, x, y in vals:
            if not (np.isnan(x) and np.isnan(y)):
                worst[key] = max(worst[key], abs(x - y) / max(1.0, abs(y)))
            if not _close(x, y):
                bad.append((a[0], key, x, y))
        with open(pa, "rb") as f, open(pb, "rb") as g:
            same += f.read() == g.read()
    print("device groups against the host loader, 100 UCB items: worst relative deviation %s; %d of 100 strips byte-identical" % (worst, same))
    assert not bad, bad


def test_sfw_loop_with_device_groups_equals_the_host_loader(golden_dir, tmp_path):
    from blindshadowremoval_amd import dataset as D
    from blindshadowremoval_amd.fsrnet import Config, FSRNetTSM
    from blindshadowremoval_amd.weights import init_weights
    for v in range(5):                                # five folders of the two labelled frames: ten items, batch 4 -> a ragged last group
        shutil.copytree(os.path.join(golden_dir, "sfw_synth", "vid0"), str(tmp_path / "data" / ("vid%d" % v)))
    w = init_weights(1, variant="tsm")
    runs = {}
    for mode in ("host", "device"):
        cfg = Config(0)
        cfg.DATA_DIR_TEST = [str(tmp_path / "data" / "*")]
        cfg.CHECKPOINT_DIR = str(tmp_path / mode)
        kw = dict(device_groups=0, device_batch=4) if mode == "device" else {}
        ds = D.Dataset(cfg, "test", dset="sfw", workers=3, **kw)
        fsr = FSRNetTSM(cfg, weights=w)
        try:
            runs[mode] = fsr.testsfw(ds, batch=4)
        finally:
            ds.close()
            fsr.log.close()
    from blindshadowremoval_amd.metrics import ssim
    assert len(runs["host"]) == len(runs["device"]) == 10
    worst = {"auc": 0.0, "psnr": 0.0, "ssim": 0.0, "con_rgb": 0.0, "mask": 0.0}
    for (na, la, fa), (nb, lb, fb) in zip(runs["device"], runs["host"]):
        assert na == nb and set(la) == set(lb) == {"auc", "psnr"}
        # FSRNetTSM.testsfw reports PSNR and AUC, both of the mask head alone; the SSIM the issue asks for is taken here, per item and
        # per run, of the restored image against the input (rows 0 and 1 of the group), as the UCB loop takes it
        fa, fb = [torch.as_tensor(f).float().cpu() for f in fa], [torch.as_tensor(f).float().cpu() for f in fb]
        la, lb = dict(la, ssim=float(ssim(fa[1], fa[0]).mean())), dict(lb, ssim=float(ssim(fb[1], fb[0]).mean()))
        for key in la:
            worst[key] = max(worst[key], abs(la[key] - lb[key]) / max(1.0, abs(lb[key])))
            assert _close(la[key], lb[key]), (na, key, la[key], lb[key])
        assert torch.allclose(fa[0], fb[0], atol=1e-6, rtol=0)                         # the input rows: the preparation's own tolerance
        # the generator's outputs of both rows: restored image in [0, 1] and shown mask in [0, 2].  Inputs 1e-6 apart give outputs a
        # float32 network's rounding apart, far under the loops' 1e-3; a wrong or mis-sliced plane moves them by the plane's own size
        for key, k in (("con_rgb", 1), ("mask", 2)):
            assert fa[k].shape == fb[k].shape and torch.isfinite(fa[k]).all()
            d = float((fa[k] - fb[k]).abs().mean())
            worst[key] = max(worst[key], d)
            assert d < REL, (na, key, d)
    print("device groups against the host loader, 10 SFW items: worst deviation %s" % worst)
