"""FSRNetTSM.test (train_with_TSM.py:369-618) on the GPU: GeneratorTSM with frame = 2 + the device post-processing
(csrc/ucb_tsm_kernels.h) + the device PNG encoder over the 100 golden UCB items, against GeneratorTSMOracle pushed through the host
statement; the host post path and batch = 1 give the same strips; the f32x3 mode runs."""
import io
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _cfg(golden_dir, out_dir):
    from blindshadowremoval_amd.fsrnet import Config
    cfg = Config(0)
    cfg.DATA_DIR_TEST = [os.path.join(golden_dir, "UCB", "train", "input", "*")]
    cfg.UCB_MASK_ROOT = os.path.join(golden_dir, "UCB_masks")
    cfg.CHECKPOINT_DIR = out_dir
    return cfg


def _loop(cfg, w, n=None, batch=16, post_device=True, return_figs=True, dtype="f32"):
    from blindshadowremoval_amd import dataset as D
    from blindshadowremoval_amd.fsrnet import FSRNetTSM
    ds = D.Dataset(cfg, "test", dset="ucb_tsm", ucb=True, workers=4)
    if n is not None:
        ds.name_list = ds.name_list[:n]
    fsr = FSRNetTSM(cfg, weights=w, dtype=dtype)
    fsr.post_device, fsr.return_figs = post_device, return_figs
    try:
        res = fsr.test(ds, batch=batch, mat_path=os.path.join(cfg.CHECKPOINT_DIR, "frac_in_nose.mat"))
        saved = list(fsr.log.saved)
    finally:
        ds.close()
        fsr.log.close()
    return res, saved


def _png(path):
    from PIL import Image
    with open(path, "rb") as f:
        return np.asarray(Image.open(io.BytesIO(f.read())).convert("RGB"))


def test_full_ucb_set_against_the_oracle(golden_dir, tmp_path):
    from blindshadowremoval_amd import dataset as D
    from blindshadowremoval_amd.ucb_post import read_masks
    from blindshadowremoval_amd.ucb_post_tsm import MASKS, strip_of, ucb_postprocess_tsm
    from blindshadowremoval_amd.weights import init_weights
    from oracle.gsc_oracle import GeneratorTSMOracle
    w = init_weights(1, variant="tsm")
    cfg = _cfg(golden_dir, str(tmp_path / "dev"))
    res, saved = _loop(cfg, w)
    assert len(res) == 100 and len(saved) == 100 and len(os.listdir(os.path.join(cfg.CHECKPOINT_DIR, "test"))) == 100
    for (name, _, _, _, figs), path in zip(res, saved):
        parts = name.replace("\\", "/").split("/")
        assert os.path.basename(path) == parts[-2] + "_" + parts[-1].split(".")[0] + "-result.png"
        assert len(figs) == 8
        np.testing.assert_array_equal(_png(path), strip_of([f.numpy() for f in figs]), err_msg=name)
    oracle = GeneratorTSMOracle(w)
    ds = D.Dataset(cfg, "test", dset="ucb_tsm", ucb=True, workers=0)
    from blindshadowremoval_amd.ucb_post import MASK_DIRS
    hair_dir = os.path.join(cfg.UCB_MASK_ROOT, MASK_DIRS["face_hair"])
    files = sorted(os.listdir(hair_dir))
    items = [next(ds.feed) for _ in range(100)]
    worst = {"ssim": 0.0, "psnr": 0.0}
    for lo in range(0, 100, 10):
        rows = torch.cat([torch.as_tensor(np.asarray(it[0]), dtype=torch.float32).reshape(2, 256, 256, 16) for it in items[lo:lo + 10]])
        with torch.no_grad():
            _, con, _, dif = oracle(rows[..., 0:3], rows[..., 6:9], rows[..., 9:15], 2, True, chuck=4)
        con, dif = con.float().numpy(), dif.float().numpy()
        for j in range(rows.shape[0] // 2):
            k = lo + j
            m = read_masks({key: os.path.join(cfg.UCB_MASK_ROOT, MASK_DIRS[key], files[k]) for key in MASKS}, grey=True)
            want, _, _, _ = ucb_postprocess_tsm(rows[2 * j, ..., 0:3].numpy(), rows[2 * j, ..., 3:6].numpy(), con[2 * j], con[2 * j + 1], dif[2 * j],
                                                np.asarray(items[k][1], np.float32).reshape(-1)[:4], m)
            for key in ("ssim", "psnr"):
                worst[key] = max(worst[key], abs(res[k][1][key] - want[key]))
    print("max |device - oracle|:", worst)
    assert worst["ssim"] < 1e-3 and worst["psnr"] < 1e-3, worst
    import scipy.io
    mat = scipy.io.loadmat(os.path.join(cfg.CHECKPOINT_DIR, "frac_in_nose.mat"))
    assert mat["frac_in_nose"].size == 100 and mat["mean_intensity"].size == 100


def test_host_post_and_batch_sizes_give_the_same_strips(golden_dir, tmp_path):
    from blindshadowremoval_amd.weights import init_weights
    w = init_weights(1, variant="tsm")
    n = 20
    dev, dev_png = _loop(_cfg(golden_dir, str(tmp_path / "dev")), w, n=n)
    host, host_png = _loop(_cfg(golden_dir, str(tmp_path / "host")), w, n=n, post_device=False)
    one, one_png = _loop(_cfg(golden_dir, str(tmp_path / "b1")), w, n=n, batch=1, return_figs=False)
    assert [r[0] for r in dev] == [r[0] for r in host] == [r[0] for r in one]
    for a, b in zip(dev, host):
        assert abs(a[1]["ssim"] - b[1]["ssim"]) < 1e-4 and abs(a[1]["psnr"] - b[1]["psnr"]) < 1e-4, (a[0], a[1], b[1])
        assert (a[2] == b[2] or (np.isnan(a[2]) and np.isnan(b[2]))) and (a[3] == b[3] or (np.isnan(a[3]) and np.isnan(b[3]))), (a[0], a[2:4], b[2:4])
        for k in range(8):
            assert torch.equal(a[4][k].cpu(), b[4][k].cpu()), (a[0], k)
    for a, b in zip(dev, one):
        assert b[4] is None
        assert abs(a[1]["ssim"] - b[1]["ssim"]) < 1e-4 and abs(a[1]["psnr"] - b[1]["psnr"]) < 1e-4
    for p, q, r in zip(dev_png, host_png, one_png):
        A = _png(p)
        assert A.shape == (256, 8 * 256, 3)
        np.testing.assert_array_equal(A, _png(q))
        np.testing.assert_array_equal(A, _png(r))


def test_f32x3_mode_runs(golden_dir, tmp_path):
    from blindshadowremoval_amd.weights import init_weights
    w = init_weights(1, variant="tsm")
    res32, _ = _loop(_cfg(golden_dir, str(tmp_path / "f32")), w, n=8, batch=4)
    res3, saved = _loop(_cfg(golden_dir, str(tmp_path / "x3")), w, n=8, batch=4, dtype="f32x3")
    assert len(res3) == 8 and len(saved) == 8
    for a, b in zip(res32, res3):
        assert np.isfinite(b[1]["ssim"]) and abs(a[1]["ssim"] - b[1]["ssim"]) < 1e-2, (a[0], a[1], b[1])
