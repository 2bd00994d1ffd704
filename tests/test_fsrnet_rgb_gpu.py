"""FSRNetRGB.test (train_RGB_test.py:357-505) on the GPU: GeneratorRGB + the device post-processing (csrc/ucb_rgb_kernels.h) + the device
PNG encoder over the 100 golden UCB items, against the CPU oracle of model_RGB.py pushed through the host statement; the host post path
and other batch sizes give the same strips."""
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


def _loop(cfg, w, n=None, batch=16, post_device=True, return_figs=True):
    from blindshadowremoval_amd import dataset as D
    from blindshadowremoval_amd.fsrnet import FSRNetRGB
    ds = D.Dataset(cfg, "test", ucb=True, workers=2, device_prep=0, device_batch=batch)
    if n is not None:
        ds.name_list = ds.name_list[:n]
    fsr = FSRNetRGB(cfg, weights=w)
    fsr.post_device, fsr.return_figs = post_device, return_figs
    try:
        res = fsr.test(ds, batch=batch)
        saved = list(fsr.log.saved)
        forwards = fsr.timings.get("forwards")
    finally:
        ds.close()
        fsr.close()
    return res, saved, forwards


def _png(path):
    from PIL import Image
    with open(path, "rb") as f:
        return np.asarray(Image.open(io.BytesIO(f.read())).convert("RGB"))


def test_full_ucb_set_against_the_oracle(golden_dir, tmp_path):
    from blindshadowremoval_amd import dataset as D
    from blindshadowremoval_amd.ucb_post import MASK_DIRS, read_masks
    from blindshadowremoval_amd.ucb_post_rgb import strip_of, ucb_postprocess_rgb
    from blindshadowremoval_amd.weights import init_weights
    from rgb_oracle import GeneratorRGBOracle
    w = init_weights(1, variant="rgb")
    cfg = _cfg(golden_dir, str(tmp_path / "dev"))
    res, saved, forwards = _loop(cfg, w)
    assert len(res) == 100 and forwards == 7
    assert len(saved) == 100 and len(set(saved)) == 100 and len(os.listdir(os.path.join(cfg.CHECKPOINT_DIR, "test"))) == 100
    for (name, figs, _), path in zip(res, saved):
        parts = name.replace("\\", "/").split("/")
        assert os.path.basename(path) == parts[-2] + "_" + parts[-1].split(".")[0] + "-result.png"
        assert len(figs) == 3
        np.testing.assert_array_equal(_png(path), strip_of([f.cpu().numpy() for f in figs]), err_msg=name)
    # the oracle: model_RGB.py restated on the CPU, the same rows (host-prepared), then the host statement of the post-processing
    oracle = GeneratorRGBOracle(w)
    ds = D.Dataset(cfg, "test", ucb=True, workers=0)
    hair_dir = os.path.join(cfg.UCB_MASK_ROOT, MASK_DIRS["face_hair"])
    masks = [os.path.join(hair_dir, f) for f in sorted(os.listdir(hair_dir))]           # train_RGB_test.py:372,381: masks[count]
    items = [next(ds.feed) for _ in range(100)]
    worst = {"ssim": 0.0, "psnr": 0.0}
    for lo in range(0, 100, 20):
        rows = torch.cat([torch.as_tensor(np.asarray(it[0]), dtype=torch.float32).reshape(-1, 256, 256, 16)[:1] for it in items[lo:lo + 20]])
        with torch.no_grad():
            con = oracle(rows[..., 0:3], rows[..., 6:9]).float().numpy()
        for j in range(rows.shape[0]):
            k = lo + j
            fh = read_masks({"face_hair": masks[k]}, grey=True)["face_hair"]
            want, _ = ucb_postprocess_rgb(rows[j, ..., 0:3].numpy(), rows[j, ..., 3:6].numpy(), con[j],
                                          np.asarray(items[k][1], np.float32).reshape(-1)[:4], fh)
            for key in ("ssim", "psnr"):
                worst[key] = max(worst[key], abs(res[k][2][key] - want[key]))
    print("max |device - oracle|:", worst)
    assert worst["ssim"] < 1e-3 and worst["psnr"] < 1e-3, worst


def test_host_post_and_batch_sizes_give_the_same_strips(golden_dir, tmp_path):
    from blindshadowremoval_amd.weights import init_weights
    w = init_weights(1, variant="rgb")
    n = 20
    dev, dev_png, _ = _loop(_cfg(golden_dir, str(tmp_path / "dev")), w, n=n)
    host, host_png, _ = _loop(_cfg(golden_dir, str(tmp_path / "host")), w, n=n, post_device=False)
    one, one_png, forwards = _loop(_cfg(golden_dir, str(tmp_path / "b1")), w, n=n, batch=1, return_figs=False)
    assert forwards == n
    assert [r[0] for r in dev] == [r[0] for r in host] == [r[0] for r in one]
    for a, b in zip(dev, host):
        assert abs(a[2]["ssim"] - b[2]["ssim"]) < 1e-4 and abs(a[2]["psnr"] - b[2]["psnr"]) < 1e-4, (a[0], a[2], b[2])
        for k in range(3):
            assert torch.equal(a[1][k].cpu(), b[1][k].cpu()), (a[0], k)
    for a, b in zip(dev, one):
        assert one[0][1] is None
        assert abs(a[2]["ssim"] - b[2]["ssim"]) < 1e-4 and abs(a[2]["psnr"] - b[2]["psnr"]) < 1e-4
    for p, q, r in zip(dev_png, host_png, one_png):
        A = _png(p)
        assert A.shape == (256, 3 * 256, 3)
        np.testing.assert_array_equal(A, _png(q))
        np.testing.assert_array_equal(A, _png(r))
