"""FSRNet.testsfw / testsfw_video (train_test_GSC.py:750-838, 893-932) on the GPU over tests/golden/sfw_synth: the HIP generator + the
device scoring (csrc/sfw_kernels.h) + the device PNG encoder, against the CPU oracle of model.py pushed through the host statement
(sfw_post.py); batch sizes, all_rows and the TSM pair element give the same results; one f32x3 run."""
import io
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _cfg(out_dir):
    from blindshadowremoval_amd.fsrnet import Config
    cfg = Config(0)
    cfg.DATA_DIR_TEST = [os.path.join(GOLDEN, "sfw_synth", "*")]
    cfg.CHECKPOINT_DIR = out_dir
    return cfg


def _loop(out_dir, w, dset="sfw_gsc", rows=1, batch=16, all_rows=False, video=False, dtype="f32"):
    from blindshadowremoval_amd.dataset import Dataset
    from blindshadowremoval_amd.fsrnet import FSRNet
    cfg = _cfg(out_dir)
    ds = Dataset(cfg, "test", dset=dset, rows=rows)
    fsr = FSRNet(cfg, weights=w, dtype=dtype)
    try:
        res = (fsr.testsfw_video if video else fsr.testsfw)(ds, batch=batch, all_rows=all_rows)
        saved = list(fsr.log.saved)
    finally:
        ds.close()
        fsr.close()
    files = {os.path.basename(p): open(p, "rb").read() for p in saved}
    return res, saved, files


def _png(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def _oracle_rows(elements, w, split):
    """row 0 of each element through the CPU oracle, given the device generator's own bmask (a cell on the 0.1 threshold of model.py:256
    would otherwise flip the whole comparison): -> [(im, con_rgb, dif, face, rest)] as numpy."""
    from blindshadowremoval_amd import Generator
    from oracle.gsc_oracle import GeneratorOracle
    rows = torch.cat([torch.as_tensor(np.asarray(e), dtype=torch.float32).reshape(-1, 256, 256, sum(split))[:1] for e in elements])
    parts = torch.split(rows, list(split), dim=3)
    im, uv = parts[0], parts[1 if len(split) == 4 else 3]
    gen = Generator(device=0, dtype="f32").load_weights(w)
    gen(im.contiguous().cuda(), uv.contiguous().cuda())
    bmask = gen.probe("bmask").cpu()
    gen.close()
    with torch.no_grad():
        _, con, _, dif = GeneratorOracle(w)(im, uv, bmask_override=bmask)
    return [(im[j].numpy(), con[j].float().numpy(), dif[j].float().numpy(), parts[-1][j].numpy(), parts) for j in range(rows.shape[0])]


def test_testsfw_against_the_oracle(tmp_path):
    from blindshadowremoval_amd.dataset import Dataset
    from blindshadowremoval_amd.sfw_post import SPLIT_SFW, sfw_postprocess, strip_of
    from blindshadowremoval_amd.weights import init_weights
    w = init_weights(1)
    res, saved, files = _loop(str(tmp_path / "b16"), w)
    assert len(res) == 2 and len(files) == 2
    elements = [e[0] for e in Dataset(_cfg(str(tmp_path)), "test", dset="sfw_gsc").feed]
    orc = _oracle_rows(elements, w, SPLIT_SFW)
    for j, ((name, losses), (im, con, dif, face, parts)) in enumerate(zip(res, orc)):
        assert list(losses) == ["ssim", "psnr", "auc"]
        want, figs = sfw_postprocess(im, con, parts[2][j].numpy(), dif, face)
        print(name, losses, want)
        assert abs(losses["ssim"] - want["ssim"]) <= 1e-4 and abs(losses["psnr"] - want["psnr"]) <= 1e-4, (losses, want)
        assert abs(losses["auc"] - want["auc"]) <= 1e-6, (losses, want)
        got = _png(files[os.path.basename(saved[j])])
        assert got.shape == (256, 1024, 3)
        diff = np.abs(got.astype(np.int16) - strip_of(figs).astype(np.int16))
        assert diff[:, 768:].max() == 0 and diff[:, :256].max() == 0                  # the label and the input: exact
        assert diff.max() <= 1                                                           # con / mask_pred: the forward's ~1e-6 may cross a rounding edge
    # batching, all rows and the TSM pair element do not change a bit
    for kw in (dict(batch=1), dict(rows=10, batch=2, all_rows=True), dict(dset="sfw", batch=2)):
        r2, _, f2 = _loop(str(tmp_path / str(len(kw)) / kw.get("dset", "gsc")), w, **kw)
        assert r2 == res, kw
        assert f2 == files, kw


def test_testsfw_video_against_the_oracle(tmp_path):
    from blindshadowremoval_amd.dataset import Dataset
    from blindshadowremoval_amd.sfw_post import SPLIT_VIDEO, sfw_video_figs, strip_of
    from blindshadowremoval_amd.weights import init_weights
    w = init_weights(1)
    res, saved, files = _loop(str(tmp_path / "v"), w, dset="sfw_video", video=True, batch=2)
    assert [r[1] for r in res] == [{}, {}]
    elements = [e[0] for e in Dataset(_cfg(str(tmp_path)), "test", dset="sfw_video").feed]
    for j, (im, con, dif, face, _) in enumerate(_oracle_rows(elements, w, SPLIT_VIDEO)):
        got = _png(files[os.path.basename(saved[j])])
        diff = np.abs(got.astype(np.int16) - strip_of(sfw_video_figs(im, con, dif, face)).astype(np.int16))
        assert got.shape == (256, 768, 3) and diff[:, :256].max() == 0 and diff.max() <= 1
    r2, _, f2 = _loop(str(tmp_path / "v1"), w, dset="sfw_video", video=True, batch=1, all_rows=True)
    assert r2 == res and f2 == files


def test_testsfw_f32x3(tmp_path):
    from blindshadowremoval_amd.weights import init_weights
    w = init_weights(1)
    ref, _, _ = _loop(str(tmp_path / "f32"), w)
    res, _, files = _loop(str(tmp_path / "x3"), w, dtype="f32x3")
    assert len(files) == 2
    for (n1, a), (n2, b) in zip(ref, res):
        assert n1 == n2
        assert abs(a["ssim"] - b["ssim"]) <= 1e-3 and abs(a["psnr"] - b["psnr"]) <= 1e-3 and abs(a["auc"] - b["auc"]) <= 1e-4, (a, b)
