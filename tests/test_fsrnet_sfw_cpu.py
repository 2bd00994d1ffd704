"""FSRNet.testsfw / testsfw_video (the GSC model's SFW evaluation, /root/reference/train_test_GSC.py:750-838, 893-932) on CPU, around a
stand-in generator with Generator's call surface, over tests/golden/sfw_synth: losses and strips equal to sfw_post.py run directly,
batching and all_rows invariance, the TSM pair element, and the refusals (FSRNetRGB, data-parallel, run_loop's arguments).  (The product
path has no CPU generator; tests/test_fsrnet_sfw_gpu.py runs the real one.)"""
import contextlib
import hashlib
import io
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


class StandInGenerator:
    """Generator's call surface ((gs, con_rgb, mask22, dif) = gen(inputs, uv, reg, chuck, training)), row-independent torch-CPU ops: con
    leaves [0, 1] in places, dif is negative in places (-0.0 products outside the face)."""
    _device = None
    dtype = "f32"
    _handle = 1

    def __call__(self, inputs, uv, reg=None, chuck=1, training=False):
        con = inputs * 1.2 - uv * 0.1 + 0.02
        dif = inputs.mean(dim=3, keepdim=True) - 0.4 + uv[..., :1] * 0.05
        return con.mean(dim=3, keepdim=True), con, dif, dif

    def close(self):
        pass


def _cfg(out_dir):
    from blindshadowremoval_amd.fsrnet import Config
    cfg = Config(0)
    cfg.CHECKPOINT_DIR = out_dir
    cfg.DATA_DIR_TEST = [os.path.join(GOLDEN, "sfw_synth", "*")]
    return cfg


def _run(out_dir, dset="sfw_gsc", rows=1, batch=16, all_rows=False, video=False):
    from blindshadowremoval_amd.dataset import Dataset
    from blindshadowremoval_amd.fsrnet import FSRNet
    cfg = _cfg(out_dir)
    ds = Dataset(cfg, "test", dset=dset, rows=rows)
    fsr = FSRNet(cfg, gen=StandInGenerator())
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        res = (fsr.testsfw_video if video else fsr.testsfw)(ds, batch=batch, all_rows=all_rows)
    fsr.log.close()
    files = sorted(os.listdir(os.path.join(out_dir, "test")))
    digests = {f: hashlib.sha256(open(os.path.join(out_dir, "test", f), "rb").read()).hexdigest() for f in files}
    return fsr, res, list(ds.name_list), buf.getvalue(), digests


def test_testsfw_matches_the_host_statement(tmp_path):
    from PIL import Image
    from blindshadowremoval_amd.dataset import Dataset
    from blindshadowremoval_amd.sfw_post import sfw_postprocess, strip_of
    fsr, res, names, out, digests = _run(str(tmp_path), batch=2)
    assert [r[0] for r in res] == [str(n) for n in names] and len(res) == 2
    assert "Testing 2/2" in out and "ssim:" in out and "psnr:" in out and "auc:" in out
    assert fsr.all_losses == res
    gen = StandInGenerator()
    ds = Dataset(_cfg(str(tmp_path)), "test", dset="sfw_gsc")
    for (name, losses), (img, box, _) in zip(res, ds.feed):
        r0 = torch.from_numpy(img[0, :1])
        im, mask, uv, face = r0[..., 0:3], r0[..., 6:7], r0[..., 7:10], r0[..., 16:17]
        _, con, _, dif = gen(im, uv)
        want, figs = sfw_postprocess(im[0].numpy(), con[0].numpy(), mask[0].numpy(), dif[0].numpy(), face[0].numpy())
        assert losses == want
        assert 0.0 < losses["auc"] < 1.0
        png = fsr.log._png_path(name)
        assert os.path.isfile(png)
        np.testing.assert_array_equal(np.asarray(Image.open(png).convert("RGB")), strip_of(figs))


def test_testsfw_batching_and_all_rows_do_not_change_results(tmp_path):
    _, r1, _, _, d1 = _run(str(tmp_path / "b1"), batch=1)
    _, r2, _, _, d2 = _run(str(tmp_path / "b2"), batch=2)
    _, r3, _, _, d3 = _run(str(tmp_path / "all"), rows=3, batch=2, all_rows=True)
    _, r4, _, _, d4 = _run(str(tmp_path / "pair"), dset="sfw", batch=2)             # the TSM pair: row 0 is the same
    assert r1 == r2 == r3 == r4
    assert d1 == d2 == d3 == d4 and len(d1) == 2


def test_testsfw_video(tmp_path):
    from PIL import Image
    from blindshadowremoval_amd.dataset import Dataset
    from blindshadowremoval_amd.sfw_post import sfw_video_figs, strip_of
    fsr, res, names, out, d1 = _run(str(tmp_path / "v1"), dset="sfw_video", batch=1, video=True)
    _, res2, _, _, d2 = _run(str(tmp_path / "v2"), dset="sfw_video", batch=2, video=True, all_rows=True)
    assert res == res2 == [(str(n), {}) for n in names] and d1 == d2
    gen = StandInGenerator()
    img = next(Dataset(_cfg(str(tmp_path)), "test", dset="sfw_video").feed)[0]
    r0 = torch.from_numpy(img[0, :1])
    im, uv, face = r0[..., 0:3], r0[..., 3:6], r0[..., 12:13]
    _, con, _, dif = gen(im, uv)
    want = strip_of(sfw_video_figs(im[0].numpy(), con[0].numpy(), dif[0].numpy(), face[0].numpy()))
    got = np.asarray(Image.open(fsr.log._png_path(res[0][0])).convert("RGB"))
    assert got.shape == (256, 768, 3)
    np.testing.assert_array_equal(got, want)


def test_test_step_sfw_returns_the_reference_figures(tmp_path):
    from blindshadowremoval_amd.dataset import Dataset
    from blindshadowremoval_amd.fsrnet import FSRNet
    cfg = _cfg(str(tmp_path))
    fsr = FSRNet(cfg, gen=StandInGenerator())
    img, box, _ = next(Dataset(cfg, "test", dset="sfw_gsc", rows=2).feed)
    losses, figs = fsr.test_step_sfw(img, box, training=False)
    losses2, figs2 = fsr.test_step_sfw(img, box, training=False, all_rows=True)
    assert list(losses) == ["ssim", "psnr", "auc"] and losses == losses2
    assert [tuple(f.shape) for f in figs] == [(1, 256, 256, 3), (1, 256, 256, 3), (1, 256, 256, 1), (1, 256, 256, 1)]
    np.testing.assert_array_equal(figs[3].numpy(), (img[0, :1, ..., 6:7] == 2).astype(np.float32))
    for a, b in zip(figs, figs2):
        np.testing.assert_array_equal(a.numpy(), b.numpy())
    with pytest.raises(ValueError):
        fsr.test_step_sfw(np.zeros((1, 1, 256, 256, 16), np.float32))                # a UCB / FFHQ element is not an SFW one
    fsr.log.close()


def test_refusals(tmp_path, monkeypatch):
    from blindshadowremoval_amd import run_loop
    from blindshadowremoval_amd.fsrnet import FSRNet, FSRNetRGB
    cfg = _cfg(str(tmp_path))
    rgb = FSRNetRGB.__new__(FSRNetRGB)
    for fn in (lambda: rgb.testsfw(None), lambda: rgb.testsfw_video(None), lambda: rgb.test_step_sfw(None)):
        with pytest.raises(NotImplementedError):
            fn()
    fsr = FSRNet(cfg, gen=StandInGenerator())
    with pytest.raises(ValueError):
        fsr.testsfw(type("D", (), {"name_list": [], "feed": iter(())})(), batch=0)
    import blindshadowremoval_amd.dist as dist
    monkeypatch.setattr(dist, "rank_world", lambda group=None: (0, 2))
    with pytest.raises(NotImplementedError):
        fsr.testsfw(type("D", (), {"name_list": [], "feed": iter(())})())
    monkeypatch.undo()
    fsr.log.close()
    err = io.StringIO()
    with contextlib.redirect_stderr(err):
        for loop in ("sfw", "sfw_video"):
            assert run_loop.main(["--model", "rgb", "--loop", loop, "--data", "x", "--checkpoint-dir", str(tmp_path)]) == 2
        monkeypatch.setenv("WORLD_SIZE", "2")
        assert run_loop.main(["--loop", "sfw", "--data", "x", "--checkpoint-dir", str(tmp_path)]) == 2
    assert "--loop sfw runs in one process" in err.getvalue() and "--model rgb" in err.getvalue()
