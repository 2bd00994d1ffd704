"""FSRNetRGB (the RGB baseline's `FSRNet.test` of train_RGB_test.py:357-505) on CPU, around a stand-in generator with GeneratorRGB's call
surface: item order, PNG names and strips, losses equal to ucb_postprocess_rgb run directly, the refusals, data-parallel world 2 over
gloo, and run_loop's --model rgb argument check.  (The product path has no CPU generator; tests/test_fsrnet_rgb_gpu.py runs the real one.)"""
import contextlib
import io
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


class StandInGeneratorRGB:
    """GeneratorRGB's call surface (con = gen(inputs, uv, reg, chuck, training)), a few torch-CPU ops per row: deterministic,
    row-independent, and outside [0, 1] in places (the composite must clip, not the prediction)."""
    _device = None
    dtype = "f32"
    _handle = 1

    def __call__(self, inputs, uv, reg=None, chuck=1, training=False):
        return inputs * 1.3 - uv * 0.2 + 0.05

    def close(self):
        pass


def _config(out_dir):
    from blindshadowremoval_amd.fsrnet import Config
    cfg = Config(0)
    cfg.CHECKPOINT_DIR = out_dir
    cfg.DATA_DIR_TEST = [os.path.join(GOLDEN, "UCB", "train", "input", "*")]
    cfg.UCB_MASK_ROOT = os.path.join(GOLDEN, "UCB_masks")
    return cfg


def _run(out_dir, n, batch=4):
    from blindshadowremoval_amd.dataset import Dataset
    from blindshadowremoval_amd.fsrnet import FSRNetRGB
    cfg = _config(out_dir)
    ds = Dataset(cfg, "test", ucb=True)
    ds.name_list = ds.name_list[:n]
    fsr = FSRNetRGB(cfg, gen=StandInGeneratorRGB())
    fsr.post_threads = 2
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        res = fsr.test(ds, batch=batch)
    fsr.log.close()
    return fsr, res, list(ds.name_list), buf.getvalue()


def test_rgb_loop_over_golden_items_matches_the_host_statement(tmp_path):
    from blindshadowremoval_amd.dataset import Dataset
    from blindshadowremoval_amd.fsrnet import FSRNet
    from blindshadowremoval_amd.pngio import read_rgb_u8
    from blindshadowremoval_amd.ucb_post import read_masks
    from blindshadowremoval_amd.ucb_post_rgb import strip_of, ucb_postprocess_rgb
    n = 6
    fsr, res, names, out = _run(str(tmp_path), n, batch=4)
    assert [r[0] for r in res] == [str(x) for x in names]                        # item order = list order, over a ragged last batch
    assert "Testing %d/%d" % (n, n) in out and "ssim:" in out and "psnr:" in out
    assert [a for a, _ in fsr.all_losses] == [r[0] for r in res]
    masks = FSRNet._ucb_masks(fsr)
    cfg = _config(str(tmp_path))
    ds = Dataset(cfg, "test", ucb=True)
    gen = StandInGeneratorRGB()
    for step, (name, figs, losses) in enumerate(res):
        img, box = next(ds.feed)[:2]
        rows = torch.as_tensor(np.asarray(img), dtype=torch.float32).reshape(-1, 256, 256, 16)[:1]
        im, gt, uv = rows[..., 0:3], rows[..., 3:6], rows[..., 6:9]
        con = gen(im, uv)[0].numpy()
        fh = read_masks({"face_hair": masks[step]["face_hair"]}, grey=True)["face_hair"]
        want_l, want_f = ucb_postprocess_rgb(im[0].numpy(), gt[0].numpy(), con, np.asarray(box, np.float32).reshape(-1)[:4], fh)
        assert losses == want_l, name
        assert len(figs) == 3
        for a, b in zip(figs, want_f):
            np.testing.assert_array_equal(a.numpy(), b)
        parts = name.replace("\\", "/").split("/")
        path = os.path.join(str(tmp_path), "test", parts[-2] + "_" + parts[-1].split(".")[0] + "-result.png")
        assert path in fsr.log.saved and os.path.isfile(path)
        np.testing.assert_array_equal(read_rgb_u8(path), strip_of(want_f))
    assert len(os.listdir(os.path.join(str(tmp_path), "test"))) == n


def test_refusals(tmp_path):
    from blindshadowremoval_amd.fsrnet import FSRNet, FSRNetRGB
    from blindshadowremoval_amd.model import Generator, GeneratorRGB, GeneratorTSM
    cfg = _config(str(tmp_path))
    with pytest.raises(ValueError, match="f32"):
        FSRNetRGB(cfg, dtype="f16", gen=StandInGeneratorRGB())
    with pytest.raises(ValueError, match="f32"):
        FSRNetRGB(cfg, dtype="f32x3")
    with pytest.raises(TypeError, match="FSRNet\\b"):
        FSRNetRGB(cfg, gen=Generator())
    with pytest.raises(TypeError, match="FSRNetTSM"):
        FSRNetRGB(cfg, gen=GeneratorTSM())
    with pytest.raises(TypeError, match="FSRNetRGB"):
        FSRNet(cfg, gen=GeneratorRGB())
    fsr = FSRNetRGB(cfg, gen=StandInGeneratorRGB())
    with pytest.raises(NotImplementedError, match="testFFHQ"):
        fsr.testFFHQ(None)


def test_run_loop_rgb_takes_only_the_ucb_loop_in_f32(capsys):
    from blindshadowremoval_amd.run_loop import main
    assert main(["--model", "rgb", "--loop", "ffhq", "--data", "x/*", "--checkpoint-dir", "unused"]) == 2
    assert "--loop ucb" in capsys.readouterr().err
    assert main(["--model", "rgb", "--loop", "ucb", "--dtype", "f16", "--data", "x/*", "--checkpoint-dir", "unused"]) == 2


def _worker(rank, world, port, out_dir, n, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["LOCAL_WORLD_SIZE"] = str(world)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        fsr, res, _, out = _run(out_dir, n, batch=2)
        q.put((rank, {"names": [r[0] for r in res], "all_losses": [(a, dict(b)) for a, b in fsr.all_losses], "saved": list(fsr.log.saved),
                      "means": {k: v[0] / max(v[1], 1) for k, v in fsr.log.losses.items()}}))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_world2_all_losses_equal_world1(tmp_path):
    n = 5
    single, res, _, _ = _run(str(tmp_path / "single"), n, batch=2)
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, str(tmp_path / "dp"), n, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=300) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    want = [(a, dict(b)) for a, b in single.all_losses]
    assert len(want) == n
    assert got[0]["names"] + got[1]["names"] == [r[0] for r in res]
    for r in (0, 1):
        assert got[r]["all_losses"] == want
        assert got[r]["means"] == {k: v[0] / max(v[1], 1) for k, v in single.log.losses.items()}
    want_png = {os.path.basename(p): open(p, "rb").read() for p in single.log.saved}
    seen = {os.path.basename(p): open(p, "rb").read() for r in (0, 1) for p in got[r]["saved"]}
    assert seen == want_png
