"""Device-side input preparation (blindshadowremoval_amd/prep.py + csrc/prep_kernels.h) against the fixtures that pin the host
path: tests/golden/sample_02165.npz — produced by the REFERENCE's own `face_crop_and_resize` / `generate_face_region` /
`generate_uv_map` / `generate_offset_map` (tools/make_sample_fixture.py) — and the host `build_row` (itself pinned to that fixture) on
the UCB items.  CPU: the host half (crop box, triangle tables) through a numpy emulation of the kernel's arithmetic.  GPU: the kernel."""
import os

import numpy as np
import pytest

from blindshadowremoval_amd import dataset as D
from blindshadowremoval_amd import prep
from prep_cases import culled_winner as _culled_winner, emulate


def _sample_part(golden_dir, size=256):
    base = os.path.join(golden_dir, "sample_imgs", "02165", "02165")
    return prep.host_part((base + ".npy", None, size))


def test_host_half_and_kernel_arithmetic_reproduce_the_reference_fixture(golden_dir):
    z = np.load(os.path.join(golden_dir, "sample_02165.npz"))
    part = _sample_part(golden_dir)
    assert np.array_equal(part[2].astype(np.float32), z["box"].reshape(-1)[:4])
    row = emulate(part, 256)
    err = np.abs(row - z["row"]).max(axis=(0, 1))
    assert err.max() <= 1e-6, err
    assert [t.shape[1] for t in part[3]] == [prep.TRI_DOUBLES] * 4 and all(0 < t.shape[0] <= prep.MAX_TRI for t in part[3])


def test_blob_layout(golden_dir):
    part = _sample_part(golden_dir)
    blob, rows_off, grid_off = prep.pack_batch([part, part], 256)
    rows = np.frombuffer(blob, prep.ROW_DTYPE, count=2, offset=rows_off)
    assert rows_off % 8 == 0 and grid_off % 8 == 0 and all(int(o) % 8 == 0 for r in rows for o in r["tri_off"])
    assert np.array_equal(np.frombuffer(blob, "<f8", count=256, offset=grid_off), np.linspace(0, 1, 256))
    r = rows[1]
    img = np.frombuffer(blob, np.uint8, count=int(r["h"]) * int(r["w"]) * 3, offset=int(r["img_off"])).reshape(int(r["h"]), int(r["w"]), 3)
    assert np.array_equal(img, part[0]) and r["gt_off"] == r["img_off"]
    t0 = np.frombuffer(blob, "<f8", count=int(r["ntri"][0]) * 18, offset=int(r["tri_off"][0])).reshape(-1, 18)
    assert np.array_equal(t0, part[3][0])


@pytest.mark.gpu
def test_device_rows_match_the_reference_fixture_and_the_host_path(golden_dir):
    import glob
    import torch
    z = np.load(os.path.join(golden_dir, "sample_02165.npz"))
    dp = prep.DevicePrep(0, 256)
    parts = [_sample_part(golden_dir)]
    ucb = sorted(glob.glob(os.path.join(golden_dir, "UCB", "train", "input", "*", "*.npy")), key=D.natural_key)
    assert len(ucb) == 100
    ucb = ucb[::4]                                    # every fourth item: 25 of the 100, all subjects
    host_rows = [z["row"]]
    for lm_path in ucb:
        parts_gt = lm_path.replace("\\", "/").split("/")
        gt = os.path.splitext("/".join(parts_gt[:-3] + ["gt"] + parts_gt[-2:]))[0] + ".png"
        parts.append(prep.host_part((lm_path, gt, 256)))
        host_rows.append(D.build_row(os.path.splitext(lm_path)[0] + ".png", lm_path, gt, 256)[0])
    out, boxes = dp.rows(parts)
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert out.shape == (len(parts), 256, 256, 16) and np.array_equal(boxes[0], z["box"].reshape(-1)[:4])
    for i, ref in enumerate(host_rows):
        err = np.abs(out[i] - ref).max(axis=(0, 1))
        assert np.isfinite(out[i]).all() and err.max() <= 1e-6, (i, err)


def _border_case(tmp_path):
    """A synthetic image whose landmarks hug the top-left corner: the crop box leaves the image on two sides (zero extension,
    utils.py:414-425)."""
    from PIL import Image
    rng = np.random.default_rng(5)
    img = (rng.random((200, 240, 3)) * 255).astype(np.uint8)
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sample_02165.npz"))
    lm0 = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sample_imgs", "02165", "02165.npy")).astype(np.float32)
    lm = (lm0 - lm0.min(0)) * 0.55 + np.float32(4.0)            # face squeezed into the corner: box starts at negative coordinates
    base = os.path.join(str(tmp_path), "corner")
    Image.fromarray(img).save(base + ".png")
    np.save(base + ".npy", lm)
    return base


def test_zero_extended_crop_matches_the_host_path(tmp_path):
    base = _border_case(tmp_path)
    part = prep.host_part((base + ".npy", None, 256))
    assert part[2][0] < 0 and part[2][1] < 0                      # the box really leaves the image
    row_host, box_host = D.build_row(base + ".png", base + ".npy", None, 256)
    assert np.array_equal(part[2].astype(np.float32), box_host)
    err = np.abs(emulate(part, 256) - row_host).max(axis=(0, 1))
    assert err.max() <= 1e-6, err


@pytest.mark.gpu
def test_device_zero_extended_crop(tmp_path):
    import torch
    base = _border_case(tmp_path)
    row_host, _ = D.build_row(base + ".png", base + ".npy", None, 256)
    out, _ = prep.DevicePrep(0, 256).rows([prep.host_part((base + ".npy", None, 256))])
    torch.cuda.synchronize()
    err = np.abs(out[0].cpu().numpy() - row_host).max(axis=(0, 1))
    assert err.max() <= 1e-6, err


def test_block_culling_keeps_every_winner(golden_dir, tmp_path):
    """Round 5: a workgroup of prep_rows_kernel walks only the triangles whose edge functions can reach -1e-9 somewhere on its 16x16-pixel
    block.  For every block of every mesh of the sample and of the corner case: wherever the full search finds a triangle `inside`
    (>= -1e-12), the culled search finds THE SAME triangle; where it finds none, neither does the culled one — the two cases the
    kernel's outputs depend on.  And the point of it: a block walks a small fraction of the mesh."""
    size = 256
    lin = np.linspace(0, 1, size)
    px, py = np.meshgrid(lin, lin)
    corner = prep.host_part((_border_case(tmp_path) + ".npy", None, size))
    walked, total = 0, 0
    for part in (_sample_part(golden_dir), corner):
        for t in part[3]:
            l = np.stack([(t[:, 3 * i][:, None, None] * px + t[:, 3 * i + 1][:, None, None] * py) + t[:, 3 * i + 2][:, None, None] for i in range(3)], 0).min(0)
            full_best = l.argmax(0)
            full_l = np.take_along_axis(l, full_best[None], 0)[0]
            for by in range(size // 16):
                for bx in range(size // 16):
                    cb, cl, n = _culled_winner(t, lin, by, bx)
                    sl = (slice(by * 16, by * 16 + 16), slice(bx * 16, bx * 16 + 16))
                    inside = full_l[sl] >= -1e-12
                    assert np.array_equal(cb[inside], full_best[sl][inside])
                    assert np.array_equal(cl >= -1e-12, inside)
                    walked += n
                    total += t.shape[0]
    assert walked < 0.2 * total, (walked, total)


@pytest.mark.gpu
@pytest.mark.parametrize("size", [64, 128])
def test_device_rows_at_other_sizes_match_the_host_path(golden_dir, size):
    """The block mapping of the kernel (16x16 pixels per workgroup, S / 16 blocks per row) at other S than the reference's 256."""
    import torch
    base = os.path.join(golden_dir, "sample_imgs", "02165", "02165")
    row_host, _ = D.build_row(base + ".png", base + ".npy", None, size)
    out, _ = prep.DevicePrep(0, size).rows([prep.host_part((base + ".npy", None, size))])
    torch.cuda.synchronize()
    got = out[0].cpu().numpy()
    assert got.shape == (size, size, 16)
    err = np.abs(got - row_host).max(axis=(0, 1))
    assert err.max() <= 1e-6, err
