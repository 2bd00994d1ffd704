"""The device PNG scanline reconstruction (bsr_png_unfilter, csrc/prep_kernels.h) at the geometries the other tests leave out, and the
ring path that feeds it (prep.host_part_ring -> DevicePrep.rows_ex, the loader end to end) against the pipe path over the corpus of
tests/ring_corpus.py: tall, short, narrow and wide images, grey / RGBA / palette / 16-bit files, masks in every form, corrupt files.
Kernel output is compared with pngio.unfilter_host bit for bit; ring rows with pipe rows by torch.equal."""
import os

import numpy as np
import pytest

import ring_corpus as RC
from unfilter_cases import filter_rows, run_unfilter

pytestmark = pytest.mark.gpu


def _rgb(img: np.ndarray) -> np.ndarray:
    c = img.shape[2]
    return img if c == 3 else (np.repeat(img, 3, axis=2) if c == 1 else img[:, :, :3])


def _check(img: np.ndarray, fts, grey: bool = False) -> None:
    from blindshadowremoval_amd import pngio
    h, w, c = img.shape
    raw = filter_rows(img, fts)
    np.testing.assert_array_equal(pngio.unfilter_host(raw, h, w, c), img)
    out = run_unfilter([(raw, h, w, c)], grey=grey)[0]
    np.testing.assert_array_equal(out, img if grey else _rgb(img))


@pytest.mark.parametrize("w", [1024, 2048, 5461])
def test_256_rows_of_long_scanlines(w):
    """h = 256 (every thread of the workgroup owns a row) at 3 to 16 KB per scanline: thousands of anti-diagonal steps."""
    rng = np.random.RandomState(w)
    img = rng.randint(0, 256, (256, w, 3)).astype(np.uint8)
    img[:, w // 3:w // 2] = img[:, w // 3:w // 3 + 1]
    _check(img, rng.randint(0, 5, 256))


@pytest.mark.parametrize("w,c", [(4, 1), (1, 4)])
@pytest.mark.parametrize("h", [1, 2, 255, 256])
def test_scanlines_of_exactly_one_dword(h, w, c):
    """w c = 4, the narrowest scanline the kernel takes (prep._layout_ex refuses w c < 4): one group of four pixels or one pixel."""
    rng = np.random.RandomState(h * 10 + w)
    _check(rng.randint(0, 256, (h, w, c)).astype(np.uint8), np.arange(h) % 5)


@pytest.mark.parametrize("S", [4, 5, 37, 255, 256])
def test_grey_output_masks(S):
    """The masks' form (grey_out: one byte per pixel) at S = 4 (the smallest raw8 masks) up to 256, odd sizes between."""
    rng = np.random.RandomState(S)
    m = (rng.rand(S, S, 1) < 0.4).astype(np.uint8) * 255
    m[S // 2:] = rng.randint(0, 256, (S - S // 2, S, 1))
    for fts in (np.arange(S) % 5, rng.randint(0, 5, S)):
        _check(m, fts, grey=True)


def _decisive_paeth_ties(img: np.ndarray, fts) -> tuple:
    """Pixels of Paeth rows where the predictor's <= order decides: pa == pc (a chosen over c, a != c) and pb == pc < pa (b chosen
    over c, b != c) — a kernel that broke those ties the other way would reconstruct a different byte there."""
    h, w, c = img.shape
    x = img.reshape(h, w * c).astype(np.int32)
    a = np.zeros_like(x); a[:, c:] = x[:, :-c]
    b = np.zeros_like(x); b[1:] = x[:-1]
    cc = np.zeros_like(x); cc[1:, c:] = x[:-1, :-c]
    p = a + b - cc
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - cc)
    rows = (np.asarray(fts) == 4)[:, None]
    return int((rows & (pa == pc) & (pa <= pb) & (a != cc)).sum()), int((rows & (pb == pc) & (pb < pa) & (b != cc)).sum())


@pytest.mark.parametrize("c", [1, 3, 4])
def test_every_filter_type_per_row_with_paeth_ties(c):
    """Rows cycling through filter types 0-4 (and runs of one type) over content of few levels, near 0 and near 255: the Paeth
    predictor's ties are frequent and decisive, and the modulo-256 sums wrap."""
    rng = np.random.RandomState(40 + c)
    h, w = 120, 67
    img = (rng.randint(0, 4, (h, w, c)) + np.where(rng.rand(h, w, c) < 0.5, 0, 252)).astype(np.uint8)
    img[h // 2:] = rng.randint(0, 6, (h - h // 2, w, c)).astype(np.uint8)
    for fts in (np.arange(h) % 5, np.repeat(np.arange(5), (h + 4) // 5)[:h], np.full(h, 4)):
        ac, bc = _decisive_paeth_ties(img, fts)
        assert ac > 0 and bc > 0, (ac, bc)
        _check(img, fts)


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    return RC.make_corpus(str(tmp_path_factory.mktemp("ring_corpus_gpu")))


def _masks_equal(a, b, dev) -> bool:
    import torch
    from blindshadowremoval_amd import prep
    return torch.equal(prep.unpack_masks([a], dev), prep.unpack_masks([b], dev))


def test_mixed_batch_through_rows_ex(corpus):
    """Every non-corrupt corpus item in ONE batch of ring records (SlotRing, device reconstruction on; the items that overflow a slot
    come back as pipe tuples) against the same items as host_part tuples: identical rows, boxes, names and masks — and once more
    with ring records and pipe tuples alternating."""
    import torch
    from blindshadowremoval_amd import prep
    n = len(RC.GOOD)
    ring = prep.SlotRing(n + 2)
    try:
        slots = [(3 + k) % (n + 2) for k in range(n)]
        recs = [prep.host_part_ring(RC.job(corpus, nm), (ring.path, s, ring.cap, True)) for nm, s in zip(RC.GOOD, slots)]
        pipes = [prep.host_part(RC.job(corpus, nm)) for nm in RC.GOOD]
        assert [prep._is_ring(r) for r in recs] == [RC.BRANCH[nm] != "pipe" for nm in RC.GOOD]
        assert {r[11] for r in recs if prep._is_ring(r)} >= {(3, 3), (0, 0), (1, 1), (4, 4), (4, 3), (0, 3), (3, 1)}
        dp = prep.DevicePrep(0, 256)
        dp.ring = ring
        dev = torch.device("cuda", 0)
        ref_rows, ref_boxes, ref_masks, ref_names = dp.rows_ex(pipes)
        mixed = [r if k % 2 else p for k, (r, p) in enumerate(zip(recs, pipes))]
        for parts in (recs, mixed):
            rows, boxes, masks, names = dp.rows_ex(parts)
            torch.cuda.synchronize()
            assert torch.equal(rows, ref_rows) and np.array_equal(boxes, ref_boxes) and names == ref_names
            assert float(rows[:, :, :, 0:6].double().sum()) > 0
            for nm, m, rm, p in zip(RC.GOOD, masks, ref_masks, parts):
                assert (m[0].startswith("dev_")) == prep._is_ring(p), nm
                assert _masks_equal(m, rm, dev), nm
        torch.cuda.synchronize()
    finally:
        prep._RING_VIEWS.pop(ring.path, None)
        ring.close()


def _dataset(names, corpus):
    from blindshadowremoval_amd import dataset as D
    from blindshadowremoval_amd.fsrnet import Config
    cfg = Config(0)
    cfg.DATA_DIR_TEST = [os.path.dirname(corpus["plain"][0])]
    ds = D.Dataset(cfg, "test", ucb=True, workers=3, device_prep=0, device_batch=8)
    ds.name_list = [corpus[nm][0] for nm in names]
    ds.ucb_mask_files = [corpus[nm][2] for nm in names]
    return ds


def test_loader_end_to_end_ring_and_pipe(corpus, monkeypatch):
    """The device-prepared UCB loader over the corpus (twice over, 28 items in batches of 8): through the ring with the device
    reconstruction (the UCB loop's default), and through the workers' pipes (BSR_LOADER_RING=0) — identical row sums, boxes, names and
    masks.  A list holding a corrupt file fails on both paths with the worker's error, in the second batch, after the first batch was
    delivered: the corrupt item never reaches a batch, so its bytes never reach the kernel."""
    import torch
    from blindshadowremoval_amd import prep
    monkeypatch.delenv("BSR_DEVICE_UNFILTER", raising=False)
    names = list(RC.GOOD) * 2
    dev = torch.device("cuda", 0)

    def run(ring: bool, items):
        monkeypatch.setenv("BSR_LOADER_RING", "1" if ring else "0")
        ds = _dataset(items, corpus)
        ds.warm()
        try:
            assert (getattr(ds, "_ring", None) is not None) == ring
            got = []
            for el in ds.feed:
                got.append((el[0].double().sum(dim=(0, 1, 2, 3)).cpu(), el[1], el[2][0], el[3][0],
                            prep.unpack_masks([el[3]], dev).cpu()))
            return got
        finally:
            ds.close()
    a, b = run(True, names), run(False, names)
    assert len(a) == len(b) == len(names)
    for nm, x, y in zip(names, a, b):
        assert torch.equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and x[2] == y[2] and torch.equal(x[4], y[4]), nm
        assert x[3].startswith("dev_") == (RC.BRANCH[nm] != "pipe") and not y[3].startswith("dev_"), (nm, x[3], y[3])
    for bad in RC.BAD:
        items = list(RC.GOOD[:10]) + [bad] + list(RC.GOOD[10:])
        for ring in (True, False):
            monkeypatch.setenv("BSR_LOADER_RING", "1" if ring else "0")
            ds = _dataset(items, corpus)
            ds.warm()
            seen = []
            try:
                with pytest.raises(RuntimeError, match="loader worker failed"):
                    for el in ds.feed:
                        seen.append(el[2][0])
            finally:
                ds.close()
            assert seen == [corpus[nm][1].encode() for nm in items[:8]], (bad, ring, len(seen))
    torch.cuda.synchronize()
