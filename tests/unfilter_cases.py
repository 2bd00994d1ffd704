"""Helpers of the PNG scanline reconstruction tests (tests/test_unfilter_gpu.py, tests/test_ring_decode_edges_gpu.py): the forward
filters of RFC 2083 section 6 in numpy, and one launch of bsr_png_unfilter over a blob built the way prep._layout_ex builds it —
16 readable bytes in front of and behind every filtered image (csrc/prep_kernels.h kUnfilterSlack)."""
import numpy as np


def filter_rows(img: np.ndarray, fts) -> np.ndarray:
    """uint8 [h,w,c] + one filter type per row -> the filtered scanlines a PNG encoder would deflate (RFC 2083 section 6)."""
    h, w, c = img.shape
    x = img.reshape(h, w * c).astype(np.int32)
    out = np.zeros((h, 1 + w * c), np.uint8)
    zero = np.zeros(w * c, np.int32)
    for y in range(h):
        cur, up = x[y], (x[y - 1] if y else zero)
        a = np.concatenate([np.zeros(c, np.int32), cur[:-c]])
        ul = np.concatenate([np.zeros(c, np.int32), up[:-c]])
        ft = int(fts[y])
        if ft == 0:
            pred = zero
        elif ft == 1:
            pred = a
        elif ft == 2:
            pred = up
        elif ft == 3:
            pred = (a + up) >> 1
        else:
            p = a + up - ul
            pa, pb, pc = np.abs(p - a), np.abs(p - up), np.abs(p - ul)
            pred = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, up, ul))
        out[y, 0] = ft
        out[y, 1:] = (cur - pred) & 255
    return out


def run_unfilter(items, grey=False):
    """items: [(raw uint8 [h, 1 + w c], h, w, c)] -> the RGB8 images the kernel wrote (grey: c = 1 images as one byte per pixel)."""
    import torch
    from blindshadowremoval_amd import _lib, prep
    lib = _lib.load()
    tab = np.zeros(len(items), prep.UNFILTER_DTYPE)
    off = ((tab.nbytes + 7) & ~7) + 16                     # (16 readable bytes in front of the first image; the output areas follow the last)
    for k, (raw, h, w, c) in enumerate(items):
        assert raw.size == h * (1 + w * c) and 1 <= h <= prep.UNFILTER_MAX_ROWS and w * c >= 4 and c in (1, 3, 4) and (c == 1 or not grey)
        tab[k] = (off, 0, h, w, c, 1 if grey else 0)
        off = (off + raw.size + 7) & ~7
    off += 16                                              # ... and 16 behind the last, however small the output areas are
    for k, (raw, h, w, c) in enumerate(items):
        tab[k]["out_off"] = off
        off = (off + h * w * (1 if grey else 3) + 7) & ~7
    blob = np.full(off, 0xA5, np.uint8)
    blob[:tab.nbytes] = tab.view(np.uint8)
    for k, (raw, h, w, c) in enumerate(items):
        blob[tab[k]["raw_off"]:tab[k]["raw_off"] + raw.size] = raw.reshape(-1)
    d = torch.from_numpy(blob).cuda()
    _lib.check(lib.bsr_png_unfilter(0, d.data_ptr(), d.numel(), 0, len(items), torch.cuda.current_stream().cuda_stream), "bsr_png_unfilter")
    torch.cuda.synchronize()
    res = d.cpu().numpy()
    ob = 1 if grey else 3
    return [res[t["out_off"]:t["out_off"] + t["h"] * t["w"] * ob].reshape(t["h"], t["w"], ob) for t in tab]
