"""A corpus of UCB items for the loader's ring path (prep.host_part_ring) at its edges, made by transforming the golden item
9156-004 (photograph, landmarks, ground truth, seven masks): tall, short, narrow and wide canvases, grey / RGBA / palette / 16-bit
files, a ground truth of another PNG kind than its input, masks in every form prep.pack_masks gives, and two files with an undefined
filter-type byte.  The crop box comes from the landmarks alone, so the 256 x 256 photograph can sit at the top-left of any canvas.

Each item names the branch host_part_ring takes with the device reconstruction on (RING_CAP slots): ("ring", rawc, mask kind) for
a ring record — rawc = channels per filtered pixel of image and ground truth, 0 = decoded in the worker — or "pipe" for an item
that overflows its slot and comes back as a host_part tuple; "error" for a file both paths must refuse."""
import os
import struct
import zlib

import numpy as np

from ucb_cases import GOLDEN

SRC = "9156-004"
FOLDER = "9156"

#        name               image        gt            masks        branch
ITEMS = (("plain",          "rgb",       "rgb",        "grey",      ("ring", (3, 3), "raw8")),
         ("tall_300x256",   "tall256",   "tall256",    "grey",      ("ring", (0, 0), "raw8")),
         ("tall_300x300",   "tall300",   "tall300",    "grey",      "pipe"),
         ("tall_bits",      "tall300",   "tall300",    "rgb",       ("ring", (0, 0), "bits")),
         ("short_200",      "short",     "short",      "grey",      ("ring", (3, 3), "raw8")),
         ("narrow_grey3",   "narrow3",   "narrow3",    "grey",      ("ring", (0, 0), "raw8")),
         ("narrow_rgba1",   "narrow1a",  "narrow1a",   "grey",      ("ring", (4, 4), "raw8")),
         ("wide_fits",      "wide320",   "wide320",    "grey",      ("ring", (3, 3), "raw8")),
         ("wide_overflows", "wide400",   "wide400",    "grey",      "pipe"),
         ("grey",           "L",         "L",          "palette",   ("ring", (1, 1), "bits")),
         ("rgba",           "RGBA",      "rgb",        "levels",    ("ring", (4, 3), "raw8")),
         ("palette",        "P",         "rgb",        "grey",      ("ring", (0, 3), "raw8")),
         ("deep16",         "rgb16",     "rgb16",      "grey",      ("ring", (0, 0), "raw8")),
         ("gt_grey",        "rgb",       "L",          "rgb_levels", ("ring", (3, 1), "u8")),
         ("bad_photo",      "bad",       "rgb",        "grey",      "error"),
         ("bad_mask",       "rgb",       "rgb",        "bad",       "error"))
GOOD = tuple(it[0] for it in ITEMS if it[4] != "error")
BAD = tuple(it[0] for it in ITEMS if it[4] == "error")
BRANCH = {it[0]: it[4] for it in ITEMS}


def _png(raw: np.ndarray, w: int, h: int, depth: int, ctype: int) -> bytes:
    """A PNG file of already filtered scanlines (a filter-type byte first on every row), one IDAT chunk, correct CRCs."""
    from blindshadowremoval_amd.pngio import _SIGNATURE, _chunk
    return b"".join((_SIGNATURE, _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ctype, 0, 0, 0)),
                     _chunk(b"IDAT", zlib.compress(np.ascontiguousarray(raw).tobytes(), 6)), _chunk(b"IEND", b"")))


def _canvas(a: np.ndarray, h: int, w: int) -> np.ndarray:
    """`a` at the top-left of an h x w canvas (cropped where the canvas is smaller), the rest a mid grey."""
    out = np.full((h, w) + a.shape[2:], 97, np.uint8)
    hh, ww = min(h, a.shape[0]), min(w, a.shape[1])
    out[:hh, :ww] = a[:hh, :ww]
    return out


def _write_image(path: str, a: np.ndarray, kind: str) -> None:
    """The RGB photograph `a` written as `kind`."""
    from PIL import Image
    if kind == "rgb":
        Image.fromarray(a).save(path)
    elif kind == "tall256":
        Image.fromarray(_canvas(a, 300, 256)).save(path)
    elif kind == "tall300":
        Image.fromarray(_canvas(a, 300, 300)).save(path)
    elif kind == "short":
        Image.fromarray(_canvas(a, 200, 256)).save(path)
    elif kind == "narrow3":                                   # w c = 3: under the kernel's one dword per scanline
        Image.fromarray(np.ascontiguousarray(a[:, 100:103, 1])).save(path)
    elif kind == "narrow1a":                                  # w c = 4 exactly
        rgba = np.concatenate([a[:, 120:121], np.full((a.shape[0], 1, 1), 200, np.uint8)], axis=2)
        Image.fromarray(np.ascontiguousarray(rgba), "RGBA").save(path)
    elif kind == "wide320":
        Image.fromarray(_canvas(a, 256, 320)).save(path)
    elif kind == "wide400":
        Image.fromarray(_canvas(a, 256, 400)).save(path)
    elif kind == "L":
        Image.fromarray(a).convert("L").save(path)
    elif kind == "RGBA":
        rgba = np.concatenate([a, (np.arange(a.shape[1], dtype=np.uint8)[None, :, None] * np.ones((a.shape[0], 1, 1), np.uint8))], axis=2)
        Image.fromarray(rgba, "RGBA").save(path)
    elif kind == "P":
        Image.fromarray(a).quantize(64).save(path)
    elif kind == "rgb16":                                     # 16-bit RGB, big-endian samples, filter type 0
        h, w, _ = a.shape
        v = a.astype(np.uint16) * 257 + (np.arange(w, dtype=np.uint16) % 7)[None, :, None]
        raw = np.zeros((h, 1 + 6 * w), np.uint8)
        raw[:, 1:] = v.astype(">u2").view(np.uint8).reshape(h, 6 * w)
        with open(path, "wb") as f:
            f.write(_png(raw, w, h, 16, 2))
    elif kind == "bad":                                       # the photograph's own filtered scanlines, one filter-type byte set to 5
        from blindshadowremoval_amd import pngio
        h, w, _ = a.shape
        raw = pngio._parse_8bit(open(os.path.join(GOLDEN, "UCB", "train", "input", FOLDER, SRC + ".png"), "rb").read())[3]
        raw = raw.reshape(h, 1 + 3 * w).copy()
        raw[137, 0] = 5
        with open(path, "wb") as f:
            f.write(_png(raw, w, h, 8, 2))
    else:
        raise ValueError(kind)


def _write_mask(path: str, m: np.ndarray, kind: str) -> None:
    """The 0 / 255 grey mask `m` written as `kind`."""
    from PIL import Image
    if kind == "grey":
        Image.fromarray(m).save(path)
    elif kind == "rgb":
        Image.fromarray(np.repeat(m[:, :, None], 3, axis=2)).save(path)
    elif kind == "palette":
        Image.fromarray(m).convert("P").save(path)
    elif kind == "levels":                                    # grey levels other than 0 / 255: "u8" through the pipe
        Image.fromarray((m // 255 * 128 + (np.arange(m.shape[1], dtype=np.uint8) % 3)[None, :]).astype(np.uint8)).save(path)
    elif kind == "rgb_levels":
        Image.fromarray(np.repeat((m // 2)[:, :, None], 3, axis=2)).save(path)
    elif kind == "bad":                                       # Up on every row, one row's filter-type byte 5
        S = m.shape[0]
        raw = np.zeros((S, 1 + S), np.uint8)
        raw[:, 0] = 2
        raw[:, 1:] = np.diff(np.concatenate([np.zeros((1, S), np.int16), m.astype(np.int16)]), axis=0) & 255
        raw[S // 2, 0] = 5
        with open(path, "wb") as f:
            f.write(_png(raw, S, S, 8, 0))
    else:
        raise ValueError(kind)


def make_corpus(root: str):
    """-> {name: (lm_path, gt_path, {mask key: path})} for every item of ITEMS, written under `root` in the UCB layout
    (<root>/UCB/train/{input,gt}/9156/<name>.png, Dataset._gt_path's convention)."""
    from PIL import Image
    from blindshadowremoval_amd.prep import MASK_ORDER
    from blindshadowremoval_amd.ucb_post import MASK_DIRS
    src_in = os.path.join(GOLDEN, "UCB", "train", "input", FOLDER, SRC)
    photo = np.asarray(Image.open(src_in + ".png").convert("RGB"))
    truth = np.asarray(Image.open(os.path.join(GOLDEN, "UCB", "train", "gt", FOLDER, SRC + ".png")).convert("RGB"))
    masks = {k: np.asarray(Image.open(os.path.join(GOLDEN, "UCB_masks", MASK_DIRS[k], "%s_%s-result.png" % (FOLDER, SRC))).convert("L"))
             for k in MASK_ORDER}
    din, dgt = os.path.join(root, "UCB", "train", "input", FOLDER), os.path.join(root, "UCB", "train", "gt", FOLDER)
    os.makedirs(din, exist_ok=True)
    os.makedirs(dgt, exist_ok=True)
    lm = np.load(src_in + ".npy")
    out = {}
    for name, ik, gk, mk, _ in ITEMS:
        lm_path, gt_path = os.path.join(din, name + ".npy"), os.path.join(dgt, name + ".png")
        np.save(lm_path, lm)
        _write_image(os.path.join(din, name + ".png"), photo, ik)
        _write_image(gt_path, truth, gk)
        mp = {}
        for j, k in enumerate(MASK_ORDER):
            d = os.path.join(root, "UCB_masks", MASK_DIRS[k])
            os.makedirs(d, exist_ok=True)
            mp[k] = os.path.join(d, "%s_%s-result.png" % (FOLDER, name))
            _write_mask(mp[k], masks[k], mk if (mk != "bad" or j == 3) else "grey")          # bad_mask: one corrupt file of seven
        out[name] = (lm_path, gt_path, mp)
    return out


def job(corpus, name, size: int = 256):
    """prep.host_part's job of one corpus item."""
    lm_path, gt_path, mp = corpus[name]
    return (lm_path, gt_path, size, mp)
