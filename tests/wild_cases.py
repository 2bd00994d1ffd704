"""Inputs of the in-the-wild crop tests (tests/test_wild_crop.py, tests/test_wild_crop_gpu.py) and of the tool that makes their fixture
(tools/make_wild_crop_fixture.py): synthetic photographs rebuilt from a seed — the fixture then only stores landmarks, boxes and crops —
and the one real photograph, tests/golden/wild/01001.

01001 is the reference's sample_uncropped_images/01001 TRIMMED to the 840 x 840 window [160:1000) x [144:984) around its face box, the
landmarks shifted by (160, 144): the whole 1024 x 1024 file is 1.4 MB, more than a committed file may be.  The box lies inside the
window, so the crop, its bytes and the landmarks in the crop's coordinates are those of the whole photograph (the fixture tool checks
that against the reference's own file); the box itself is shifted by the same (160, 144)."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
WILD = os.path.join(GOLDEN, "wild")
FIXTURE = os.path.join(GOLDEN, "wild_crop.npz")
TRIM = (160, 144)                                   # x, y of the window's corner in the reference's 1024 x 1024 photograph


def photo(h: int, w: int, seed: int) -> np.ndarray:
    """uint8 [h,w,3]: random 21 x 15 pixel tiles with a soft ramp across each — tap pairs differ along the tile edges and inside the
    tiles, and the crops still compress (the fixture holds them)."""
    rng = np.random.RandomState(seed)
    tiles = rng.randint(0, 240, ((h + 20) // 21, (w + 14) // 15, 3))
    big = np.kron(tiles, np.ones((21, 15, 1), np.int64))[:h, :w]
    return (big + (np.arange(w)[None, :, None] % 15)).astype(np.uint8)


def noise(h: int, w: int, seed: int) -> np.ndarray:
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def landmarks(cx: float, cy: float, ex: float, ey: float, seed: int, frac: bool = False) -> np.ndarray:
    """68 float32 points filling [cx - ex, cx + ex] x [cy - ey, cy + ey], the extremes reached; frac: none of them on an integer."""
    rng = np.random.RandomState(seed)
    lm = np.stack([rng.uniform(cx - ex, cx + ex, 68), rng.uniform(cy - ey, cy + ey, 68)], axis=1)
    if not frac:
        lm = np.rint(lm)
    lm[0], lm[1] = (cx - ex, cy - ey), (cx + ex, cy + ey)
    return lm.astype(np.float32)


PHOTO_H, PHOTO_W = 640, 600
# name -> (cx, cy, ex, ey, fractional landmarks): with ex = ey = 180 the half-length is 261 and the box 522 pixels wide:
# [cx - 261, cy - 313, cx + 261, cy + 209] in a 600 x 640 photograph
CASES = {
    "inside": (300, 330, 180, 180, False),
    "inside_frac": (300.3, 330.6, 180.35, 175.2, True),
    "edge_exact": (339, 431, 180, 180, False),      # right and bottom edges of the box ARE w and h: no padding
    "left": (250, 330, 180, 180, False),
    "right": (350, 330, 180, 180, False),
    "top": (300, 300, 180, 180, False),
    "bottom": (300, 440, 180, 180, False),
    "left_top": (250, 300, 180, 180, False),
    "right_bottom_frac": (350.2, 440.7, 181.5, 179.25, True),
    "skip": (300, 330, 170, 170, False),            # half-length 246.5: the script writes nothing
    "just_kept": (300, 330, 172.5, 172.5, True),    # half-length 250.125: the smallest the rule keeps, give or take
}


def case_inputs(name: str):
    """(photograph, landmarks) of a synthetic case."""
    cx, cy, ex, ey, frac = CASES[name]
    seed = sorted(CASES).index(name)
    return photo(PHOTO_H, PHOTO_W, 100 + seed), landmarks(cx, cy, ex, ey, 200 + seed, frac)
