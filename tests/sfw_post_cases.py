"""The cases of the SFW scoring fixture (tests/golden/sfw_post_gsc.npz): row 0 of a GSC SFW element and the generator outputs it is scored
against.  Shared by tools/make_sfw_post_fixture.py (which runs the reference's own test_step_sfw over them) and the tests.

Each case is (key, img [S,S,3], con_rgb [S,S,3], mask [S,S,1] grey levels, dif [S,S,1], face [S,S,1]), float32, S = 256, built from a
seeded generator.  They cover what the exact AUC has to get right: heavy ties (mask_pred exactly 0 outside the face), -0.0 products
(negative dif times face = 0), subnormal products, an item whose only positive is the forced one, a face region that is positive
everywhere, and mask levels just next to 2.0 that must not count as labels."""
import numpy as np

S = 256


def _base(rng):
    yy, xx = np.mgrid[0:S, 0:S].astype(np.float32)
    img = rng.random((S, S, 3), dtype=np.float32)
    con = (img + rng.normal(0.0, 0.3, (S, S, 3))).astype(np.float32)                  # outside [0, 1] in places: the figure clips
    r2 = ((yy - 128) ** 2 + (xx - 120) ** 2) / (90.0 ** 2)
    face = np.clip(1.3 - r2, 0.0, 1.0).astype(np.float32)[..., None]                  # 0 outside an ellipse, a ramp to 1 inside
    levels = np.digitize(img.mean(axis=2), [0.35, 0.6]).astype(np.float32)            # 0 / 1 / 2
    return img, con, levels[..., None], face


def cases():
    rng = np.random.default_rng(20261015)
    out = []
    # ties: mask_pred = 0 wherever face = 0 (~60 % of the pixels) and a coarse score grid inside
    img, con, mask, face = _base(rng)
    dif = (np.round(rng.random((S, S, 1)) * 8) / 8).astype(np.float32)
    out.append(("ties", img, con, mask, dif, face))
    # -0.0: negative dif times face = 0 next to +0.0 products and negative scores inside the face
    img, con, mask, face = _base(rng)
    dif = (rng.random((S, S, 1)) - 0.5).astype(np.float32)
    out.append(("negzero", img, con, mask, dif, face))
    # subnormal products: dif ~ 1e-36 times a face ramp, so many products fall below 2^-126 and some to 0
    img, con, mask, face = _base(rng)
    dif = (rng.random((S, S, 1)) * 3e-36 * np.where(rng.random((S, S, 1)) < 0.5, 1, -1)).astype(np.float32)
    face = (face * np.float32(1e-3)).astype(np.float32)
    out.append(("subnormal", img, con, mask, dif, face))
    # no pixel with mask == 2: only the forced positive
    img, con, mask, face = _base(rng)
    mask = np.minimum(mask, np.float32(1.5)).astype(np.float32)
    dif = rng.random((S, S, 1), dtype=np.float32)
    out.append(("nopos", img, con, mask, dif, face))
    # a face region positive everywhere: no forced zeros, every score distinct almost surely
    img, con, mask, _ = _base(rng)
    face = (0.25 + 0.75 * rng.random((S, S, 1))).astype(np.float32)
    dif = rng.normal(0.2, 0.3, (S, S, 1)).astype(np.float32)
    out.append(("allface", img, con, mask, dif, face))
    # mask levels just next to 2.0 (interpolated labels): only exact 2.0 is a positive
    img, con, mask, face = _base(rng)
    near = np.array([2.0, np.nextafter(np.float32(2), np.float32(3)), np.nextafter(np.float32(2), np.float32(0)), 1.9999, 2.0001, 2.0], np.float32)
    mask = np.where(mask == 2, near[rng.integers(0, len(near), (S, S, 1))], mask).astype(np.float32)
    dif = rng.random((S, S, 1), dtype=np.float32)
    out.append(("near2", img, con, mask, dif, face))
    return out


def element(img, con, mask, dif, face, rows: int = 10):
    """A [rows,S,S,17] element whose row 0 carries the case (img 3 | cmap 3 | mask 1 | uv 3 | reg 6 | face 1); cmap, uv, reg are zero."""
    row = np.concatenate([img, np.zeros((S, S, 3), np.float32), mask, np.zeros((S, S, 9), np.float32), face], axis=2)
    return np.repeat(row[None], rows, axis=0).astype(np.float32)
