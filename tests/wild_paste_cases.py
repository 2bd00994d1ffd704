"""Constructed cases of the paste-back tests (tests/test_wild_paste.py on the host statement, tests/test_wild_paste_gpu.py on the kernel):
small photographs of odd sizes, boxes of every side and position that takes another path through the arithmetic, and planes that make
the clip, the face weight and the rounding matter.  Everything comes from ONE seeded generator, so both files see the same bytes."""
import numpy as np

SEED = 20261018
SIZES = (32, 64)                                     # S
PHOTOS = ((97, 83), (130, 61))                       # h, w: odd, no multiple of the 16 x 16 tile


def canvas_box(box, h, w):
    """dataprocess.py:49-62 for a box in photograph coordinates: -> (box in canvas coordinates, preset_x, preset_y)."""
    px = max(-box[0], box[2] - w) if (box[0] < 0 or box[2] > w) else 0
    py = max(-box[1], box[3] - h) if (box[1] < 0 or box[3] > h) else 0
    return [box[0] + px, box[1] + py, box[2] + px, box[3] + py], px, py


def sides(S):
    return (2, 17, S - 1, S, S + 1, 3 * S + 5)


def positions(n, h, w):
    """name -> (x0, y0) of a square box of side n in photograph coordinates; a position the side does not allow is left out."""
    k = max(1, n // 3)
    pos = {}
    if n + 8 <= w and n + 8 <= h:
        pos["inside"] = (3, 5)
    if n <= w and n <= h:
        pos.update(flush_left=(0, 7 if n + 7 <= h else 0), flush_top=(4 if n + 4 <= w else 0, 0), flush_right=(w - n, 0 if n + 2 > h else 2),
                   flush_bottom=(0 if n + 1 > w else 1, h - n))
        pos.update(out_left=(-k, (h - n) // 2), out_right=(w - n + k, (h - n) // 2), out_top=((w - n) // 2, -k), out_bottom=((w - n) // 2, h - n + k),
                   out_left_top=(-k, -k), out_right_bottom=(w - n + k, h - n + k))
    else:
        # the side exceeds the photograph along at least one axis: centred (leaves it on two opposite sides, or is larger than the whole
        # photograph) and pushed to a corner
        pos.update(over_centred=((w - n) // 2, (h - n) // 2), over_corner=(-3, h - n + 2 if n <= h else -5))
    return pos


def _planes(rng, S, face_kind):
    im = rng.uniform(0, 1, (S, S, 3)).astype(np.float32)
    con = (im + rng.uniform(-0.6, 0.6, (S, S, 3))).astype(np.float32)          # leaves [0, 1] in many places: the clip matters
    con[0, 0], con[S - 1, S - 1], con[S // 2, S // 3] = -0.3, 1.4, (1.0, 0.0, 2.5)
    if face_kind == "ones":
        face = np.ones((S, S, 1), np.float32)
    elif face_kind == "zeros":
        face = np.zeros((S, S, 1), np.float32)
    else:                                                                       # a soft ramp, 0 at two edges
        r = np.sin(np.linspace(0, np.pi, S)).astype(np.float32)
        face = (r[:, None] * np.linspace(0, 1, S).astype(np.float32)[None, :])[:, :, None].astype(np.float32)
    return im, con, face


def _half_case(S):
    """Values that land on .5 before rounding (mode "residual"): n == S, so every tap weight is exactly 1 or 0; face is 1; the residual is
    exactly +k/510 (im = 0) or -k/510 (con = 0) for the k whose float32 product with 255 is exactly k/2; the photograph's bytes include 0
    and 255, so both saturations occur.  `want` is the box's exact result."""
    h, w = PHOTOS[0]
    x0, y0 = 10, 20
    ks = [k for k in range(1, 64) if float(np.float32(np.float32(k / 510.0) * np.float32(255))) == k / 2.0]
    odd = [k for k in ks if k % 2]
    assert len(odd) >= 8, "too few residuals k/510 whose float32 product with 255 is exactly k/2"
    yy, xx = np.mgrid[0:S, 0:S]
    k = np.array(ks)[(yy * 7 + xx * 3) % len(ks)]
    neg = ((yy + xx) % 2).astype(bool)
    r = (k / 510.0).astype(np.float32)
    im = np.zeros((S, S, 3), np.float32)
    con = np.zeros((S, S, 3), np.float32)
    con[~neg] = r[~neg][:, None]
    im[neg] = r[neg][:, None]
    bytes_ = np.array([0, 255, 10, 11, 128, 1, 254, 127], np.uint8)
    photo = np.full((h, w, 3), 77, np.uint8)
    photo[y0:y0 + S, x0:x0 + S] = bytes_[(yy * 5 + xx) % len(bytes_)][:, :, None]
    exact = photo[y0:y0 + S, x0:x0 + S, 0].astype(np.float64) + np.where(neg, -1.0, 1.0) * (k / 2.0)
    want = np.clip(np.rint(exact), 0, 255).astype(np.uint8)                    # float64 holds these sums exactly; rint is half to even
    return dict(name="half_S%d" % S, S=S, photo=photo, box=[x0, y0, x0 + S, y0 + S], preset_x=0, preset_y=0, im=im, con=con,
                face=np.ones((S, S, 1), np.float32), want=np.repeat(want[:, :, None], 3, axis=2), n=S, position="inside", face_kind="ones")


_CASES = None


def cases():
    """[{name, S, photo, box (canvas), preset_x, preset_y, im, con, face, n, position, face_kind, want | None}]"""
    global _CASES
    if _CASES is not None:
        return _CASES
    rng = np.random.RandomState(SEED)
    out = []
    kinds = ("ones", "ramp", "zeros", "ramp")
    for S in SIZES:
        for n in sides(S):
            for h, w in PHOTOS:
                for pname, (x0, y0) in sorted(positions(n, h, w).items()):
                    photo = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
                    photo[::9, ::7] = 0
                    photo[4::9, 3::7] = 255
                    kind = kinds[len(out) % len(kinds)]
                    im, con, face = _planes(rng, S, kind)
                    box, px, py = canvas_box([x0, y0, x0 + n, y0 + n], h, w)
                    out.append(dict(name="S%d_n%d_%dx%d_%s" % (S, n, h, w, pname), S=S, photo=photo, box=box, preset_x=px, preset_y=py, im=im, con=con,
                                    face=face, n=n, position=pname, face_kind=kind, want=None))
        out.append(_half_case(S))
    _CASES = out
    return out
