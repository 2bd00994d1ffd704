"""Constructed inputs for the UCB post-processing (blindshadowremoval_amd/ucb_post.py, csrc/ucb_kernels.h): images whose connected
components and rule decisions are known by construction, at S = 32, 64, 128 and 256.

Every item has the crop box [0, 0, S, S], so the resize is the identity and the rounded masks are the drawn ones.  The *topology* items
are rule-inert: face_hair = 1 everywhere, dif = 2 on the drawn pattern and 0 elsewhere, no eyebrow (the forehead rule is off), a
one-pixel nose and mouth — so `detected` before the keep filter IS the pattern, whatever the thresholds (they never exceed 1.0), and the
keep filter can be restated independently (tests/test_ucb_post_edges.py).  Most of them carry a *probe*: a solid block of
ceil(0.45 * largest) - 1 pixels below the pattern, dropped when the pattern is labelled right and kept as soon as its largest component
comes out smaller.  The *rule* items put each threshold rule, the nose rule and the keep filter's size / hair tests on both sides of
their edges; the *status* items are those where the host statement raises (an empty mask it takes a bounding box of).

cases() yields (key, (img, gt, con, dif), box, masks_u8, intent): img / gt / con [S,S,3] float32, dif [S,S,1] float32, box [4] float32,
masks_u8 [7,S,S] uint8 in MASK_ORDER, and intent = {"what": text, "trace": {key: value the host statement's trace must show},
"inert": bool, "px": [(y, x, detected 0/1)], "raises": bool, "heavy": bool}.
"""
import math

import numpy as np

SIZES = (32, 64, 128, 256)
MASK_ORDER = ("face_hair", "face", "mouth", "nose", "eyebrow", "eye", "glasses")      # = blindshadowremoval_amd.prep.MASK_ORDER
F32 = np.float32


def _item(key, S, what, seed, dif=None, img=None, masks=None, trace=None, inert=False, px=(), raises=False, heavy=False):
    rng = np.random.RandomState(seed)
    m = {k: np.zeros((S, S), bool) for k in MASK_ORDER}
    m["face_hair"][:] = True
    m["face"][:] = True
    m["mouth"][S - 1, S - 1] = True
    m["nose"][0, 0] = True
    m["eye"][S // 4:S // 4 + 2, S // 4:S // 2] = True            # not read by the rules: anything will do
    m.update(masks or {})
    if img is None:
        img = rng.uniform(0.05, 0.95, (S, S, 3))
    gt = np.clip(np.asarray(img, np.float64) + rng.normal(0, 0.05, (S, S, 3)), 0, 1)
    con = np.clip(gt + rng.normal(0, 0.03, (S, S, 3)), 0, 1)
    dif = np.zeros((S, S, 1), F32) if dif is None else np.asarray(dif, F32).reshape(S, S, 1)
    masks_u8 = np.stack([m[k].astype(np.uint8) * 255 for k in MASK_ORDER])
    intent = {"what": what, "trace": dict(trace or {}), "inert": inert, "px": list(px), "raises": raises, "heavy": heavy, "S": S}
    return key, (np.asarray(img, F32), gt.astype(F32), con.astype(F32), dif), np.array([0, 0, S, S], F32), masks_u8, intent


def masks_dict(masks_u8, grey=True):
    """masks_u8 [7,S,S] -> the host statement's {name: [S,S,1] float64} (cv2.imread(...) / 255.0, one channel, as read_masks(grey=True))."""
    return {k: (masks_u8[i].astype(np.float64) / 255.0)[:, :, None] for i, k in enumerate(MASK_ORDER)}


# ---- topologies (boolean [H, W] patterns)

def checkerboard(H, W):
    return (np.add.outer(np.arange(H), np.arange(W)) % 2) == 0


def staircases(H, W):
    """2-pixel-wide diagonal bands: each is ONE 4-connected staircase whose rows join only through the row above (long union chains)."""
    return (np.subtract.outer(np.arange(W), np.arange(H)).T % 8) < 2


def diagonals(H, W):
    """1-pixel diagonals: 8-connected lines, every pixel its own 4-connected component (sparser at W = 256: the host statement's cost
    grows with the number of components)."""
    return (np.subtract.outer(np.arange(W), np.arange(H)).T % (6 if W < 256 else 24)) == 0


def comb(H, W):
    """Teeth on the even columns that meet only in the last row: the last merges join S / 2 long components."""
    a = np.zeros((H, W), bool)
    a[:, 0::2] = True
    a[H - 1, :] = True
    return a


def spiral(H, W):
    """A 1-pixel-wide square spiral with 1-pixel gaps: one component, a single path of about H * W / 2 pixels."""
    a = np.zeros((H, W), bool)
    y = x = 0
    a[0, 0] = True
    lens = [W - 1, H - 1, W - 1]
    k = 3
    while True:
        n = (H if k % 2 else W) - 1 - 2 * ((k - 1) // 2)
        if n < 2:                                           # a 1-pixel turn would run alongside the previous segment
            break
        lens.append(n)
        k += 1
    for i, n in enumerate(lens):
        dy, dx = ((0, 1), (1, 0), (0, -1), (-1, 0))[i % 4]
        for _ in range(n):
            y, x = y + dy, x + dx
            a[y, x] = True
    return a


def square_rings(H, W):
    """Concentric 1-pixel square rings 2 pixels apart: ring sizes grow with the radius, so the keep filter keeps the outer ones."""
    cy, cx = (H - 1) // 2, (W - 1) // 2
    d = np.maximum(np.abs(np.arange(H) - cy)[:, None], np.abs(np.arange(W) - cx)[None, :])
    return (d % 2) == 0


def circles(H, W):
    """Euclidean rings one pixel thick: 8-connected curves that fall apart into many 4-connected arcs of different sizes."""
    yy, xx = np.mgrid[0:H, 0:W]
    r = np.hypot(yy - (H - 1) / 2.0, xx - (W - 1) / 2.0)
    return (np.floor(r).astype(int) % 4) == 0


def lines(H, W):
    """A full-width row and full-height columns on both sides of the wave boundaries (x = 63 | 64, 127 | 128) and at the edges."""
    a = np.zeros((H, W), bool)
    a[H // 2, :] = True
    for x in (0, 31, 32, 63, 64, 127, 128, W - 1):
        if x < W:
            a[:, x] = True
    return a


def columns(H, W):
    """The same columns without the row: {63, 64} and {127, 128} are two components each, the others one column."""
    a = lines(H, W)
    a[H // 2, :] = False
    for x in (0, 31, 32, 63, 64, 127, 128, W - 1):
        if x < W:
            a[H // 2, x] = True
    return a


def wave_blocks(H, W):
    """Runs that start at lane 0 and end at lane 63 of a wave (x = 64k .. 64k + 63; at W = 32 a wave is two whole rows), in blocks two
    rows high that touch their neighbours only at corners."""
    yy, xx = np.mgrid[0:H, 0:W]
    if W >= 64:
        return ((xx // 64 + yy // 2) % 2) == 0
    return ((yy // 2) % 2) == 0


def wave_crossing(H, W):
    """Runs that cross wave boundaries (x = 64k - a .. 64k + b, lengths varying with the row) and runs of one row that end at x = W - 1
    above runs that start at x = 0 in the next row — which are NOT neighbours."""
    a = np.zeros((H, W), bool)
    for y in range(0, H - 1, 4):
        i = y // 4
        if W >= 128:
            for b in range(64, W, 64):
                a[y, max(b - 1 - i % 7, 0):min(b + 1 + (3 * i) % 11, W)] = True
        a[y + 1, W - 1 - i % 5:W] = True
        if y + 2 < H:
            a[y + 2, 0:1 + (2 * i) % 5] = True
    return a


def row_ends(H, W):
    """(y, W-1) and (y+1, 0) only: on one wave at W = 32 (lanes 31 | 32), on two at W = 64.  The pair's runs have lengths 1..4 and
    2..5, so a wrong join would change which survive the 0.45 filter."""
    a = np.zeros((H, W), bool)
    for y in range(0, H - 1, 3):
        i = y // 3
        a[y, W - 1 - i % 4:W] = True
        a[y + 1, 0:2 + (i * 3) % 4] = True
    return a


def percolation(H, W, seed):
    return np.random.RandomState(seed).uniform(size=(H, W)) < 0.59


def _components(pattern):
    from scipy import ndimage
    lab, n = ndimage.label(pattern, structure=[[0, 1, 0], [1, 1, 1], [0, 1, 0]])
    return lab, n, np.bincount(lab.reshape(-1), minlength=n + 1)[1:]


def with_probe(pattern, S):
    """pattern [H, S] (H < S) on top, one blank row, then a probe of ceil(0.45 * largest) - 1 pixels filled row by row (one component):
    the probe is dropped exactly when the pattern's largest component is as large as drawn.  None when it does not fit."""
    H = pattern.shape[0]
    _, n, sizes = _components(pattern)
    if n == 0:
        return None
    r = math.ceil(0.45 * int(sizes.max())) - 1
    if r < 1 or r > (S - H - 1) * S:
        return None
    a = np.zeros((S, S), bool)
    a[:H] = pattern
    flat = np.zeros((S - H - 1) * S, bool)
    flat[:r] = True
    a[H + 1:] = flat.reshape(S - H - 1, S)
    return a


def topology_cases(S):
    H = (3 * S) // 4
    out = []
    gens = [("checker", checkerboard), ("stairs", staircases), ("diagonals", diagonals), ("comb", comb), ("spiral", spiral),
            ("rings", square_rings), ("circles", circles), ("lines", lines), ("columns", columns), ("wave_blocks", wave_blocks),
            ("wave_crossing", wave_crossing), ("row_ends", row_ends), ("percolation", lambda h, w: percolation(h, w, 59 + w))]
    for name, gen in gens:
        if name == "checker" and S == 256:                # 32 768 components cost the host statement seconds: a 64 x 96 block, over x = 64
            pat = np.zeros((S, S), bool)
            pat[8:72, 40:136] = checkerboard(64, 96)
            pat[100, 10:13] = True                        # probe: 3 pixels, so the single pixels are dropped
            out.append(("checker_block", pat, "checkerboard block over a wave boundary (no 4-joins) + a 3-pixel probe", True))
            continue
        full = gen(S, S)
        heavy = name in ("percolation", "spiral", "comb", "stairs")
        if name != "checker":
            out.append((name, full, gen.__doc__ or name, heavy))
        probed = with_probe(gen(H, S), S)
        if probed is not None:
            out.append((name + "_probe", probed, "%s over %d rows + a probe block" % (name, H), heavy))
    if S <= 128:
        pat = np.zeros((S, S), bool)
        pat[:S - 3] = checkerboard(S - 3, S)
        pat[S - 1, 0:3] = True
        out.append(("checker", pat, "checkerboard (no 4-joins) + a 3-pixel probe: only the probe survives", True))
    out.append(("all", np.ones((S, S), bool), "every pixel detected: one component of S*S", True))
    out.append(("empty", np.zeros((S, S), bool), "nothing detected: no component, mean_intensity = 0/0", False))
    return out


def _blocks(S, sizes, y0=1):
    """Solid components of the given pixel counts, laid out row by row with blank gaps: -> (bool [S,S], [pixel lists])."""
    a = np.zeros((S, S), bool)
    comps = []
    y, x, hrow = y0, 1, 0
    for n in sizes:
        w = min(n, max(4, int(math.sqrt(n))))
        h = -(-n // w)
        if x + w + 1 > S:
            y, x, hrow = y + hrow + 1, 1, 0
        assert y + h < S, "blocks do not fit"
        flat = np.zeros(h * w, bool)
        flat[:n] = True
        blk = flat.reshape(h, w)
        a[y:y + h, x:x + w] |= blk
        comps.append([(y + i, x + j) for i, j in zip(*np.nonzero(blk))])
        x, hrow = x + w + 1, max(hrow, h)
    return a, comps


def keep_filter_cases(S):
    """Sizes at 0.45 * largest (0.45 * 20k is an integer in float64), equal largest components, hair fractions at 0.8."""
    out = []
    big = 100 if S >= 64 else 40
    pat, comps = _blocks(S, [big, big * 45 // 100, big * 45 // 100 - 1, big // 2])
    out.append(("minsize", pat, "sizes %d (largest), %d == 0.45 * largest (kept), %d (dropped)" % (big, big * 45 // 100, big * 45 // 100 - 1),
                {"largest": big, "min_size": 0.45 * big, "n_big": 3, "n_kept": 3}, None, [(*comps[1][0], 1), (*comps[2][0], 0)]))
    pat, comps = _blocks(S, [big, big, big, big // 3, 1])
    out.append(("equal_largest", pat, "three equal largest components + two small ones", {"largest": big, "n_kept": 3, "ncomp": 5}, None,
                [(*comps[2][0], 1), (*comps[3][0], 0)]))
    # hair fractions: 0.8 exactly (dropped), just below (kept), 0 (kept); hair pixels are where face = 0 (face_hair = 1)
    n_a, n_b = (100, 90) if S >= 64 else (40, 36)
    pat, comps = _blocks(S, [n_a, n_b, n_a, n_a * 4 // 5])
    face = np.ones((S, S), bool)
    for (y, x) in comps[0][:n_a * 8 // 10]:                 # 0.8 exactly
        face[y, x] = False
    for (y, x) in comps[1][:math.ceil(0.8 * n_b) - 1]:      # one pixel short of 0.8: just below
        face[y, x] = False
    for (y, x) in comps[3][:n_a * 4 // 5 * 8 // 10 + 1]:    # just above 0.8
        face[y, x] = False
    out.append(("hair_frac", pat, "hair fractions 0.8 (dropped), %d/%d (kept), 0 (kept), > 0.8 (dropped)" % (math.ceil(0.8 * n_b) - 1, n_b),
                {"n_hair": 2, "n_kept": 2}, {"face": face}, [(*comps[0][0], 0), (*comps[1][0], 1), (*comps[2][0], 1), (*comps[3][0], 0)]))
    return out


def _rule_masks(S, **kw):
    m = {k: np.zeros((S, S), bool) for k in ("mouth", "nose", "eyebrow")}
    m.update(kw)
    return m


def below_cases(S, seed):
    """The three "mouth and below" windows: a roi (face at and below the mouth's top row) of exactly 1000 pixels, k of them shadowed
    (dif = 0.5), the input constant v there: frac = k / 1000 (float32(k) / float32(1000) equals float32(0.252), float32(0.3),
    float32(0.295) at k = 252, 300, 295 — the rules compare in float32, see ucb_post.py), mean_below ~ v."""
    out = []
    rows = -(-1000 // S)
    r0 = max(S - rows - 2, 0)
    face = np.zeros((S, S), bool)
    flat = face[r0:].reshape(-1)
    flat[:1000] = True
    face[r0:] = flat.reshape(S - r0, S)
    ys, xs = np.nonzero(face)
    mouth = np.zeros((S, S), bool)
    mouth[r0, 0] = True
    nose = np.zeros((S, S), bool)
    nose[S - 1, S - 1] = True                                   # outside the roi (face = 0 there): frac_nose = 0
    table = [(252, 0.30, (False, False, False)), (253, 0.30, (True, False, False)), (267, 0.30, (True, False, False)),
             (268, 0.30, (False, False, False)), (300, 0.37, (False, False, False)), (301, 0.37, (False, True, False)),
             (301, 0.35, (False, False, False)), (309, 0.37, (False, True, False)), (310, 0.37, (False, False, False)),
             (295, 0.23, (False, False, False)), (296, 0.23, (False, False, True)), (296, 0.21, (False, False, False)),
             (299, 0.23, (False, False, True)), (299, 0.21, (False, False, False))]
    for k, v, rules in table:
        dif = np.zeros((S, S), F32)
        dif[ys[:k], xs[:k]] = 0.5
        img = np.random.RandomState(seed + k).uniform(0.05, 0.95, (S, S, 3))
        img[ys[:k], xs[:k]] = v
        px = [(int(ys[0]), int(xs[0]), 0 if any(rules) else 1)]
        out.append(_item("below_k%d_v%03d_S%d" % (k, int(round(v * 100)), S), S, "frac = %d/1000, mean_below ~ %.2f" % (k, v), seed + k,
                         dif=dif, img=img, masks=dict(face=face, mouth=mouth, nose=nose),
                         trace={"frac": F32(k) / F32(1000), "below_rules": rules, "roi_off": any(rules)}, px=px))
    return out


def forehead_cases(S, seed):
    """np.sum(brow) = 3 * count against 30 (10 pixels: off, 11: on) and the region [f_top+20 : upper_brow-40, f_left+40 : f_right-40]
    with Python's slice rules — bounds that go negative count from the end, an empty column range.  The input is dark (< 0.4) so every
    pixel of the region is detected (mp = 0 > -0.001); inside the region 85 % of the pixels are hair (face = 0) and 10 % negative hair
    (face_hair = 0, face = 1): the signed fraction 0.75 keeps the component, the positive part alone (0.85) would not."""
    out = []
    geoms = []                                                  # (tag, f_top, f_left, f_right, upper_brow)
    if S == 256:
        geoms += [("plain", 10, 20, 235, 130), ("brow_lt_40", 0, 20, 235, 30), ("cols_cross", 10, 100, 150, 130)]
    elif S == 128:
        geoms += [("plain", 4, 2, 125, 90), ("brow_lt_40", 0, 2, 125, 30), ("cols_empty", 4, 40, 90, 90)]
    elif S == 64:
        geoms += [("right_lt_40", 0, 0, 30, 30), ("rows_right_lt_40", 0, 0, 30, 61), ("cols_empty", 0, 0, 63, 61), ("neg", 0, 0, 30, 30)]
    else:
        geoms += [("cols_empty", 0, 0, 31, 20)]
    if S >= 128:                                                # mostly negative hair: a negative signed fraction
        geoms += [("neg", 0, 2, S - 3, 30)]
    for tag, ft, fl, fr, by in geoms:
        mix = "neg" if tag == "neg" else "pos"
        for nb in (10, 11):
            img = np.full((S, S, 3), 0.2)
            face = np.zeros((S, S), bool)
            face[ft, fl:fr + 1] = True
            face[ft:by, fl] = face[ft:by, fr] = True
            face[by:, :] = True                                 # below the eyebrows: anything (the forehead box only sees rows < upper_brow)
            brow = np.zeros((S, S), bool)
            bx = min(fl + 3, S - 12)
            brow[by, bx:bx + nb] = True
            fh = np.ones((S, S), bool)
            r = slice(*slice(ft + 20, by - 40).indices(S)[:2])
            c = slice(*slice(fl + 40, fr - 40).indices(S)[:2])
            region = np.zeros((S, S), bool)
            region[r, c] = True
            ry, rx = np.nonzero(region)
            inside = (ry >= by) | ((rx >= fl) & (rx <= fr))       # face = 1 here cannot widen the forehead's bounding box
            face[ry[inside], rx[inside]] = True
            i = np.arange(len(ry)) % 20
            hair, neg = (i < 17, (i >= 17) & (i < 19)) if mix == "pos" else (np.zeros(len(ry), bool), i < 15)
            hair |= ~inside
            neg &= inside
            face[ry[hair], rx[hair]] = False
            fh[ry[neg], rx[neg]] = False
            mouth = np.zeros((S, S), bool)
            mouth[S - 1, S // 2] = True
            nose = np.zeros((S, S), bool)
            nose[S - 2, S // 2] = True
            on = nb == 11
            npx = int(region.sum()) if on else 0
            img[mouth | nose] = 0.9
            tr = {"forehead": on, "forehead_px": npx, "ncomp": 1 if npx else 0}
            if npx:                                             # one component, the region: its signed hair fraction decides
                hfrac = int(np.sum(fh[region].astype(int) - face[region])) / npx
                tr.update(n_kept=int(hfrac < 0.8), n_hair=int(not hfrac < 0.8), n_negative_hair=int(hfrac < 0))
            px = [(int(ry[0]), int(rx[0]), tr.get("n_kept", 0))] if len(ry) else []
            out.append(_item("forehead_%s_b%d_S%d" % (tag, nb, S), S, "forehead rule %s, eyebrow of %d pixels" % (tag, nb), seed + nb,
                             img=img, masks=dict(face=face, face_hair=fh, eyebrow=brow, mouth=mouth, nose=nose), trace=tr, px=px))
    return out


def left_brow_cases(S, seed):
    """The left-eyebrow rule: taken when the eyebrow's leftmost column is the face's (then threshold 1.0 where the eyebrow lies left of
    int(0.8 * left_face + 0.2 * right_face) and the input is brighter than 0.1), not taken one column further right."""
    out = []
    for tag, lf, rf, shift, v in (("edge", 0, 20, 0, 0.5), ("edge_dark", 0, 20, 0, 0.05), ("off", 0, 20, 1, 0.5),
                                  ("wide", 2, S - 3, 0, 0.5), ("exact", 0, 25, 0, 0.5)):
        face = np.zeros((S, S), bool)
        face[S // 4:S - 2, lf:rf + 1] = True
        brow = np.zeros((S, S), bool)
        by = S // 4 + 2
        brow[by, lf + shift:lf + shift + 8] = True
        dif = np.zeros((S, S), F32)
        dif[brow] = 0.5
        img = np.random.RandomState(seed).uniform(0.3, 0.9, (S, S, 3))
        img[brow] = v
        mouth = np.zeros((S, S), bool)
        mouth[S - 1, S - 1] = True
        nose = np.zeros((S, S), bool)
        nose[0, S - 1] = True
        hi = int(lf * 0.8 + rf * 0.2)
        rule = shift == 0
        cleared = int(np.sum(brow[:, :hi])) if rule and v > 0.1 else 0
        px = [(by, lf + shift, 0 if (rule and v > 0.1 and lf + shift < hi) else 1), (by, lf + shift + 7, 0 if (rule and v > 0.1 and lf + shift + 7 < hi) else 1)]
        out.append(_item("left_%s_S%d" % (tag, S), S, "left-eyebrow rule %s (left_hi = %d)" % (tag, hi), seed, dif=dif, img=img,
                         masks=dict(face=face, eyebrow=brow, mouth=mouth, nose=nose), trace={"left_rule": rule, "left_px": cleared, "forehead": False},
                         px=px))
    return out


def gate_cases(S, seed):
    """The magnitude exactly AT each threshold and one float32 step beyond it: the mustache gate (mp < 0.018 under the nose), the mouth
    gate (< 0.02), the plain threshold (> 0.01), the hair thresholds (> 0.02; > 0.004 where the input is darker than 0.13)."""
    img = np.random.RandomState(seed).uniform(0.3, 0.9, (S, S, 3))
    face = np.ones((S, S), bool)
    nose = np.zeros((S, S), bool)
    mouth = np.zeros((S, S), bool)
    nose[1:4, 2:S - 2] = True                                   # mid_nose_height = 2
    mouth[S // 2:S // 2 + 4, 2:S - 2] = True                    # mustache rows [2, S/2), mouth rows [S/2, S/2 + 3), cols [2, S - 3)
    dif = np.zeros((S, S), F32)
    up = lambda t: np.nextafter(F32(t), F32(1))
    dn = lambda t: np.nextafter(F32(t), F32(0))
    px = []
    blocks = [(6, 4, F32(0.018), 1), (6, 10, dn(0.018), 0),                 # mustache region
              (S // 2, 4, F32(0.02), 1), (S // 2, 10, dn(0.02), 0),         # mouth region
              (S - 8, 4, F32(0.01), 0), (S - 8, 10, up(0.01), 1),           # plain face
              (S - 8, 16, F32(0.02), 0), (S - 8, 22, up(0.02), 1),          # hair, bright
              (S - 4, 16, F32(0.004), 0), (S - 4, 22, up(0.004), 1)]        # hair, dark
    for y, x, v, det in blocks:
        dif[y:y + 2, x:x + 4] = v
        px.append((y, x, det))
    for y, x in ((S - 8, 16), (S - 8, 22), (S - 4, 16), (S - 4, 22)):   # hair pixels alone would be dropped as hair: two hair columns
        face[y:y + 2, x:x + 2] = False                                  # at the value under test, two face columns that are detected
        dif[y:y + 2, x + 2:x + 4] = 0.5
    img[S - 4:S - 2, 16:26] = 0.1
    return [_item("gates_S%d" % S, S, "magnitudes at the 0.018 / 0.02 gates and the 0.01 / 0.02 / 0.004 thresholds", seed, dif=dif, img=img,
                  masks=dict(face=face, nose=nose, mouth=mouth), px=px, trace={"forehead": False, "n_kept": 7, "n_hair": 0})]


def nose_cases(S, seed):
    """The nose rule's three frac_nose windows on both sides of each edge (a nose of 200 pixels, j of them under the kept shadow:
    frac_nose = j / 200 in float64), reach 5 (mean intensity < 0.15) and 65, and the column slice int(mid_nose_width - 35) that is
    negative at small S (it then counts from the end)."""
    out = []
    ny, nx = 2, (6 if S < 64 else (20 if S == 64 else 100))
    nose = np.zeros((S, S), bool)
    nose[ny:ny + 10, nx:nx + 20] = True
    ys, xs = np.nonzero(nose)
    mouth = np.zeros((S, S), bool)
    mouth[S - 1, S - 1] = True
    tail_y = ny + 10 + 8                                        # below lower_nose + 5, above lower_nose + 65
    for j, win in ((30, None), (31, 0), (49, 0), (50, None), (60, None), (61, 1), (62, None), (68, None), (69, 2), (70, None)):
        for v in ((0.1, 0.2) if j in (31, 61, 69) else (0.2,)):
            dif = np.zeros((S, S), F32)
            dif[ys[:j], xs[:j]] = 0.5
            dif[tail_y:tail_y + 3, nx:nx + 20] = 0.5
            img = np.random.RandomState(seed + j).uniform(0.3, 0.9, (S, S, 3))
            img[dif > 0] = v
            windows = tuple(win == i for i in range(3))
            tr = {"frac_nose": j / 200.0, "nose_windows": windows, "nose_hit": win is not None,
                  "reach": (5 if v < 0.15 else 65) if win is not None else None}
            out.append(_item("nose_j%d_v%02d_S%d" % (j, int(v * 100), S), S, "frac_nose = %d/200, mean intensity %.2f" % (j, v), seed + j,
                             dif=dif, img=img, masks=dict(nose=nose, mouth=mouth), trace=tr))
    return out


def status_cases(S, seed):
    """Where the host statement raises: an empty forehead (eyebrow in row 0), an empty face with eyebrows present, an empty mouth, an
    empty nose."""
    out = []
    b = np.zeros((S, S), bool)
    b[0, 2:14] = True
    out.append(_item("status_forehead_S%d" % S, S, "eyebrow (12 px) in row 0: the forehead is empty", seed, masks=dict(eyebrow=b), raises=True))
    b = np.zeros((S, S), bool)
    b[S // 2, 2:7] = True
    out.append(_item("status_face_S%d" % S, S, "no face, a 5-pixel eyebrow (forehead rule off)", seed,
                     masks=dict(eyebrow=b, face=np.zeros((S, S), bool)), raises=True))
    out.append(_item("status_mouth_S%d" % S, S, "no mouth", seed, masks=dict(mouth=np.zeros((S, S), bool)), raises=True))
    out.append(_item("status_nose_S%d" % S, S, "no nose", seed, masks=dict(nose=np.zeros((S, S), bool)), raises=True))
    return out


def topology_items(S):
    items = []
    for i, (name, pat, what, heavy) in enumerate(topology_cases(S)):
        items.append(_item("%s_S%d" % (name, S), S, what, 1000 * S + i, dif=np.where(pat, F32(2), F32(0)), inert=True, heavy=heavy))
    for i, (name, pat, what, trace, masks, px) in enumerate(keep_filter_cases(S)):
        items.append(_item("%s_S%d" % (name, S), S, what, 2000 * S + i, dif=np.where(pat, F32(2), F32(0)), inert=True, masks=masks,
                           trace=trace, px=px))
    return items


def cases(sizes=SIZES):
    for S in sizes:
        yield from topology_items(S)
        yield from below_cases(S, 3000 * S)
        yield from forehead_cases(S, 4000 * S)
        yield from left_brow_cases(S, 5000 * S)
        yield from gate_cases(S, 6000 * S)
        yield from nose_cases(S, 7000 * S)
        yield from status_cases(S, 8000 * S)
