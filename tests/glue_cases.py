"""Shared by the tests of the forward's glue arithmetic (csrc/glue_kernels.h, the heads / colour-tail epilogues of csrc/conv_n16.h): ONE
float32 statement of what TensorFlow's separate ops compute there, in plain numpy.  Every operation below is one rounded float32 operation
(numpy's elementwise float32 ufuncs: no fused multiply-add), in the order the reference's graph runs them (model.py:237,250-252,256,288,
model_with_TSM.py:204-229, warp.py:71-165) with the resize in the arithmetic of TensorFlow's CPU kernel (compute_lerp of
resize_bilinear_op.cc), the one ``ucb_post.resize_bilinear`` states:

    top = tl + (tr - tl) * x_lerp;  bottom = bl + (br - bl) * x_lerp;  out = top + (bottom - top) * y_lerp

The ``contract=`` / ``order=`` arguments give what a kernel that is subtly wrong would compute — a product fused into its add (formed in
float64, rounded once), the 0.5 * (0.5 a + 0.5 b) + 0.5 * (0.5 c + 0.5 d) resize the kernels ran before — and exist only so that the tests
can show that the exact comparison has teeth on the inputs they use.  Also here: the seeded stand-in fields and the constructed inputs of
the GPU cases, so that the CPU tests state the conditions under which the GPU tests mean something.  No test functions here."""
import numpy as np

f32 = np.float32
GRAY_W = (f32(0.2989), f32(0.5870), f32(0.1140))
THRESHOLD = f32(0.1)                       # model.py:256, strict >
GRAY_CONTRACTIONS = ("first", "second", "third", "all")
HALF = f32(0.5)


def _f(x):
    return np.ascontiguousarray(np.asarray(x), dtype=np.float32)


def _fma(a, b, c):
    """fl(a * b + c) for float32 operands: the product of two float32 is exact in float64; one rounding of the float64 sum, then one to
    float32 (the teeth variants only need to differ from the statement the way a fused multiply-add does)."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


# ---- the statement ----

def gray(x, contract=None):
    """tf.image.rgb_to_grayscale, left to right: (r * 0.2989f + g * 0.5870f) + b * 0.1140f  ([..., 3] -> [..., 1]).
    contract: "first" / "second" fuse r's / g's product into the first add, "third" b's into the second, "all" = first + third."""
    x = _f(x)
    r, g, b = x[..., 0:1], x[..., 1:2], x[..., 2:3]
    if contract is None:
        return (r * GRAY_W[0] + g * GRAY_W[1]) + b * GRAY_W[2]
    assert contract in GRAY_CONTRACTIONS, contract
    if contract in ("first", "all"):
        s = _fma(r, GRAY_W[0], g * GRAY_W[1])
    elif contract == "second":
        s = _fma(g, GRAY_W[1], r * GRAY_W[0])
    else:
        s = r * GRAY_W[0] + g * GRAY_W[1]
    return _fma(b, GRAY_W[2], s) if contract in ("third", "all") else s + b * GRAY_W[2]


def heads(mask, con, inputs, contract=False):
    """model.py:250,252 from the heads' two values per pixel: gs = fl(fl(g0 * fl(1 + mask)) + con), mask22 = [max(mask, 0), mask * 0,
    max(-mask, 0)].  mask [..., 1], con [..., 1] or a scalar.  contract: gs = fl(g0 * t + con) in one rounding."""
    mask, g0 = _f(mask), gray(inputs)
    con = np.broadcast_to(_f(con), mask.shape)
    t = f32(1) + mask
    gs = _fma(g0, t, con) if contract else g0 * t + con
    mask22 = np.concatenate([np.maximum(mask, f32(0)), mask * f32(0), np.maximum(-mask, f32(0))], axis=-1)
    return gs, mask22


def final_dif(con_rgb, inputs, contract=None):
    """model.py:288: fl(gray(con_rgb) - gray(inputs))."""
    return gray(con_rgb, contract) - gray(inputs, contract)


def _taps8(x):
    x = _f(x)
    assert x.ndim == 4 and x.shape[1] % 8 == 0 and x.shape[2] % 8 == 0, x.shape
    return x[:, 3::8, 3::8], x[:, 3::8, 4::8], x[:, 4::8, 3::8], x[:, 4::8, 4::8]      # tl, tr, bl, br


def lerp4(tl, tr, bl, br, order="lerp"):
    """compute_lerp with both weights 0.5.  order="old": the sum of halves the kernels ran before (teeth only)."""
    if order == "old":
        return HALF * (HALF * tl + HALF * tr) + HALF * (HALF * bl + HALF * br)
    assert order == "lerp", order
    top = tl + (tr - tl) * HALF
    bottom = bl + (br - bl) * HALF
    return top + (bottom - top) * HALF


def resize8(x, order="lerp"):
    """tf.image.resize(x, [H/8, W/8]) (bilinear, half-pixel centres) of [B,H,W,C]: the sample point of cell (o, p) is (8o + 3.5, 8p + 3.5),
    so the taps are rows 8o+3, 8o+4 x columns 8p+3, 8p+4 and both lerps are 0.5 — in compute_lerp's order."""
    return lerp4(*_taps8(x), order=order)


def d32_bmask(gs, inputs, contract=None, order="lerp"):
    """model.py:251,256: d32 = resize8(fl(gs - gray(inputs))), bmask = d32 > 0.1f (strict) as 0 / 1 float32."""
    d32 = resize8(_f(gs) - gray(inputs, contract), order)
    return d32, (d32 > THRESHOLD).astype(np.float32)


def max_zero_ordered(a, b):
    """max(a, b) with -0 < +0 (IEEE 754 maximum; the device's v_max_f32): numpy's maximum keeps whichever zero comes first."""
    m = np.maximum(a, b)
    both_zero = (a == 0) & (b == 0)
    return np.where(both_zero, np.where(np.signbit(a) & np.signbit(b), f32(-0.0), f32(0.0)), m).astype(np.float32)


def _warp32(x, off0, off1):
    """tf_batch_map_coordinates (warp.py:71-115) in float32: x [B,S,S,C], off0 / off1 [B,S,S] offsets in cells along axis 0 / 1."""
    B, S = x.shape[0], x.shape[1]
    ii, jj = np.meshgrid(np.arange(S, dtype=np.float32), np.arange(S, dtype=np.float32), indexing="ij")
    c0 = np.minimum(np.maximum(off0 + ii, f32(0)), f32(S - 1))
    c1 = np.minimum(np.maximum(off1 + jj, f32(0)), f32(S - 1))
    f0, f1 = np.floor(c0), np.floor(c1)
    i0, i1, j0, j1 = f0.astype(np.int64), np.ceil(c0).astype(np.int64), f1.astype(np.int64), np.ceil(c1).astype(np.int64)
    o0, o1 = (c0 - f0)[..., None], (c1 - f1)[..., None]
    b = np.arange(B)[:, None, None]
    lt, rt, lb, rb = x[b, i0, j0], x[b, i1, j0], x[b, i0, j1], x[b, i1, j1]
    vt = lt + (rt - lt) * o0                     # (i0, j0) -> (i1, j0): along axis 0 first
    vb = lb + (rb - lb) * o0
    return vt + (vb - vt) * o1


def _group_share(xw, frame):
    """[B,S,S,C] -> [B,S,S,2C]: max | sum / frame over each group of `frame` consecutive rows, in frame order, tiled back over the group."""
    B = xw.shape[0]
    assert B % frame == 0
    g = xw.reshape(B // frame, frame, *xw.shape[1:])
    mx = np.full(g[:, 0].shape, -np.inf, np.float32)
    sm = np.zeros(g[:, 0].shape, np.float32)
    for f in range(frame):
        mx = max_zero_ordered(mx, g[:, f])
        sm = sm + g[:, f]
    sh = np.concatenate([mx, sm / f32(frame)], axis=-1)
    return np.repeat(sh, frame, axis=0)


def share_layer32(x, reg, frame):
    """ShareLayer.call (model_with_TSM.py:204-229) with share=True in float32: x [B,S,S,C], reg [B,8S,8S,6] = reg_in | reg_out.
    reg32 = resize8(reg)[..., (0,1,3,4)] * S; warp by reg_in; group max | mean; tile; warp by reg_out."""
    x, reg = _f(x), _f(reg)
    S = x.shape[1]
    assert x.shape[2] == S and reg.shape[1:] == (8 * S, 8 * S, 6), (x.shape, reg.shape)
    reg32 = resize8(reg)[..., (0, 1, 3, 4)] * f32(S)
    sh = _group_share(_warp32(x, reg32[..., 0], reg32[..., 1]), frame)
    return _warp32(sh, reg32[..., 2], reg32[..., 3])


def share_layer_gather(x, k_in, k_out, frame):
    """The ShareLayer for whole-cell offsets k_in / k_out [B,S,S,2] (integers): every warp is a clamped integer gather, no lerp."""
    x = _f(x)
    B, S = x.shape[0], x.shape[1]
    ii, jj = np.meshgrid(np.arange(S), np.arange(S), indexing="ij")
    b = np.arange(B)[:, None, None]

    def gather(t, k):
        # a lerp of weight 0 between a value and itself returns the value, except that -0 + (+0) = +0
        return t[b, np.clip(ii + k[..., 0], 0, S - 1), np.clip(jj + k[..., 1], 0, S - 1)] + f32(0)
    return gather(_group_share(gather(x, k_in), frame), k_out)


# ---- seeded stand-in fields and constructed inputs of the GPU cases ----

GSC_SHAPES = ((3, 32, 256), (1, 64, 512))        # the smallest sizes the GSC forward accepts: non-square, > 1 cell row and column block
TSM_SHAPE = (4, 256, 256)                        # the TSM forward needs a square image with a side that is a multiple of 256
FUSED_SHAPE = (256, 32, 256)                     # B * H / 8 = 1024 row strips: the heads' fused epilogue runs (conv_n16_fuse_pays)
CON_BIAS = f32(0.25)                             # case B: conv3's kernel is zero, so con is exactly this bias


def uniform_field(shape, seed, lo=0.0, hi=1.0):
    """[*shape, 3] float32 uniform in [lo, hi)."""
    rng = np.random.default_rng(seed)
    return (rng.random((*shape, 3), dtype=np.float32) * f32(hi - lo) + f32(lo)).astype(np.float32)


def standin_mask(shape, seed):
    """[*shape, 1]: tanh(N(0, 1)), what the mask head's range looks like (the CPU teeth tests; the GPU tests read the device's mask)."""
    rng = np.random.default_rng(seed)
    return np.tanh(rng.standard_normal((*shape, 1))).astype(np.float32)


def head_weights(w, conv2_live, con_bias, mask_bias=0.0):
    """A copy of the generator weights `w` with conv3 (the con head) reduced to a bias, and conv2 (the mask head) either live or reduced
    to `mask_bias` as well."""
    w = {k: v.copy() for k, v in w.items()}
    w["conv3/conv/kernel"] = np.zeros_like(w["conv3/conv/kernel"])
    w["conv3/conv/bias"] = np.full_like(w["conv3/conv/bias"], con_bias)
    if not conv2_live:
        w["conv2/conv/kernel"] = np.zeros_like(w["conv2/conv/kernel"])
        w["conv2/conv/bias"] = np.full_like(w["conv2/conv/bias"], mask_bias)
    return w


PLANT_SHAPE = (2, 32, 256)            # 2 x 4 x 32 = 256 cells
PLANT_CLASSES = ("only_lerp_above", "only_old_above", "equal_threshold", "next_above_threshold")
PLANT_PER_CLASS = 40


def planted_threshold(seed=2024):
    """Case E.  With mask == 1 and con == 0, gs = 2 g0 and fl(gs - g0) = g0, so the four taps of a cell are the gray values of its four
    centre pixels.  Those pixels are grey (r = g = b = v): three values are drawn from [0, 0.13], the fourth is searched within +-8 ulp of
    (0.4 - ta - tb - tc) / 0.9999 (ta.. the taps of the three) at a drawn position, and a candidate is kept for the first class it falls in:
        only_lerp_above        d32 > 0.1f in the compute_lerp order, not in the old order
        only_old_above         the reverse
        equal_threshold        d32 == 0.1f in the compute_lerp order (strict >: not in the mask)
        next_above_threshold   d32 == nextafter(0.1f, 1) in the compute_lerp order
    PLANT_PER_CLASS cells of each are planted into cells [k * PLANT_PER_CLASS, (k + 1) * PLANT_PER_CLASS) in PLANT_CLASSES order (cells
    counted row-major over [B, H/8, W/8]); the other cells get four equal pixels drawn from [0, 0.3): ordinary values on both sides.
    -> (inputs [B,H,W,3], {class: cell indices})."""
    rng = np.random.default_rng(seed)
    B, H, W = PLANT_SHAPE
    ncell = B * (H // 8) * (W // 8)
    up = np.nextafter(THRESHOLD, f32(1))
    found = {c: [] for c in PLANT_CLASSES}

    def tap(v):
        return gray(np.repeat(v[..., None], 3, axis=-1))[..., 0]

    for _ in range(64):
        n = 4096
        abc = (rng.random((n, 3), dtype=np.float32) * f32(0.13)).astype(np.float32)
        pos = rng.integers(0, 4, n)
        t = tap(abc)
        centre = ((f32(0.4) - t[:, 0] - t[:, 1] - t[:, 2]) / f32(0.9999)).astype(np.float32)
        for step in range(-8, 9):
            d = centre.copy()
            for _s in range(abs(step)):
                d = np.nextafter(d, f32(1) if step > 0 else f32(-1))
            v = np.empty((n, 4), np.float32)                                               # one cell: tl, tr, bl, br
            rest = np.array([[j for j in range(4) if j != p] for p in range(4)])[pos]      # the positions of a, b, c
            v[np.arange(n), pos] = d
            v[np.arange(n)[:, None], rest] = abc
            taps = tap(v).T
            lerp, old = lerp4(*taps), lerp4(*taps, order="old")
            cls = np.full(n, -1)
            cls[(lerp > THRESHOLD) & ~(old > THRESHOLD)] = 0
            cls[~(lerp > THRESHOLD) & (old > THRESHOLD)] = 1
            cls[(cls < 0) & (lerp == THRESHOLD)] = 2
            cls[(cls < 0) & (lerp == up)] = 3
            for k, c in enumerate(PLANT_CLASSES):
                for row in v[cls == k]:
                    if len(found[c]) < PLANT_PER_CLASS:
                        found[c].append(row)
        if all(len(found[c]) >= PLANT_PER_CLASS for c in PLANT_CLASSES):
            break
    cells = np.repeat((rng.random((ncell, 1), dtype=np.float32) * f32(0.3)).astype(np.float32), 4, axis=1)
    index = {}
    for k, c in enumerate(PLANT_CLASSES):
        index[c] = np.arange(k * PLANT_PER_CLASS, k * PLANT_PER_CLASS + len(found[c]))
        if found[c]:
            cells[index[c]] = np.stack(found[c])
    inputs = uniform_field((B, H, W), seed + 1)
    grid = cells.reshape(B, H // 8, W // 8, 2, 2)
    for dy in range(2):
        for dx in range(2):
            inputs[:, 3 + dy::8, 3 + dx::8, :] = grid[..., dy, dx][..., None]
    return inputs, index


INT_OFFSETS = (0.0, 1.0, -1.0, 3.0, -3.0, 40.0, -40.0, -0.0)      # whole cells; +-40 leaves the 32-cell map on either side: both clamps
HALF_OFFSETS = INT_OFFSETS + (0.5, -0.5, 1.5, -2.5)


def block_reg(B, S, palette, seed):
    """An offset field [B,8S,8S,6] that is constant over each 8x8 block, so that every resize order returns the block's value exactly:
    per cell and channel one of `palette` (in cells) / S — exact for a power-of-two S.  Channels 2 and 5, which the ShareLayer never reads,
    hold 7 / S.  -> (reg, k [B,S,S,4] the offsets in cells of channels 0, 1, 3, 4)."""
    assert S & (S - 1) == 0
    rng = np.random.default_rng(seed)
    k = np.asarray(palette, np.float32)[rng.integers(0, len(palette), (B, S, S, 4))]
    cell = np.full((B, S, S, 6), f32(7) / f32(S), np.float32)
    cell[..., (0, 1, 3, 4)] = k / f32(S)
    return np.repeat(np.repeat(cell, 8, axis=1), 8, axis=2), k
