"""Shared by the tests of the device input preparation (csrc/prep_kernels.h, csrc/prep_group_kernels.h): the numpy statement of the two
kernels — float64, the host's operation order — for lists of prep.HostPart records, a float32 variant of it that only the test proving
the bit-for-bit bar has teeth uses, and constructed parts that reach what the faces of the golden data never do: full 256-triangle
tables, grid points on edges and vertices, meshes that do not cover the square, every reflected tap of the blur, crops that upsample,
copy, shrink by a non-integer factor, leave the image or have no pixels.  No test functions here."""
import numpy as np

from blindshadowremoval_amd import dataset as D
from blindshadowremoval_amd import prep


# ---- the statement ----

def _resize(img, size, dt=np.float64):
    """dataset.resize_linear with every operand of type `dt` (float64: the same bits as dataset.resize_linear)."""
    img = np.ascontiguousarray(img, dt)

    def axis(n):
        src = np.maximum((np.arange(size).astype(dt) + dt(0.5)) * (dt(n) / dt(size)) - dt(0.5), dt(0.0))
        i0 = np.minimum(np.floor(src).astype(np.int64), n - 1)
        return i0, np.minimum(i0 + 1, n - 1), src - i0.astype(dt)
    y0, y1, wy = axis(img.shape[0])
    x0, x1, wx = axis(img.shape[1])
    wx = wx[None, :, None]
    top = img[y0][:, x0] * (1 - wx) + img[y0][:, x1] * wx
    bot = img[y1][:, x0] * (1 - wx) + img[y1][:, x1] * wx
    wy = wy[:, None, None]
    return top * (1 - wy) + bot * wy


def zero_extended_crop(im, box, div=255.0, dt=np.float64):
    """The n x n crop (n = box[2] - box[0]) whose top-left corner is (box[0], box[1]): image pixels / div, 0 outside the image."""
    n = int(box[2] - box[0])
    im = im if im.ndim == 3 else im[:, :, None]
    c = np.zeros((n, n, im.shape[2]), dt)
    ys, xs = np.arange(n) + int(box[1]), np.arange(n) + int(box[0])
    oky, okx = (ys >= 0) & (ys < im.shape[0]), (xs >= 0) & (xs < im.shape[1])
    c[np.ix_(oky, okx)] = im[np.ix_(ys[oky], xs[okx])].astype(dt) / dt(div)
    return c


def crop_planes(im, box, size, div=255.0, dt=np.float64):
    """The kernels' crop + INTER_LINEAR resize of one image: [size, size, channels]; a box without pixels gives zeros."""
    n = int(box[2] - box[0])
    if n <= 0:
        return np.zeros((size, size, 1 if im.ndim == 2 else im.shape[2]), dt)
    return _resize(zero_extended_crop(im, box, div, dt), size, dt)


def locate(t, size):
    """Point location of prep_meshes without the cull, on the size x size grid: -> (index of the winning triangle per pixel — the first of
    equal maxima of min(l_i) in table order —, its min(l_i), inside = that value >= -1e-12)."""
    lin = np.linspace(0, 1, size)
    best, lm = np.zeros((size, size), np.int64), np.zeros((size, size), np.float64)
    e = [t[:, j][:, None, None] for j in range(9)]
    for r in range(0, size, 16):                                  # in bands of rows: the [ntri, rows, size] temporaries stay in the cache
        px, py = np.meshgrid(lin, lin[r:r + 16])
        l = np.minimum(np.minimum((e[0] * px + e[1] * py) + e[2], (e[3] * px + e[4] * py) + e[5]), (e[6] * px + e[7] * py) + e[8])
        best[r:r + 16] = l.argmax(0)
        lm[r:r + 16] = np.take_along_axis(l, best[None, r:r + 16], 0)[0]
    return best, lm, lm >= -1e-12


def planes_at(t, best, size, dt=np.float64):
    """(a px + b py) + c of the winning triangles' three channels, every operand of type `dt`."""
    lin = np.linspace(0, 1, size)
    px, py = np.meshgrid(lin.astype(dt), lin.astype(dt))
    t = t.astype(dt)
    return [(t[best, 9 + 3 * k] * px + t[best, 10 + 3 * k] * py) + t[best, 11 + 3 * k] for k in range(3)]


def mesh_channels(tabs, size, dt=np.float64):
    """The ten channels behind the crop planes for four tables: uvm3, reg_in3, reg_out3 and the blurred hull mask, float64 [size, size, 10]
    (plane evaluation in `dt`; location, blur and everything else in float64)."""
    out = np.zeros((size, size, 10), np.float64)
    hull = None
    for m, t in enumerate(tabs):
        best, _, inside = locate(t, size)
        z = [np.asarray(v, np.float64) for v in planes_at(t, best, size, dt)]
        if m == 0:
            for k in range(3):
                out[..., k] = np.where(inside, z[k], 0.0)
        elif m < 3:
            my, mx = np.where(inside, z[0], np.nan), np.where(inside, z[1], np.nan)
            out[..., 3 * m], out[..., 3 * m + 1], out[..., 3 * m + 2] = my, mx, mx * 0
        else:
            hull = (inside & (z[0] > 0)).astype(np.float32)
    out[..., 9] = D.gaussian_blur5(hull)
    return out


def emulate(part, size, dt=np.float64):
    """numpy statement of csrc/prep_kernels.h for one row (test infrastructure)."""
    img, gt, box, tabs = part[:4]
    out = np.zeros((size, size, 16), np.float64)
    out[..., 0:3] = crop_planes(img, box, size, 255.0, dt)
    out[..., 3:6] = crop_planes(gt if gt is not None else img, box, size, 255.0, dt)
    with np.errstate(invalid="ignore"):
        out[..., 6:16] = mesh_channels(tabs[:4], size, dt)
    return out.astype(np.float32)


def statement_rows(parts, S):
    """prep_rows_kernel + prep_blur_kernel for a list of HostPart records: float32 [B, S, S, 16]."""
    return np.stack([emulate(p, S) for p in parts], 0)


def fp32_statement_rows(parts, S):
    """statement_rows with the crop-resize and the plane evaluation (a px + b py) + c done in float32 (point location stays float64):
    what a kernel quietly demoted to float32 would give."""
    return np.stack([emulate(p, S, np.float32) for p in parts], 0)


def statement_groups(parts, S, planes):
    """prep_groups_kernel<planes> + prep_blur_kernel for a list of HostPart records with eight tables: float32 [B, 2, S, S, planes + 10].
    Row 0 is the row kernel's statement (plus, with seven planes, the label plane's grey levels as they are); row 1 carries row 0's crop
    planes flipped in x and tables 4..7 on the same grid."""
    assert planes in (6, 7)
    out = np.zeros((len(parts), 2, S, S, planes + 10), np.float64)
    for b, p in enumerate(parts):
        assert len(p.tabs) == 8
        crop = [crop_planes(p.img, p.box, S), crop_planes(p.gt if p.gt is not None else p.img, p.box, S)]
        if planes == 7:
            crop.append(crop_planes(p.label, p.box, S, 1.0))
        crop = np.concatenate(crop, axis=2)
        out[b, 0, :, :, :planes], out[b, 1, :, :, :planes] = crop, crop[:, ::-1, :]
        with np.errstate(invalid="ignore"):
            out[b, 0, :, :, planes:], out[b, 1, :, :, planes:] = mesh_channels(p.tabs[:4], S), mesh_channels(p.tabs[4:], S)
    return out.astype(np.float32)


def culled_winner(t, lin, by, bx):
    """numpy statement of prep_rows_kernel's round-5 block culling for one 16x16-pixel block of one mesh: -> (index of the winning
    triangle per pixel, -1 when every triangle was culled; its min barycentric; how many triangles the block walks)."""
    gx0, gx1, gy0, gy1 = lin[bx * 16], lin[bx * 16 + 15], lin[by * 16], lin[by * 16 + 15]
    keep = np.ones(t.shape[0], bool)
    for i in range(3):
        mx = np.maximum(t[:, 3 * i] * gx0, t[:, 3 * i] * gx1)
        my = np.maximum(t[:, 3 * i + 1] * gy0, t[:, 3 * i + 1] * gy1)
        keep &= ((mx + my) + t[:, 3 * i + 2] >= -1.0e-9)
    idx = np.nonzero(keep)[0]                                   # survivors in their original order
    px, py = np.meshgrid(lin[bx * 16:bx * 16 + 16], lin[by * 16:by * 16 + 16])
    if idx.size == 0:
        return np.full(px.shape, -1), np.full(px.shape, -1.0e300), 0
    s = t[idx]
    l = np.stack([(s[:, 3 * i][:, None, None] * px + s[:, 3 * i + 1][:, None, None] * py) + s[:, 3 * i + 2][:, None, None] for i in range(3)], 0).min(0)
    best = l.argmax(0)                                          # first of equal maxima, as the kernel's strict `>`
    return idx[best], np.take_along_axis(l, best[None], 0)[0], int(idx.size)


def same_bits(got, want):
    """-> number of elements whose float32 bits differ, NaN (any payload) counting as equal to NaN."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape, (got.shape, want.shape)
    nan = np.isnan(want)
    return int(((got.view(np.uint32) != want.view(np.uint32)) & ~nan).sum() + (np.isnan(got) != nan).sum())


# ---- constructed meshes ----

def grid_mesh(mx, my, x0=0.0, x1=1.0, y0=0.0, y1=1.0, jitter=0.0, seed=0, snap=None, dtype=np.float64):
    """An explicit matplotlib.tri.Triangulation of (mx + 1) x (my + 1) vertices over [x0, x1] x [y0, y1], the cells' diagonals alternating:
    2 mx my triangles.  jitter: interior vertices moved by up to +-jitter in x and y (seeded).  snap = S: a vertex coordinate that is a
    multiple of 1 / (S - 1) becomes np.linspace(0, 1, S)'s own value, the bits of the kernels' grid."""
    import matplotlib.tri as mtri
    xs, ys = np.linspace(x0, x1, mx + 1), np.linspace(y0, y1, my + 1)
    if snap:
        lin = np.linspace(0, 1, snap)

        def snapped(v):
            k = np.rint(v * (snap - 1)).astype(int)
            return np.where(np.abs(v * (snap - 1) - k) < 1e-9, lin[k], v)
        xs, ys = snapped(xs), snapped(ys)
    x, y = [a.copy() for a in np.meshgrid(xs, ys)]
    if jitter:
        rng = np.random.default_rng(seed)
        x[1:-1, 1:-1] += rng.uniform(-jitter, jitter, (my - 1, mx - 1))
        y[1:-1, 1:-1] += rng.uniform(-jitter, jitter, (my - 1, mx - 1))
    tris = []
    for j in range(my):
        for i in range(mx):
            a, b, c, d = j * (mx + 1) + i, j * (mx + 1) + i + 1, (j + 1) * (mx + 1) + i + 1, (j + 1) * (mx + 1) + i
            tris += [[a, b, c], [a, c, d]] if (i + j) % 2 == 0 else [[a, b, d], [b, c, d]]
    x, y = x.reshape(-1).astype(dtype), y.reshape(-1).astype(dtype)
    tri = mtri.Triangulation(x, y, np.asarray(tris, np.int32))
    xd, yd = x.astype(np.float64), y.astype(np.float64)
    t = tri.triangles
    area = (xd[t[:, 1]] - xd[t[:, 0]]) * (yd[t[:, 2]] - yd[t[:, 0]]) - (xd[t[:, 2]] - xd[t[:, 0]]) * (yd[t[:, 1]] - yd[t[:, 0]])
    assert (area > 0).all() and t.shape[0] == 2 * mx * my          # the jitter folded no cell
    return tri


def values(tri, seed, hull_sign=None):
    """Three channels of seeded N(0, 1) float32 vertex values; hull_sign(x, y) -> the sign pattern of channel 0 (the hull's)."""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((3, tri.x.shape[0])).astype(np.float32)
    if hull_sign is not None:
        pos = hull_sign(np.asarray(tri.x), np.asarray(tri.y)) > 0              # large where positive: the zero crossing lies next to the others
        z[0] = np.where(pos, np.float32(2) + np.abs(z[0]), -(np.float32(0.25) + np.float32(0.1) * np.abs(z[0]))).astype(np.float32)
    return z


def table(tri, seed, hull_sign=None):
    return prep._tri_table(tri, list(values(tri, seed, hull_sign)))


def _image(seed, h, w):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _part(name, tabs, box=(2, 3, 34, 35), hw=(40, 44), seed=1, gt=False, label=None):
    img = _image(seed, *hw)
    return prep.HostPart(img, _image(seed + 1000, *hw) if gt else None, np.asarray(box, np.int32), list(tabs), name.encode(), None, label)


def _sliver_mesh():
    """grid_mesh(4, 4) whose cell [0.25, 0.5]^2 carries a fifth vertex P next to the midpoint of its diagonal a-c, so that the triangle
    (a, c, P) has 1e-6 of the square's area: its edge functions and plane coefficients are ~1e6.  The sliver stands FIRST in the table:
    the grid points of S = 32 on that diagonal lie on its edge."""
    import matplotlib.tri as mtri
    g = grid_mesh(4, 4)
    x, y, t = np.asarray(g.x), np.asarray(g.y), np.asarray(g.triangles)
    a, b, c, d = 1 * 5 + 1, 1 * 5 + 2, 2 * 5 + 2, 2 * 5 + 1          # the cell (i, j) = (1, 1): diagonal a-c
    cell = [k for k, tr in enumerate(t.tolist()) if set(tr) <= {a, b, c, d}]
    assert sorted(map(sorted, t[cell].tolist())) == sorted([sorted([a, b, c]), sorted([a, c, d])])
    diag = np.hypot(x[c] - x[a], y[c] - y[a])
    h = 2.0e-6 / diag                                               # area = diag * h / 2
    nx, ny = -(y[c] - y[a]) / diag, (x[c] - x[a]) / diag            # the unit normal towards d
    p = len(x)
    x, y = np.append(x, (x[a] + x[c]) / 2 + h * nx), np.append(y, (y[a] + y[c]) / 2 + h * ny)
    keep = [tr for k, tr in enumerate(t.tolist()) if k not in cell]
    tris = [[a, c, p]] + keep + [[a, b, c], [a, p, d], [p, c, d]]
    tri = mtri.Triangulation(x, y, np.asarray(tris, np.int32))
    t = tri.triangles
    area = 0.5 * ((x[t[:, 1]] - x[t[:, 0]]) * (y[t[:, 2]] - y[t[:, 0]]) - (x[t[:, 2]] - x[t[:, 0]]) * (y[t[:, 1]] - y[t[:, 0]]))
    assert (area > 0).all() and abs(area[0] - 1e-6) < 1e-9 and abs(area.sum() - 1.0) < 1e-12
    return tri


def _one_triangle():
    import matplotlib.tri as mtri
    return mtri.Triangulation(np.array([0.05, 0.97, 0.21]), np.array([0.03, 0.4, 0.9]), np.array([[0, 1, 2]], np.int32))


ORDINARY = dict(mx=5, my=4, jitter=0.03)                            # 40 triangles over the unit square


def _ordinary(seed):
    return table(grid_mesh(seed=seed, **ORDINARY), seed)


class MeshCase:
    """One constructed mesh case: the HostPart, its S, and the (Triangulation, vertex values) of each slot for the comparison with
    matplotlib's LinearTriInterpolator."""

    def __init__(self, name, S, slots, **part_kw):
        self.name, self.S, self.slots = name, S, slots
        self.part = _part(name, [prep._tri_table(tri, list(z)) for tri, z in slots], **part_kw)


def _same4(tri, seed, hull_sign=None):
    return [(tri, values(tri, seed, hull_sign))] * 4


def _border_sign(x, y):
    edge = (np.abs(x) < 1e-12) | (np.abs(x - 1) < 1e-12) | (np.abs(y) < 1e-12) | (np.abs(y - 1) < 1e-12)
    return np.where(edge, 1.0, -1.0)


def mesh_cases():
    """{name: MeshCase} of the issue's mesh table."""
    cases = [
        MeshCase("full256", 32, _same4(grid_mesh(16, 8), 11)),
        MeshCase("full256_jitter", 32, _same4(grid_mesh(16, 8, jitter=0.02, seed=12), 12)),
        MeshCase("on_edges_16", 16, _same4(grid_mesh(15, 5, snap=16), 13)),
        MeshCase("on_edges_32", 32, _same4(grid_mesh(31, 4, snap=32), 14)),
        MeshCase("on_edges_64", 64, _same4(grid_mesh(21, 6, snap=64), 15)),
        MeshCase("inset", 32, _same4(grid_mesh(16, 8, 0.1, 0.9, 0.2, 0.7, jitter=0.01, seed=16), 16)),
        # the inset mesh leaves no 16x16 block of S <= 64 without a surviving triangle (the cull is conservative); this one, in the top-left
        # corner, leaves the blocks to the right of and below it empty: the kernel then reads no triangle at all
        MeshCase("corner", 64, _same4(grid_mesh(4, 4, 0.0, 0.3, 0.0, 0.3, jitter=0.01, seed=22), 22)),
        MeshCase("border_hull", 32, _same4(grid_mesh(6, 6), 17, _border_sign)),
        MeshCase("sliver", 32, _same4(_sliver_mesh(), 18)),
    ]
    one, ordinary = _one_triangle(), grid_mesh(seed=19, **ORDINARY)
    cases.append(MeshCase("one_triangle", 32, [(one, values(one, 19)), (ordinary, values(ordinary, 19)), (one, values(one, 20)),
                                               (ordinary, values(ordinary, 21))]))
    return {c.name: c for c in cases}


# ---- constructed crops: an ordinary mesh, a random uint8 image ----

def crop_cases():
    """{name: (HostPart, S)}: every crop case of the issue at S = 32."""
    S = 32
    c = {
        "up_9": _part("up_9", [_ordinary(31)] * 4, (5, 7, 14, 16), (40, 50), 31),                    # n < S: upsampling
        "copy_32": _part("copy_32", [_ordinary(32)] * 4, (3, 4, 35, 36), (48, 40), 32),              # n = S
        "n_1": _part("n_1", [_ordinary(33)] * 4, (5, 6, 6, 7), (20, 30), 33),
        "n_2": _part("n_2", [_ordinary(34)] * 4, (5, 6, 7, 8), (20, 30), 34),
        "shrink_119": _part("shrink_119", [_ordinary(35)] * 4, (10, 5, 129, 124), (130, 140), 35),   # 119 / 32: no integer factor
        "right_bottom": _part("right_bottom", [_ordinary(36)] * 4, (30, 20, 94, 84), (60, 70), 36),
        "all_sides": _part("all_sides", [_ordinary(37)] * 4, (-10, -8, 54, 56), (20, 24), 37),       # an image smaller than the box
        "outside": _part("outside", [_ordinary(38)] * 4, (100, 90, 140, 130), (50, 50), 38),         # a box wholly outside: zeros
        "n_0": _part("n_0", [_ordinary(39)] * 4, (5, 5, 5, 5), (20, 30), 39),
        "tall": _part("tall", [_ordinary(40)] * 4, (3, 20, 43, 60), (91, 47), 40),                   # h != w
        "wide": _part("wide", [_ordinary(41)] * 4, (20, 3, 60, 43), (47, 91), 41),
        "with_gt": _part("with_gt", [_ordinary(42)] * 4, (4, 4, 52, 52), (60, 64), 42, gt=True),
    }
    return {k: (v, S) for k, v in c.items()}


def mixed_batch():
    """Nine parts of S = 32 with different h, w, ntri and box in one batch: the offsets in the blob."""
    m, c = mesh_cases(), crop_cases()
    parts = [m["full256"].part, c["shrink_119"][0], m["one_triangle"].part, c["with_gt"][0], m["inset"].part, c["n_0"][0], c["all_sides"][0],
             m["sliver"].part, c["tall"][0]]
    assert len({p.img.shape[:2] for p in parts}) >= 6 and len({p.tabs[0].shape[0] for p in parts}) >= 4
    return parts


# ---- groups: the item's tables and, for the mirror slots, a different, asymmetric mesh ----

def mirror_tables(seed=51):
    """Four tables for slots 4..7: fine cells on the left, one coarse column on the right, jittered — nothing about it is symmetric in x,
    so a block box taken from the wrong side culls triangles a pixel needs."""
    import matplotlib.tri as mtri
    g = grid_mesh(9, 5, jitter=0.015, seed=seed)
    x = np.asarray(g.x).copy()
    x = np.where(x < 1.0, x * x * 0.9, x)                               # columns crowd towards x = 0
    tri = mtri.Triangulation(x, np.asarray(g.y), np.asarray(g.triangles))
    t, y = tri.triangles, np.asarray(g.y)
    assert ((x[t[:, 1]] - x[t[:, 0]]) * (y[t[:, 2]] - y[t[:, 0]]) - (x[t[:, 2]] - x[t[:, 0]]) * (y[t[:, 1]] - y[t[:, 0]]) > 0).all()
    inset = grid_mesh(7, 3, 0.05, 0.6, 0.1, 0.95, jitter=0.01, seed=seed + 1)      # covers the left part of the square only
    return [table(tri, seed), table(inset, seed + 1), table(tri, seed + 2), table(inset, seed + 3)]


def as_group(part, label=None):
    """The row part as a group part: its four tables, then mirror_tables()."""
    return part._replace(tabs=list(part.tabs[:4]) + mirror_tables(), label=label)


def grey_label(h, w, seed=61):
    """A label plane holding the grey levels 0 / 1 / 2."""
    return np.ascontiguousarray(np.random.default_rng(seed).integers(0, 3, (h, w), dtype=np.uint8))


def hull_margin(part, size, slots=(3,)):
    """The smallest |z0| of the hull slots over the grid points inside their mesh: the `z0 > 0` threshold must not be a rounding question."""
    lo = np.inf
    for s in slots:
        best, _, inside = locate(part.tabs[s], size)
        z0 = planes_at(part.tabs[s], best, size)[0]
        if inside.any():
            lo = min(lo, float(np.abs(z0[inside]).min()))
    return lo
