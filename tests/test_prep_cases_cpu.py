"""The numpy statement of the preparation kernels (tests/prep_cases.py) held to the host path it restates, without a GPU: matplotlib's
LinearTriInterpolator on the constructed meshes, dataset.resize_linear on the constructed crops, dataset.gaussian_blur5, and
dataset.build_row on golden UCB items — and the proof that the bit-for-bit bar of tests/test_prep_edges_gpu.py has teeth: the same
statement with float32 planes and crops fails it on most elements while staying inside the old 1e-6."""
import os

import numpy as np
import pytest

from blindshadowremoval_amd import dataset as D
from blindshadowremoval_amd import prep
import prep_cases as C
from tsm_group_cases import ucb_items

MESH = C.mesh_cases()
CROP = C.crop_cases()
TIE_CAP = 0.005            # values may differ from matplotlib's (by one float32 ulp) on at most this share of a case's inside elements


def _ulp_apart(a, b):
    """|a - b| in units of the float32 spacing at the larger magnitude."""
    a, b = a.astype(np.float32), b.astype(np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(a), np.abs(b))).astype(np.float64)


@pytest.mark.parametrize("name", sorted(MESH))
def test_statement_against_matplotlib(name):
    import matplotlib.tri as mtri
    case = MESH[name]
    S = case.S
    xi, yi = np.meshgrid(np.linspace(0, 1, S), np.linspace(0, 1, S))
    n_in = n_diff = 0
    seen = {}
    for m, (tri, z) in enumerate(case.slots):
        if id(tri) in seen and seen[id(tri)] is z:
            continue                                              # the same table in several slots
        seen[id(tri)] = z
        t = case.part.tabs[m]
        best, _, inside = C.locate(t, S)
        got = C.planes_at(t, best, S)
        for k in range(3):
            ref = mtri.LinearTriInterpolator(tri, z[k].astype(np.float64))(xi, yi)
            ref_in = ~np.ma.getmaskarray(ref)
            assert np.array_equal(ref_in, inside), (name, m, k, int((ref_in != inside).sum()))
            a, b = got[k][inside].astype(np.float32), np.ma.filled(ref, np.nan)[inside].astype(np.float32)
            assert (_ulp_apart(a, b) <= 1.0).all(), (name, m, k, float(_ulp_apart(a, b).max()))
            n_in += a.size
            n_diff += int((a.view(np.uint32) != b.view(np.uint32)).sum())
    print("%s: %d of %d inside elements differ from LinearTriInterpolator by one float32 ulp (%.3f %%)" % (name, n_diff, n_in, 100.0 * n_diff / n_in))
    assert n_diff <= TIE_CAP * n_in, (name, n_diff, n_in)
    margin = C.hull_margin(case.part, S)
    assert margin >= 1e-9, (name, margin)                         # z0 > 0 is never a rounding question


def _on_edge(t, S):
    """Grid points whose winning triangle has min(l_i) within rounding of 0: on an edge or a vertex of the mesh."""
    _, lm, inside = C.locate(t, S)
    return int((inside & (np.abs(lm) < 1e-12)).sum())


def test_the_cases_reach_what_they_are_for():
    assert all(t.shape[0] == 256 for n in ("full256", "full256_jitter", "inset") for t in MESH[n].part.tabs)
    assert MESH["on_edges_32"].part.tabs[0].shape[0] == 248 and MESH["on_edges_64"].part.tabs[0].shape[0] == 252
    assert _on_edge(MESH["on_edges_16"].part.tabs[0], 16) == 256 and _on_edge(MESH["on_edges_32"].part.tabs[0], 32) == 1024
    assert _on_edge(MESH["on_edges_64"].part.tabs[0], 64) == 1702
    assert _on_edge(MESH["sliver"].part.tabs[0], 32) > 0 and np.abs(MESH["sliver"].part.tabs[0][0, :9]).max() > 1e5
    assert [t.shape[0] for t in MESH["one_triangle"].part.tabs] == [1, 40, 1, 40]
    # inset: NaN outside in the offset slots (mx * 0 too), 0 in the uv slot and the hull plane; and, for `corner`,
    # whole blocks without a surviving triangle
    row = C.statement_rows([MESH["inset"].part], 32)[0]
    out = ~C.locate(MESH["inset"].part.tabs[0], 32)[2]
    assert out.any() and np.isnan(row[out][:, 9:15]).all() and not row[out][:, 6:9].any() and np.isfinite(row[~out]).all()
    lin = np.linspace(0, 1, 64)
    walked = [C.culled_winner(MESH["corner"].part.tabs[0], lin, by, bx)[2] for by in range(4) for bx in range(4)]
    assert walked.count(0) >= 4 and walked[0] == 32, walked
    # border_hull: ones along all four borders and in the corners, zeros in the middle -> every reflected tap of the blur is live
    best, _, inside = C.locate(MESH["border_hull"].part.tabs[3], 32)
    hull = inside & (C.planes_at(MESH["border_hull"].part.tabs[3], best, 32)[0] > 0)
    assert hull[:2].all() and hull[-2:].all() and hull[:, :2].all() and hull[:, -2:].all() and not hull[12:20, 12:20].any()
    face = C.statement_rows([MESH["border_hull"].part], 32)[0, :, :, 15]
    assert face[0, 0] == 1 and face[-1, -1] == 1 and face[16, 16] == 0 and ((face > 0) & (face < 1)).any()


@pytest.mark.parametrize("name", sorted(MESH))
def test_block_culling_keeps_every_winner_on_the_constructed_meshes(name):
    """tests/test_prep_gpu.py::test_block_culling_keeps_every_winner on the constructed tables, at every S the GPU test runs them."""
    case = MESH[name]
    for S in sorted({case.S} | ({16, 32, 48, 64} if name in ("full256", "inset") else set())):
        lin = np.linspace(0, 1, S)
        for t in {id(t): t for t in case.part.tabs}.values():
            full_best, full_l, inside = C.locate(t, S)
            for by in range(S // 16):
                for bx in range(S // 16):
                    cb, cl, _ = C.culled_winner(t, lin, by, bx)
                    sl = (slice(by * 16, by * 16 + 16), slice(bx * 16, bx * 16 + 16))
                    assert np.array_equal(cb[inside[sl]], full_best[sl][inside[sl]]), (name, S, by, bx)
                    assert np.array_equal(cl >= -1e-12, inside[sl]), (name, S, by, bx)


def _plain_crop(im, box):
    """The zero-extended n x n crop, written pixel by pixel."""
    n = int(box[2] - box[0])
    c = np.zeros((n, n, 3), np.float64)
    for y in range(n):
        for x in range(n):
            iy, ix = y + int(box[1]), x + int(box[0])
            if 0 <= iy < im.shape[0] and 0 <= ix < im.shape[1]:
                c[y, x] = im[iy, ix] / 255.0
    return c


@pytest.mark.parametrize("name", sorted(CROP))
def test_crop_planes_against_resize_linear(name):
    part, S = CROP[name]
    got = C.statement_rows([part], S)[0, :, :, :6]
    n = int(part.box[2] - part.box[0])
    for which, im in enumerate((part.img, part.gt if part.gt is not None else part.img)):
        want = D.resize_linear(_plain_crop(im, part.box), S).astype(np.float32) if n > 0 else np.zeros((S, S, 3), np.float32)
        assert np.array_equal(got[..., 3 * which:3 * which + 3].view(np.uint32), want.view(np.uint32)), (name, which)
    x0, y0 = int(part.box[0]), int(part.box[1])
    if name == "copy_32":
        assert np.array_equal(got[..., :3], (part.img[y0:y0 + S, x0:x0 + S].astype(np.float64) / 255.0).astype(np.float32))
    if name in ("outside", "n_0"):
        assert not got.any()
    if name == "n_1":
        assert np.array_equal(got[..., :3], np.broadcast_to((part.img[y0, x0].astype(np.float64) / 255.0).astype(np.float32), (S, S, 3)))
    if name in ("right_bottom", "all_sides"):
        assert not got[-1, -1].any() and got[6, 6, :3].any()
        assert (not got[0, 0].any()) == (name == "all_sides")
    if name == "with_gt":
        assert not np.array_equal(got[..., :3], got[..., 3:])
    else:
        assert np.array_equal(got[..., :3], got[..., 3:])


def _kernel_blur(h):
    """prep_blur_kernel as written: reflected indices, the inner sum along x from the left, the outer along y from the top."""
    S = h.shape[0]
    k = [1.0 / 16.0, 4.0 / 16.0, 6.0 / 16.0, 4.0 / 16.0, 1.0 / 16.0]
    refl = lambda i: -i if i < 0 else (2 * S - 2 - i if i >= S else i)
    out = np.zeros((S, S), np.float64)
    for oy in range(S):
        for ox in range(S):
            acc = 0.0
            for i in range(5):
                tmp = 0.0
                for j in range(5):
                    tmp = tmp + k[j] * float(h[refl(oy + i - 2), refl(ox + j - 2)])
                acc = acc + k[i] * tmp
            out[oy, ox] = acc
    return out


def test_blur_against_gaussian_blur5():
    best, _, inside = C.locate(MESH["border_hull"].part.tabs[3], 32)
    masks = [(inside & (C.planes_at(MESH["border_hull"].part.tabs[3], best, 32)[0] > 0)).astype(np.float32)]
    rng = np.random.default_rng(3)
    masks += [(rng.random((S, S)) < 0.5).astype(np.float32) for S in (16, 48)]
    for h in masks:
        assert np.array_equal(_kernel_blur(h), D.gaussian_blur5(h))
    assert np.array_equal(C.statement_rows([MESH["border_hull"].part], 32)[0, :, :, 15], D.gaussian_blur5(masks[0]).astype(np.float32))


@pytest.mark.parametrize("k", range(8))
def test_statement_equals_build_row_on_golden_items(k):
    """Every element of the row, NaNs in the same places: nothing in the host chain forces a tolerance."""
    lm_path, gt = ucb_items()[6 + 12 * k]                          # eight of the 100, spread over the subjects
    want = D.build_row(os.path.splitext(lm_path)[0] + ".png", lm_path, gt, 256)[0]
    got = C.statement_rows([prep.host_part((lm_path, gt, 256))], 256)[0]
    assert C.same_bits(got, want) == 0, (lm_path, C.same_bits(got, want))


def test_groups_statement_restates_the_rows():
    part = C.as_group(CROP["right_bottom"][0], C.grey_label(60, 70))
    g = C.statement_groups([part], 32, 7)[0]
    r = C.statement_rows([part], 32)[0]
    assert g.shape == (2, 32, 32, 17)
    assert C.same_bits(g[0, :, :, :6], r[..., :6]) == 0 and C.same_bits(g[0, :, :, 7:], r[..., 6:]) == 0
    assert C.same_bits(g[1, :, :, :7], g[0, :, ::-1, :7]) == 0
    assert C.same_bits(g[1, :, :, 7:], C.statement_rows([part._replace(tabs=part.tabs[4:])], 32)[0, :, :, 6:]) == 0
    assert set(np.unique(g[0, :, :, 6][:8, :8])) <= {0.0, 1.0, 2.0} or g[0, :, :, 6].max() <= 2.0       # grey levels, not / 255
    assert g[0, :, :, 6].max() > 1.0
    assert not C.statement_groups([C.as_group(CROP["n_0"][0])], 32, 6)[0, :, :, :, :6].any()
    assert np.isnan(g[1, :, :, 10:13]).any()                       # the mirror slots' inset mesh leaves part of the square uncovered


def test_mixed_batch_packs():
    parts = C.mixed_batch()
    blob, rows_off, _ = prep.pack_batch(parts, 32)
    rows = np.frombuffer(blob, prep.ROW_DTYPE, count=len(parts), offset=rows_off)
    assert len(parts) >= 7 and len({int(r["img_off"]) for r in rows}) == len(parts)
    assert [r["gt_off"] == r["img_off"] for r in rows] == [p.gt is None for p in parts]


def test_float32_planes_and_crops_fail_the_bit_bar_but_pass_1e_6(golden_dir):
    """What the bit-for-bit comparison sees and the 1e-6 comparison cannot: the plane evaluation and the crop-resize in float32."""
    part = MESH["full256"].part
    want, got = C.statement_rows([part], 32)[0], C.fp32_statement_rows([part], 32)[0]
    interp = [6, 7, 8, 9, 10, 12, 13]                              # the seven interpolated channels (11 and 14 are mx * 0)
    share = float((want[..., interp].view(np.uint32) != got[..., interp].view(np.uint32)).mean())
    print("full256: float32 planes differ in %.1f %% of the interpolated elements, by at most %.2e" % (100 * share, np.abs(want - got).max()))
    assert share > 0.5
    part, S = CROP["shrink_119"]
    want, got = C.statement_rows([part], S)[0, :, :, :6], C.fp32_statement_rows([part], S)[0, :, :, :6]
    n = int((want.view(np.uint32) != got.view(np.uint32)).sum())
    print("shrink_119: float32 crop-resize differs in %d of %d crop elements, by at most %.2e" % (n, want.size, np.abs(want - got).max()))
    assert n >= 1 and np.abs(want - got).max() <= 1e-6
    # the data the 1e-6 tests run on: the golden sample at S = 256
    base = os.path.join(golden_dir, "sample_imgs", "02165", "02165")
    part = prep.host_part((base + ".npy", None, 256))
    want, got = C.statement_rows([part], 256)[0], C.fp32_statement_rows([part], 256)[0]
    share = float((want[..., interp].view(np.uint32) != got[..., interp].view(np.uint32)).mean())
    print("sample 02165: float32 planes and crops differ in %.1f %% of the interpolated elements, by at most %.2e" % (100 * share, np.abs(want - got).max()))
    assert share > 0.25 and C.same_bits(got[..., :6], want[..., :6]) > 0 and np.abs(want - got).max() <= 1e-6


def test_tri_table_refuses_more_than_256_triangles():
    tri = C.grid_mesh(43, 3)
    assert tri.triangles.shape[0] == 258
    with pytest.raises(ValueError):
        prep._tri_table(tri, [np.zeros(tri.x.shape[0])])
    assert prep._tri_table(C.grid_mesh(16, 8), [np.zeros(17 * 9)]).shape == (256, prep.TRI_DOUBLES)
