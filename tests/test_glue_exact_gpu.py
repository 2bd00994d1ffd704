"""-m gpu: the forward's glue arithmetic — gray / gs / mask22 / dif, the 8x resizes behind d32, bmask, uv_s and the TSM offsets, and the
ShareLayer warp — held to the float32 statement of tests/glue_cases.py bit for bit.  `bmask = d32 > 0.1` (model.py:256) is a hard
threshold: one ulp of d32 flips an 8x8 block of the image and everything downstream, so these kernels are not held to a tolerance.

Every case feeds the statement the device's own upstream tensors (the pattern of tests/stage_parity.py) and compares `.view(uint32)`;
the one exception is the relu lanes 0 and 2 of mask22, compared with ==, because the reference does not pin the sign of max(+-0, 0).
Each case also shows that the comparison has teeth: the contracted / re-ordered variants of the statement differ from what the device
wrote, so a kernel computing them could not pass.  The figures each case prints are recorded in DESIGN.md (the glue row)."""
import numpy as np
import pytest
import torch

import glue_cases as G
from blindshadowremoval_amd.weights import init_weights

pytestmark = pytest.mark.gpu

f32 = np.float32
DTYPES = ("f32", "f32x3", "f16")
C_X, C_R = 96, 291            # TSM: x0 = [x 96 | share 192 | uv 3], xh = [x_hole 291 | bmask | share 582 | uv 3]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _ndiff(got, want):
    assert got.shape == want.shape, (got.shape, want.shape)
    return int((_bits(got) != _bits(want)).sum())


def _line(what, got, want):
    """One report line for `got` against the statement `want`, and whether they are the same bits."""
    n = _ndiff(got, want)
    line = "%s: %d of %d differ (%.2f %%)" % (what, n, got.size, 100.0 * n / got.size)
    if n:
        i = np.unravel_index(int(np.argmax(_bits(got) != _bits(want))), got.shape)
        line += ", first at %s: device %r statement %r" % (tuple(int(k) for k in i), float(got[i]), float(want[i]))
    print(line)
    return line, n == 0


class _Check:
    """Collects the lines of a case so that every shape's figure is printed before the case fails."""

    def __init__(self):
        self.bad = []

    def same(self, what, got, want):
        line, ok = _line(what, got, want)
        if not ok:
            self.bad.append(line)

    def teeth(self, what, got, variant):
        n = _ndiff(got, variant)
        print("teeth %s: differs from the device in %d of %d (%.1f %%)" % (what, n, got.size, 100.0 * n / got.size))
        if n == 0:
            self.bad.append("%s: a kernel computing this variant would have passed" % what)

    def done(self):
        assert not self.bad, "\n".join(self.bad)


# ---- handles and forwards, shared by the cases of this module ----

_BASE = {}


def _weights(variant, key):
    if variant not in _BASE:
        _BASE[variant] = init_weights(1, variant=variant)
    w = _BASE[variant]
    if key == "init":
        return w
    if key == "con_bias":                       # con == 0.25 exactly, mask live
        return G.head_weights(w, True, G.CON_BIAS)
    if key == "both_bias":                      # con == 0.25, mask == tanh(0)
        return G.head_weights(w, False, G.CON_BIAS, 0.0)
    assert key == "plant"                       # con == 0, mask == tanh(20)
    return G.head_weights(w, False, 0.0, 20.0)


@pytest.fixture(scope="module")
def run():
    """run(variant, dtype, key, inputs, uv, reg=None, frame=0, packed=False, timing=False) -> the forward's outputs and glue probes as
    numpy arrays (cached: the cases share forwards), plus `launches` when timed."""
    from blindshadowremoval_amd import Generator, GeneratorTSM
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    gens, runs = {}, {}

    def go(variant, dtype, key, tag, inputs, uv, reg=None, frame=0, packed=False, timing=False):
        rk = (variant, dtype, key, tag, frame, packed, timing)
        if rk in runs:
            return runs[rk]
        gk = (variant, dtype, key)
        if gk not in gens:
            gens[gk] = (GeneratorTSM if variant == "tsm" else Generator)(dtype=dtype).load_weights(_weights(variant, key))
        gen = gens[gk]
        ti, tu = torch.from_numpy(inputs).cuda(), torch.from_numpy(uv).cuda()
        if timing:
            gen.set_timing(True)
        if variant == "tsm":
            out = gen(ti, tu, torch.from_numpy(reg).cuda(), frame, True)
        elif packed:
            buf = torch.full((*inputs.shape[:3], 4), float("nan"), device="cuda")
            out = gen(ti, tu, packed_out=buf)
        else:
            out = gen(ti, tu)
        torch.cuda.synchronize()
        r = {k: t.cpu().numpy() for k, t in zip(("gs", "con_rgb", "mask22", "dif"), out)}
        if packed:
            r["packed"] = buf.cpu().numpy()
        if timing:
            r["launches"] = [n for n, _, _ in gen.get_launch_timing()]
            gen.set_timing(False)
        if tag != "fused":                      # the fused case reads the outputs only
            r.update({k: gen.probe(k).cpu().numpy() for k in ("d32", "bmask", "x0", "xh")})
        r.update(inputs=inputs, uv=uv, reg=reg)
        runs[rk] = r
        return r

    yield go
    for g in gens.values():
        g.close()


def _gsc_fields(uv_kind="uniform"):
    for B, H, W in G.GSC_SHAPES:
        uv = G.uniform_field((B, H, W), 400 + H)
        if uv_kind == "wide":
            uv = ((uv - f32(0.5)) * f32(8)).astype(np.float32)              # +-4: wide-range taps are where the resize orders part
        yield (B, H, W), "%dx%dx%d/%s" % (B, H, W, uv_kind), G.uniform_field((B, H, W), 100 + H), uv


def _smooth_reg(frame):
    from stage_parity import smooth_reg
    return smooth_reg(G.TSM_SHAPE[0], G.TSM_SHAPE[1], torch.Generator().manual_seed(500 + frame)).numpy()


def _tsm_fields(uv_kind="uniform"):
    B, H, W = G.TSM_SHAPE
    uv = G.uniform_field((B, H, W), 400 + H)
    if uv_kind == "wide":
        uv = ((uv - f32(0.5)) * f32(8)).astype(np.float32)
    return "tsm/%s" % uv_kind, G.uniform_field((B, H, W), 100 + H), uv


def _all_runs(run, dtype, uv_kind="uniform", key="init"):
    """The GSC shapes and the TSM frames of a case: (label, forward)."""
    for shape, tag, inputs, uv in _gsc_fields(uv_kind):
        yield "gsc %s %s" % (dtype, tag), run("gsc", dtype, key, tag, inputs, uv)
    tag, inputs, uv = _tsm_fields(uv_kind)
    for frame in (2, 4):
        yield "tsm %s %s frame %d" % (dtype, tag, frame), run("tsm", dtype, key, tag + "/smooth", inputs, uv, _smooth_reg(frame), frame)


# ---- A. the final dif (model.py:288, the colour tail's epilogue in csrc/conv_n16.h) ----

@pytest.mark.parametrize("dtype", DTYPES)
def test_final_dif_is_the_float32_statement(run, dtype):
    c = _Check()
    for label, r in _all_runs(run, dtype):
        c.same("A %s dif" % label, r["dif"], G.final_dif(r["con_rgb"], r["inputs"]))
        for v in G.GRAY_CONTRACTIONS:
            c.teeth("A %s dif with gray contracted %s" % (label, v), r["dif"], G.final_dif(r["con_rgb"], r["inputs"], v))
    for shape, tag, inputs, uv in _gsc_fields():
        plain, r = run("gsc", dtype, "init", tag, inputs, uv), run("gsc", dtype, "init", tag, inputs, uv, packed=True)
        c.same("A gsc %s %s packed lanes 0:3 against the plain con_rgb" % (dtype, tag), r["packed"][..., :3], plain["con_rgb"])
        c.same("A gsc %s %s packed lane 3 against the plain dif" % (dtype, tag), r["packed"][..., 3:], plain["dif"])
        c.same("A gsc %s %s packed dif" % (dtype, tag), r["packed"][..., 3:], G.final_dif(r["packed"][..., :3], inputs))
        for k in ("gs", "mask22"):
            c.same("A gsc %s %s packed form's %s" % (dtype, tag, k), r[k], plain[k])
    c.done()


# ---- B. gs and mask22 (model.py:250,252: heads_post_kernel, and heads_emit of the fused epilogue) ----

def _check_heads(c, label, r):
    """gs / mask22 of a forward whose con head is the bias 0.25: the mask is read back from the device's mask22."""
    m22 = r["mask22"]
    mask = m22[..., 0:1] - m22[..., 2:3]                                   # one of the two is zero: exact
    mask = np.where(mask == 0, m22[..., 1:2], mask)                        # a zero mask has the sign lane 1 = mask * 0 carries
    gs, want22 = G.heads(mask, G.CON_BIAS, r["inputs"])
    c.same("B %s gs" % label, r["gs"], gs)
    if not ((m22[..., 0] == want22[..., 0]).all() and (m22[..., 2] == want22[..., 2]).all()):
        c.bad.append("B %s: mask22 lanes 0 / 2 are not relu(mask) / relu(-mask)" % label)
    if not ((m22[..., 0] * m22[..., 2] == 0).all() and m22.min() >= 0 and m22.max() <= 1):
        c.bad.append("B %s: mask22 lanes 0 / 2 overlap or leave [0, 1]" % label)
    c.same("B %s mask22 lane 1 (mask * 0)" % label, m22[..., 1:2], want22[..., 1:2])
    c.teeth("B %s gs as one fused multiply-add" % label, r["gs"], G.heads(mask, G.CON_BIAS, r["inputs"], contract=True)[0])
    assert float(np.abs(mask).max()) > 0.1, "the mask head is live"


@pytest.mark.parametrize("dtype", DTYPES)
def test_gs_and_mask22_are_the_float32_statement(run, dtype):
    c = _Check()
    for shape, tag, inputs, uv in _gsc_fields():
        label = "gsc %s %s" % (dtype, tag)
        r0 = run("gsc", dtype, "both_bias", tag, inputs, uv)               # nothing but the bias enters con, nothing at all the mask
        c.same("B %s gs with both heads reduced to their biases" % label, r0["gs"], G.gray(inputs) + G.CON_BIAS)
        c.same("B %s mask22 of a zero mask" % label, r0["mask22"], np.zeros_like(r0["mask22"]))
        r = run("gsc", dtype, "con_bias", tag, inputs, uv, timing=True)
        assert "heads" in r["launches"] and "heads_post" in r["launches"], label      # the two-launch form (these batches)
        _check_heads(c, label + " two launches", r)
    c.done()


@pytest.mark.parametrize("dtype", DTYPES)
def test_fused_heads_epilogue_is_the_float32_statement(run, dtype):
    """B * H / 8 = 1024 row strips (the count of the 32 x 256 x 256 batch tests/test_gpu_parity.py shows fused): heads_emit runs."""
    B, H, W = G.FUSED_SHAPE
    inputs, uv = G.uniform_field((B, H, W), 600), G.uniform_field((B, H, W), 601)
    r = run("gsc", dtype, "con_bias", "fused", inputs, uv, timing=True)
    assert "heads" in r["launches"] and "heads_post" not in r["launches"], "the fused epilogue did not run: raise B"
    c = _Check()
    _check_heads(c, "gsc %s %dx%dx%d fused" % (dtype, B, H, W), r)
    c.done()


# ---- C. d32 and bmask (model.py:251,256: bmask_xhole_kernel) ----

@pytest.mark.parametrize("dtype", DTYPES)
def test_d32_and_bmask_are_the_float32_statement(run, dtype):
    """Measured before the kernels took compute_lerp's order (the sum-of-halves resize): see DESIGN.md, the glue row."""
    c = _Check()
    for label, r in _all_runs(run, dtype):
        d32, bm = G.d32_bmask(r["gs"], r["inputs"])
        c.same("C %s d32" % label, r["d32"], d32)
        c.same("C %s bmask" % label, r["bmask"], bm)
        lane = C_R if label.startswith("tsm") else 257
        c.same("C %s xh[..., %d] against the bmask probe" % (label, lane), r["xh"][..., lane:lane + 1], r["bmask"])
        print("C %s: %d of %d cells in the mask" % (label, int(bm.sum()), bm.size))
        c.teeth("C %s d32 in the old resize order" % label, r["d32"], G.d32_bmask(r["gs"], r["inputs"], order="old")[0])
        for v in G.GRAY_CONTRACTIONS:
            c.teeth("C %s d32 with gray contracted %s" % (label, v), r["d32"], G.d32_bmask(r["gs"], r["inputs"], v)[0])
    c.done()


# ---- D. uv_s (model.py:237-238,259: uv_resize8_kernel) ----

@pytest.mark.parametrize("dtype", DTYPES)
def test_uv_s_is_the_float32_statement(run, dtype):
    c = _Check()
    for kind in ("uniform", "wide"):
        for label, r in _all_runs(run, dtype, kind):
            want = G.resize8(r["uv"])
            a = slice(288, 291) if label.startswith("tsm") else slice(96, 99)
            c.same("D %s uv lanes of x0" % label, r["x0"][..., a], want)
            c.same("D %s uv lanes of xh" % label, r["xh"][..., -3:], want)
            if not label.startswith("tsm"):
                assert r["xh"].shape[-1] == 261
            c.teeth("D %s uv_s in the old resize order" % label, r["x0"][..., a], G.resize8(r["uv"], "old"))
    c.done()


# ---- E. the threshold, planted ----

def test_planted_threshold_cells_fall_on_the_statements_side(run):
    inputs, index = G.planted_threshold()
    r = run("gsc", "f32", "plant", "plant", inputs, G.uniform_field(G.PLANT_SHAPE, 700))
    g0 = G.gray(inputs)
    # the preconditions, on the device: tanhf(20) == 1, and then gs = 2 g0 and fl(gs - g0) = g0, so a cell's taps are the planted grays
    assert (r["mask22"][..., 0] == 1).all() and (r["mask22"][..., 1:] == 0).all()
    assert _ndiff(r["gs"], f32(2) * g0) == 0 and _ndiff(r["gs"] - g0, g0) == 0
    d32, bm = G.d32_bmask(r["gs"], inputs)
    got_d, got_b = r["d32"].ravel(), r["bmask"].ravel()
    lines = []
    for cls in G.PLANT_CLASSES:
        i = index[cls]
        nd, nb = _ndiff(got_d[i], d32.ravel()[i]), int((got_b[i] != bm.ravel()[i]).sum())
        lines.append("E %-22s %d cells: d32 differs in %d, bmask in %d" % (cls, len(i), nd, nb))
    rest = np.setdiff1d(np.arange(d32.size), np.concatenate(list(index.values())))
    lines.append("E %-22s %d cells: d32 differs in %d, bmask in %d" % ("ordinary", len(rest), _ndiff(got_d[rest], d32.ravel()[rest]),
                                                                       int((got_b[rest] != bm.ravel()[rest]).sum())))
    print("\n".join(lines))
    assert _ndiff(r["d32"], d32) == 0 and (r["bmask"] == bm).all(), "\n".join(lines)
    assert _ndiff(r["xh"][..., 257:258], bm) == 0


# ---- F. the TSM ShareLayer (reg_resize8_kernel, share_reduce_kernel, share_unwarp_kernel) ----

@pytest.mark.parametrize("frame", [2, 4])
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_share_layer_is_the_float32_statement(run, dtype, frame):
    tag, inputs, uv = _tsm_fields()
    B, S = G.TSM_SHAPE[0], G.TSM_SHAPE[1] // 8
    reg_int, k_int = G.block_reg(B, S, G.INT_OFFSETS, 800 + frame)
    reg_half, _ = G.block_reg(B, S, G.HALF_OFFSETS, 810 + frame)
    c = _Check()
    for kind, reg in (("smooth", _smooth_reg(frame)), ("whole cells", reg_int), ("half cells", reg_half)):
        r = run("tsm", dtype, "init", tag + "/" + kind, inputs, uv, reg, frame)
        label = "F tsm %s frame %d %s offsets" % (dtype, frame, kind)
        x0, xh = r["x0"], r["xh"]
        assert x0.shape[-1] == C_R and xh.shape[-1] == 3 * C_R + 4
        c.same(label + ": share lanes of x0", x0[..., C_X:3 * C_X], G.share_layer32(x0[..., :C_X], reg, frame))
        c.same(label + ": share lanes of xh", xh[..., C_R + 1:3 * C_R + 1], G.share_layer32(xh[..., :C_R], reg, frame))
        if kind == "whole cells":
            ki = k_int.astype(np.int64)
            c.same(label + ": share lanes of x0 as a gather", x0[..., C_X:3 * C_X], G.share_layer_gather(x0[..., :C_X], ki[..., :2], ki[..., 2:], frame))
            c.same(label + ": share lanes of xh as a gather", xh[..., C_R + 1:3 * C_R + 1],
                   G.share_layer_gather(xh[..., :C_R], ki[..., :2], ki[..., 2:], frame))
            for b0 in range(0, B, frame):       # the max lanes only move values of the group's x about (+0 for a -0 the lerp passed)
                grp = x0[b0:b0 + frame, ..., :C_X]
                if not np.isin(x0[b0:b0 + frame, ..., C_X:2 * C_X], grp + f32(0)).all():
                    c.bad.append(label + ": the max lanes of x0 hold a value that is not in x")
    c.done()
