"""-m gpu: the fp32 colour tail alone in Winograd F(2x2, 3x3) form (csrc/wino_clr.h, through bsr_debug_wino_clr) against the float64 statement
of the tail (wino_clr_cases.tail64: the oracle's colour_tail arithmetic in float64) on constructed inputs, and the whole forward in both forms.

Tolerance of the kernel alone: max|gpu - ref| / max|ref| <= 1e-5 for con_rgb and for dif, the project's fp32 stage ceiling
(tests/test_stage_parity_gpu.py: F32_CEILING).  The float32 emulation of the kernel's arithmetic lands at 3.0e-7 .. 4.1e-7 for clr_conv1
(tests/test_wino_clr_cpu.py).  Whole forward, Winograd against direct form: con_rgb / dif within 3 x the emulated error of max|output|.

Measured on MI355X: see MEASURED below (filled from the test's own printout)."""
import ctypes

import numpy as np
import pytest
import torch

from blindshadowremoval_amd.weights import init_weights
from wino_clr_cases import EMULATED_ERROR, images, random_inputs, random_weights, tail64

TOL = 1e-5              # F32_CEILING
CANARY = -77.25
GUARD = 4096            # floats on each side of each output allocation

# max|gpu - ref| / max|ref| (con_rgb, dif) as printed by the tests below on MI355X
MEASURED = ("random cases con_rgb 3.2e-7 .. 4.3e-7, dif 2.6e-7 .. 5.3e-7 (the direct form on the same inputs: 5.4e-7 .. 6.5e-7, 3.5e-7 .. 7.3e-7); "
            "stride 96 3.7e-7, 4.8e-7; impulses in f 2.5e-7, 1.3e-7, in gs 3.0e-7, 2.3e-7; whole forward, the two forms apart: con_rgb 8.5e-7, dif 1.5e-7 of max|output|")


def _run(gs, f, inputs, w, wino=1, packed=False, in_cs=64):
    """-> (con_rgb [B,H,W,3], dif [B,H,W,1]) on the host; the outputs' guards and, with in_cs > 64, the unread channels are checked here."""
    from blindshadowremoval_amd import _lib
    lib = _lib.load()
    B, H, W, _ = f.shape
    direct, w_gs, bias, tail = images(w)
    fs = torch.full((B, H, W, in_cs), 1e30)                     # the channels past 64 must not be read
    fs[..., :64] = torch.from_numpy(f)
    d_gs, d_f, d_in = torch.from_numpy(gs).cuda(), fs.cuda(), torch.from_numpy(inputs).cuda()
    npix = B * H * W
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)

    def guarded(n):
        buf = torch.full((n + 2 * GUARD,), CANARY).cuda()
        return buf, buf[GUARD:GUARD + n]

    def untouched(buf, n):
        host = buf.cpu()
        assert bool((host[:GUARD] == CANARY).all()) and bool((host[GUARD + n:] == CANARY).all()), "guard region written"
        return host[GUARD:GUARD + n]

    if packed:
        bp, p = guarded(npix * 4)
        _lib.check(lib.bsr_debug_wino_clr(d_gs.data_ptr(), d_f.data_ptr(), in_cs, d_in.data_ptr(), ptr(direct), ptr(w_gs), ptr(bias), ptr(tail),
                                          None, None, p.data_ptr(), B, H, W, wino, None), "bsr_debug_wino_clr")
        torch.cuda.synchronize()
        out = untouched(bp, npix * 4).reshape(B, H, W, 4)
        return out[..., :3].contiguous(), out[..., 3:].contiguous()
    bc, c = guarded(npix * 3)
    bd, d = guarded(npix)
    _lib.check(lib.bsr_debug_wino_clr(d_gs.data_ptr(), d_f.data_ptr(), in_cs, d_in.data_ptr(), ptr(direct), ptr(w_gs), ptr(bias), ptr(tail),
                                      c.data_ptr(), d.data_ptr(), None, B, H, W, wino, None), "bsr_debug_wino_clr")
    torch.cuda.synchronize()
    return untouched(bc, npix * 3).reshape(B, H, W, 3), untouched(bd, npix).reshape(B, H, W, 1)


def _rel(got, ref) -> float:
    return float(np.abs(got.double().numpy() - ref).max() / np.abs(ref).max())


def _check(tag, got, ref):
    for g, r, name in zip(got, ref, ("con_rgb", "dif")):
        err = _rel(g, r)
        print("wino clr %s %s: rel err %.3e (tolerance %.1e)" % (tag, name, err, TOL))
        assert torch.isfinite(g).all()
        assert err <= TOL, name


# one tile with all four image borders inside it; interior tile seams in both directions; the smallest forward shape; 768 tiles = more than
# the resident workgroups of an MI355X (512), so the persistent loop takes a second, ragged trip
CASES = [(1, 8, 32), (2, 16, 64), (3, 32, 256), (3, 256, 256)]


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,W", CASES)
def test_random_inputs_track_the_fp64_tail(B, H, W):
    w = random_weights(H + W)
    gs, f, inputs = random_inputs(B, H, W, seed=B + H + W, f_scale=1.0 if H != 16 else 8.0)
    ref = tail64(gs, f, inputs, w)
    got = _run(gs, f, inputs, w)
    _check("B=%d %dx%d" % (B, H, W), got, ref)
    # the direct form passes the same check, and two runs give the same bits
    _check("B=%d %dx%d direct form" % (B, H, W), _run(gs, f, inputs, w, wino=0), ref)
    again = _run(gs, f, inputs, w)
    assert torch.equal(again[0], got[0]) and torch.equal(again[1], got[1])


@pytest.mark.gpu
def test_spare_channels_of_a_wider_stride_are_not_read():
    """f at channel stride 96: channels 64..95 hold 1e30."""
    w = random_weights(7)
    gs, f, inputs = random_inputs(2, 16, 64, seed=8)
    ref = tail64(gs, f, inputs, w)
    got = _run(gs, f, inputs, w, in_cs=96)
    _check("in_cs=96", got, ref)
    plain = _run(gs, f, inputs, w)
    assert torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1])


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["f", "gs"])
def test_impulses_in_the_corners_and_on_the_edges(which):
    """One image per impulse position: the four corners and the middle of the four edges, in f (one channel per position) or in gs; everything
    else of that input is zero.  A wrong halo, a read past an edge or a dropped border tap shows."""
    H, W = 16, 64
    spots = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2 - 1), (H - 1, W // 2), (H // 2 - 1, 0), (H // 2, W - 1)]
    w = random_weights(11)
    gs, f, inputs = random_inputs(len(spots), H, W, seed=12)
    if which == "f":
        f[:] = 0
    else:
        gs[:] = 0
    for i, (y, x) in enumerate(spots):
        if which == "f":
            f[i, y, x, (7 * i + 3) % 64] = 4.0
        else:
            gs[i, y, x, 0] = 4.0
    ref = tail64(gs, f, inputs, w)
    _check("impulses in %s" % which, _run(gs, f, inputs, w), ref)


@pytest.mark.gpu
def test_packed_output_has_the_bits_of_the_unpacked_one():
    w = random_weights(13)
    gs, f, inputs = random_inputs(2, 16, 64, seed=14)
    a = _run(gs, f, inputs, w)
    b = _run(gs, f, inputs, w, packed=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.gpu
def test_an_image_gets_the_same_bits_alone_and_among_three():
    w = random_weights(15)
    gs, f, inputs = random_inputs(3, 16, 64, seed=16)
    full = _run(gs, f, inputs, w)
    alone = _run(gs[2:3], f[2:3], inputs[2:3], w)
    assert torch.equal(alone[0][0], full[0][2]) and torch.equal(alone[1][0], full[1][2])


@pytest.mark.gpu
def test_bad_shapes_are_refused_and_nothing_is_written():
    from blindshadowremoval_amd import _lib
    lib = _lib.load()
    direct, w_gs, bias, tail = images(random_weights(17))
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    gs, f, inp = torch.ones(1, 8, 32, 1).cuda(), torch.ones(1, 8, 32, 64).cuda(), torch.ones(1, 8, 32, 3).cuda()
    c, d = torch.full((1, 8, 32, 3), CANARY).cuda(), torch.full((1, 8, 32, 1), CANARY).cuda()
    for (H, W, in_cs) in ((4, 32, 64), (8, 16, 64), (8, 32, 32), (8, 32, 66)):
        rc = lib.bsr_debug_wino_clr(gs.data_ptr(), f.data_ptr(), in_cs, inp.data_ptr(), ptr(direct), ptr(w_gs), ptr(bias), ptr(tail),
                                    c.data_ptr(), d.data_ptr(), None, 1, H, W, 1, None)
        assert rc != 0, (H, W, in_cs)
    torch.cuda.synchronize()
    assert bool((c == CANARY).all()) and bool((d == CANARY).all())


@pytest.mark.gpu
def test_whole_forward_agrees_in_both_forms(monkeypatch):
    """B = 2 at 32x256: nothing upstream of the colour tail changed, so gs, mask22 and bmask are bit-identical between the default forward
    and BSR_WINO_CLR=0; con_rgb / dif agree within 3 x the emulated error of max|output|."""
    from blindshadowremoval_amd import Generator
    w = init_weights(5)
    new = Generator(dtype="f32").load_weights(w)
    monkeypatch.setenv("BSR_WINO_CLR", "0")
    old = Generator(dtype="f32").load_weights(w)
    monkeypatch.delenv("BSR_WINO_CLR")
    g = torch.Generator().manual_seed(19)
    inp, uv = torch.rand(2, 32, 256, 3, generator=g).cuda(), torch.rand(2, 32, 256, 3, generator=g).cuda()
    a = [t.clone() for t in new(inp, uv)]
    bm_a = new.probe("bmask").clone()
    b = [t.clone() for t in old(inp, uv)]
    bm_b = old.probe("bmask").clone()
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and torch.equal(bm_a, bm_b)
    assert not torch.equal(a[1], b[1]), "the switch selected the same kernel twice"
    for i, name in ((1, "con_rgb"), (3, "dif")):
        scale = float(b[i].abs().max())
        e = float((a[i] - b[i]).abs().max()) / scale
        print("wino clr vs direct forward, %s: max abs diff / max|output| %.3e (bound %.3e)" % (name, e, 3 * EMULATED_ERROR))
        assert e <= 3 * EMULATED_ERROR, name
    new.close()
    old.close()
