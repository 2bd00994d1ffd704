"""-m gpu: the 25-product transposed-conv kernel of the fp32 GSC up2 / up3 / clr_up3 alone (csrc/wino_convt.h, through
bsr_debug_wino_convt) against the fp64 phase definition of the layer (tools/wino_convt_error.py: convt_direct64) on constructed inputs,
and the whole forward in both forms.

Tolerance: max|gpu - ref| / max|ref| <= 1e-5, the project's fp32 stage ceiling (tests/test_stage_parity_gpu.py).  The float32 emulation of
the kernel's arithmetic lands at 5.5e-7 .. 9.0e-7 on the layers' real inputs (profiles/wino_convt_error.txt).

Measured on MI355X: see MEASURED below (filled from the test's own printout)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from blindshadowremoval_amd import pack
from blindshadowremoval_amd.weights import init_weights
from wino_convt_cases import random_case, random_weights

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
from wino_convt_error import convt_direct64      # noqa: E402

TOL = 1e-5
CANARY = -77.25
GUARD = 4096            # floats on each side of the output allocation

# max|gpu - ref| / max|ref| as printed by the tests below on MI355X
MEASURED = "random cases 3.5e-7 .. 9.1e-7; one-border inputs 4.5e-7 .. 7.7e-7; strides 4.1e-7; 288 tiles 6.0e-7 (profiles/wino_convt_gpu_errors.txt)"


def _run(x: np.ndarray, k9: np.ndarray, b: np.ndarray, act: int = 1, in_cs: int = 0, out_cs: int = 64):
    """x [B,H,W,cin] -> (y [B,2H,2W,64], the whole output allocation incl. guards and the channels the kernel must not touch)."""
    from blindshadowremoval_amd import _lib
    lib = _lib.load()
    B, H, W, cin = x.shape
    in_cs = in_cs or cin
    direct, bias = pack.pack_taps(k9.astype(np.float32), b, 32, (cin + 31) // 32 * 32, 64)
    direct = np.ascontiguousarray(direct)
    xs = torch.full((B, H, W, in_cs), 1e30)                     # the channels past cin must not be read
    xs[..., :cin] = torch.from_numpy(x)
    dx, db = xs.cuda(), torch.from_numpy(bias).cuda()
    n = B * 4 * H * W * out_cs
    buf = torch.full((n + 2 * GUARD,), CANARY).cuda()
    y = buf[GUARD:GUARD + n]
    _lib.check(lib.bsr_debug_wino_convt(dx.data_ptr(), direct.ctypes.data_as(ctypes.c_void_p), db.data_ptr(), y.data_ptr(), B, H, W, cin, 64,
                                        in_cs, out_cs, act, None), "bsr_debug_wino_convt")
    torch.cuda.synchronize()
    host = buf.cpu()
    return host[GUARD:GUARD + n].reshape(B, 2 * H, 2 * W, out_cs), host


def _check_untouched(host, out_cs, B, H, W):
    n = B * 4 * H * W * out_cs
    assert bool((host[:GUARD] == CANARY).all()) and bool((host[GUARD + n:] == CANARY).all()), "guard region written"
    if out_cs > 64:
        assert bool((host[GUARD:GUARD + n].reshape(-1, out_cs)[:, 64:] == CANARY).all()), "channels 64.. written"


def _rel(got, ref) -> float:
    return float(np.abs(got.double().numpy() - ref).max() / np.abs(ref).max())


# Cin = 96 / 128 / 160 at one full tile (6 / 8 / 10 chunks); ragged tiles: fewer patch rows than a tile, a partial tile in x and in y;
# the smallest accepted image's up2 / up3 inputs
CASES = [(2, 4, 32, 96), (2, 4, 32, 128), (2, 4, 32, 160), (1, 2, 32, 128), (1, 4, 40, 96), (1, 6, 34, 160), (1, 8, 64, 160), (1, 16, 128, 128)]


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,W,cin", CASES)
def test_random_inputs_track_the_fp64_phase_definition(B, H, W, cin):
    x, k9, b = random_case(B, H, W, cin, seed=H + W + cin)
    for act in (1, 0):
        ref = convt_direct64(x, k9.astype(np.float32), b.astype(np.float32), act=bool(act))
        got, host = _run(x, k9, b, act)
        err = _rel(got, ref)
        print("wino convt B=%d %dx%d cin=%d act=%d: rel err %.3e (tolerance %.1e)" % (B, H, W, cin, act, err, TOL))
        assert torch.isfinite(got).all()
        assert err <= TOL
        _check_untouched(host, 64, B, H, W)
    # two runs give the same bits
    assert torch.equal(_run(x, k9, b, 0)[0], got)


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["row0", "col0", "last_row", "last_col"])
def test_inputs_on_one_border_only(where):
    """Non-zero only in row 0 / column 0 / the last row / the last column, on a map with a partial tile in x and in y: a wrong halo or a
    read past the edge shows."""
    H, W, cin = 6, 34, 96
    x, k9, b = random_case(2, H, W, cin, seed=5)
    keep = np.zeros((H, W), bool)
    if where == "row0": keep[0] = True
    if where == "col0": keep[:, 0] = True
    if where == "last_row": keep[-1] = True
    if where == "last_col": keep[:, -1] = True
    x = x * keep[None, :, :, None]
    ref = convt_direct64(x, k9.astype(np.float32), b.astype(np.float32))
    got, host = _run(x, k9, b)
    err = _rel(got, ref)
    print("wino convt border %s: rel err %.3e (tolerance %.1e)" % (where, err, TOL))
    assert err <= TOL
    _check_untouched(host, 64, 2, H, W)


@pytest.mark.gpu
def test_channel_strides_and_untouched_neighbours():
    """in_cs > Cin (up2 reads 160 of c2's channels, here 96 of 128) and out_cs = 128 with 64 channels written (up2 into c3): channels 64..127
    and the allocation's guards keep their canary."""
    B, H, W, cin = 2, 6, 34, 96
    x, k9, b = random_case(B, H, W, cin, seed=9)
    ref = convt_direct64(x, k9.astype(np.float32), b.astype(np.float32))
    got, host = _run(x, k9, b, 1, in_cs=128, out_cs=128)
    err = _rel(got[..., :64], ref)
    print("wino convt strides in_cs=128 out_cs=128: rel err %.3e (tolerance %.1e)" % (err, TOL))
    assert err <= TOL
    _check_untouched(host, 128, B, H, W)
    assert torch.equal(got[..., :64], _run(x, k9, b, 1)[0])


@pytest.mark.gpu
def test_an_image_gets_the_same_bits_in_any_batch():
    x, k9, b = random_case(3, 8, 64, 160, seed=21)
    full, _ = _run(x, k9, b)
    alone, _ = _run(x[2:3], k9, b)
    assert torch.equal(alone[0], full[2])


@pytest.mark.gpu
def test_workgroups_that_walk_more_than_one_tile():
    """The launcher starts one workgroup per compute unit and each walks its tiles: 9 x 8 x 4 = 288 tiles are more than the 256 compute
    units of an MI355X, so the tiles of the last image are second tiles.  That image alone (32 tiles, one per workgroup) gives the same bits."""
    x, k9, b = random_case(9, 32, 128, 96, seed=31)
    ref = convt_direct64(x, k9.astype(np.float32), b.astype(np.float32))
    got, host = _run(x, k9, b)
    err = _rel(got, ref)
    print("wino convt 288 tiles: rel err %.3e (tolerance %.1e)" % (err, TOL))
    assert err <= TOL
    _check_untouched(host, 64, 9, 32, 128)
    assert torch.equal(_run(x[8:9], k9, b)[0][0], got[8])


@pytest.mark.gpu
def test_bad_shapes_are_refused_and_nothing_is_written():
    from blindshadowremoval_amd import _lib
    lib = _lib.load()
    k9, b = random_weights(128, 1)
    direct, bias = pack.pack_taps(k9.astype(np.float32), b, 32, 128, 64)
    direct = np.ascontiguousarray(direct)
    x = torch.ones(1, 8, 32, 128).cuda()
    y = torch.full((1, 16, 64, 64), CANARY).cuda()
    db = torch.from_numpy(bias).cuda()
    for (H, W, cin, cout) in ((7, 32, 128, 64), (8, 31, 128, 64), (8, 32, 100, 64), (8, 32, 128, 96)):
        rc = lib.bsr_debug_wino_convt(x.data_ptr(), direct.ctypes.data_as(ctypes.c_void_p), db.data_ptr(), y.data_ptr(), 1, H, W, cin, cout,
                                      128, 64, 1, None)
        assert rc != 0, (H, W, cin, cout)
    torch.cuda.synchronize()
    assert bool((y == CANARY).all())


@pytest.mark.gpu
def test_whole_forward_agrees_in_both_forms(monkeypatch):
    """B = 2 at 256x256 (row 0 = the golden input, row 1 random): the default forward and BSR_WINO_CONVT=0 agree on all four outputs within
    the whole-network tolerance of test_gpu_parity.py (parity_util.TOL); bmask agrees exactly on the golden input, and on the other row it may
    differ only where d32 is within FLIP_TOL of the threshold."""
    from blindshadowremoval_amd import Generator
    from parity_util import FLIP_TOL, TOL as NET_TOL
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "model_py_gsc_256.npz"))
    w = init_weights(int(z["weights_seed"]))
    new = Generator(dtype="f32").load_weights(w)
    monkeypatch.setenv("BSR_WINO_CONVT", "0")
    old = Generator(dtype="f32").load_weights(w)
    monkeypatch.delenv("BSR_WINO_CONVT")
    g = torch.Generator().manual_seed(93)
    inp = torch.cat([torch.from_numpy(z["inputs"][:1]).float(), torch.rand(1, 256, 256, 3, generator=g)]).cuda()
    uv = torch.cat([torch.from_numpy(z["uv"][:1]).float(), torch.rand(1, 256, 256, 3, generator=g)]).cuda()
    a = [t.clone() for t in new(inp, uv)]
    pa = {n: new.probe(n).clone() for n in ("bmask", "d32", "up2", "y")}
    c = [t.clone() for t in old(inp, uv)]
    pb = {n: old.probe(n).clone() for n in pa}
    assert torch.equal(pa["bmask"][0], pb["bmask"][0])
    differ = pa["bmask"] != pb["bmask"]
    assert not differ.any() or float((pb["d32"][differ] - 0.1).abs().max()) < FLIP_TOL
    same = ~differ.flatten(1).any(dim=1)
    for x, y, name in zip(a, c, ("gs", "con_rgb", "mask22", "dif")):
        rows = torch.ones_like(same) if name in ("gs", "mask22") else same
        e = float((x[rows] - y[rows]).abs().max())
        print("wino convt vs direct forward, %s: max abs diff %.3e (tolerance %.1e)" % (name, e, NET_TOL))
        assert e <= NET_TOL, name
    assert not torch.equal(pa["y"], pb["y"]), "the switch selected the same kernel twice"
    new.set_timing(True)
    new(inp, uv)
    torch.cuda.synchronize()
    names = [n for n, _, _ in new.get_launch_timing()]
    new.set_timing(False)
    assert all(n in names for n in ("up2", "up3", "clr_up3"))
    new.close()
    old.close()
