"""The 25-position filter transform of pack.py for the transposed 3x3 layers up2 / up3 / clr_up3 (csrc/wino_convt.h) and the library's
own copy of it.  No GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest

from blindshadowremoval_amd import pack
from blindshadowremoval_amd.weights import init_weights

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
from wino_convt_error import convt_direct64, convt_wino32      # noqa: E402


def _wino64(x, k9, bias):
    """The 25-product form in float64 with pack.wino_convt_filter_transform's U: per 2x2 input patch t = Bt d Bt^T, m = sum_k t . U,
    4x4 outputs = At m At^T.  No activation."""
    B, H, W, K = x.shape
    U = pack.wino_convt_filter_transform(k9, np.float64).reshape(5, 5, K, -1)
    xp = np.zeros((B, H + 1, W + 1, K))
    xp[:, 1:, 1:] = x
    d = np.stack([np.stack([xp[:, a:a + H:2, b:b + W:2] for b in range(3)]) for a in range(3)])      # [3, 3, B, H/2, W/2, K]
    V = np.einsum("xa,abnhwk,yb->xynhwk", pack.WINO_CONVT_BT, d, pack.WINO_CONVT_BT)
    m = np.einsum("xynhwk,xykc->xynhwc", V, U)
    return np.einsum("ix,xynhwc,jy->nhiwjc", pack.WINO_CONVT_AT, m, pack.WINO_CONVT_AT).reshape(B, 2 * H, 2 * W, -1) + bias


@pytest.mark.parametrize("cin", [96, 128, 160])
def test_the_25_product_form_equals_the_phase_definition_in_fp64(cin):
    rng = np.random.default_rng(cin)
    k9, bias = rng.standard_normal((9, cin, 64)), rng.standard_normal(64)
    x = rng.standard_normal((2, 6, 8, cin))
    ref = convt_direct64(x, k9, bias, act=False)
    got = _wino64(x, k9, bias)
    assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()


def test_the_phase_definition_is_the_oracles_transposed_convolution():
    """convt_direct64 (what the GPU test compares against) is the layer as the fp64 oracle computes it, on a real layer's weights."""
    import torch
    from oracle.gsc_oracle import GeneratorOracle
    w = init_weights(1)
    o = GeneratorOracle(w, dtype=torch.float64)
    x = np.random.default_rng(2).standard_normal((1, 4, 6, 96))
    ref = o.convt_block(torch.from_numpy(x), "clr_up3").numpy()
    k9, b = pack.layer_matrices(w)["clr_up3"]
    got = convt_direct64(x, k9, b)
    assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()


def test_the_documented_stream_layout_holds_and_the_library_derives_the_same_stream():
    """pack_wino_convt on the three real layers: the documented fragment-order layout, and the transform bsr_create applies to the blob's
    direct image (bsr_debug_wino_convt_filter: host arithmetic, no GPU) gives the same float32 values bit for bit (every U is a float32
    weight or the float64 sum of two or four of them, rounded once).  The blob itself keeps its layout."""
    from blindshadowremoval_amd import _lib
    w = init_weights(1)
    blob = pack.pack_generator(w, "f32")
    names = {}
    for i in range(pack._HEADER.unpack_from(blob, 0)[2]):
        nm, off, nfl, *dims = pack._ENTRY.unpack_from(blob, pack._HEADER.size + i * pack._ENTRY.size)
        names[nm.rstrip(b"\0").decode()] = (off, nfl, tuple(dims))
    assert not [n for n in names if "wino" in n]
    lib = _lib.load()
    for layer, cin in (("up2", 160), ("up3", 128), ("clr_up3", 96)):
        k9, b = pack.layer_matrices(w)[layer]
        assert k9.shape == (9, cin, 64)
        arr, bias = pack.pack_wino_convt(k9, b)
        assert arr.shape == (cin // 16, 25, 2, 2, 64, 4) and arr.dtype == np.float32 and bias.shape == (64,)
        U = pack.wino_convt_filter_transform(k9.astype(np.float32))
        for (c, p, hf, g, h, n, j) in ((0, 0, 0, 0, 0, 0, 0), (cin // 16 - 1, 24, 1, 1, 1, 31, 3), (3, 13, 1, 0, 1, 7, 2), (2, 7, 0, 1, 0, 30, 1)):
            assert arr[c, p, hf, g, 32 * h + n, j] == U[p, 16 * c + 8 * g + 4 * h + j, 32 * hf + n]
        # per axis u = (w1, w1, w2, w0 + w2, w0): position (0, 1) is tap (1, 1), position (3, 4) is taps (0, 0) + (2, 0)
        k32 = k9.astype(np.float32)
        assert np.array_equal(U[1], k32[4]) and np.array_equal(U[19], (k32[0].astype(np.float64) + k32[6]).astype(np.float32))
        off, nfl, dims = names[layer + ".w"]
        assert dims == (cin // 32, 9, 64, 36)
        direct = np.frombuffer(blob, "<f4", nfl, off).copy()
        out = np.full(arr.size, np.nan, np.float32)
        assert lib.bsr_debug_wino_convt_filter(direct.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p), cin) == 0
        assert np.array_equal(out.reshape(arr.shape), arr)
    assert lib.bsr_debug_wino_convt_filter(direct.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p), 100) != 0


def test_emulated_kernel_arithmetic_is_inside_half_the_fp32_stage_budget():
    """The float32 step-by-step emulation (tools/wino_convt_error.py: convt_wino32) on the constructed random case of
    tests/test_wino_convt_gpu.py stays within the tool's gate: the GPU test's tolerance is about the arithmetic, not the inputs."""
    from wino_convt_cases import random_case
    x, k9, b = random_case(2, 4, 32, 128, seed=11)
    ref = convt_direct64(x, k9, b)
    err = np.abs(convt_wino32(x, k9, b).astype(np.float64) - ref).max() / np.abs(ref).max()
    print("emulated 25-product error on the constructed random case: %.3e" % err)
    assert err <= 0.5e-5
