"""The Winograd F(2x2, 3x3) filter transform of pack.py (res*.conv2, csrc/wino_conv2.h) and the library's own copy of it.  No GPU."""
import os
import sys

import numpy as np

from blindshadowremoval_amd import pack
from blindshadowremoval_amd.weights import init_weights

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
from wino_conv2_error import direct64, wino32      # noqa: E402

# Measured by tools/wino_conv2_error.py (float32 emulation of the kernel's arithmetic against the fp64 direct convolution on every res
# block's conv1 output of the tests/golden/model_py_gsc_{64,256} inputs): worst max|t2 - ref| / max|ref| = 7.3e-7 (the direct kernel's
# arithmetic, emulated the same way: 1.5e-6 — 128-term sums against 1152-term ones).
WINO_EMULATED_ERR = 7.3e-7


def _wino64(x, k9, bias):
    """F(2x2, 3x3) in float64 with the transformed filter of pack.wino_filter_transform: Y = A^T [sum_k U . (B^T d B)] A."""
    B, H, W, K = x.shape
    U = pack.wino_filter_transform(k9, np.float64).reshape(4, 4, K, -1)
    Bt = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], np.float64)
    At = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], np.float64)
    xp = np.zeros((B, H + 2, W + 2, K))
    xp[:, 1:-1, 1:-1] = x
    d = np.stack([np.stack([xp[:, a:a + H:2, b:b + W:2] for b in range(4)]) for a in range(4)])     # [4, 4, B, H/2, W/2, K]
    V = np.einsum("xa,abnhwk,yb->xynhwk", Bt, d, Bt)
    m = np.einsum("xynhwk,xykc->xynhwc", V, U)
    y = np.einsum("ix,xynhwc,jy->nhiwjc", At, m, At).reshape(B, H, W, -1) + bias
    return np.where(y > 0, y, 0.3 * y)


def test_transformed_filter_convolves_like_the_direct_one_in_fp64():
    rng = np.random.default_rng(5)
    k9, bias = rng.standard_normal((9, 24, 40)), rng.standard_normal(40)
    x = rng.standard_normal((2, 8, 12, 24))
    ref, got = direct64(x, k9, bias), _wino64(x, k9, bias)
    assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()


def test_real_layer_weights_transform_exactly_and_the_library_derives_the_same_stream():
    """pack_wino on a real layer: exact in fp64, the documented layout — and the transform bsr_create applies to the blob's direct image
    (bsr_debug_wino_filter: host arithmetic, no GPU) gives the same float32 values (both are float64 sums of float32 weights scaled by
    0.25 / 0.5 / 1, rounded once: equal but for a rounding tie, so one float32 ulp is allowed).  The blob itself keeps its layout."""
    import ctypes
    from blindshadowremoval_amd import _lib
    w = init_weights(1)
    k9, b = pack.layer_matrices(w)["res4.conv2"]
    x = np.random.default_rng(6).standard_normal((1, 4, 6, 128))
    ref = direct64(x, k9, b)
    assert np.abs(_wino64(x, k9, b) - ref).max() <= 1e-12 * np.abs(ref).max()
    arr, bias = pack.pack_wino(k9, b)
    assert arr.shape == (8, 16, 128, 16) and arr.dtype == np.float32 and bias.shape == (128,)
    U = pack.wino_filter_transform(k9.astype(np.float32))
    for (c, p, n, k) in ((0, 0, 0, 0), (7, 15, 127, 15), (3, 5, 77, 9)):
        assert arr[c, p, n, k] == U[p, 16 * c + k, n]
    blob = pack.pack_generator(w, "f32")
    names = {}
    for i in range(pack._HEADER.unpack_from(blob, 0)[2]):
        nm, off, nfl, *dims = pack._ENTRY.unpack_from(blob, pack._HEADER.size + i * pack._ENTRY.size)
        names[nm.rstrip(b"\0").decode()] = (off, nfl, tuple(dims))
    assert not [n for n in names if "wino" in n or "conv2w" in n]
    off, nfl, dims = names["res4.conv2.w"]
    assert dims == (4, 9, 128, 36)
    direct = np.frombuffer(blob, "<f4", nfl, off).copy()
    out = np.full(arr.size, np.nan, np.float32)
    lib = _lib.load()
    assert lib.bsr_debug_wino_filter(direct.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p)) == 0
    np.testing.assert_allclose(out.reshape(arr.shape), arr, rtol=1.2e-7, atol=0)
    assert (out.reshape(arr.shape) != arr).mean() < 1e-4


def test_emulated_kernel_arithmetic_is_inside_the_measured_error():
    """The float32 step-by-step emulation (tools/wino_conv2_error.py: wino32) on the constructed inputs of tests/test_wino_conv2_gpu.py
    stays within the figure measured on the golden inputs: the GPU test's tolerance (3x that figure) is about the arithmetic, not the inputs."""
    from wino_cases import random_case
    x, k9, b = random_case(2, 8, 32, seed=11)
    ref = direct64(x, k9, b)
    err = np.abs(wino32(x, k9, b).astype(np.float64) - ref).max() / np.abs(ref).max()
    print("emulated wino error on the constructed random case: %.3e" % err)
    assert err <= WINO_EMULATED_ERR
