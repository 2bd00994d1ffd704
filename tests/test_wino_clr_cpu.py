"""No GPU: the filter transform bsr_create applies to clr_conv1 (bsr_debug_wino_clr_filter, host only) against pack.pack_wino_clr and against
a direct float64 G g G^T, and a numpy float32 emulation of csrc/wino_clr.h's arithmetic against the float64 direct convolution.

Emulation, max|emulated - fp64| / max|fp64| of clr_conv1 before its activation (random inputs, 16x64, gs in [0, 1], f at scales 1 and 8):
see wino_clr_cases.EMULATED_ERROR, filled from this test's own printout.  Bound asserted here: 1e-6, a tenth of the project's fp32 stage
ceiling — the sum of 65 x 16 float32 products whose operands carry two rounded additions each stays below 16 eps of max|ref|
(eps = 6e-8) when the rounding errors add like a random walk, which is what both forms show."""
import ctypes

import numpy as np
import pytest

from blindshadowremoval_amd import pack
from wino_clr_cases import EMULATED_ERROR, conv1_64, conv1_direct32, conv1_wino32, images, random_inputs, random_weights

EMULATION_BOUND = 1e-6


def _lib_transform(direct, w_gs):
    from blindshadowremoval_amd import _lib
    lib = _lib.load()
    out = np.full(16 * 4 * 64 * 4 + 256, np.nan, np.float32)
    _lib.check(lib.bsr_debug_wino_clr_filter(direct.ctypes.data_as(ctypes.c_void_p), w_gs.ctypes.data_as(ctypes.c_void_p),
                                             out.ctypes.data_as(ctypes.c_void_p)), "bsr_debug_wino_clr_filter")
    return out


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_library_transform_is_the_pack_statement_and_G_g_Gt(seed):
    w = random_weights(seed)
    direct, w_gs, _, _ = images(w)
    got = _lib_transform(direct, w_gs)
    want = pack.pack_wino_clr(w["k1"][:, 1:, :], w["k1"][:, 0, :])
    assert got.shape == want.shape and np.array_equal(got, want)
    # a direct float64 G g G^T per (channel, cout), element by element, read back through the image's index rule
    G = np.array([[1.0, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]])
    k1 = w["k1"].astype(np.float64).reshape(3, 3, 65, 16)
    for k in range(65):
        for n in range(16):
            u = (G @ k1[:, :, k, n] @ G.T).astype(np.float32).reshape(16)
            if k == 0:
                mine = got[16384:].reshape(16, 16)[:, n]
            else:
                c = k - 1
                mine = got[:16384].reshape(16, 4, 4, 16, 4)[:, c // 16, (c % 16) // 4, n, c % 4]
            assert np.array_equal(mine, u), (k, n)


def test_null_arguments_are_refused():
    from blindshadowremoval_amd import _lib
    lib = _lib.load()
    assert lib.bsr_debug_wino_clr_filter(None, None, None) != 0


@pytest.mark.parametrize("seed,f_scale", [(0, 1.0), (1, 1.0), (2, 8.0), (3, 8.0)])
def test_float32_emulation_tracks_the_float64_convolution(seed, f_scale):
    w = random_weights(seed)
    gs, f, _ = random_inputs(1, 16, 64, seed + 10, f_scale)
    ref = conv1_64(gs, f, w)
    scale = np.abs(ref).max()
    e_wino = float(np.abs(conv1_wino32(gs, f, w).astype(np.float64) - ref).max() / scale)
    e_direct = float(np.abs(conv1_direct32(gs, f, w).astype(np.float64) - ref).max() / scale)
    print("wino clr emulation seed %d f x%g: Winograd form %.3e, direct fp32 chain %.3e (bound %.1e, recorded %.1e)"
          % (seed, f_scale, e_wino, e_direct, EMULATION_BOUND, EMULATED_ERROR))
    assert e_wino <= EMULATION_BOUND
    assert e_wino <= EMULATED_ERROR, "the recorded figure no longer covers the emulation"
