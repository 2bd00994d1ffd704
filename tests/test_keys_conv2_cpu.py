"""conv2's output as the attention keys (csrc/bsr_api.hip: keys_compose, env BSR_KEYS_CONV2): the algebra, the library's composed
res*.c3q image against pack.py's statement, and the float32 rounding of the two forms.  No GPU."""
import os
import sys

import numpy as np
import pytest

from blindshadowremoval_amd import pack
from blindshadowremoval_amd.weights import init_weights

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
from keys_conv2_error import both_forms, rel      # noqa: E402

# Measured by tools/keys_conv2_error.py (profiles/keys_conv2_error.txt: float32 emulation of both forms against the fp64 attention on
# every res block's t2 of the tests/golden/model_py_gsc_{64,256} inputs): worst max|att - ref| / max|ref| of the composed form; the
# projected form, emulated the same way, gives 2.4e-6.  The GPU tests' form-against-form tolerance is 3x this figure.
KEYS_EMULATED_ERR = 2.6e-6


def _softmax64(s):
    p = np.exp(s - s.max(axis=1, keepdims=True))
    return p / p.sum(axis=1, keepdims=True)


@pytest.mark.parametrize("bias_scale", [0.1, 1.0, 8.0])
def test_softmax_of_composed_queries_on_raw_keys_equals_the_projected_form(bias_scale):
    """softmax_j(theta_i . phi_j) == softmax_j(q'_i . t_j) in fp64, 64 tokens x 128 channels, non-zero biases — with phi's bias at scale 8 the
    term the softmax removes, theta_i . bk, exceeds the spread of every query's logits."""
    rng = np.random.default_rng(7)
    T, D = 64, 128
    t = rng.standard_normal((T, D)) * 0.5
    wq, wk = rng.standard_normal((D, D)) / np.sqrt(D), rng.standard_normal((D, D)) / np.sqrt(D)
    bq, bk = rng.standard_normal(D), rng.standard_normal(D) * bias_scale
    theta, phi = t @ wq + bq, t @ wk + bk
    f = theta @ phi.T
    a, ab = pack.compose_keys(wq, bq, wk)
    f2 = (t @ a + ab) @ t.T
    if bias_scale >= 8.0:
        assert np.abs(theta @ bk).max() > (f.max(axis=1) - f.min(axis=1)).max()
    assert np.abs((f - f2) - (theta @ bk)[:, None]).max() <= 1e-9 * np.abs(f).max()      # the logits differ by a per-query constant only
    assert np.abs(_softmax64(f) - _softmax64(f2)).max() <= 1e-12


def _entries(blob):
    names = {}
    for i in range(pack._HEADER.unpack_from(blob, 0)[2]):
        nm, off, nfl, *dims = pack._ENTRY.unpack_from(blob, pack._HEADER.size + i * pack._ENTRY.size)
        names[nm.rstrip(b"\0").decode()] = (off, nfl, tuple(dims))
    return names


@pytest.mark.parametrize("variant", ["gsc", "tsm"])
def test_the_library_composes_the_image_pack_py_states(variant):
    """bsr_debug_keys_compose (the host arithmetic bsr_create runs on every res<i>.c3q of an fp32 blob) against pack.compose_keys_c3q:
    the copied rows (y3, g, their biases) to the bit; the composed rows are float64 sums of 128 products rounded once on both sides,
    summed in different orders, so they are equal but for a rounding tie — one float32 ulp is allowed, on very few elements.  The
    blob itself keeps its layout."""
    import ctypes
    from blindshadowremoval_amd import _lib
    w = init_weights(1, variant=variant) if variant != "gsc" else init_weights(1)
    blob = pack.pack_generator(w, "f32")
    names = _entries(blob)
    assert not [n for n in names if "keys" in n]
    lib = _lib.load()
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    for i in range(6):
        off, nfl, dims = names["res%d.c3q.w" % i]
        assert dims == (4, 1, 768, 36)
        c3q_w = np.frombuffer(blob, "<f4", nfl, off).copy()
        off, nfl, _ = names["res%d.c3q.b" % i]
        c3q_b = np.frombuffer(blob, "<f4", nfl, off).copy()
        want_w, want_b = pack.compose_keys_c3q(c3q_w.reshape(4, 1, 768, 36), c3q_b)
        assert want_w.shape == (4, 1, pack.KEYS_N_PAD, 36) and want_b.shape == (pack.KEYS_N_PAD,)
        got_w, got_b = np.full(want_w.size, np.nan, np.float32), np.full(want_b.size, np.nan, np.float32)
        assert lib.bsr_debug_keys_compose(ptr(c3q_w), ptr(c3q_b), ptr(got_w), ptr(got_b)) == 0
        got_w = got_w.reshape(want_w.shape)
        for rows in (slice(0, 288), slice(416, pack.KEYS_N_PAD)):
            assert np.array_equal(got_w[:, :, rows], want_w[:, :, rows]) and np.array_equal(got_b[rows], want_b[rows])
        assert not got_w[:, :, pack.KEYS_N:].any() and not got_w[..., 32:].any() and not got_b[pack.KEYS_N:].any()
        np.testing.assert_allclose(got_w, want_w, rtol=1.2e-7, atol=0)
        np.testing.assert_allclose(got_b, want_b, rtol=1.2e-7, atol=0)
        assert (got_w != want_w).mean() < 1e-4
        # the composed rows are what the algebra says of the layer's own theta / phi columns: K index in the image's row order
        kn = c3q_w.reshape(4, 768, 36)[:, :, :32].transpose(0, 2, 1).reshape(128, 768).astype(np.float64)
        a = kn[:, 288:416] @ kn[:, 416:544].T
        for (k, m) in ((0, 0), (127, 127), (37, 90)):
            assert abs(float(got_w[k // 32, 0, 288 + m, k % 32]) - a[k, m]) <= 1e-6 * np.abs(a).max()


def test_emulated_rounding_of_the_composed_form_is_no_worse_than_twice_the_projected_one():
    """The float32 emulation of both forms (tools/keys_conv2_error.py) on a constructed t2 with a real layer's weights, logits in the range
    of the golden inputs (|logit| up to ~23 there) and well beyond it: the composed form's attention error stays within 2x of the projected
    form's — the rule the change ships under (the golden-input figures are in profiles/keys_conv2_error.txt)."""
    w = init_weights(1)
    kc, bc = pack.layer_matrices(w)["res5.c3q"]
    t2 = np.random.default_rng(12).standard_normal((256, 128)).astype(np.float32)
    t2 = np.where(t2 > 0, t2, 0.3 * t2).astype(np.float32)          # conv2 ends in a LeakyReLU
    for scale in (0.4, 1.0):
        old, new, ref, logit = both_forms(t2 * np.float32(scale), kc[0], bc)
        eo, en = rel(old, ref), rel(new, ref)
        print("emulated attention error, t2 scale %.1f: projected %.3e composed %.3e (max |logit| %.1f)" % (scale, eo, en, logit))
        assert en <= 2 * eo
