"""CPU tests of the single-stage RGB baseline (/root/reference/model_RGB.py): inventory, oracle, packing, variant detection.

tests/golden/model_py_rgb_*.npz hold the reference's own model_RGB.py executed over the TF stand-in (tools/make_model_rgb_fixture.py):
its output `con` and the inventory of variables its forward created (names and shapes)."""
import hashlib
import os
import struct

import numpy as np
import pytest
import torch

from blindshadowremoval_amd import weights as W
from blindshadowremoval_amd.pack import (BLOB_MAGIC, _ENTRY, _HEADER, geometry, layer_matrices_rgb, pack_generator, pack_taps,
                                         rgb_tail_weights)
from rgb_oracle import GeneratorRGBOracle, load_fixture

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = ["model_py_rgb_64.npz", "model_py_rgb_256.npz"]
TOL = 5e-5          # fp32 torch oracle vs the float64 stand-in (the bound of test_model_py_fixture.py)


def _fixture(name):
    path = os.path.join(GOLD, name)
    if not os.path.isfile(path):
        pytest.skip("%s was not generated" % name)
    z = np.load(path)
    return {k: z[k] for k in z.files}


def test_inventory_matches_the_reference_forward():
    """generator_variable_shapes("rgb") is exactly what model_RGB.py's forward builds: clr_*, res_stack[3:6] and info_share are
    constructed but never called, so they own no variables."""
    z = _fixture("model_py_rgb_64.npz")
    recorded = {str(n): tuple(int(v) for v in str(s).strip("[]").split(",")) for n, s in zip(z["inventory_names"], z["inventory_shapes"])}
    spec = W.generator_variable_shapes("rgb")
    assert dict(spec) == recorded
    assert not any(k.startswith(("clr_", "res_stack/3", "res_stack/4", "res_stack/5", "info_share")) for k in spec)
    assert spec["res_stack/1/non_local/theta/kernel"] == (1, 1, 513, 256)
    assert spec["up2/conv/kernel"] == (3, 3, 128, 256)          # cat[y 192, x3 64] -> 128


@pytest.mark.parametrize("fixture", FIXTURES)
def test_oracle_reproduces_reference_model_rgb_py(fixture):
    z = _fixture(fixture)
    assert str(z["backend"]) == "standin-np_loops"
    inp, uv, ref, s = load_fixture(os.path.join(GOLD, fixture))
    oracle = GeneratorRGBOracle(W.init_weights(int(z["weights_seed"]), variant="rgb"))
    con = oracle(inp, uv)[:, ::s, ::s]
    assert con.shape == ref.shape
    err = float(np.abs(con.numpy() - ref).max())
    assert err < TOL, err


def test_fp64_and_fp32_oracles_agree():
    w = W.init_weights(3, variant="rgb")
    g = torch.Generator().manual_seed(4)
    inp, uv = torch.rand(2, 64, 64, 3, generator=g), torch.rand(2, 64, 64, 3, generator=g)
    p32, p64 = {}, {}
    GeneratorRGBOracle(w)(inp, uv, probes=p32)
    GeneratorRGBOracle(w, dtype=torch.float64)(inp, uv, probes=p64)
    assert p64["con"].dtype == torch.float64
    for k in ("x1", "x2", "x3", "x0", "res0", "res1", "res2", "up1", "up2", "up3", "y", "con"):
        err = float((p32[k].double() - p64[k]).abs().max()) / float(p64[k].abs().max())
        assert err < 1e-5, (k, err)


def test_geometry_padding_is_consistent():
    geo = geometry("rgb")
    w = W.init_weights(1, variant="rgb")
    mats = layer_matrices_rgb(w)
    assert set(geo) == set(mats)
    for name, (cc, k_pad, n_pad) in geo.items():
        k, _ = mats[name]
        assert k_pad % cc == 0 and n_pad % 32 == 0, name
        assert k.shape[1] <= k_pad and k.shape[2] <= n_pad, name
    # the GEMMs read whole groups of NI = 3 tiles past the last real one (gemm_nloop.h): zero slack tiles
    assert geo["res0.c3q"][2] >= (544 // 32 + 768 // 32 + 2) * 32 and geo["res0.w"][2] >= (544 // 32 + 2) * 32
    with pytest.raises(ValueError, match="f32 only"):
        geometry("rgb", "f16")


def _entries(blob):
    magic, version, n, dtype = _HEADER.unpack_from(blob, 0)
    assert magic == BLOB_MAGIC
    out = {}
    for i in range(n):
        name, off, nf, *dims = _ENTRY.unpack_from(blob, _HEADER.size + i * _ENTRY.size)
        out[name.rstrip(b"\0").decode()] = (np.frombuffer(blob, "<f4", nf, off), dims)
    return out


def test_packed_blob_round_trips_the_folded_weights():
    w = W.init_weights(1, variant="rgb")
    e = _entries(pack_generator(w))
    geo = geometry("rgb")
    for name, (k, b) in layer_matrices_rgb(w).items():
        cc, k_pad, n_pad = geo[name]
        arr, bias = pack_taps(k, b, cc, k_pad, n_pad)
        got, dims = e[name + ".w"]
        assert tuple(dims) == arr.shape and np.array_equal(got, arr.reshape(-1)), name
        # unpack: [chunk, tap, n, cc] -> [tap, k, n] equals the folded float32 matrix
        un = got.reshape(arr.shape)[..., :cc].transpose(1, 0, 3, 2).reshape(k.shape[0], k_pad, n_pad)
        assert np.array_equal(un[:, :k.shape[1], :k.shape[2]], k.astype(np.float32)), name
        assert not un[:, k.shape[1]:].any() and not un[:, :, k.shape[2]:].any(), name
        assert np.array_equal(e[name + ".b"][0][:b.shape[0]], b.astype(np.float32)), name
    assert np.array_equal(e["rgb.tail"][0], rgb_tail_weights(w))
    assert np.array_equal(e["rgb.head_bias"][0], w["conv2/conv/bias"])
    # c3q = [conv3+BN (513) | 0 | (conv3+BN) composed with theta | phi | g]
    k3 = w["res_stack/0/conv3/kernel"][0, 0].astype(np.float64)
    kc, _ = layer_matrices_rgb(w)["res0.c3q"]
    s = w["res_stack/0/bnorm3/gamma"] / np.sqrt(w["res_stack/0/bnorm3/moving_variance"].astype(np.float64) + W.BN_EPS)
    assert np.allclose(kc[0, :, :513], k3 * s) and not kc[0, :, 513:544].any()
    th = w["res_stack/0/non_local/theta/kernel"][0, 0]
    assert np.allclose(kc[0, :, 544:800], (k3 * s) @ th)


def test_detect_variant_tells_the_three_apart():
    for v in ("gsc", "tsm", "rgb"):
        w = W.init_weights(1, variant=v)
        assert W.detect_variant(w) == v
        W.check_weights(w, v)
    with pytest.raises(ValueError):
        W.check_weights(W.init_weights(1, variant="rgb"), "gsc")


# sha256[:16] of pack_generator(init_weights(1, variant=v), dtype) at the parent commit: GSC and TSM packing is unchanged byte for byte
GSC_TSM_BLOBS = {("gsc", "f32"): "a132cb9838b9b980", ("gsc", "f32x3"): "3795984ac2dfaece", ("gsc", "f16"): "226a22d80c3dccec",
                 ("tsm", "f32"): "cc6378c116b330a4", ("tsm", "f32x3"): "45a4606dbbef3d6d", ("tsm", "f16"): "f8fc75fc724ad609"}


@pytest.mark.parametrize("variant,dtype", sorted(GSC_TSM_BLOBS))
def test_gsc_and_tsm_packing_is_unchanged(variant, dtype):
    blob = pack_generator(W.init_weights(1, variant=variant), dtype)
    assert hashlib.sha256(blob).hexdigest()[:16] == GSC_TSM_BLOBS[(variant, dtype)]


def test_rgb_is_f32_only():
    from blindshadowremoval_amd import GeneratorRGB
    for dt in ("f32x3", "f16"):
        with pytest.raises(ValueError, match="'f32' only"):
            GeneratorRGB(dtype=dt)
        with pytest.raises(ValueError, match="f32 only"):
            pack_generator(W.init_weights(1, variant="rgb"), dt)
    GeneratorRGB()          # constructing needs no GPU


def test_rgb_generator_refuses_other_weights():
    from blindshadowremoval_amd import GeneratorRGB
    with pytest.raises(ValueError, match="RGB baseline"):
        GeneratorRGB().load_weights(W.init_weights(1))


def test_bsr_header_declares_the_rgb_entries():
    root = os.path.dirname(GOLD)
    with open(os.path.join(root, "..", "include", "bsr_hip.h")) as f:
        text = f.read()
    assert "int bsr_forward_rgb(bsr_handle* h, const float* inputs, const float* uv, int B, int H, int W, float* con, void* stream);" in text
    assert "int bsr_debug_attention_rgb(" in text
    assert struct.calcsize("<4I") == _HEADER.size


def test_checkpoint_bundle_round_trip(tmp_path):
    """GeneratorRGB.restore reads the checkpoint through tf_bundle, which is variant-agnostic: an RGB bundle comes back whole and is
    recognised as RGB."""
    from blindshadowremoval_amd.tf_bundle import load_generator_weights, write_bundle
    w = W.init_weights(5, variant="rgb")
    prefix = str(tmp_path / "ckpt-7")
    write_bundle(prefix, w)
    back = load_generator_weights(prefix)
    assert set(back) == set(w) and all(np.array_equal(back[k], w[k]) for k in w)
    assert W.detect_variant(back) == "rgb"
