"""The host statement blindshadowremoval_amd/perceptual.py against tests/golden/perceptual_*.npz: the reference's own
style_content_loss, vgg_feat_extractor and train_step statements, executed over a numpy stand-in by tools/make_perceptual_fixture.py.
Tolerance: 4 x the differences the tool measured and recorded, never above 1e-5 relative."""
import importlib.util
import os

import numpy as np
import pytest

from blindshadowremoval_amd import objective
from blindshadowremoval_amd import perceptual as host
from blindshadowremoval_amd.weights import init_vgg_weights


def loss_terms(seed):
    """tools/make_perceptual_fixture.loss_terms: the float32 terms the totals read beside per."""
    rng = np.random.default_rng(seed)
    scale = (0.05, 0.05, 1.0, 0.5, 1.0, 1.0)
    names = ("recon_loss_gs", "recon_loss_c", "gan_loss", "grad_loss", "d_loss_r", "d_loss_s")
    return {n: np.float32(rng.uniform(0.2, 1.0) * s * (-1 if n == "gan_loss" else 1)) for n, s in zip(names, scale)}


@pytest.mark.parametrize("S", (32, 64))
def test_host_statement_matches_the_reference_fixture(golden_dir, S):
    case = np.load(os.path.join(golden_dir, "perceptual_%d.npz" % S))
    B, seed = int(case["B"]), int(case["seed"])
    assert int(case["S"]) == S and case["tap_means"].shape == (5,) and case["tap_means"].dtype == np.float64
    tol_m, tol_t = 4 * float(case["measured_mean_rel"]), 4 * float(case["measured_total_rel"])
    assert 0 < tol_m <= 1e-5 and 0 < tol_t <= 1e-5
    r = host.per_loss(init_vgg_weights(seed), *host.example_inputs(S, B, seed))
    total = r["sums"].sum(axis=0)
    means = np.array([total[k] / (B * h * h * host.TAP_CH[k]) for k, h in enumerate(host.tap_sides(S))])
    print("perceptual fixture S=%d: tap means %s (fixture %s), per %.9g (fixture %.9g)" % (S, means, case["tap_means"], r["loss"][0], float(case["per"])))
    np.testing.assert_allclose(means, case["tap_means"], rtol=tol_m, atol=0)
    np.testing.assert_allclose(float(r["loss"][0]), float(case["per"]), rtol=tol_m, atol=0)
    tm = loss_terms(seed)
    g = objective.g_total_loss(tm["recon_loss_gs"], tm["recon_loss_c"], tm["grad_loss"], tm["gan_loss"], r["loss"][0])
    d = objective.d_total_loss(tm["d_loss_r"], tm["d_loss_s"])
    assert g.dtype == np.float32 and d.dtype == np.float32
    np.testing.assert_allclose([float(g), float(d)], [float(case["g_total"]), float(case["d_total"])], rtol=tol_t, atol=0)


def test_the_fixtures_hold_numbers_only(golden_dir):
    for S in (32, 64):
        path = os.path.join(golden_dir, "perceptual_%d.npz" % S)
        assert os.path.getsize(path) < 4096
        with np.load(path) as z:
            assert sorted(z.files) == sorted(["seed", "B", "S", "backend", "tap_means", "per", "g_total", "d_total", "measured_mean_rel", "measured_total_rel"])


def test_the_tool_draws_the_same_loss_terms():
    tool = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "make_perceptual_fixture.py")
    src = open(tool).read()
    ns = {"np": np, "TERM_NAMES": ("recon_loss_gs", "recon_loss_c", "gan_loss", "grad_loss", "d_loss_r", "d_loss_s")}
    body = src[src.index("def loss_terms(seed):"):src.index("def cut(")]
    exec(body, ns)
    assert ns["loss_terms"](432) == loss_terms(432)
