"""CPU side of the per-stage parity tests (tests/stage_parity.py, tests/test_stage_parity_gpu.py): the fp64 oracle, the wiring of
the stage table, and that the table's budgets separate fp32-class arithmetic from fp16 operands."""

import numpy as np
import pytest
import torch

from blindshadowremoval_amd.weights import init_weights
from oracle.gsc_oracle import GeneratorOracle, GeneratorTSMOracle
from stage_parity import EXACT_STAGES, GSC_STAGES, oracle_probes, run_gsc_stages, run_tsm_stages
from test_stage_parity_gpu import DTYPES, F16_MIN_MARGIN, F32_CEILING, SPLIT_IN_F16, TOL

B, H, W = 2, 128, 128


@pytest.fixture(scope="module")
def case():
    torch.manual_seed(4)
    inp, uv = torch.rand(B, H, W, 3), torch.rand(B, H, W, 3)
    uv[:, :, :16] = 0
    w = init_weights(1)
    o64 = GeneratorOracle(w, dtype=torch.float64)
    return w, inp, uv, o64, oracle_probes(o64, inp, uv)


def _rel(a, b):
    return float((a.double() - b).abs().max()) / max(float(b.abs().max()), 1e-30)


def test_fp64_oracle_is_fp64_throughout(case):
    _, _, _, o64, p64 = case
    for k, t in p64.items():
        if k not in ("inputs", "uv"):
            assert t.dtype == torch.float64, k


def test_fp64_oracle_agrees_with_the_fp32_oracle(case):
    """Every probe and output of the default (fp32) oracle within 1e-5 of the fp64 one, scale-relative (measured: <= 2e-6)."""
    w, inp, uv, _, p64 = case
    p32 = oracle_probes(GeneratorOracle(w), inp, uv, bmask_override=p64["bmask"])
    assert float((p32["d32"].double() - p64["d32"]).abs().max()) < 1e-5
    for k, t in p64.items():
        assert p32[k].dtype == (torch.float32 if k not in ("inputs", "uv") else t.dtype), k
        assert _rel(p32[k], t) <= 1e-5, (k, _rel(p32[k], t))


def test_tsm_fp64_oracle_agrees_with_the_fp32_oracle():
    torch.manual_seed(5)
    inp, uv = torch.rand(4, H, W, 3), torch.rand(4, H, W, 3)
    reg = (torch.rand(4, H, W, 6) - 0.5) * 0.2
    w = init_weights(1, variant="tsm")
    for frame in (2, 4):
        p64 = {}
        ref = GeneratorTSMOracle(w, dtype=torch.float64)(inp, uv, reg, frame, probes=p64)
        p32 = {}
        out = GeneratorTSMOracle(w)(inp, uv, reg, frame, probes=p32, bmask_override=p64["bmask"])
        for a, b in zip(out, ref):
            assert b.dtype == torch.float64 and _rel(a, b) <= 1e-5
        for k in ("x0", "x_share1", "x_share2", "res2", "res5"):
            assert p64[k].dtype == torch.float64 and _rel(p32[k], p64[k]) <= 1e-5, k


def test_stage_table_reproduces_the_fp64_oracle_probes(case):
    """Wiring: fed the fp64 oracle's own probes, every stage gives back its output probe — a wrong input probe, concat order or
    channel slice in the table would not."""
    _, _, _, o64, p64 = case
    res = run_gsc_stages(o64, p64)
    assert set(res.by_kind()) == set(GSC_STAGES)
    assert len(res.errs) == 4 + 3 * 6 + 3 + 3 + 1 + 3 + 2
    for key, err in res.errs.items():
        assert err <= 1e-12, key


def test_stage_table_catches_a_wrong_input():
    """... and the wiring check has teeth: an input probe off by 1e-9 relative, or an inverted bmask, is caught."""
    torch.manual_seed(6)
    inp, uv = torch.rand(1, 64, 64, 3), torch.rand(1, 64, 64, 3)
    o64 = GeneratorOracle(init_weights(2), dtype=torch.float64)
    p = oracle_probes(o64, inp, uv)
    q = dict(p, up1=p["up1"] * (1 + 1e-9))
    assert run_gsc_stages(o64, q).errs[("up2", "up2", "up2")] > 1e-12
    q = dict(p, bmask=1 - p["bmask"])
    assert run_gsc_stages(o64, q).errs[("res3_input", "res3_input", "xh")] > 0


def test_tsm_stage_reproduces_the_fp64_oracle():
    torch.manual_seed(7)
    inp, uv = torch.rand(4, 64, 64, 3), torch.rand(4, 64, 64, 3)
    reg = (torch.rand(4, 64, 64, 6) - 0.5) * 0.2
    o64 = GeneratorTSMOracle(init_weights(1, variant="tsm"), dtype=torch.float64)
    for frame in (2, 4):
        pr = {}
        o64(inp, uv, reg, frame, probes=pr)
        res = run_tsm_stages(o64, {"x3": pr["x3"], "x0": pr["x0"], "uv": uv, "reg": reg}, frame)
        assert max(res.errs.values()) <= 1e-12


def test_fp32_arithmetic_passes_the_f32_budgets(case):
    """Sensitivity, lower side: the fp32 oracle's probes (fp32 arithmetic done right) pass the f32 and f32x3 budgets."""
    w, inp, uv, o64, p64 = case
    res = run_gsc_stages(o64, oracle_probes(GeneratorOracle(w), inp, uv, bmask_override=p64["bmask"]))
    for kind, err in res.by_kind().items():
        for dtype in ("f32", "f32x3"):
            assert err <= TOL[kind][dtype][0], (kind, dtype, err)


def test_fp16_weights_fail_every_conv_stage(case):
    """Sensitivity, upper side: the same forward with every weight rounded to fp16 (what a lost lo plane does to the operand it
    belonged to) fails the f32 and f32x3 budget of every stage that has arithmetic — measured 2e-4 .. 1e-3."""
    w, inp, uv, o64, p64 = case
    w16 = {k: v.astype(np.float16).astype(np.float32) for k, v in w.items()}
    res = run_gsc_stages(o64, oracle_probes(GeneratorOracle(w16), inp, uv, bmask_override=p64["bmask"]))
    for key, err in res.errs.items():
        if key[0] in EXACT_STAGES:
            assert err == 0.0
            continue
        for dtype in ("f32", "f32x3"):
            assert err > TOL[key[0]][dtype][0], (key, dtype, err)
        assert err >= 10 * TOL[key[0]]["f32x3"][0], key       # the f32x3 budget separates fp16 operands by 10x, as the f16 rule asks


def test_tolerance_table_obeys_its_rules():
    """f32 / f32x3 budgets <= 1e-5; f32x3 <= the f16 mode's measured error / 10 (split precision must not pass with fp16 operands)
    wherever the f16 mode has fp16 operands, and where it does not, the f16 budget is fp32-class too; the measured f16 error leaves
    F16_MIN_MARGIN of its budget; exact stages have budget 0."""
    assert set(TOL) == set(GSC_STAGES) | {"tsm_down3_share"}
    for kind, row in TOL.items():
        assert set(row) == set(DTYPES), kind
        if kind in EXACT_STAGES:
            assert all(tol == 0.0 for tol, _ in row.values()), kind
            continue
        for dtype in ("f32", "f32x3"):
            tol, measured = row[dtype]
            assert tol <= F32_CEILING and measured <= tol, (kind, dtype)
        tol16, measured16 = row["f16"]
        assert measured16 <= (1 - F16_MIN_MARGIN) * tol16, kind
        if kind in SPLIT_IN_F16:          # split precision in the f16 mode too: fp32-class budget (separation: the CPU emulation)
            assert tol16 <= F32_CEILING, kind
        else:
            assert row["f32x3"][0] <= measured16 / 10, kind
