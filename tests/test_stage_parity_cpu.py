"""CPU side of the per-stage parity tests (tests/stage_parity.py, tests/test_stage_parity_gpu.py): the fp64 oracle, the wiring of
the stage table, and that the table's budgets separate fp32-class arithmetic from fp16 operands."""

import numpy as np
import pytest
import torch

from blindshadowremoval_amd.weights import init_weights
from oracle.gsc_oracle import GeneratorOracle, GeneratorTSMOracle, leaky_relu, share_layer
from stage_parity import (EXACT_STAGES, GSC_STAGES, TSM_FULL_STAGES, WEIGHTLESS_STAGES, oracle_probes, run_gsc_stages, run_tsm_full_stages,
                          run_tsm_stages, smooth_reg)
from test_stage_parity_gpu import (DTYPES, F16_MIN_MARGIN, F32_CEILING, SPLIT_IN_F16, TOL, TSM_F16_RATIO, TSM_F16_TOL, TSM_MEASURED, TSM_SHAPES,
                                   tolerance)

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


# (B, side, frame, share) of the TSM table's CPU cases: both group sizes, and the copy form of both ShareLayers
TSM_CASES = {"frame2": (4, 128, 2, True), "frame4": (4, 128, 4, True), "noshare": (2, 128, 2, False)}


@pytest.fixture(scope="module")
def tsm_cases():
    w = init_weights(1, variant="tsm")
    o64 = GeneratorTSMOracle(w, dtype=torch.float64)
    out = {}
    for name, (b, s, frame, share) in TSM_CASES.items():
        g = torch.Generator().manual_seed(8 + frame + share)
        inp, uv = torch.rand(b, s, s, 3, generator=g), torch.rand(b, s, s, 3, generator=g)
        uv[:, :, :s // 8] = 0
        reg = smooth_reg(b, s, g)
        out[name] = (inp, uv, reg, frame, share, oracle_probes(o64, inp, uv, reg=reg, frame=frame, share=share))
    return w, o64, out


def test_tsm_oracle_records_the_gsc_probes_without_changing_a_value(tsm_cases):
    """The TSM oracle hands out what the GSC one does, and recording changes nothing: the outputs with and without ``probes`` are the
    same bits, and xh / res<i> / x0 are the concatenations model_with_TSM.py:272,293 states."""
    w, o64, cases = tsm_cases
    inp, uv, reg, frame, share, p = cases["frame2"]
    for a, b in zip(o64(inp, uv, reg, frame, share), (p["gs"], p["con_rgb"], p["mask22"], p["dif"])):
        assert torch.equal(a, b)
    assert p["x0"].shape[-1] == 291 and p["xh"].shape[-1] == 877
    assert all(p["res%d" % i].shape[-1] == (291 if i < 3 else 877) for i in range(6))
    assert p["up1"].shape[-1] == 96 and p["f1"].shape[-1] == 128 and p["y"].shape[-1] == 64
    pr = {}
    o64(inp, uv, reg, frame, share, probes=pr)
    assert torch.equal(p["xh"], torch.cat([p["res2"] * (1 - p["bmask"]), p["bmask"], pr["x_share2"], p["x0"][..., -3:]], dim=3))
    assert 0 < float(p["bmask"].mean()) < 1, "the case must have cells on both sides of the bmask select"


@pytest.mark.parametrize("name", list(TSM_CASES))
def test_tsm_table_reproduces_the_fp64_oracle_probes(tsm_cases, name):
    """Wiring of the TSM table: fed the fp64 TSM oracle's own probes every stage gives back its output probe, for frame 2 and 4 and
    for share=False (where the ShareLayer lines are copies and come out exactly 0)."""
    _, o64, cases = tsm_cases
    _, _, _, frame, share, p = cases[name]
    res = run_tsm_full_stages(o64, p, frame, share)
    assert set(res.by_kind()) == set(TSM_FULL_STAGES)
    assert len(res.errs) == 4 + 4 * 6 + 3 + 3 + 2 + 3 + 2 + (0 if share else 1)
    for key, err in res.errs.items():
        assert err <= 1e-12, key
        if key[0] in EXACT_STAGES or (key[0] == "tsm_share2" and not share):
            assert err == 0.0, key
    groups = p["x3"].shape[0] // frame
    with pytest.raises(AssertionError):                     # half a frame group cannot be handed to the table
        run_tsm_full_stages(o64, {k: v[:frame * groups - 1] for k, v in p.items()}, frame, share)


def test_tsm_table_catches_wrong_inputs(tsm_cases):
    """Teeth: each line fails if the stage it guards were dropped from the table (the keys would be missing) or its input were
    wrong — a 1e-9 relative nudge upstream, reg_in / reg_out swapped, the bmask lane written one lane low, a frame group of the wrong
    size, a tail lane that skipped the LeakyReLU."""
    _, o64, cases = tsm_cases
    _, _, _, frame, share, p = cases["frame2"]
    run = lambda q, f=frame: run_tsm_full_stages(o64, q, f, True).errs
    for probe, key in (("res1", ("res_block", "res2", "res")), ("res1", ("tsm_res_tail", "res2", "tail")), ("res2", ("up1", "up1", "up1")),
                       ("xh", ("res_head", "res3", "y3x")), ("xh", ("tsm_res_tail", "res3", "tail")), ("res5", ("clr_up1", "clr_up1", "f1")),
                       ("x3", ("tsm_down3_share", "tsm_down3_share", "x0"))):
        assert run(dict(p, **{probe: p[probe] * (1 + 1e-9)}))[key] > 1e-12, (probe, key)
    swapped = torch.cat([p["reg"][..., 3:], p["reg"][..., :3]], dim=3)
    errs = run(dict(p, reg=swapped))
    assert errs[("tsm_share2", "share2", "xh")] > 1e-3 and errs[("tsm_down3_share", "tsm_down3_share", "x0")] > 1e-3
    assert run(p, 4)[("tsm_share2", "share2", "xh")] > 1e-3                 # groups of 4 where the forward shared pairs
    xh = p["xh"].clone()
    xh[..., 290], xh[..., 291] = p["xh"][..., 291], p["xh"][..., 290]       # bmask written at lane 290
    assert run(dict(p, xh=xh))[("tsm_res3_select", "res3_input", "xh")] > 0
    xh = p["xh"].clone()
    xh[..., -3:] = p["xh"][..., -6:-3]                                      # the uv slot three lanes low
    assert run(dict(p, xh=xh))[("tsm_res3_select", "res3_input", "xh")] > 0
    res3 = p["res3"].clone()
    res3[..., 288:] = p["xh"][..., 288:]                                    # the lanes beyond 288 copied without the LeakyReLU
    errs = run(dict(p, res3=res3))
    assert errs[("tsm_res_tail", "res3", "tail")] > 1e-3
    res0 = p["res0"].clone()
    res0[..., 288:] = 0                                                     # the three lanes of res0 the GEMM does not cover, left at zero
    assert run(dict(p, res0=res0))[("tsm_res_tail", "res0", "tail")] == 1.0
    _, _, _, f2, _, q = cases["noshare"]                                    # share=False compared as if the layers had shared
    errs = run_tsm_full_stages(o64, q, f2, True).errs
    assert errs[("tsm_share2", "share2", "xh")] > 1e-3


@pytest.mark.parametrize("name", list(TSM_CASES))
def test_tsm_fp32_arithmetic_passes_the_f32_budgets(tsm_cases, name):
    """Lower side on the TSM widths: the fp32 TSM oracle's probes pass every f32 / f32x3 budget, tsm_share2 under its own slice's
    normalisation included."""
    w, o64, cases = tsm_cases
    inp, uv, reg, frame, share, p64 = cases[name]
    p32 = oracle_probes(GeneratorTSMOracle(w), inp, uv, bmask_override=p64["bmask"], reg=reg, frame=frame, share=share)
    res = run_tsm_full_stages(o64, p32, frame, share)
    print("\n".join(res.lines("fp32-oracle %s" % name)))
    assert set(res.by_kind()) == set(TSM_FULL_STAGES)
    for kind, err in res.by_kind().items():
        for dtype in ("f32", "f32x3"):
            assert err <= TOL[kind][dtype][0], (kind, dtype, err)
    if not share:
        assert all(e == 0.0 for k, e in res.errs.items() if k[0] == "tsm_share2")


def test_tsm_fp16_weights_fail_every_arithmetic_stage(tsm_cases):
    """Upper side on the TSM widths (K = 291 / 877): every weight rounded to fp16 fails every stage that has a weight by >= 10x the
    f32x3 budget.  Not part of this check, because no weight enters them: the exact stages (which must stay 0) and WEIGHTLESS_STAGES
    (tsm_res_tail, tsm_share2), which must stay inside their budget — their teeth are test_tsm_table_catches_wrong_inputs."""
    w, o64, cases = tsm_cases
    inp, uv, reg, frame, share, p64 = cases["frame2"]
    w16 = {k: v.astype(np.float16).astype(np.float32) for k, v in w.items()}
    res = run_tsm_full_stages(o64, oracle_probes(GeneratorTSMOracle(w16), inp, uv, bmask_override=p64["bmask"], reg=reg, frame=frame, share=share),
                              frame, share)
    print("\n".join(res.lines("fp16-weights")))
    seen = set()
    for key, err in res.errs.items():
        if key[0] in EXACT_STAGES:
            assert err == 0.0, key
        elif key[0] in WEIGHTLESS_STAGES:
            assert err <= TOL[key[0]]["f32x3"][0], key
        else:
            seen.add(key[0])
            assert err >= 10 * TOL[key[0]]["f32x3"][0], (key, err)
    assert seen == set(TSM_FULL_STAGES) - set(EXACT_STAGES) - set(WEIGHTLESS_STAGES)


@pytest.mark.parametrize("side,frame", [(32, 2), (32, 4), (64, 2)])
def test_share_layer_fp32_error_at_the_tested_map_sizes(side, frame):
    """tsm_share2's budget at the map sides the GPU shapes use (256 -> 32, 512 -> 64): coordinates reach side - 1 and carry one fp32
    ulp of that, so the error grows with the map.  The fp32 ShareLayer on 291 x_hole-like channels (LeakyReLU outputs, masked cells)
    against fp64, normalised by its own slice as the table does, stays under half of F32_CEILING (measured 1.7e-6 at 32, 3.3e-6 at 64; the kernel lerps in the same order, so it
    differs from this by fma contraction only).
    A shape with a larger map needs this check redone before it is added."""
    assert {s // 8 for _, s, *_ in TSM_SHAPES.values()} <= {32, 64}
    g = torch.Generator().manual_seed(side + frame)
    x = leaky_relu(torch.randn(4, side, side, 291, generator=g)) * (torch.rand(4, side, side, 1, generator=g) > 0.3)
    reg = smooth_reg(4, side * 8, g)
    ref = share_layer(x.double(), reg.double(), frame)
    err = _rel(share_layer(x, reg, frame), ref)
    print("share_layer fp32 vs fp64, side %d frame %d: %.3e" % (side, frame, err))
    assert 0 < err <= F32_CEILING / 2


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
    assert set(TOL) == set(GSC_STAGES) | {"tsm_down3_share"} | {"tsm_res_tail", "tsm_res3_select", "tsm_share2"}
    assert set(TOL) == set(GSC_STAGES) | set(TSM_FULL_STAGES) and set(WEIGHTLESS_STAGES) <= set(SPLIT_IN_F16)
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


def test_tsm_f16_budgets_follow_the_emulated_ratio():
    """The TSM table's own f16 budgets are the GSC rows scaled by the CPU emulation's TSM / GSC ratio (tools/f16_stage_emulation.py; its
    output is profiles/tsm_f16_stage_emulation.txt and must state the ratios used here), and the values measured on the TSM shapes obey
    the rules of test_tolerance_table_obeys_its_rules."""
    import os
    rec = {}
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "tsm_f16_stage_emulation.txt")) as f:
        for line in f:
            t = line.split()
            if len(t) == 4 and t[0] in TOL:
                rec[t[0]] = float(t[3])
    assert set(TSM_F16_TOL) == set(TSM_F16_RATIO) == {"res_head", "res_block", "up1", "clr_up1"}
    for kind, ratio in TSM_F16_RATIO.items():
        assert rec[kind] == ratio, kind
        assert abs(TSM_F16_TOL[kind] / (TOL[kind]["f16"][0] * ratio) - 1) <= 0.03, kind          # two significant digits
        assert tolerance(kind, "f16", tsm=True) == TSM_F16_TOL[kind] and tolerance(kind, "f16") == TOL[kind]["f16"][0]
    assert set(TSM_MEASURED) == set(TSM_FULL_STAGES)
    for kind, row in TSM_MEASURED.items():
        assert set(row) == set(DTYPES), kind
        if kind in EXACT_STAGES:
            assert all(v == 0.0 for v in row.values()), kind
            continue
        for dtype in ("f32", "f32x3"):
            assert row[dtype] <= tolerance(kind, dtype, True) <= F32_CEILING, (kind, dtype)
        assert row["f16"] <= (1 - F16_MIN_MARGIN) * tolerance(kind, "f16", True), kind
        if kind in SPLIT_IN_F16:
            assert tolerance(kind, "f16", True) <= F32_CEILING, kind
        else:
            assert tolerance(kind, "f32x3", True) <= row["f16"] / 10, kind
