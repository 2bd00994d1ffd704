"""-m gpu: every stage of the forward against the fp64 oracle, teacher-forced (tests/stage_parity.py), in the three modes.

The whole-network tests (test_gpu_parity.py, 1e-3 absolute) mix every upstream layer's error into each probe and compare with an fp32
oracle, so they cannot hold one layer to the ~1e-6 the fp32 / f32x3 arithmetic gives, nor tell split precision from fp16 operands.
Here each stage gets the GPU's own input probes in fp64 and its output is held to a per-(stage, mode) budget of
max|gpu - ref64| / max|ref64|:
  f32, f32x3  <= 1e-5 everywhere: correct fp32-class arithmetic lands at ~1e-6, a split product dropped (hi*lo) or an operand staged
              at fp16 at ~2e-4 (CPU emulation: tests/test_stage_parity_cpu.py::test_fp16_weights_fail_every_conv_stage);
  f32x3       <= measured f16 / 10, so the split-precision mode cannot pass with the f16 mode's arithmetic (where the f16 mode has
              fp16 operands; see SPLIT_IN_F16);
  f16         its own budget per stage with the F16_MIN_MARGIN headroom rule of test_gpu_parity.py.

Shapes: each selects different kernel shapes (bsr_api.hip) — B = 2 the small-batch tiles; B = 32 the full batch (fused attention + `w`,
fused heads, resident conv1 GEMM), once more with BSR_FUSE_ATTW=0 for the att<i> probes; B = 16 at 288x256 / 256x512 the ragged
full-batch tiles; 3x32x256 the smallest accepted image; TSM at frame 2 and 4 for the ShareLayer stage.  Rows of big batches are
independent (test_rows_are_independent_and_deterministic), so the first and last rows stand for the batch.

The TSM generator gets the whole table too (TSM_SHAPES, run_tsm_full_stages): its widths (K = 312 / 888 in fp32, 320 / 896 in the 16-bit
modes), the second ShareLayer written in place into xh, the lanes beyond 288 of every block output (lrelu_copy_kernel) each on a line of
their own, and share=False.  The ShareLayer mixes the rows of a frame group, so there whole groups are compared, the first and the last.
Run with -rP (or -s) to see the table of measured errors."""

import pytest
import torch

from blindshadowremoval_amd.weights import init_weights
from stage_parity import (GSC_STAGES, TSM_STAGES, TSM_FULL_STAGES, EXACT_STAGES, gpu_probes, run_gsc_stages, run_tsm_full_stages, run_tsm_stages,
                          smooth_reg)

F32_CEILING = 1e-5
F16_MIN_MARGIN = 0.20      # the headroom rule of test_gpu_parity.py: a measured f16 error must leave 20 % of its tolerance

# TOL[stage kind][dtype] = (tolerance, measured on the MI355X: max over every shape, block and compared row of this file).
# f16 budgets are ~1.7x their measured value (F16_MIN_MARGIN needs <= 0.8x).  heads and colour_tail run split precision in the f16 mode
# too (conv_n16.h with hi/lo planes, only its input is fp16), so there the f16 mode is held to the fp32-class budget and the fp16-operand
# yardstick of the f32x3 budget is the CPU emulation instead (test_fp16_weights_fail_every_conv_stage: >= 10x every f32x3 budget).
# Attention (no 1/sqrt(d) on the logits, model.py:51): measured max |theta.phi| 25 (res5) on these inputs, softmax error 2e-6 in f32.
TOL = {
    "stem":            {"f32": (1e-5, 5.4e-7), "f32x3": (1e-5, 5.1e-7), "f16": (6e-4, 3.5e-4)},
    "down1":           {"f32": (1e-5, 6.4e-7), "f32x3": (1e-5, 4.4e-7), "f16": (8e-4, 4.7e-4)},
    "down2":           {"f32": (1e-5, 1.2e-6), "f32x3": (1e-5, 8.4e-7), "f16": (8e-4, 4.5e-4)},
    "down3_uv":        {"f32": (1e-5, 1.2e-6), "f32x3": (1e-5, 6.9e-7), "f16": (3.5e-4, 2.0e-4)},
    "res_head":        {"f32": (1e-5, 6.4e-7), "f32x3": (1e-5, 5.2e-7), "f16": (3.5e-4, 2.0e-4)},
    "res_att":         {"f32": (1e-5, 2.0e-6), "f32x3": (1e-5, 1.9e-6), "f16": (1e-3, 6.0e-4)},
    "res_block":       {"f32": (1e-5, 6.6e-7), "f32x3": (1e-5, 7.4e-7), "f16": (4e-4, 2.2e-4)},
    "up1":             {"f32": (1e-5, 1.7e-6), "f32x3": (1e-5, 1.1e-6), "f16": (1e-3, 5.8e-4)},
    "up2":             {"f32": (1e-5, 1.1e-6), "f32x3": (1e-5, 8.6e-7), "f16": (9e-4, 5.2e-4)},
    "up3":             {"f32": (1e-5, 1.4e-6), "f32x3": (1e-5, 8.3e-7), "f16": (8e-4, 4.7e-4)},
    "heads":           {"f32": (1e-5, 1.0e-6), "f32x3": (1e-5, 1.5e-6), "f16": (1e-5, 1.4e-6)},
    "res3_input":      {"f32": (0.0, 0.0), "f32x3": (0.0, 0.0), "f16": (0.0, 0.0)},
    "clr_up1":         {"f32": (1e-5, 2.3e-6), "f32x3": (1e-5, 1.3e-6), "f16": (1e-3, 5.8e-4)},
    "clr_up2":         {"f32": (1e-5, 1.0e-6), "f32x3": (1e-5, 7.9e-7), "f16": (9e-4, 5.4e-4)},
    "clr_up3":         {"f32": (1e-5, 9.2e-7), "f32x3": (1e-5, 6.4e-7), "f16": (9e-4, 5.2e-4)},
    "colour_tail":     {"f32": (1e-5, 7.2e-7), "f32x3": (1e-5, 7.5e-7), "f16": (1e-5, 5.9e-7)},
    "tsm_down3_share": {"f32": (1e-5, 1.1e-6), "f32x3": (1e-5, 9.2e-7), "f16": (3.5e-4, 2.0e-4)},
    "tsm_res_tail":    {"f32": (1e-5, 3.3e-09), "f32x3": (1e-5, 3.3e-09), "f16": (1e-5, 3.3e-09)},
    "tsm_res3_select": {"f32": (0.0, 0.0), "f32x3": (0.0, 0.0), "f16": (0.0, 0.0)},
    "tsm_share2":      {"f32": (1e-5, 2.6e-06), "f32x3": (1e-5, 2.6e-06), "f16": (1e-5, 2.7e-06)},
}
# tsm_res_tail and tsm_share2 read and write the fp32 trunk in every mode: fp32-class in f16 too.  tsm_share2 is normalised by its own
# slice (the fp32 oracle alone: 5e-7 at a 16x16 map, test_stage_parity_cpu.py::test_share_layer_fp32_error_at_the_tested_map_sizes for 32 / 64).
SPLIT_IN_F16 = ("heads", "colour_tail", "tsm_res_tail", "tsm_share2")

# The TSM table's own f16 budgets, for the kinds that are a GSC kernel at another K (res*.conv1 and the c3q residual at 291 / 877 in
# place of 99 / 257 / 261, up1 at K = 291, clr_up1 at K = 877): the GSC row's f16 budget times the ratio of the two CPU emulations of
# fp16 operands (tools/f16_stage_emulation.py, recorded in profiles/tsm_f16_stage_emulation.txt).  Every other kind keeps its TOL row.
TSM_F16_RATIO = {"res_head": 0.80, "res_block": 0.83, "up1": 0.85, "clr_up1": 1.53}
TSM_F16_TOL = {"res_head": 2.8e-4, "res_block": 3.3e-4, "up1": 8.5e-4, "clr_up1": 1.5e-3}
# measured on the MI355X over TSM_SHAPES (max over shapes, blocks and compared rows), the kinds TOL's measured column does not cover
TSM_MEASURED = {
    "stem":            {"f32": 6.4e-07, "f32x3": 4.6e-07, "f16": 3.5e-04},
    "down1":           {"f32": 8.5e-07, "f32x3": 5.3e-07, "f16": 4.6e-04},
    "down2":           {"f32": 1.3e-06, "f32x3": 8.2e-07, "f16": 4.3e-04},
    "tsm_down3_share": {"f32": 1.4e-06, "f32x3": 1.3e-06, "f16": 2.0e-04},
    "res_head":        {"f32": 4.2e-07, "f32x3": 5.0e-07, "f16": 2.0e-04},
    "res_att":         {"f32": 1.3e-06, "f32x3": 1.7e-06, "f16": 3.9e-04},
    "res_block":       {"f32": 4.3e-07, "f32x3": 9.0e-07, "f16": 2.0e-04},
    "tsm_res_tail":    {"f32": 3.3e-09, "f32x3": 3.3e-09, "f16": 3.3e-09},
    "up1":             {"f32": 1.6e-06, "f32x3": 1.2e-06, "f16": 5.6e-04},
    "up2":             {"f32": 1.6e-06, "f32x3": 1.0e-06, "f16": 4.7e-04},
    "up3":             {"f32": 1.1e-06, "f32x3": 7.1e-07, "f16": 4.8e-04},
    "heads":           {"f32": 1.2e-06, "f32x3": 1.9e-06, "f16": 1.8e-06},
    "tsm_res3_select": {"f32": 0.0, "f32x3": 0.0, "f16": 0.0},
    "tsm_share2":      {"f32": 2.6e-06, "f32x3": 2.6e-06, "f16": 2.7e-06},
    "clr_up1":         {"f32": 3.5e-06, "f32x3": 2.7e-06, "f16": 6.0e-04},
    "clr_up2":         {"f32": 1.3e-06, "f32x3": 8.5e-07, "f16": 4.4e-04},
    "clr_up3":         {"f32": 1.5e-06, "f32x3": 7.3e-07, "f16": 4.4e-04},
    "colour_tail":     {"f32": 8.9e-07, "f32x3": 7.1e-07, "f16": 5.1e-07},
}


def tolerance(kind: str, dtype: str, tsm: bool = False) -> float:
    if tsm and dtype == "f16" and kind in TSM_F16_TOL:
        return TSM_F16_TOL[kind]
    return TOL[kind][dtype][0]


DTYPES = ("f32", "f32x3", "f16")

# (B, H, W, environment, rows compared)
SHAPES = {
    "b2_256x256": (2, 256, 256, {}, [0, 1]),
    "b32_256x256": (32, 256, 256, {}, [0, 31]),
    "b32_256x256_unfused_attw": (32, 256, 256, {"BSR_FUSE_ATTW": "0"}, [0, 31]),
    "b16_288x256": (16, 288, 256, {}, [0, 15]),
    "b16_256x512": (16, 256, 512, {}, [0, 15]),
    "b3_32x256": (3, 32, 256, {}, [0, 1, 2]),
}


@pytest.fixture(scope="module")
def oracles():
    from oracle.gsc_oracle import GeneratorOracle, GeneratorTSMOracle
    w, wt = init_weights(1), init_weights(1, variant="tsm")
    return w, GeneratorOracle(w, dtype=torch.float64), wt, GeneratorTSMOracle(wt, dtype=torch.float64)


# (B, side, frame, share, environment, rows compared, att<i> exists in f32: None = whichever the launch heuristic picks)
TSM_SHAPES = {
    "tsm_b4_256_frame2": (4, 256, 2, True, {}, [0, 1, 2, 3], True),
    "tsm_b4_256_frame4": (4, 256, 4, True, {}, [0, 1, 2, 3], True),
    "tsm_b2_256_noshare": (2, 256, 2, False, {}, [0, 1], True),
    "tsm_b8_512_frame2": (8, 512, 2, True, {}, [6, 7], None),                    # the configs[4] per-rank shape: 64x64 warp map, 4096 tokens
    "tsm_b32_256_frame4": (32, 256, 4, True, {}, [0, 1, 2, 3, 28, 29, 30, 31], False),   # full batch: fused heads, fp32 fused attention + `w`
    "tsm_b32_256_frame4_unfused_attw": (32, 256, 4, True, {"BSR_FUSE_ATTW": "0"}, [0, 1, 2, 3, 28, 29, 30, 31], True),
}


def _check(dtype: str, tag: str, res, want_kinds, tsm: bool = False) -> None:
    print("\n".join(res.lines("%-5s %-26s" % (dtype, tag))))
    got = res.by_kind()
    assert set(got) == set(want_kinds), (sorted(got), sorted(want_kinds))
    bad = []
    for kind, err in got.items():
        tol = tolerance(kind, dtype, tsm)
        limit = (1.0 - F16_MIN_MARGIN) * tol if dtype == "f16" and kind not in EXACT_STAGES else tol
        if not err <= limit:
            bad.append("%s: %.3e > %.3e" % (kind, err, limit))
    assert not bad, "%s %s: %s" % (dtype, tag, "; ".join(bad))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("dtype", DTYPES)
def test_every_stage_tracks_the_fp64_oracle(oracles, dtype, shape, monkeypatch):
    from blindshadowremoval_amd import Generator
    w, o64 = oracles[:2]
    B, H, W, env, rows = SHAPES[shape]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    gen = Generator(dtype=dtype).load_weights(w)
    for k in env:
        monkeypatch.delenv(k)
    torch.manual_seed(31)
    inp, uv = torch.rand(B, H, W, 3), torch.rand(B, H, W, 3)
    uv[:, :, :W // 8] = 0                  # real uv maps are ~60 % zeros outside the landmark hull
    out = gen(inp.cuda(), uv.cuda())
    try:
        gen.probe("att0")
        att = True
    except RuntimeError:                   # fused attention + `w`: the attention output never left LDS
        att = False
    assert att or "BSR_FUSE_ATTW" not in env, "BSR_FUSE_ATTW=0 keeps attention and `w` two launches"
    p = gpu_probes(gen, inp, uv, out, rows, att)
    gen.close()
    res = run_gsc_stages(o64, p)
    _check(dtype, shape, res, [k for k in GSC_STAGES if att or k != "res_att"])


@pytest.mark.gpu
@pytest.mark.parametrize("frame", [2, 4])
@pytest.mark.parametrize("dtype", DTYPES)
def test_tsm_share_layer_stage_tracks_the_fp64_oracle(oracles, dtype, frame):
    from blindshadowremoval_amd import GeneratorTSM
    wt, o64 = oracles[2:]
    gen = GeneratorTSM(dtype=dtype).load_weights(wt)
    torch.manual_seed(41 + frame)
    B = 4
    inp, uv = torch.rand(B, 256, 256, 3), torch.rand(B, 256, 256, 3)
    # smooth offset fields of a few cells amplitude, some leaving the map (as test_tsm_variant_matches_oracle)
    reg = torch.nn.functional.interpolate((torch.rand(B, 6, 9, 9) - 0.5) * 0.3, size=(256, 256), mode="bicubic", align_corners=True).permute(0, 2, 3, 1).contiguous()
    reg[..., 2] = 0
    reg[..., 5] = 0
    gen(inp.cuda(), uv.cuda(), reg.cuda(), frame, True)
    p = {"x3": gen.probe("x3").cpu(), "x0": gen.probe("x0").cpu(), "uv": uv, "reg": reg}
    gen.close()
    _check(dtype, "tsm_frame%d" % frame, run_tsm_stages(o64, p, frame), TSM_STAGES)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(TSM_SHAPES))
@pytest.mark.parametrize("dtype", DTYPES)
def test_every_tsm_stage_tracks_the_fp64_oracle(oracles, dtype, shape, monkeypatch):
    from blindshadowremoval_amd import GeneratorTSM
    wt, o64 = oracles[2:]
    B, S, frame, share, env, rows, att_f32 = TSM_SHAPES[shape]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    gen = GeneratorTSM(dtype=dtype).load_weights(wt)
    for k in env:
        monkeypatch.delenv(k)
    g = torch.Generator().manual_seed(61 + B + S + frame)
    inp, uv = torch.rand(B, S, S, 3, generator=g), torch.rand(B, S, S, 3, generator=g)
    uv[:, :, :S // 8] = 0
    reg = smooth_reg(B, S, g)
    # warp.py:134-165: coords = offsets * side of the map + grid; offsets of several cells, negative ones in the first row (grid 0) and
    # positive ones in the last: both ends of the clamp are hit, for reg_in and reg_out
    assert float(reg.abs().max()) * (S // 8) > 2
    assert float(reg[:, :4, :, [0, 3]].amax(dim=(0, 1, 2)).min()) > 0 > float(reg[:, :4, :, [0, 3]].amin(dim=(0, 1, 2)).max())
    assert float(reg[:, -4:, :, [0, 3]].amax(dim=(0, 1, 2)).min()) > 0
    out = gen(inp.cuda(), uv.cuda(), reg.cuda(), frame, share)
    try:
        gen.probe("att0")
        att = True
    except RuntimeError:                   # fused attention + `w`: the attention output never left LDS
        att = False
    # the 16-bit modes run attention + `w` as one launch at every batch; fp32 only at full batches (attention_auto_qw == 4)
    want_att = bool(env) if dtype != "f32" else att_f32
    assert want_att is None or att == want_att, "%s %s: att0 %s" % (dtype, shape, "exists" if att else "is refused")
    p = gpu_probes(gen, inp, uv, out, rows, att, reg=reg)
    gen.close()
    assert p["xh"].shape[-1] == 877 and p["x0"].shape[-1] == 291
    res = run_tsm_full_stages(o64, p, frame, share)
    _check(dtype, shape, res, [k for k in TSM_FULL_STAGES if att or k != "res_att"], tsm=True)
    if not share:                          # both ShareLayers are copies: exactly 0, not merely inside the 1e-5 budget
        copies = {k: e for k, e in res.errs.items() if k[0] == "tsm_share2"}
        assert len(copies) == 2 and all(e == 0.0 for e in copies.values()), copies
