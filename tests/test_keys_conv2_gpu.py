"""-m gpu: the fp32 forward with conv2's output as the attention keys (the default: res*.c3q computes N = [y3 | q' | g] in place
around the key slot of the qkv rows; csrc/bsr_api.hip keys_compose) — against the fp64 oracle stage by stage, against the form that
projects phi (BSR_KEYS_CONV2=0), across batch sizes, and with hot logits.

Cases (CASES): each forward runs once per form and is shared by the tests.
  b2_32x256    128 tokens, the smallest trunk the library accepts.  (A 64x64 image — 64 tokens — is refused by Generator and bsr_forward: W must be a
               multiple of 256 and the tokens a multiple of 128; test_a_64x64_image_is_refused holds that, so this is the smallest case there is.)
  b3_256x256   the small-batch attention shapes, attention and `w` as two launches (att<i> probes exist)
  b17_256x256  attention_auto_qw(B, 1024) is 4 from B = 17 on at 256 CUs (17 * 8 = 136 blocks of 128 queries: one round of 8-wave
               workgroups costs 17, two rounds of 4-wave ones 20; at B = 16 the 4-wave shape costs 10): the smallest batch of the reference
               image size that runs attention + `w` as ONE launch with 8-wave workgroups (FUSEW).  _auto_qw restates the function.
  tsm_b2_256   GeneratorTSM at its smallest tested shape (B = 2, 256x256, frame 2)

Form against form: 3x the float32 emulation's figure (tools/keys_conv2_error.py, profiles/keys_conv2_error.txt: 2.6e-6 of max|att|),
relative to each probe's largest magnitude — the rule of tests/test_wino_forms_gpu.py.  y3x0 is bit-identical (the y3 columns of the
first block's GEMM have the same operands in the same order); from block 1 on the block INPUT differs between the forms, so y3x1..5 are
held to the tolerance like the res<i> probes.  bmask under parity_util's flip rule."""
import pytest
import torch

from blindshadowremoval_amd.weights import init_weights
from parity_util import FLIP_TOL
from stage_parity import GSC_STAGES, TSM_FULL_STAGES, gpu_probes, run_gsc_stages, run_tsm_full_stages, smooth_reg
from test_keys_conv2_cpu import KEYS_EMULATED_ERR
from test_stage_parity_gpu import _check

FORM_TOL = 3 * KEYS_EMULATED_ERR
THRESHOLD = 0.1
FUSEW_BATCH = 17

# name -> (B, H, W, tsm frame or 0, rows handed to the stage table)
CASES = {
    "b2_32x256": (2, 32, 256, 0, [0, 1]),
    "b3_256x256": (3, 256, 256, 0, [0, 1, 2]),
    "b17_256x256": (FUSEW_BATCH, 256, 256, 0, [0, FUSEW_BATCH - 1]),
    "tsm_b2_256": (2, 256, 256, 2, [0, 1]),
}
PROBES = ["y3x%d" % i for i in range(6)] + ["res%d" % i for i in range(6)] + ["bmask", "d32"]


def _auto_qw(batch: int, tokens: int, cus: int) -> int:
    """csrc/attention.h: attention_auto_qw."""
    best, qw = -1, 4
    for cand in (4, 2, 1):
        cost = ((batch * (tokens // 128) * (4 // cand) + cus - 1) // cus) * (17 if cand == 4 else 10)
        if best < 0 or cost < best:
            best, qw = cost, cand
    return qw


def _inputs(name):
    B, H, W, frame, _ = CASES[name]
    g = torch.Generator().manual_seed(300 + B + H)
    inp, uv = torch.rand(B, H, W, 3, generator=g), torch.rand(B, H, W, 3, generator=g)
    uv[:, :, :W // 8] = 0
    reg = smooth_reg(B, H, g) if frame else None
    return inp, uv, reg


def _forward(gen, name, inp=None):
    """One forward of a case: (outputs on the CPU, probe dict of the stage table's rows, the form-against-form probes, att exists)."""
    B, H, W, frame, rows = CASES[name]
    inp0, uv, reg = _inputs(name)
    inp = inp0 if inp is None else inp
    out = gen(inp.cuda(), uv.cuda(), reg.cuda(), frame, True) if frame else gen(inp.cuda(), uv.cuda())
    try:
        gen.probe("att0")
        att = True
    except RuntimeError:                   # fused attention + `w`: the attention output never left LDS
        att = False
    p = gpu_probes(gen, inp, uv, out, rows, att, reg=reg)
    return [t.cpu() for t in out], p, {n: gen.probe(n).cpu() for n in PROBES}, att


@pytest.fixture(scope="module")
def runs():
    """Both forms' forwards of every case, once: runs[form][case] = _forward(...); form "keys" (default) or "phi" (BSR_KEYS_CONV2=0)."""
    from blindshadowremoval_amd import Generator, GeneratorTSM
    import os
    w, wt = init_weights(1), init_weights(1, variant="tsm")
    out = {}
    for form in ("keys", "phi"):
        old = os.environ.get("BSR_KEYS_CONV2")
        if form == "phi":
            os.environ["BSR_KEYS_CONV2"] = "0"
        try:
            gsc, tsm = Generator(dtype="f32").load_weights(w), GeneratorTSM(dtype="f32").load_weights(wt)      # the switch is read at bsr_create
        finally:
            if form == "phi":
                if old is None:
                    del os.environ["BSR_KEYS_CONV2"]
                else:
                    os.environ["BSR_KEYS_CONV2"] = old
        out[form] = {name: _forward(tsm if CASES[name][3] else gsc, name) for name in CASES}
        if form == "keys":
            out["gsc_keys"] = gsc
            tsm.close()
        else:
            gsc.close()
            tsm.close()
    yield out
    out["gsc_keys"].close()


@pytest.fixture(scope="module")
def oracles():
    from oracle.gsc_oracle import GeneratorOracle, GeneratorTSMOracle
    return GeneratorOracle(init_weights(1), dtype=torch.float64), GeneratorTSMOracle(init_weights(1, variant="tsm"), dtype=torch.float64)


@pytest.mark.gpu
def test_a_64x64_image_is_refused(runs):
    with pytest.raises(ValueError, match="W of 256"):           # Generator's own size check; bsr_forward states the same rule behind it
        runs["gsc_keys"](torch.rand(2, 64, 64, 3).cuda(), torch.rand(2, 64, 64, 3).cuda())


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_every_stage_of_the_new_form_tracks_the_fp64_oracle(runs, oracles, case):
    B, H, W, frame, rows = CASES[case]
    _, p, _, att = runs["keys"][case]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    fused = _auto_qw(B, (H // 8) * (W // 8), cus) == 4
    assert att == (not fused), "att<i> exists exactly when attention and `w` are two launches"
    if case == "b17_256x256":
        assert fused and _auto_qw(FUSEW_BATCH - 1, 1024, cus) != 4, "B = %d is the smallest FUSEW batch at 256x256 on %d CUs" % (FUSEW_BATCH, cus)
    if frame:
        res = run_tsm_full_stages(oracles[1], p, frame, True)
        _check("f32", case, res, [k for k in TSM_FULL_STAGES if att or k != "res_att"], tsm=True)
    else:
        res = run_gsc_stages(oracles[0], p)
        _check("f32", case, res, [k for k in GSC_STAGES if att or k != "res_att"])


def _rel(a, b) -> float:
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_new_form_agrees_with_the_projected_phi_form(runs, case):
    a, _, pa, _ = runs["keys"][case]
    b, _, pb, _ = runs["phi"][case]
    assert torch.equal(pa["y3x0"], pb["y3x0"]), "the y3 columns of res0.c3q have the same operands in the same order in both forms"
    assert not torch.equal(pa["res0"], pb["res0"]), "the switch selected the same form twice"
    differ = pa["bmask"] != pb["bmask"]
    if differ.any():
        assert float((pb["d32"][differ] - THRESHOLD).abs().max()) < FLIP_TOL, case
    same = ~differ.flatten(1).any(dim=1)                         # images whose threshold decisions agree
    assert same.any(), case
    every = torch.ones_like(same)
    worst, bad = 0.0, []
    for n in PROBES[:12]:
        rows = same if n in ("y3x3", "y3x4", "y3x5", "res3", "res4", "res5") else every
        e = _rel(pa[n][rows], pb[n][rows])
        worst = max(worst, e)
        print("keys vs phi %-12s %-8s %.3e" % (case, n, e))
        if not e <= FORM_TOL:
            bad.append((n, e))
    for x, y, name in zip(a, b, ("gs", "con_rgb", "mask22", "dif")):
        rows = every if name in ("gs", "mask22") else same
        e = _rel(x[rows], y[rows])
        worst = max(worst, e)
        print("keys vs phi %-12s %-8s %.3e" % (case, name, e))
        if not e <= FORM_TOL:
            bad.append((name, e))
    print("keys vs phi %s: worst rel diff %.3e (tolerance %.2e), bmask cells differing %d" % (case, worst, FORM_TOL, int(differ.sum())))
    assert not bad, (case, bad)


@pytest.mark.gpu
def test_an_image_gets_the_same_bits_alone_and_in_a_batch(runs):
    """The in-place c3q across batch sizes 1, 3 and the FUSEW batch: image 0 of b17_256x256, alone and with its first two neighbours."""
    gen = runs["gsc_keys"]
    inp, uv, _ = _inputs("b17_256x256")
    out17, _, p17, _ = runs["keys"]["b17_256x256"]
    for B in (1, 3):
        out = [t.cpu() for t in gen(inp[:B].cuda(), uv[:B].cuda())]
        for x, y, name in zip(out, out17, ("gs", "con_rgb", "mask22", "dif")):
            assert torch.equal(x, y[:B]), (B, name)
        for n in PROBES:
            assert torch.equal(gen.probe(n).cpu(), p17[n][:B]), (B, n)


@pytest.mark.gpu
def test_hot_logits_keep_the_block_outputs_inside_the_stage_budget(runs, oracles):
    """The b3_256x256 input at twice its amplitude: the logits (quadratic in the activations, no 1/sqrt(d): model.py:51) pass 50, the range
    tests/test_gpu_parity.py::test_attention_kernel_forced_rescale forces; att<i> and res<i> stay inside the fp32 stage budgets."""
    inp, _, _ = _inputs("b3_256x256")
    _, p, _, att = _forward(runs["gsc_keys"], "b3_256x256", inp=inp * 2.0)
    assert att
    res = run_gsc_stages(oracles[0], p)
    logits = [float(l.rsplit(" ", 1)[1]) for l in res.info if "attention logits" in l]
    print("hot logits: max |theta.phi| per block %s" % logits)
    assert len(logits) == 6 and max(logits) > 50.0
    _check("f32", "hot_logits", res, GSC_STAGES)
