"""-m gpu: the fp32 forward with conv2's output as the attention values as well (the default: res*.c3q computes N = [y3 | q'], the qkv rows
are [q' | t2] at stride 256, ONE LDS tile serves both products of the attention kernels and the `w` GEMM takes the image with g composed
onto it; csrc/bsr_api.hip values_compose) — the shared-tile kernel alone, the forward against the fp64 oracle stage by stage, against the
form that projects g (BSR_VALUES_CONV2=0), fused against two launches, across batch sizes, and with hot logits.

The cases, the probes compared and the bmask flip rule are those of tests/test_keys_conv2_gpu.py.  Form against form:
3 x VALUES_EMULATED_ERR (tools/values_conv2_error.py, profiles/values_conv2_error.txt) of each probe's largest magnitude.

attv<i> is checked on block 5: the six blocks share ONE qkv buffer, so after a forward the `qkv` probe holds the rows the LAST block's
attention read, and attv5 is the attention over exactly those rows."""
import os

import pytest
import torch

import attention_cases as ac
from blindshadowremoval_amd.weights import init_weights
from parity_util import FLIP_TOL
from stage_parity import GSC_STAGES, TSM_FULL_STAGES, run_gsc_stages, run_tsm_full_stages
from test_keys_conv2_gpu import CASES, FUSEW_BATCH, PROBES, THRESHOLD, _auto_qw, _forward, _inputs, _rel
from test_stage_parity_gpu import TOL, _check
from test_values_conv2_cpu import VALUES_EMULATED_ERR

FORM_TOL = 3 * VALUES_EMULATED_ERR

pytestmark = pytest.mark.gpu


def _lib():
    from blindshadowremoval_amd import _lib as L
    return L, L.load()


def _kernel(entry: str, x: torch.Tensor, qw: int) -> torch.Tensor:
    """One debug entry on rows x [B, T, C] -> [B, T, 128]; the output is NaN-prefilled with a guard block of T rows behind it."""
    L, lib = _lib()
    B, T, _ = x.shape
    buf = torch.full((B + 1, T, 128), float("nan"), device="cuda")
    L.check(getattr(lib, entry)(x.data_ptr(), buf.data_ptr(), B, T, qw, None), entry)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(buf[:B]).all()), (entry, qw, T, "rows left unwritten or not finite")
    assert bool(torch.isnan(buf[B]).all()), (entry, qw, T, "rows behind the output were written")
    return buf[:B]


def _same_bits_both_kernels(q: torch.Tensor, kv: torch.Tensor, qw: int) -> torch.Tensor:
    two = torch.cat((q, kv), dim=2).contiguous().cuda()
    three = torch.cat((q, kv, kv), dim=2).contiguous().cuda()
    got, want = _kernel("bsr_debug_attention_kv1", two, qw), _kernel("bsr_debug_attention_qw", three, qw)
    assert torch.equal(got, want), (qw, q.shape, float((got - want).abs().max()))
    return got


@pytest.mark.parametrize("qw", [4, 2, 1])
@pytest.mark.parametrize("T", [128, 256, 384])
def test_shared_tile_kernel_has_the_bits_of_the_three_slot_kernel(T, qw):
    """[q | x] through the shared-tile kernel against [q | x | x] through the three-slot one: same matrix operands in the same order.
    B = 3 images (the plain workgroup -> image map; with 8 the XCD-congruent one) at one, two and three trips of the key loop."""
    g = torch.Generator().manual_seed(900 + T + qw)
    for B in (3, 8):
        _same_bits_both_kernels(torch.randn(B, T, 128, generator=g) * 0.5, torch.randn(B, T, 128, generator=g) * 0.5, qw)


@pytest.mark.parametrize("case", ["late_spike_even", "late_spike_odd"])
def test_shared_tile_kernel_on_a_forced_rescale(case):
    """tests/attention_cases.py's late spike (one key far above the running maximum, late in either key stream: the rescale branch runs
    after the accumulators are loaded) with its phi as keys AND values: equal bits."""
    T = 256
    qkv = ac.make_case(case, 2, T, 128)
    q, kv = qkv[..., :128], qkv[..., 128:256]
    lg = ac.logits64(qkv)
    assert float((lg.max(dim=2).values - lg[:, :, :32].max(dim=2).values).min()) * 1.4426950408889634 > 8.0, "the spike forces a rescale in every row"
    _same_bits_both_kernels(q, kv, 4)


def _make(env: dict, tsm: bool = False):
    """A handle created under `env` (the switches are read at bsr_create)."""
    from blindshadowremoval_amd import Generator, GeneratorTSM
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return (GeneratorTSM if tsm else Generator)(dtype="f32").load_weights(init_weights(1, variant="tsm") if tsm else init_weights(1))
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def runs():
    """Both forms' forwards of every case, once: runs[form][case] = _forward(...); form "values" (default) or "g" (BSR_VALUES_CONV2=0)."""
    out = {}
    for form, env in (("values", {}), ("g", {"BSR_VALUES_CONV2": "0"})):
        gsc, tsm = _make(env), _make(env, tsm=True)
        out[form] = {name: _forward(tsm if CASES[name][3] else gsc, name) for name in CASES}
        tsm.close()
        if form == "values":
            out["gsc_values"] = gsc
        else:
            gsc.close()
    yield out
    out["gsc_values"].close()


@pytest.fixture(scope="module")
def oracles():
    from oracle.gsc_oracle import GeneratorOracle, GeneratorTSMOracle
    return GeneratorOracle(init_weights(1), dtype=torch.float64), GeneratorTSMOracle(init_weights(1, variant="tsm"), dtype=torch.float64)


@pytest.mark.parametrize("case", list(CASES))
def test_every_stage_of_the_values_form_tracks_the_fp64_oracle(runs, oracles, case):
    """Every stage through _check; res_att is the DERIVED probe (att = O Wg + bg) wherever attention and `w` are two launches."""
    B, H, W, frame, rows = CASES[case]
    _, p, _, att = runs["values"][case]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert att == (_auto_qw(B, (H // 8) * (W // 8), cus) != 4), "att<i> exists exactly when attention and `w` are two launches"
    if frame:
        res = run_tsm_full_stages(oracles[1], p, frame, True)
        _check("f32", case, res, [k for k in TSM_FULL_STAGES if att or k != "res_att"], tsm=True)
    else:
        res = run_gsc_stages(oracles[0], p)
        _check("f32", case, res, [k for k in GSC_STAGES if att or k != "res_att"])


@pytest.mark.parametrize("case", list(CASES))
def test_values_form_agrees_with_the_projected_g_form(runs, case):
    a, _, pa, _ = runs["values"][case]
    b, _, pb, _ = runs["g"][case]
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
        print("values vs g %-12s %-8s %.3e" % (case, n, e))
        if not e <= FORM_TOL:
            bad.append((n, e))
    for x, y, name in zip(a, b, ("gs", "con_rgb", "mask22", "dif")):
        rows = every if name in ("gs", "mask22") else same
        e = _rel(x[rows], y[rows])
        worst = max(worst, e)
        print("values vs g %-12s %-8s %.3e" % (case, name, e))
        if not e <= FORM_TOL:
            bad.append((name, e))
    print("values vs g %s: worst rel diff %.3e (tolerance %.2e), bmask cells differing %d" % (case, worst, FORM_TOL, int(differ.sum())))
    assert not bad, (case, bad)


def test_attv_is_the_attention_over_the_rows_the_kernel_read(runs):
    """attv5 of the B = 3 forward against softmax(q' t2^T) t2 in fp64 from the GPU's own `qkv` probe rows (the last block's), within the
    res_att budget's measured column; att5 = attv5 Wg + bg (the derived probe) differs from it, and `qkv` is [q' | t2] at 256."""
    gen = runs["gsc_values"]
    inp, uv, _ = _inputs("b3_256x256")
    gen(inp.cuda(), uv.cuda())
    qkv, o, att = gen.probe("qkv").cpu(), gen.probe("attv5").cpu(), gen.probe("att5").cpu()
    assert qkv.shape == (3, 32, 32, 256) and o.shape == (3, 32, 32, 128) and att.shape == o.shape and not torch.equal(o, att)
    q, t2 = qkv[..., :128].reshape(3, 1024, 128).double(), qkv[..., 128:].reshape(3, 1024, 128).double()
    ref = torch.softmax(q @ t2.transpose(1, 2), dim=-1) @ t2
    e = _rel(o.reshape(3, 1024, 128), ref)
    print("attv5 against fp64 softmax(q' t2^T) t2 of the qkv probe: %.3e (budget %.1e)" % (e, TOL["res_att"]["f32"][1]))
    assert e <= TOL["res_att"]["f32"][1]


def test_attv_is_refused_on_other_forms_and_after_a_fused_forward(runs):
    gen = runs["gsc_values"]
    inp, uv, _ = _inputs("b17_256x256")
    gen(inp.cuda(), uv.cuda())
    for name in ("att0", "attv0"):
        with pytest.raises(RuntimeError, match="never left LDS"):
            gen.probe(name)
    g = _make({"BSR_VALUES_CONV2": "0"})
    g(inp[:3].cuda(), uv[:3].cuda())
    with pytest.raises(RuntimeError, match="attv"):
        g.probe("attv0")
    g.close()


def test_fused_and_two_launch_forwards_have_the_same_bits(runs):
    """B = 17 (attention + `w` as one launch) against the same handle form with BSR_FUSE_ATTW=0: res0..5 and the four outputs."""
    out, _, p, att = runs["values"]["b17_256x256"]
    assert not att
    gen = _make({"BSR_FUSE_ATTW": "0"})
    inp, uv, _ = _inputs("b17_256x256")
    out2 = [t.cpu() for t in gen(inp.cuda(), uv.cuda())]
    gen.probe("att0")
    for x, y, name in zip(out2, out, ("gs", "con_rgb", "mask22", "dif")):
        assert torch.equal(x, y), name
    for i in range(6):
        assert torch.equal(gen.probe("res%d" % i).cpu(), p["res%d" % i]), i
    gen.close()


def test_an_image_gets_the_same_bits_alone_and_in_a_batch(runs):
    gen = runs["gsc_values"]
    inp, uv, _ = _inputs("b17_256x256")
    out17, _, p17, _ = runs["values"]["b17_256x256"]
    for B in (1, 3):
        out = [t.cpu() for t in gen(inp[:B].cuda(), uv[:B].cuda())]
        for x, y, name in zip(out, out17, ("gs", "con_rgb", "mask22", "dif")):
            assert torch.equal(x, y[:B]), (B, name)
        for n in PROBES:
            assert torch.equal(gen.probe(n).cpu(), p17[n][:B]), (B, n)


def test_hot_logits_keep_the_block_outputs_inside_the_stage_budget(runs, oracles):
    """The b3_256x256 input at twice its amplitude (max |logit| > 50): att<i> (derived) and res<i> stay inside the fp32 stage budgets."""
    inp, _, _ = _inputs("b3_256x256")
    _, p, _, att = _forward(runs["gsc_values"], "b3_256x256", inp=inp * 2.0)
    assert att
    res = run_gsc_stages(oracles[0], p)
    logits = [float(l.rsplit(" ", 1)[1]) for l in res.info if "attention logits" in l]
    print("hot logits: max |theta.phi| per block %s" % logits)
    assert len(logits) == 6 and max(logits) > 50.0
    _check("f32", "hot_logits", res, GSC_STAGES)
