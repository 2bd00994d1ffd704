"""-m gpu: the single-stage RGB baseline (/root/reference/model_RGB.py) on the MI355X — GeneratorRGB / bsr_forward_rgb.

* whole forward against the fp32 oracle (tests/rgb_oracle.py) at 1e-3 absolute, at four shapes: (32,256,256) the full batch,
  (2,256,256) a small one, (16,288,256) a ragged token count (1152), (3,32,256) the smallest image (128 tokens, one query block);
  rows of a batch are independent (no op mixes images), so big batches are compared on their first and last rows;
* the same forward against the reference's own model_RGB.py run over the TF stand-in (tests/golden/model_py_rgb_*.npz);
* the teacher-forced stage table against the fp64 oracle at the fp32-class budget of tests/stage_parity.py (1e-5, scale-relative);
* the d = 256 attention kernel alone (bsr_debug_attention_rgb) against fp64 softmax(theta phi^T) g, with logits large enough to force the
  online rescale;
* the refusals (wrong entry, wrong dtype), bit-identical repeats, and an allocation-free forward after reserve().
Run with -rP (or -s) to see the measured errors."""
import ctypes
import os

import numpy as np
import pytest
import torch

from blindshadowremoval_amd import GeneratorRGB, Generator, init_weights
from blindshadowremoval_amd import _lib
from blindshadowremoval_amd.pack import pack_generator
from rgb_oracle import GeneratorRGBOracle, load_fixture
from oracle.gsc_oracle import resize_bilinear
from stage_parity import Result, _cat

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL_ABS = 1e-3            # whole forward vs the fp32 oracle (the GSC bar of test_gpu_parity.py)
STAGE_BUDGET = 1e-5       # fp32-class per-stage budget (tests/stage_parity.py)
SHAPES = [(32, 256, 256), (2, 256, 256), (16, 288, 256), (3, 32, 256)]
ERR_ARG = 1


def _rows(B):
    return [0, B - 1] if B > 3 else list(range(B))


def _inputs(B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(B, H, W, 3, generator=g), torch.rand(B, H, W, 3, generator=g)


@pytest.fixture(scope="module")
def rgb():
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    w = init_weights(1, variant="rgb")
    gen = GeneratorRGB().load_weights(w)
    yield gen, w
    gen.close()


@pytest.mark.parametrize("B,H,W", SHAPES)
def test_forward_matches_oracle(rgb, B, H, W):
    gen, w = rgb
    inp, uv = _inputs(B, H, W, 100 + B)
    con = gen(inp.cuda(), uv.cuda()).cpu()
    assert con.shape == (B, H, W, 3) and bool(torch.isfinite(con).all())
    rows = _rows(B)
    ref = GeneratorRGBOracle(w)(inp[rows], uv[rows])
    err = float((con[rows] - ref).abs().max())
    print("rgb forward %s rows %s: max abs err %.3e (scale %.3f)" % ((B, H, W), rows, err, float(ref.abs().max())))
    assert err <= TOL_ABS


@pytest.mark.parametrize("fixture", ["model_py_rgb_256.npz"])      # the 64x64 fixture is below the kernels' W % 256 rule (CPU-tested only)
def test_forward_matches_reference_model_rgb_py(rgb, fixture):
    path = os.path.join(GOLD, fixture)
    if not os.path.isfile(path):
        pytest.skip("%s was not generated (tools/make_model_rgb_fixture.py)" % fixture)
    gen, _ = rgb
    assert int(np.load(path)["weights_seed"]) == 1
    inp, uv, ref, s = load_fixture(path)
    con = gen(inp.cuda(), uv.cuda()).cpu().numpy()[:, ::s, ::s]
    assert con.shape == ref.shape
    err = float(np.abs(con - ref).max())
    print("rgb forward vs %s: max abs err %.3e" % (fixture, err))
    assert err <= TOL_ABS


def _probes(gen, names):
    return {n: gen.probe(n).cpu() for n in names}


def run_rgb_stages(o64, p):
    """Teacher-forced stages of the RGB forward: each fed the GPU's own input probes (fp64), compared with fp64 (stage_parity.py)."""
    r = Result()
    p = {k: v.detach().cpu().to(torch.float64) for k, v in p.items()}
    r.add("stem", "stem", "x1", p["x1"], o64.conv_block(p["inputs"], "conv1"))
    r.add("down1", "down1", "x2", p["x2"], o64.conv_block(p["x1"], "down1", 2))
    r.add("down2", "down2", "x3", p["x3"], o64.conv_block(p["x2"], "down2", 2))
    x = o64.conv_block(p["x3"], "down3", 2)
    r.add("down3_uv", "down3_uv", "x0", p["x0"], _cat(x, resize_bilinear(p["uv"], x.shape[1:3])))
    for i, src in enumerate(("x0", "res0", "res1")):
        xin, pr = p[src], {}
        res = o64.res_bottleneck(xin, i, pr)
        y3 = pr["res_stack/%d/y3" % i]
        y3x = y3.clone()
        y3x[..., :xin.shape[-1]] += xin
        r.add("res_head", "res%d" % i, "y3x", p["y3x%d" % i], y3x)
        r.add("res_att", "res%d" % i, "att", p["att%d" % i], pr["res_stack/%d/non_local/att" % i])
        r.add("res_block", "res%d" % i, "res", p["res%d" % i], res)
    r.add("up1", "up1", "up1", p["up1"], o64.convt_block(p["res2"], "up1"))
    r.add("up2", "up2", "up2", p["up2"], o64.convt_block(_cat(p["up1"], p["x3"]), "up2"))
    r.add("up3", "up3", "up3", p["up3"], o64.convt_block(_cat(p["up2"], p["x2"]), "up3"))
    r.add("head", "head", "y", p["y"], o64.conv_block(p["up3"], "conv2", bn=False, act=False))
    r.add("tail", "tail", "con", p["con"], o64.conv_block(p["y"], "conv3", bn=False, act=False))
    return r


RGB_STAGES = ("stem", "down1", "down2", "down3_uv", "res_head", "res_att", "res_block", "up1", "up2", "up3", "head", "tail")
PROBES = ("x1", "x2", "x3", "x0", "y3x0", "att0", "res0", "y3x1", "att1", "res1", "y3x2", "att2", "res2", "up1", "up2", "up3", "y", "con")


@pytest.mark.parametrize("B,H,W", SHAPES)
def test_stage_table_fp64(rgb, B, H, W):
    gen, w = rgb
    inp, uv = _inputs(B, H, W, 200 + B)
    con = gen(inp.cuda(), uv.cuda())
    p = _probes(gen, PROBES)
    assert torch.equal(p["con"], con.cpu())                   # the con probe is the returned tensor
    rows = [0] if B > 3 else list(range(B))
    p = {k: v[rows] for k, v in p.items()}
    p.update(inputs=inp[rows], uv=uv[rows])
    r = run_rgb_stages(GeneratorRGBOracle(w, dtype=torch.float64), p)
    for line in r.lines("rgb %s" % ((B, H, W),)):
        print(line)
    kinds = r.by_kind()
    assert set(kinds) == set(RGB_STAGES)
    bad = {k: e for k, e in kinds.items() if not e <= STAGE_BUDGET}
    assert not bad, bad


def _att64(qkv):
    q, k, v = (qkv[..., 256 * j:256 * (j + 1)].double() for j in range(3))
    return torch.softmax(q @ k.transpose(1, 2), dim=-1) @ v


@pytest.mark.parametrize("tokens", [64, 1024, 1152])
@pytest.mark.parametrize("big", [False, True])
def test_attention256_kernel_matches_fp64(tokens, big):
    """bsr_debug_attention_rgb against fp64 softmax(theta phi^T) g (no 1/sqrt(d): model.py:51-53).  ``big``: key scales grow along
    the token axis so the running maximum climbs by far more than the rescale threshold over the key loop (logits 30-60)."""
    lib = _lib.load()
    g = torch.Generator().manual_seed(tokens + big)
    B = 2
    qkv = torch.randn(B, tokens, 768, generator=g) * (0.45 if big else 0.12)
    if big:
        qkv[..., 256:512] *= torch.linspace(0.2, 3.0, tokens)[None, :, None]
    ref = _att64(qkv)
    logit = float((qkv[..., :256].double() @ qkv[..., 256:512].double().transpose(1, 2)).abs().max())
    d_qkv, y = qkv.cuda(), torch.full((B, tokens, 256), float("nan"), device="cuda")
    _lib.check(lib.bsr_debug_attention_rgb(d_qkv.data_ptr(), y.data_ptr(), B, tokens, None), "bsr_debug_attention_rgb")
    torch.cuda.synchronize()
    err = float((y.cpu().double() - ref).abs().max()) / float(ref.abs().max())
    print("attention256 tokens %d big %s: max|logit| %.1f, scale-relative err %.3e" % (tokens, big, logit, err))
    if big:
        assert logit > 25          # the running maximum climbs by several rescale thresholds (8 log2 units) over the key loop
    assert err <= STAGE_BUDGET


def test_attention256_rejects_bad_tokens():
    lib = _lib.load()
    x = torch.zeros(1, 48, 768, device="cuda")
    y = torch.zeros(1, 48, 256, device="cuda")
    assert lib.bsr_debug_attention_rgb(x.data_ptr(), y.data_ptr(), 1, 48, None) == ERR_ARG


def test_wrong_entry_refusals(rgb):
    gen, _ = rgb
    lib = _lib.load()
    B, H, W = 1, 256, 256
    inp, uv = (t.cuda() for t in _inputs(B, H, W, 5))
    o1 = torch.empty(B, H, W, 1, device="cuda")
    o3 = torch.empty(B, H, W, 3, device="cuda")
    o3b = torch.empty(B, H, W, 3, device="cuda")
    o1b = torch.empty(B, H, W, 1, device="cuda")
    reg = torch.zeros(B, H, W, 6, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    # an RGB handle refuses the GSC and TSM entries ...
    rc = lib.bsr_forward(gen._handle, inp.data_ptr(), uv.data_ptr(), B, H, W, o1.data_ptr(), o3.data_ptr(), o3b.data_ptr(), o1b.data_ptr(), s)
    assert rc == ERR_ARG and b"bsr_forward_rgb" in lib.bsr_last_error()
    rc = lib.bsr_forward_tsm(gen._handle, inp.data_ptr(), uv.data_ptr(), reg.data_ptr(), B, H, W, 1, 1, o1.data_ptr(), o3.data_ptr(),
                             o3b.data_ptr(), o1b.data_ptr(), s)
    assert rc == ERR_ARG and b"bsr_forward_rgb" in lib.bsr_last_error()
    # ... and a GSC / TSM handle refuses the RGB one
    for variant in ("gsc", "tsm"):
        g = Generator().load_weights(init_weights(1, variant=variant))
        rc = lib.bsr_forward_rgb(g._handle, inp.data_ptr(), uv.data_ptr(), B, H, W, o3.data_ptr(), s)
        assert rc == ERR_ARG and variant.upper().encode() in lib.bsr_last_error()
        g.close()


def test_wrong_dtype_refusal():
    """RGB weights with a blob / handle dtype other than BSR_DTYPE_F32 fail in bsr_create with BSR_ERR_ARG and a clear message."""
    lib = _lib.load()
    blob = bytearray(pack_generator(init_weights(1, variant="rgb"), "f32"))
    for code in (1, 2):                                        # BSR_DTYPE_F16, BSR_DTYPE_F32X3 (the header records the dtype)
        blob[12:16] = code.to_bytes(4, "little")
        buf = (ctypes.c_char * len(blob)).from_buffer_copy(bytes(blob))
        h = ctypes.c_void_p()
        rc = lib.bsr_create(ctypes.byref(h), 0, ctypes.cast(buf, ctypes.c_void_p), len(blob), code)
        assert rc == ERR_ARG and not h.value
        assert b"BSR_DTYPE_F32 only" in lib.bsr_last_error()


def test_two_forwards_are_bit_identical(rgb):
    gen, _ = rgb
    inp, uv = (t.cuda() for t in _inputs(4, 256, 256, 9))
    a = gen(inp, uv).clone()
    b = gen(inp, uv)
    assert torch.equal(a, b)


def test_reserve_makes_the_forward_allocation_free():
    w = init_weights(2, variant="rgb")
    B, H, W = 8, 256, 256
    inp, uv = (t.cuda() for t in _inputs(B, H, W, 11))
    out = torch.empty(B, H, W, 3, device="cuda")
    warm = GeneratorRGB().load_weights(w)                      # loads the code objects
    warm(inp[:1], uv[:1])
    warm.close()
    gen = GeneratorRGB().load_weights(w)
    need = gen.workspace_bytes(B, H, W)
    gen.reserve(B, H, W)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    gen(inp, uv, out=out)
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info()[0]
    print("reserve: workspace %.1f MB, free memory change over the forward %.1f MB" % (need / 2**20, (free0 - free1) / 2**20))
    assert free0 - free1 < need // 4
    gen(inp[:4], uv[:4])                                       # a smaller forward fits the reserved workspace too
    torch.cuda.synchronize()
    assert free0 - torch.cuda.mem_get_info()[0] < need // 4
    gen.close()


def test_timing_names_the_rgb_layers(rgb):
    gen, _ = rgb
    inp, uv = (t.cuda() for t in _inputs(2, 256, 256, 13))
    gen.set_timing(True)
    gen(inp, uv)
    names = [n for n, _, _ in gen.get_launch_timing()]
    gen.set_timing(False)
    for n in ("conv1", "res0.attention", "res2.w", "up3", "rgb_head", "rgb_tail"):
        assert n in names, (n, names)
