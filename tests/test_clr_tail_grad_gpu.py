"""bsr_clr_tail_grad (csrc/clr_tail_grad_kernels.h) against the host statement blindshadowremoval_amd/generator_grad.py: tail_grad.

Stage by stage: each of the chain's launches, fed the DEVICE's own inputs, against the float64 statement of that launch alone within
max|got - ref| / max|ref| <= 1e-5, the project's fp32-class stage budget (tests/stage_parity.py).  End to end: the twelve outputs
against tail_grad(acts = the device's a1, a2), each on the scale of its own largest reference magnitude, within 4 x E2E_MEASURED, the
largest figure measured on the MI355X over these sizes (tools/clr_tail_bench.py --parity, profiles/clr_tail_grad_bench.json, DESIGN
section 18), never above 1e-3; the difference from the statement on its own float64 forward is printed and not asserted, since masks flip
at pre-activations that round across 0.

Sizes (H, W, B): (8, 32, 1) is one tile, every pixel a border pixel; (16, 64, 2) has interior tile edges both ways; (24, 96, 3) three
tiles each way and an odd batch, 27 tiles for P = 7 partials, which divides neither the tile count nor the 6912 pixels; (32, 256, 1) is
the smallest image the generator takes."""
import ctypes

import numpy as np
import pytest

from blindshadowremoval_amd import generator_grad as host

import clr_tail_grad_cases as cases

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
f32 = np.float32
STAGE_BUDGET = 1e-5
E2E_MEASURED = 1.08e-6         # the largest scaled error of an output measured on SIZES: d gamma1 at (24, 96, 3) (tools/clr_tail_bench.py --parity)
E2E_BOUND = min(4 * E2E_MEASURED, 1e-3)
SIZES = ((8, 32, 1), (16, 64, 2), (24, 96, 3), (32, 256, 1))


@pytest.fixture(scope="module")
def runner():
    from blindshadowremoval_amd import ColourTail
    r = ColourTail(0)
    r.load_weights(cases.tail_weights())
    return r


def to_dev(*arrays):
    dev = torch.device("cuda", 0)
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def to_host(res):
    return {k: v.cpu().numpy() for k, v in res.items()}


def device_run(runner, w, gs, f, g_con, g_gs):
    if w is not None:
        runner.load_weights(w)
    res = runner.tail_grad(*to_dev(gs, f, g_con, g_gs), keep=True)
    torch.cuda.synchronize()
    out = to_host(res)
    out["dtype"] = f32
    return out


def scaled_error(got, ref):
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / np.abs(ref).max())


@pytest.fixture(scope="module")
def device_results(runner):
    """Inputs, the device's result and what it left in the scratch, once per size."""
    out = {}
    for H, W, B in SIZES:
        w, *arrays = cases.case(H, W, B, 1)
        res = device_run(runner, w, *arrays)
        maps = to_host(runner.maps(B, H, W))
        out[(H, W, B)] = (w, arrays, res, maps)
    return out


@pytest.mark.parametrize("check", cases.CONSTRUCTED, ids=lambda c: c.__name__)
def test_constructed_case(runner, check):
    check(lambda *a: device_run(runner, *a))
    runner.load_weights(cases.tail_weights())


@pytest.mark.parametrize("H,W,B", SIZES)
def test_stage_by_stage(device_results, H, W, B):
    from blindshadowremoval_amd import pack
    w, (gs, f, g_con, g_gs), res, maps = device_results[(H, W, B)]
    rec = {k: v.astype(np.float64) for k, v in pack.clr_tail_grad_record(w).items()}

    def hold(what, got, want):
        got, want = np.asarray(got), np.asarray(want)
        assert got.shape == want.shape, what
        e = scaled_error(got, want)
        print("colour tail grad H=%d W=%d B=%d %s fed the device's input: scaled error %.3g" % (H, W, B, what, e))
        assert e <= STAGE_BUDGET, (what, e)

    # launch 1: a1, the forward's arithmetic
    fw = host.tail_forward(w, gs, f)
    hold("launch 1 a1", maps["a1"], fw["a1"])
    # launch 2 from the device's a1: a2, then gz1 with the device's masks
    a1, a2 = maps["a1"].astype(np.float64), maps["a2"].astype(np.float64)
    z2 = a1 @ rec["tail/k2f"] + rec["tail/b2f"]
    hold("launch 2 a2", maps["a2"], np.where(z2 >= 0, z2, 0.3 * z2))
    st = host.tail_grad(w, gs, f, g_con, g_gs, acts={"a1": maps["a1"], "a2": maps["a2"]})
    hold("launch 2 gz1", maps["gz1"], st["gz1"])
    S, G = maps["S"], np.asarray(g_con, np.float64)
    ax = (0, 1, 2)
    hold("launch 2 sum a1 (x) gz2", S[:256].reshape(16, 16), np.tensordot(a1, st["gz2"], axes=(ax, ax)))
    hold("launch 2 sum a2 (x) G", S[256:304].reshape(16, 3), np.tensordot(a2, G, axes=(ax, ax)))
    hold("launch 2 sum G", S[304:307], G.sum(axis=ax))
    hold("launch 2 sum gz1", S[307:323], maps["gz1"].astype(np.float64).sum(axis=ax))
    hold("launch 2 sum gz2", S[323:339], st["gz2"].sum(axis=ax))
    # launch 3 from the device's gz1: the kernel gradient before the BN factor
    x = np.concatenate([gs, f], axis=3)
    hold("launch 3 W1", maps["W1"], host.conv3x3_same_wgrad(x, maps["gz1"]))
    # launch 4 from the device's gz1: the data gradient
    _, inv1, mean1, rstd1, _ = host.bn_vectors(w, "clr_conv1")
    dx = host.conv3x3_same_dgrad(maps["gz1"].astype(np.float64) * inv1, w["clr_conv1/conv/kernel"])
    hold("launch 4 d_f", res["d_f"], dx[..., 1:])
    hold("launch 4 d_gs", res["d_gs"], dx[..., :1] + np.asarray(g_gs, np.float64))
    # launches 5 and 6 from the device's W1 and S
    b2, inv2, mean2, rstd2, _ = host.bn_vectors(w, "clr_conv2")
    b1 = np.asarray(w["clr_conv1/conv/bias"], np.float64)
    K1, K2 = np.asarray(w["clr_conv1/conv/kernel"], np.float64), np.asarray(w["clr_conv2/conv/kernel"], np.float64)[0, 0]
    hold("launch 5 d K1", res["clr_conv1/conv/kernel"], maps["W1"] * inv1)
    S1, S2 = S[307:323], S[323:339]
    hold("launch 6 d beta1", res["clr_conv1/bnorm/beta"], S1)
    hold("launch 6 d bias1", res["clr_conv1/conv/bias"], inv1 * S1)
    hold("launch 6 d gamma1", res["clr_conv1/bnorm/gamma"], (((K1 * maps["W1"]).sum(axis=(0, 1, 2)) + b1 * S1) - mean1 * S1) * rstd1)
    hold("launch 6 d beta2", res["clr_conv2/bnorm/beta"], S2)
    hold("launch 6 d bias2", res["clr_conv2/conv/bias"], inv2 * S2)
    hold("launch 6 d gamma2", res["clr_conv2/bnorm/gamma"], (((K2 * S[:256].reshape(16, 16)).sum(axis=0) + b2 * S2) - mean2 * S2) * rstd2)
    hold("launch 6 d K2", res["clr_conv2/conv/kernel"], (S[:256].reshape(16, 16) * inv2).reshape(1, 1, 16, 16))
    hold("launch 6 d K3", res["clr_conv3/conv/kernel"], S[256:304].reshape(1, 1, 16, 3))
    hold("launch 6 d b3", res["clr_conv3/conv/bias"], S[304:307])
    # d gamma as the statement writes it, a second pass over the activations, from the device's gz1
    c1 = fw["c1"]
    hold("launch 6 d gamma1 (statement's form)", res["clr_conv1/bnorm/gamma"], (maps["gz1"].astype(np.float64) * ((c1 - mean1) * rstd1)).sum(axis=ax))


@pytest.mark.parametrize("H,W,B", SIZES)
def test_end_to_end(runner, device_results, H, W, B):
    from blindshadowremoval_amd import _lib
    w, (gs, f, g_con, g_gs), res, maps = device_results[(H, W, B)]
    if (H, W, B) == (24, 96, 3):
        P, tiles = int(_lib.load().bsr_clr_tail_grad_partials(B, H, W)), B * (H // 8) * (W // 32)
        assert P > 1 and tiles % P != 0 and (B * H * W) % P != 0, (P, tiles)
    st = host.tail_grad(w, gs, f, g_con, g_gs, acts={"a1": res["a1"], "a2": res["a2"]})
    for name in cases.OUTPUTS:
        e = scaled_error(res[name], st[name])
        print("colour tail grad H=%d W=%d B=%d %s against the statement on the device's activations: scaled error %.3g (bound %.3g)"
              % (H, W, B, name, e, E2E_BOUND))
    d, at = cases.worst_scaled_diff(res, st)
    own, own_at = cases.worst_scaled_diff(res, host.tail_grad(w, gs, f, g_con, g_gs))
    print("colour tail grad H=%d W=%d B=%d: worst %.3g at %s; against the statement on its own float64 forward %.3g at %s (not asserted)"
          % (H, W, B, d, at, own, own_at))
    assert d <= E2E_BOUND, (d, at)


def flat_bytes(res):
    return [res[k].cpu().numpy().tobytes() for k in ("", "d_f", "d_gs")]


def test_a_repeated_call_and_two_sizes_on_one_scratch(runner, device_results):
    w, arrays3, _, _ = device_results[(24, 96, 3)]
    _, arrays1, _, _ = device_results[(8, 32, 1)]
    t3, t1 = to_dev(*arrays3), to_dev(*arrays1)
    first3 = flat_bytes(runner.tail_grad(*t3))
    first1 = flat_bytes(runner.tail_grad(*t1))             # B = 3 then B = 1 on the larger call's scratch
    assert flat_bytes(runner.tail_grad(*t3)) == first3
    assert flat_bytes(runner.tail_grad(*t1)) == first1
    fresh = type(runner)(0)
    fresh.load_weights(w)
    assert flat_bytes(fresh.tail_grad(*t1)) == first1       # a scratch of its own size gives the same bytes


def test_g_gs_none_and_zero_give_the_same_bytes(runner, device_results):
    _, (gs, f, g_con, g_gs), _, _ = device_results[(16, 64, 2)]
    t = to_dev(gs, f, g_con)
    assert flat_bytes(runner.tail_grad(*t, None)) == flat_bytes(runner.tail_grad(*t, torch.zeros_like(t[0])))


def test_debug_stops(runner, device_results):
    from blindshadowremoval_amd.clr_tail_gpu import LAUNCHES
    _, arrays, res, _ = device_results[(16, 64, 2)]
    t = to_dev(*arrays)
    assert len(LAUNCHES) == 6
    for stop in range(7):
        got = to_host(runner.stages(*t, stop))
        wrote_dgrad, wrote_k1, wrote_rest = stop >= 4, stop >= 5, stop >= 6
        for name in ("d_f", "d_gs"):
            assert (got[name].tobytes() == res[name].tobytes()) if wrote_dgrad else not got[name].any(), (stop, name)
        views = type(runner).split_grads(torch.from_numpy(got[""]))
        for name in cases.NAMES:
            v = views[name].numpy()
            done = wrote_k1 if name == "clr_conv1/conv/kernel" else wrote_rest
            assert (v.tobytes() == res[name].tobytes()) if done else not v.any(), (stop, name)
    with pytest.raises(ValueError, match="stop_after"):
        runner.stages(*t, 7)


def test_the_chain_is_captured_into_a_graph_and_replays_the_same_bytes(runner, device_results):
    """Stream capture refuses a host synchronisation and work on another stream that is not joined: a call that is captured, replayed
    and gives the eager call's bytes has neither.  The chain is a line of launches: the captured graph has no branches."""
    _, arrays, _, _ = device_results[(16, 64, 2)]
    t = to_dev(*arrays)
    eager = flat_bytes(runner.tail_grad(*t))
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        runner.tail_grad(*t)
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=side):
            res = runner.tail_grad(*t)
    torch.cuda.current_stream().wait_stream(side)
    for k in ("", "d_f", "d_gs"):
        res[k].zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert flat_bytes(res) == eager


def test_argument_errors_raise_before_any_launch(runner, device_results):
    from blindshadowremoval_amd import ColourTail, _lib
    from blindshadowremoval_amd.clr_tail_gpu import NO_WEIGHTS_TEXT, SIZE_TEXT
    dev = torch.device("cuda", 0)
    _, arrays, _, _ = device_results[(8, 32, 1)]
    gs, f, g_con, g_gs = to_dev(*arrays)
    with pytest.raises(ValueError) as e:
        ColourTail(0).tail_grad(gs, f, g_con, g_gs)
    assert str(e.value) == NO_WEIGHTS_TEXT
    with pytest.raises(TypeError) as e:
        runner.tail_grad(gs, f.cpu(), g_con, g_gs)
    assert str(e.value) == "f must be a float32 tensor [B,H,W,64] on %s" % dev
    with pytest.raises(ValueError) as e:
        runner.tail_grad(gs, f[:, :, :, :63].contiguous(), g_con, g_gs)
    assert str(e.value) == "f must be [1,8,32,64] like gs, got (1, 8, 32, 63)"
    odd = [torch.zeros((1, 12, 32, c), device=dev) for c in (1, 64, 3, 1)]
    with pytest.raises(ValueError) as e:
        runner.tail_grad(*odd)
    assert str(e.value) == SIZE_TEXT % (1, 12, 32)
    # the entry point itself: nothing is launched, the outputs keep their bytes
    lib = _lib.load()
    d_f, d_gs = torch.full((1, 8, 32, 64), 7.0, device=dev), torch.full((1, 8, 32, 1), 7.0, device=dev)
    flat = torch.full((int(lib.bsr_clr_tail_grad_floats()),), 7.0, device=dev)
    scratch = runner.scratch3(1, 8, 32)
    p = lambda t: ctypes.c_void_p(t.data_ptr())                                      # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(h=8, w=32, f_cs=64, nbytes=runner._blob.numel(), scr=scratch):
        return lib.bsr_clr_tail_grad(0, p(runner._blob), nbytes, p(gs), p(f), f_cs, p(g_con), p(g_gs), 1, h, w, p(d_f), p(d_gs), p(flat), 0,
                                     ctypes.c_void_p(scr), stream), lib.bsr_last_error().decode()

    for kw, text in ((dict(h=12), "B must be positive, H a multiple of 8 and W a multiple of 32 (conv_n16_kernel's tile), at most 2^26 pixels in all"),
                     (dict(w=48), "B must be positive, H a multiple of 8 and W a multiple of 32 (conv_n16_kernel's tile), at most 2^26 pixels in all"),
                     (dict(f_cs=63), "f_cs must be a multiple of 4 and at least 64"),
                     (dict(nbytes=16), "blob_bytes must be bsr_clr_tail_grad_blob_bytes() (pack.pack_clr_tail_grad)"),
                     (dict(scr=scratch + 8), "scratch must be 256-byte aligned")):
        assert call(**kw) == (1, "bsr_clr_tail_grad: " + text), kw
    torch.cuda.synchronize()
    for t in (d_f, d_gs, flat):
        assert bool((t == 7.0).all())


# ---- the generator's own f, in place
@pytest.fixture(scope="module")
def generated():
    """A seeded generator's forward at (32, 256), B = 2, its outputs and a copy of its f."""
    from blindshadowremoval_amd import Generator
    w = cases.tail_weights()
    gen = Generator(device=0)
    gen.load_weights(w)
    with pytest.raises(RuntimeError, match="no forward has run"):
        gen.last_f()
    rng = np.random.default_rng(21)
    inputs, uv = to_dev(rng.uniform(0, 1, (2, 32, 256, 3)).astype(f32), rng.uniform(0, 1, (2, 32, 256, 3)).astype(f32))
    outs = gen(inputs, uv)
    torch.cuda.synchronize()
    return gen, w, outs, gen.probe("f").clone()


def test_backward_reads_the_generators_f_in_place(runner, generated):
    gen, w, outs, f_copy = generated
    runner.load_weights(w)
    gs, con_rgb = outs[0], outs[1]
    before = [o.cpu().numpy().tobytes() for o in outs]
    _, _, g_con_a, g_gs_a = host.example_inputs(32, 256, 2, 9)
    g_con, g_gs = to_dev(g_con_a, g_gs_a)
    ptr, cs, shape = gen.last_f()
    assert shape == (2, 32, 256, 64) and cs >= 64 and ptr % 16 == 0
    in_place = runner.backward(gen, gs, g_con, g_gs)
    copied = runner.tail_grad(gs, f_copy, g_con, g_gs)
    torch.cuda.synchronize()
    assert flat_bytes(in_place) == flat_bytes(copied)
    assert [o.cpu().numpy().tobytes() for o in outs] == before                 # the generator's four outputs are untouched
    assert gen.probe("f").cpu().numpy().tobytes() == f_copy.cpu().numpy().tobytes()
    # the chain differentiates the function the forward computed
    con = host.tail_forward(w, gs.cpu().numpy(), f_copy.cpu().numpy())["con_rgb"]
    e = scaled_error(con_rgb.cpu().numpy(), con)
    print("colour tail: the generator's con_rgb against tail_forward on its own gs and f in float64: scaled error %.3g" % e)
    assert e <= 1e-5
    with pytest.raises(ValueError, match="last forward was"):
        runner.backward(gen, gs[:1].contiguous(), g_con[:1].contiguous(), None)


def test_last_f_is_refused_for_a_sixteen_bit_generator():
    from blindshadowremoval_amd import Generator
    gen = Generator(device=0, dtype="f16")
    gen.load_weights(cases.tail_weights())
    rng = np.random.default_rng(22)
    inputs, uv = to_dev(rng.uniform(0, 1, (1, 32, 256, 3)).astype(f32), rng.uniform(0, 1, (1, 32, 256, 3)).astype(f32))
    gen(inputs, uv)
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="BSR_DTYPE_F32 handles only"):
        gen.last_f()
