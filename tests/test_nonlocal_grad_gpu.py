"""bsr_nonlocal_grad (csrc/nonlocal_grad_kernels.h) against the host statement blindshadowremoval_amd/generator_grad.py: nonlocal_grad.

Stage by stage: each of the chain's launches, fed the DEVICE's own inputs, against the float64 statement of that launch alone within
max|got - ref| / max|ref| <= 1e-5, the project's fp32-class stage budget.  End to end: the twelve outputs against nonlocal_grad(acts =
the device's own out), each on the scale of its own largest reference magnitude, within cases.E2E_BOUND = 4 x the largest figure measured
on the MI355X over these shapes (tools/nonlocal_grad_bench.py --parity, profiles/nonlocal_grad_bench.json).  The
hard-softmax case is held to 4 x the error of the statement run in float32 (cases.HARD_BOUND): logit rounding grows with |S|.

Image sizes (H, W, B) and their tokens per image T: (32, 256, 1) T = 128, two key and two query blocks of 64 and one row slice;
(64, 256, 2) T = 256, seams between blocks and between items; (96, 256, 3) T = 384, an odd block count; (32, 512, 1) T = 256, wide;
(256, 256, 1) T = 1024, the workload's token count, run once."""
import ctypes

import numpy as np
import pytest

from blindshadowremoval_amd import generator_grad as host

import nonlocal_grad_cases as cases

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
f32 = np.float32
ST = cases.ST
SIZES = ((32, 256, 1), (64, 256, 2), (96, 256, 3), (32, 512, 1), (256, 256, 1))
OUT_KEYS = ("", "d_y3", "d_skip")


@pytest.fixture(scope="module")
def runner():
    from blindshadowremoval_amd import NonLocalGrad
    r = NonLocalGrad(0)
    r.load_weights(cases.nl_weights())
    return r


def to_dev(*arrays):
    dev = torch.device("cuda", 0)
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def to_host(res):
    return {k: v.cpu().numpy() for k, v in res.items()}


def device_run(runner, w, y3, xin, d_out, acts=None):
    """The `run` of cases.check_*."""
    runner.load_weights(w)
    arrays, y3_used = cases.device_inputs(w, y3, xin, d_out, None if acts is None else acts["out"])
    res = runner.nonlocal_grad(*to_dev(*arrays), keep=True)
    torch.cuda.synchronize()
    out = to_host(res)
    out.update({"out": arrays[2], "y3": y3_used, "dtype": f32})
    return out


def scaled_error(got, ref):
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / np.abs(ref).max())


@pytest.fixture(scope="module")
def device_results(runner):
    """Inputs, the device's result and what it left in the scratch, once per size."""
    out = {}
    for H, W, B in SIZES:
        w, y3, xin, d_out = cases.case(H // 8, W // 8, B, 1)
        arrays, y3_used = cases.device_inputs(w, y3, xin, d_out)
        res = runner.nonlocal_grad(*to_dev(*arrays), keep=True)
        torch.cuda.synchronize()
        out[(H, W, B)] = (w, arrays, y3_used, to_host(res), to_host(runner.maps(B, H // 8, W // 8)))
    return out


@pytest.mark.parametrize("check", cases.CONSTRUCTED, ids=lambda c: c.__name__)
def test_constructed_case(runner, check):
    check(lambda *a: device_run(runner, *a))
    runner.load_weights(cases.nl_weights())


@pytest.mark.parametrize("H,W,B", SIZES)
def test_stage_by_stage(device_results, H, W, B):
    w, (y3x, xin, out, d_out), y3_used, res, maps = device_results[(H, W, B)]
    T = (H // 8) * (W // 8)

    def hold(what, got, want):
        got, want = np.asarray(got), np.asarray(want)
        assert got.shape == want.shape, what
        e = scaled_error(got, want)
        print("non-local grad H=%d W=%d B=%d %s fed the device's input: scaled error %.3g" % (H, W, B, what, e))
        assert e <= cases.STAGE_BUDGET, (what, e)

    m = {k: v.astype(np.float64) for k, v in maps.items()}
    Wt, Wp, Wg, Ww = (np.asarray(w[ST + k + "/kernel"], np.float64)[0, 0] for k in ("theta", "phi", "g", "w"))
    bw, inv, mean, rstd, _, _ = host.nonlocal_bn_vectors(w)
    # launch 1: the entry, exact
    gz = host.leaky_grad(d_out, out).astype(f32)
    assert res["d_skip"].tobytes() == gz.tobytes()
    assert maps["dz"].tobytes() == np.ascontiguousarray(gz[..., :257]).tobytes()
    assert maps["y3"].tobytes() == y3_used.tobytes()
    # launch 2: the projections from the device's y3
    for k, Wk in (("theta", Wt), ("phi", Wp), ("g", Wg)):
        hold("launch 2 " + k, maps[k], m["y3"] @ Wk + np.asarray(w[ST + k + "/bias"], np.float64))
    # launch 3: L and A from the device's projections
    S = m["theta"] @ np.transpose(m["phi"], (0, 2, 1))
    mx = S.max(axis=2)
    hold("launch 3 m", maps["m"], mx)
    hold("launch 3 r", maps["r"], 1 / np.exp(S - mx[:, :, None]).sum(axis=2))
    P = np.exp(S - m["m"][:, :, None]) * m["r"][:, :, None]               # what launches 5 and 6 form: the device's own (m, r)
    hold("launch 3 A", maps["A"], (P / P.sum(axis=2, keepdims=True)) @ m["g"])
    # launch 4: dA and D from the device's dz and A
    hold("launch 4 dA", maps["dA"], (m["dz"] * inv) @ Ww.T)
    hold("launch 4 D", maps["D"], (m["dA"] * m["A"]).sum(axis=2))
    # launches 5 and 6: the attention gradient from the device's projections, dA, D and L
    dS = P * (m["dA"] @ np.transpose(m["g"], (0, 2, 1)) - m["D"][:, :, None])
    hold("launch 5 d_g", maps["d_g"], np.transpose(P, (0, 2, 1)) @ m["dA"])
    hold("launch 5 d_phi", maps["d_phi"], np.transpose(dS, (0, 2, 1)) @ m["theta"])
    hold("launch 6 d_theta", maps["d_theta"], dS @ m["phi"])
    # launches 7, 8, 11: the kernels from the device's maps
    ax = ([0, 1], [0, 1])
    for k in ("theta", "phi", "g"):
        hold("launches 7, 11 d W" + k, res[ST + k + "/kernel"][0, 0], np.tensordot(m["y3"], m["d_" + k], axes=ax))
    hold("launches 8, 11 Wgd", maps["Wgd"], np.tensordot(m["A"], m["dz"], axes=ax))
    hold("launch 11 d Ww", res[ST + "w/kernel"][0, 0], m["Wgd"] * inv)
    # launches 9, 12: the projections' biases; d phi/bias is a sum that cancels, held on d theta/bias' scale
    want = {k: m["d_" + k].sum(axis=(0, 1)) for k in ("theta", "phi", "g")}
    hold("launches 9, 12 d bt", res[ST + "theta/bias"], want["theta"])
    hold("launches 9, 12 d bg", res[ST + "g/bias"], want["g"])
    e = float(np.abs(res[ST + "phi/bias"] - want["phi"]).max() / np.abs(want["theta"]).max())
    print("non-local grad H=%d W=%d B=%d launches 9, 12 d bp on d bt's scale: %.3g" % (H, W, B, e))
    assert e <= cases.STAGE_BUDGET
    # launch 10: d_y3 from the device's maps
    hold("launch 10 d_y3", res["d_y3"].reshape(B, T, 257), m["dz"] + m["d_theta"] @ Wt.T + m["d_phi"] @ Wp.T + m["d_g"] @ Wg.T)
    # launch 12 from the device's dz and Wgd
    Sz = m["dz"].sum(axis=(0, 1))
    hold("launch 12 Sz", maps["Sz"], Sz)
    hold("launch 12 d beta", res[ST + "bnorm/beta"], m["Sz"])
    hold("launch 12 d bw", res[ST + "w/bias"], inv * m["Sz"])
    hold("launch 12 d gamma", res[ST + "bnorm/gamma"], (((Ww * m["Wgd"]).sum(axis=0) + bw * m["Sz"]) - mean * m["Sz"]) * rstd)


@pytest.mark.parametrize("H,W,B", SIZES)
def test_end_to_end(device_results, H, W, B):
    w, (y3x, xin, out, d_out), y3_used, res, maps = device_results[(H, W, B)]
    st = host.nonlocal_grad(w, y3_used, xin, d_out, acts={"out": out})
    for name in cases.OUTPUTS:
        print("non-local grad H=%d W=%d B=%d %s against the statement on the device's out: scaled error %.3g (bound %.3g)"
              % (H, W, B, name, cases.worst_scaled_diff(res, st, (name,))[0], cases.E2E_BOUND))
    d, at = cases.worst_scaled_diff(res, st)
    print("non-local grad H=%d W=%d B=%d: worst %.3g at %s" % (H, W, B, d, at))
    assert d <= cases.E2E_BOUND, (d, at)


def test_hard_softmax(runner):
    """max |S| > 200 (asserted by hard_case, with a near-one-hot and an ordinary row): finite everywhere and within 4 x the float32
    statement's own error against the float64 one."""
    w, y3, xin, d_out = cases.hard_case()
    r = device_run(runner, w, y3, xin, d_out)
    runner.load_weights(cases.nl_weights())
    for name in cases.OUTPUTS + host.NONLOCAL_MAPS:
        assert np.isfinite(r[name]).all(), name
    st = host.nonlocal_grad(w, r["y3"], xin, d_out, acts={"out": r["out"]})
    for name in cases.OUTPUTS:
        print("non-local grad, hard softmax: %s scaled error %.3g (bound %.3g)" % (name, cases.worst_scaled_diff(r, st, (name,))[0], cases.HARD_BOUND))
    d, at = cases.worst_scaled_diff(r, st)
    assert d <= cases.HARD_BOUND, (d, at)


def flat_bytes(res):
    return [res[k].cpu().numpy().tobytes() for k in OUT_KEYS]


def test_a_repeated_call_and_two_sizes_on_one_scratch(runner, device_results):
    w, arrays3, _, _, _ = device_results[(96, 256, 3)]
    _, arrays1, _, _, _ = device_results[(32, 256, 1)]
    t3, t1 = to_dev(*arrays3), to_dev(*arrays1)
    first3 = flat_bytes(runner.nonlocal_grad(*t3))
    first1 = flat_bytes(runner.nonlocal_grad(*t1))            # B = 3 then B = 1 on the larger call's scratch
    assert flat_bytes(runner.nonlocal_grad(*t3)) == first3
    assert flat_bytes(runner.nonlocal_grad(*t1)) == first1
    assert flat_bytes(runner.nonlocal_grad(*t1, keep=True)) == first1     # keeping the maps changes no output
    for t, a in zip(t1, arrays1):
        assert t.cpu().numpy().tobytes() == a.tobytes()                   # no input is ever written
    fresh = type(runner)(0)
    fresh.load_weights(w)
    assert flat_bytes(fresh.nonlocal_grad(*t1)) == first1      # a scratch of its own size gives the same bytes


def test_debug_stops(runner, device_results):
    from blindshadowremoval_amd.nonlocal_grad_gpu import LAUNCHES
    _, arrays, _, res, maps = device_results[(64, 256, 2)]
    t = to_dev(*arrays)
    assert len(LAUNCHES) == 12
    runner.stages(*t, 0)
    first = {"y3": 1, "dz": 1, "theta": 2, "phi": 2, "g": 2, "m": 3, "r": 3, "A": 3, "dA": 4, "D": 4, "d_phi": 5, "d_g": 5, "d_theta": 6, "Wgd": 11, "Sz": 12}
    kernels = tuple(n for n in cases.NAMES if n.endswith("/kernel"))
    for stop in range(13):
        got = to_host(runner.stages(*t, stop))
        assert (got["d_skip"].tobytes() == res["d_skip"].tobytes()) if stop >= 1 else not got["d_skip"].any(), stop
        assert (got["d_y3"].tobytes() == res["d_y3"].tobytes()) if stop >= 10 else not got["d_y3"].any(), stop
        views = type(runner).split_grads(torch.from_numpy(got[""]))
        for name in cases.NAMES:
            v = views[name].numpy()
            done = stop >= 11 if name in kernels else stop >= 12
            assert (v.tobytes() == res[name].tobytes()) if done else not v.any(), (stop, name)
        for name, at in first.items():
            if stop >= at:
                assert got[name].tobytes() == maps[name].tobytes(), (stop, name)
    with pytest.raises(ValueError, match="stop_after"):
        runner.stages(*t, 13)


def test_the_chain_is_captured_into_a_graph_and_replays_the_same_bytes(runner, device_results):
    """Stream capture refuses a host synchronisation and work on another stream that is not joined: a call that is captured, replayed
    and gives the eager call's bytes has neither.  The chain is a line of launches: the captured graph has no branches."""
    _, arrays, _, _, _ = device_results[(32, 256, 1)]
    t = to_dev(*arrays)
    eager = flat_bytes(runner.nonlocal_grad(*t))
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        runner.nonlocal_grad(*t)
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=side):
            res = runner.nonlocal_grad(*t)
    torch.cuda.current_stream().wait_stream(side)
    for k in OUT_KEYS:
        res[k].zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert flat_bytes(res) == eager


def test_argument_errors_raise_before_any_launch(runner, device_results):
    from blindshadowremoval_amd import NonLocalGrad, _lib
    from blindshadowremoval_amd.nonlocal_grad_gpu import NO_WEIGHTS_TEXT, SIZE_TEXT
    dev = torch.device("cuda", 0)
    _, arrays, _, _, _ = device_results[(32, 256, 1)]
    y3x, xin, out, d_out = to_dev(*arrays)
    with pytest.raises(ValueError) as e:
        NonLocalGrad(0).nonlocal_grad(y3x, xin, out, d_out)
    assert str(e.value) == NO_WEIGHTS_TEXT
    with pytest.raises(TypeError) as e:
        runner.nonlocal_grad(y3x, xin.cpu(), out, d_out)
    assert str(e.value) == "xin must be a float32 tensor [B,h,w,261] on %s" % dev
    with pytest.raises(ValueError) as e:
        runner.nonlocal_grad(y3x, xin[..., :260].contiguous(), out, d_out)
    assert str(e.value) == "xin must be [1,4,32,261] for this d_out, got (1, 4, 32, 260)"
    with pytest.raises(ValueError) as e:
        runner.nonlocal_grad(*[torch.zeros((1, 6, 32, c), device=dev) for c in (257, 261, 261, 261)])
    assert str(e.value) == SIZE_TEXT % (1, 6, 32)
    # the entry point itself: nothing is launched, the outputs keep their bytes
    lib = _lib.load()
    d_y3 = torch.full((1, 4, 32, 257), 7.0, device=dev)
    d_skip = torch.full((1, 4, 32, 261), 7.0, device=dev)
    flat = torch.full((int(lib.bsr_nonlocal_grad_floats()),), 7.0, device=dev)
    scratch = runner.scratch3(1, 4, 32)
    p = lambda t: ctypes.c_void_p(t.data_ptr())                                      # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(h=4, w=32, y3x_cs=257, xin_cs=261, nbytes=runner._blob.numel(), scr=scratch):
        return lib.bsr_nonlocal_grad(0, p(runner._blob), nbytes, p(y3x), y3x_cs, p(xin), xin_cs, p(out), 261, p(d_out), 1, h, w, p(d_y3), p(d_skip),
                                     p(flat), ctypes.c_void_p(scr), stream), lib.bsr_last_error().decode()

    size = "B must be positive, h a multiple of 4 and w a multiple of 32 (the generator's rule at 1/8 resolution), at most 2^21 tokens in all"
    cs = "y3x_cs must be at least 257, xin_cs and out_cs at least 261"
    for kw, text in ((dict(h=6), size), (dict(w=16), size), (dict(y3x_cs=256), cs), (dict(xin_cs=260), cs),
                     (dict(nbytes=16), "blob_bytes must be bsr_nonlocal_grad_blob_bytes() (pack.pack_nonlocal_grad; the GSC width 261 only, not TSM's 877)"),
                     (dict(scr=scratch + 8), "scratch must be 256-byte aligned")):
        assert call(**kw) == (1, "bsr_nonlocal_grad: " + text), kw
    torch.cuda.synchronize()
    for t in (d_y3, d_skip, flat):
        assert bool((t == 7.0).all())


# ---- the generator's own tensors, in place
PROBES = ("y3x5", "res4", "res5")


@pytest.fixture(scope="module")
def generated():
    """A seeded generator's forward at (32, 256), B = 2, its outputs and copies of the block's three tensors."""
    from blindshadowremoval_amd import Generator
    w = cases.nl_weights()
    gen = Generator(device=0)
    gen.load_weights(w)
    with pytest.raises(RuntimeError, match="no forward has run"):
        gen.last_block5()
    rng = np.random.default_rng(21)
    inputs, uv = to_dev(rng.uniform(0, 1, (2, 32, 256, 3)).astype(f32), rng.uniform(0, 1, (2, 32, 256, 3)).astype(f32))
    outs = gen(inputs, uv)
    torch.cuda.synchronize()
    return gen, w, outs, [gen.probe(k).clone() for k in PROBES]


def test_backward_reads_the_generators_tensors_in_place(runner, generated):
    gen, w, outs, copies = generated
    runner.load_weights(w)
    before = [o.cpu().numpy().tobytes() for o in outs]
    d_x, = to_dev(host.nonlocal_example_inputs(4, 32, 2, 9)[2])
    ptrs, strides, shape = gen.last_block5()
    assert shape == (2, 4, 32, 261) and strides[0] >= 257 and min(strides[1:]) >= 261 and all(p % 4 == 0 for p in ptrs)
    assert tuple(copies[1].shape) == tuple(copies[2].shape) == (2, 4, 32, 261) and copies[0].shape[3] >= 257
    in_place = runner.backward(gen, d_x)
    copied = runner.nonlocal_grad(copies[0][..., :257].contiguous(), copies[1], copies[2], d_x)
    torch.cuda.synchronize()
    assert flat_bytes(in_place) == flat_bytes(copied)
    assert [o.cpu().numpy().tobytes() for o in outs] == before                 # the generator's four outputs are untouched
    for k, c in zip(PROBES, copies):
        assert gen.probe(k).cpu().numpy().tobytes() == c.cpu().numpy().tobytes(), k
    # the chain differentiates the function the forward computed: res5 against nonlocal_forward on y3 = y3x5 - pad(res4)
    y3x, xin, out = (c.cpu().numpy() for c in copies)
    y3 = (y3x[..., :257] - xin[..., :257]).astype(f32)
    e = scaled_error(out, host.nonlocal_forward(w, y3, xin)["out"])
    print("non-local grad: the generator's res5 against nonlocal_forward on its own y3x5 - pad(res4) in float64: scaled error %.3g" % e)
    assert e <= 1e-5
    with pytest.raises(ValueError, match="last forward was"):
        runner.backward(gen, d_x[:1].contiguous())


def test_tail_decoder_and_nonlocal_chained(generated):
    """The device walk over the tail, the decoder and the non-local block (ColourTail.backward, ColourDecoder.backward and
    NonLocalGrad.backward) on one forward at (32, 256), against the three statements chained on the device's own activations."""
    from blindshadowremoval_amd import objective
    import clr_decoder_grad_cases as dec_cases
    import test_clr_tail_grad_gpu as tail_gpu
    gen, w, outs, copies = generated
    _, _, g_con_a, g_gs_a = host.example_inputs(32, 256, 2, 9)
    g_con, g_gs = to_dev(g_con_a, g_gs_a)
    walked = objective.device_walk(objective.device_runners(objective.STAGES[:3], w), gen, dict(gs=outs[0], grad_con=g_con, grad_gs=g_gs), keep=("tail",))
    t, n = walked["tail"], to_host(walked["nonlocal"])
    torch.cuda.synchronize()
    f1, f2, f = (gen.probe(k).cpu().numpy() for k in ("f1", "f2", "f"))
    y3x, xin, out = (c.cpu().numpy() for c in copies)
    st_t = host.tail_grad(w, outs[0].cpu().numpy(), f, g_con_a, g_gs_a, acts={"a1": t["a1"].cpu().numpy(), "a2": t["a2"].cpu().numpy()})
    st_d = host.decoder_grad(w, out, st_t["d_f"], acts={"f1": f1, "f2": f2, "f": f})
    st_n = host.nonlocal_grad(w, (y3x[..., :257] - xin[..., :257]).astype(f32), xin, st_d["d_x"], acts={"out": out})
    worst, at = cases.worst_scaled_diff(n, st_n)
    bound = tail_gpu.E2E_BOUND + dec_cases.E2E_BOUND + cases.E2E_BOUND
    print("colour tail, decoder and non-local block chained: worst scaled error %.3g at %s (bound %.3g)" % (worst, at, bound))
    assert worst <= bound, (worst, at)


def test_last_block5_is_refused_for_a_sixteen_bit_generator():
    from blindshadowremoval_amd import Generator
    gen = Generator(device=0, dtype="f16")
    gen.load_weights(cases.nl_weights())
    rng = np.random.default_rng(22)
    inputs, uv = to_dev(rng.uniform(0, 1, (1, 32, 256, 3)).astype(f32), rng.uniform(0, 1, (1, 32, 256, 3)).astype(f32))
    gen(inputs, uv)
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="BSR_DTYPE_F32 handles only"):
        gen.last_block5()


# ---- the command
def test_command_nonlocal_device_route_matches_the_host_route(tmp_path_factory, capsys):
    """--grad-total --tail --decoder --nonlocal on one item at 256 x 256: both routes print the same fields, the non-local block's 24
    norms after the decoder's, and each agrees within 1e-3 of its own magnitude, the ceiling of every end-to-end bound of the project
    (the routes feed the block d_x's that already differ by the chains' own end-to-end errors above it).  d phi/bias, a sum that cancels
    to rounding, is held on d theta/bias' scale.  Without --decoder the flag is refused."""
    import pairs_cases
    from blindshadowremoval_amd import objective
    from blindshadowremoval_amd.weights import init_vgg_weights, save_vgg_weights
    folder = pairs_cases.write_pairs(tmp_path_factory.mktemp("nonlocal_pairs"))
    vgg = str(tmp_path_factory.mktemp("nonlocal_vgg") / "vgg.npz")
    save_vgg_weights(vgg, init_vgg_weights(21))
    names = objective.nonlocal_grad_names()
    printed = []
    for extra in ([], ["--host"]):
        assert objective.main([folder, "--vgg", vgg, "--batch", "1", "--grad-total", "--tail", "--decoder", "--nonlocal"] + extra) == 0
        lines = capsys.readouterr().out.strip().split("\n")
        assert len(lines) == 2 and lines[0].startswith("1/1 ")
        fields = dict(f.rsplit(":", 1) for f in lines[0][4:].split(", "))
        assert tuple(fields) == (objective.ALL_NAMES + objective.TOTAL_GRAD_NAMES + tuple(objective.tail_grad_names())
                                 + tuple(objective.decoder_grad_names()) + tuple(names))
        printed.append({k: float(v) for k, v in fields.items()})
    dev_route, host_route = printed
    for k in names:
        scale = host_route[k.replace("phi/bias", "theta/bias")]
        d = abs(dev_route[k] - host_route[k])
        print("objective command --nonlocal %s: device %.9g host %.9g, difference over scale %.3g" % (k, dev_route[k], host_route[k], d / scale))
        assert scale > 0 and d <= 1e-3 * scale, k
    with pytest.raises(SystemExit):
        objective.main([folder, "--vgg", vgg, "--grad-total", "--tail", "--nonlocal"])
    capsys.readouterr()
