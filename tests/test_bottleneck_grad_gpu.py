"""bsr_bottleneck_grad (csrc/bottleneck_grad_kernels.h) against the host statement blindshadowremoval_amd/generator_grad.py:
bottleneck_grad.

Stage by stage: each of the chain's launches, fed the DEVICE's own inputs, against the float64 statement of that launch alone within
max|got - ref| / max|ref| <= 1e-5, the project's fp32-class stage budget.  End to end: the thirteen outputs against bottleneck_grad(acts =
the device's own a1, a2), each on the scale of its own largest reference magnitude, within cases.E2E_BOUND = 4 x the largest figure
measured on the MI355X over these sizes.

Grids (h, w, B): (4, 32, 1) one tile row, every pixel's halo meets a border or the tile edge; (8, 32, 2) tile seams and the seam between
items; (12, 32, 3) an odd tile count; (4, 64, 1) wide; (32, 32, 1) the workload's grid."""
import ctypes

import numpy as np
import pytest

from blindshadowremoval_amd import generator_grad as host
from blindshadowremoval_amd import pack

import bottleneck_grad_cases as cases

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
f32 = np.float32
ST = cases.ST
SIZES = cases.GPU_SIZES
OUT_KEYS = ("", "d_xin")


@pytest.fixture(scope="module")
def runner():
    from blindshadowremoval_amd import BottleneckGrad
    r = BottleneckGrad(0)
    r.load_weights(cases.bn_weights())
    return r


def to_dev(*arrays):
    dev = torch.device("cuda", 0)
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def to_host(res):
    return {k: v.cpu().numpy() for k, v in res.items()}


def device_run(runner, w, xin, d_y3, d_skip, acts=None):
    """The `run` of cases.check_*: the chain forms its own a1 and a2, so `acts` is never given."""
    assert acts is None
    runner.load_weights(w)
    res = runner.bottleneck_grad(*to_dev(xin, d_y3, d_skip), keep=True)
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
    for h, w, B in SIZES:
        wt, xin, d_y3, d_skip = cases.case(h, w, B, 1)
        res = runner.bottleneck_grad(*to_dev(xin, d_y3, d_skip), keep=True)
        torch.cuda.synchronize()
        out[(h, w, B)] = (wt, (xin, d_y3, d_skip), to_host(res), to_host(runner.maps(B, h, w)))
    return out


@pytest.mark.parametrize("check", cases.CONSTRUCTED, ids=lambda c: c.__name__)
def test_constructed_case(runner, check):
    check(lambda *a: device_run(runner, *a))
    runner.load_weights(cases.bn_weights())


@pytest.mark.parametrize("h,w,B", SIZES)
def test_stage_by_stage(device_results, h, w, B):
    wt, (xin, d_y3, d_skip), res, maps = device_results[(h, w, B)]

    def hold(what, got, want):
        got, want = np.asarray(got), np.asarray(want)
        assert got.shape == want.shape, what
        e = scaled_error(got, want)
        print("bottleneck grad h=%d w=%d B=%d %s fed the device's input: scaled error %.3g" % (h, w, B, what, e))
        assert e <= cases.STAGE_BUDGET, (what, e)

    m = {k: v.astype(np.float64) for k, v in maps.items()}
    K1, K2, K3 = (np.asarray(wt[ST + "conv%d/kernel" % j], np.float64) for j in (1, 2, 3))
    v = {j: host.bottleneck_bn_vectors(wt, j) for j in (1, 2, 3)}          # bias, inv, mean, rstd, gamma, beta
    lrelu = lambda z: np.where(z >= 0, z, 0.3 * z)                         # noqa: E731

    def bn(c, j):
        return (c - v[j][2]) * v[j][3] * v[j][4] + v[j][5]

    # launch 1: the padded copies, exact
    assert maps["xp"].tobytes() == xin.tobytes() and maps["dyp"].tobytes() == d_y3.tobytes()
    # launches 2, 3: the activations from the device's inputs
    hold("launch 2 a1", maps["a1"], lrelu(bn(m["xp"] @ K1[0, 0] + v[1][0], 1)))
    hold("launch 3 a2", maps["a2"], lrelu(bn(host.conv3x3_same(m["a1"], K2) + v[2][0], 2)))
    # launches 4, 5: the two masked data gradients from the device's maps
    hold("launch 4 gz2", maps["gz2"], host.leaky_grad((m["dyp"] * v[3][1]) @ K3[0, 0].T, m["a2"]))
    hold("launch 5 gz1", maps["gz1"], host.leaky_grad(host.conv3x3_same_dgrad(m["gz2"] * v[2][1], K2), m["a1"]))
    # launches 6, 7, 8, 11: the kernels from the device's maps
    ax = ([0, 1, 2], [0, 1, 2])
    hold("launches 6, 11 Wg2", maps["Wg2"], host.conv3x3_same_wgrad(m["a1"], m["gz2"]))
    hold("launches 7, 11 Wg3", maps["Wg3"], np.tensordot(m["a2"], m["dyp"], axes=ax))
    hold("launches 8, 11 Wg1", maps["Wg1"], np.tensordot(m["xp"], m["gz1"], axes=ax))
    for j, shape in ((1, K1.shape), (2, K2.shape), (3, K3.shape)):
        hold("launch 11 d K%d" % j, res[ST + "conv%d/kernel" % j], m["Wg%d" % j].reshape(shape) * v[j][1])
    # launch 9: d_xin from the device's gz1
    hold("launch 9 d_xin", res["d_xin"], d_skip.astype(np.float64) + (m["gz1"] * v[1][1]) @ K1[0, 0].T)
    # launches 10, 12: the sums and the channel triples from the device's maps
    for j, gz, K in ((1, m["gz1"], K1), (2, m["gz2"], K2), (3, m["dyp"], K3)):
        hold("launch 12 S%d" % j, maps["S%d" % j], gz.sum(axis=(0, 1, 2)))
        S = m["S%d" % j]
        KW = (K * m["Wg%d" % j].reshape(K.shape)).sum(axis=(0, 1, 2))
        hold("launch 12 d beta%d" % j, res[ST + "bnorm%d/beta" % j], S)
        hold("launch 12 d bias%d" % j, res[ST + "conv%d/bias" % j], v[j][1] * S)
        hold("launch 12 d gamma%d" % j, res[ST + "bnorm%d/gamma" % j], ((KW + v[j][0] * S) - v[j][2] * S) * v[j][3])


@pytest.mark.parametrize("h,w,B", SIZES)
def test_end_to_end(device_results, h, w, B):
    wt, (xin, d_y3, d_skip), res, maps = device_results[(h, w, B)]
    for k in ("a1", "a2", "gz2", "gz1"):
        assert res[k].tobytes() == maps[k].tobytes(), k                    # what keep=True returns is what the scratch holds
    st = host.bottleneck_grad(wt, xin, d_y3, d_skip, acts={"a1": res["a1"], "a2": res["a2"]})
    for name in cases.OUTPUTS:
        print("bottleneck grad h=%d w=%d B=%d %s against the statement on the device's a1, a2: scaled error %.3g (bound %.3g)"
              % (h, w, B, name, cases.worst_scaled_diff(res, st, (name,))[0], cases.E2E_BOUND))
    d, at = cases.worst_scaled_diff(res, st)
    print("bottleneck grad h=%d w=%d B=%d: worst %.3g at %s" % (h, w, B, d, at))
    assert d <= cases.E2E_BOUND, (d, at)
    # the device's activations are the statement's own within the stage budget, and both signs are present
    fw = host.bottleneck_forward(wt, xin)
    for k in ("a1", "a2"):
        assert scaled_error(res[k], fw[k]) <= cases.STAGE_BUDGET, k
        assert (res[k] > 0).any() and (res[k] < 0).any(), k


def test_block_3_weights(runner):
    """Block 3's variables through the same chain at (8, 32, 2), against the statement of block 3."""
    h, w, B = 8, 32, 2
    wt, xin, d_y3, d_skip = cases.case(h, w, B, 2)
    runner.load_weights(wt, block=3)
    res = to_host(runner.bottleneck_grad(*to_dev(xin, d_y3, d_skip), keep=True))
    runner.load_weights(cases.bn_weights())
    st = host.bottleneck_grad(wt, xin, d_y3, d_skip, block=3, acts={"a1": res["a1"], "a2": res["a2"]})
    as5 = {n5: st[n5.replace("res_stack/5/", "res_stack/3/")] for n5 in cases.NAMES}
    as5["d_xin"] = st["d_xin"]
    d, at = cases.worst_scaled_diff(res, as5)
    print("bottleneck grad, block 3's weights: worst %.3g at %s (bound %.3g)" % (d, at, cases.E2E_BOUND))
    assert d <= cases.E2E_BOUND, (d, at)
    five = host.bottleneck_grad(wt, xin, d_y3, d_skip)
    assert cases.worst_scaled_diff(res, five)[0] > 1e-2                     # and not block 5's


def flat_bytes(res):
    return [res[k].cpu().numpy().tobytes() for k in OUT_KEYS]


def test_a_repeated_call_and_two_sizes_on_one_scratch(runner, device_results):
    w, arrays3, _, _ = device_results[(12, 32, 3)]
    _, arrays1, _, _ = device_results[(4, 32, 1)]
    t3, t1 = to_dev(*arrays3), to_dev(*arrays1)
    first3 = flat_bytes(runner.bottleneck_grad(*t3))
    first1 = flat_bytes(runner.bottleneck_grad(*t1))            # B = 3 then B = 1 on the larger call's scratch
    assert flat_bytes(runner.bottleneck_grad(*t3)) == first3
    assert flat_bytes(runner.bottleneck_grad(*t1)) == first1
    assert flat_bytes(runner.bottleneck_grad(*t1, keep=True)) == first1     # keeping the maps changes no output
    for t, a in zip(t1, arrays1):
        assert t.cpu().numpy().tobytes() == a.tobytes()                     # no input is ever written
    fresh = type(runner)(0)
    fresh.load_weights(w)
    assert flat_bytes(fresh.bottleneck_grad(*t1)) == first1      # a scratch of its own size gives the same bytes


def test_no_d_skip_is_a_zero_d_skip(runner, device_results):
    _, (xin, d_y3, d_skip), _, _ = device_results[(8, 32, 2)]
    x, g = to_dev(xin, d_y3)
    none = runner.bottleneck_grad(x, g)
    zero = runner.bottleneck_grad(x, g, torch.zeros_like(x))
    assert flat_bytes(none) == flat_bytes(zero)
    assert flat_bytes(runner.bottleneck_grad(x, g, None, keep=True)) == flat_bytes(none)


def test_debug_stops(runner, device_results):
    from blindshadowremoval_amd.bottleneck_grad_gpu import LAUNCHES
    _, arrays, res, maps = device_results[(8, 32, 2)]
    t = to_dev(*arrays)
    assert len(LAUNCHES) == 12
    runner.stages(*t, 0)
    first = {"xp": 1, "dyp": 1, "a1": 2, "a2": 3, "gz2": 4, "gz1": 5, "Wg1": 11, "Wg2": 11, "Wg3": 11, "S1": 12, "S2": 12, "S3": 12}
    kernels = tuple(n for n in cases.NAMES if n.endswith("/kernel"))
    for stop in range(13):
        got = to_host(runner.stages(*t, stop))
        assert (got["d_xin"].tobytes() == res["d_xin"].tobytes()) if stop >= 9 else not got["d_xin"].any(), stop
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
    _, arrays, _, _ = device_results[(4, 32, 1)]
    t = to_dev(*arrays)
    eager = flat_bytes(runner.bottleneck_grad(*t))
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        runner.bottleneck_grad(*t)
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=side):
            res = runner.bottleneck_grad(*t)
    torch.cuda.current_stream().wait_stream(side)
    for k in OUT_KEYS:
        res[k].zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert flat_bytes(res) == eager


def test_argument_errors_raise_before_any_launch(runner, device_results):
    from blindshadowremoval_amd import BottleneckGrad, _lib
    from blindshadowremoval_amd.bottleneck_grad_gpu import NO_WEIGHTS_TEXT, SIZE_TEXT
    dev = torch.device("cuda", 0)
    _, arrays, _, _ = device_results[(4, 32, 1)]
    xin, d_y3, d_skip = to_dev(*arrays)
    with pytest.raises(ValueError) as e:
        BottleneckGrad(0).bottleneck_grad(xin, d_y3, d_skip)
    assert str(e.value) == NO_WEIGHTS_TEXT
    with pytest.raises(TypeError) as e:
        runner.bottleneck_grad(xin.cpu(), d_y3, d_skip)
    assert str(e.value) == "xin must be a float32 tensor [B,h,w,261] on %s" % dev
    with pytest.raises(ValueError) as e:
        runner.bottleneck_grad(xin, d_y3, d_skip[..., :260].contiguous())
    assert str(e.value) == "d_skip must be [1,4,32,261] for this d_y3, got (1, 4, 32, 260)"
    with pytest.raises(ValueError) as e:
        runner.bottleneck_grad(*[torch.zeros((1, 6, 32, c), device=dev) for c in (261, 257, 261)])
    assert str(e.value) == SIZE_TEXT % (1, 6, 32)
    with pytest.raises(ValueError) as e:
        runner.load_weights(cases.bn_weights(variant="tsm"))
    assert str(e.value) == pack.BOTTLENECK_TSM_TEXT
    # the entry point itself: nothing is launched, the outputs keep their bytes
    lib = _lib.load()
    d_xin = torch.full((1, 4, 32, 261), 7.0, device=dev)
    flat = torch.full((int(lib.bsr_bottleneck_grad_floats()),), 7.0, device=dev)
    scratch = runner.scratch3(1, 4, 32)
    p = lambda t: ctypes.c_void_p(t.data_ptr())                                      # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(h=4, w=32, xin_cs=261, nbytes=runner._blob.numel(), scr=scratch):
        return lib.bsr_bottleneck_grad(0, p(runner._blob), nbytes, p(xin), xin_cs, p(d_y3), p(d_skip), 1, h, w, p(d_xin), p(flat),
                                       ctypes.c_void_p(scr), stream), lib.bsr_last_error().decode()

    size = "B must be positive, h a multiple of 4 and w a multiple of 32 (the generator's rule at 1/8 resolution), at most 2^21 pixels in all"
    for kw, text in ((dict(h=6), size), (dict(w=16), size), (dict(xin_cs=260), "xin_cs must be at least 261"),
                     (dict(nbytes=16), "blob_bytes must be bsr_bottleneck_grad_blob_bytes() (pack.pack_bottleneck_grad; the GSC width 261 only, not TSM's 877)"),
                     (dict(scr=scratch + 8), "scratch must be 256-byte aligned")):
        assert call(**kw) == (1, "bsr_bottleneck_grad: " + text), kw
    torch.cuda.synchronize()
    for t in (d_xin, flat):
        assert bool((t == 7.0).all())


# ---- the generator's own tensors, in place
PROBES = ("y3x5", "res4", "res5")


@pytest.fixture(scope="module")
def generated():
    """A seeded generator's forward at (32, 256), B = 2, its outputs and copies of the block's three tensors."""
    from blindshadowremoval_amd import Generator
    w = cases.bn_weights()
    gen = Generator(device=0)
    gen.load_weights(w)
    with pytest.raises(RuntimeError, match="no forward has run"):
        gen.last_block5_input()
    rng = np.random.default_rng(21)
    inputs, uv = to_dev(rng.uniform(0, 1, (2, 32, 256, 3)).astype(f32), rng.uniform(0, 1, (2, 32, 256, 3)).astype(f32))
    outs = gen(inputs, uv)
    torch.cuda.synchronize()
    return gen, w, outs, [gen.probe(k).clone() for k in PROBES]


def test_backward_reads_the_generators_input_in_place(runner, generated):
    gen, w, outs, copies = generated
    runner.load_weights(w)
    before = [o.cpu().numpy().tobytes() for o in outs]
    _, d_y3_a, d_skip_a = host.bottleneck_example_inputs(4, 32, 2, 9)
    d_y3, d_skip = to_dev(d_y3_a, d_skip_a)
    ptr, stride, shape = gen.last_block5_input()
    ptrs, strides, shape5 = gen.last_block5()
    assert shape == shape5 == (2, 4, 32, 261) and ptr == ptrs[1] and stride == strides[1] >= 261 and ptr % 4 == 0
    for skip in (d_skip, None):
        in_place = runner.backward(gen, d_y3, skip)
        copied = runner.bottleneck_grad(copies[1], d_y3, skip)
        torch.cuda.synchronize()
        assert flat_bytes(in_place) == flat_bytes(copied)
    kept = runner.backward(gen, d_y3, d_skip, keep=True)
    assert flat_bytes(kept) == flat_bytes(runner.backward(gen, d_y3, d_skip)) and all(k in kept for k in ("gz2", "gz1", "a1", "a2"))
    assert [o.cpu().numpy().tobytes() for o in outs] == before                 # the generator's four outputs are untouched
    for k, c in zip(PROBES, copies):
        assert gen.probe(k).cpu().numpy().tobytes() == c.cpu().numpy().tobytes(), k
    # the chain differentiates the function the forward computed: y3 = y3x5 - pad(res4) against bottleneck_forward on res4
    y3x, xin, _ = (c.cpu().numpy() for c in copies)
    y3 = (y3x[..., :257] - xin[..., :257]).astype(f32)
    e = scaled_error(y3, host.bottleneck_forward(w, xin)["y3"])
    print("bottleneck grad: the generator's y3x5 - pad(res4) against bottleneck_forward on its own res4 in float64: scaled error %.3g" % e)
    assert e <= 1e-5
    with pytest.raises(ValueError, match="last forward was"):
        runner.backward(gen, d_y3[:1].contiguous())


def test_backward_is_refused_before_a_forward_and_for_a_sixteen_bit_generator(runner):
    from blindshadowremoval_amd import Generator
    d_y3, = to_dev(host.bottleneck_example_inputs(4, 32, 1, 9)[1])
    gen = Generator(device=0)
    gen.load_weights(cases.bn_weights())
    with pytest.raises(RuntimeError, match="no forward has run"):
        runner.backward(gen, d_y3)
    gen.close()
    gen = Generator(device=0, dtype="f16")
    gen.load_weights(cases.bn_weights())
    rng = np.random.default_rng(22)
    inputs, uv = to_dev(rng.uniform(0, 1, (1, 32, 256, 3)).astype(f32), rng.uniform(0, 1, (1, 32, 256, 3)).astype(f32))
    gen(inputs, uv)
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="BSR_DTYPE_F32 handles only"):
        runner.backward(gen, d_y3)
    gen.close()


def test_tail_decoder_nonlocal_and_bottleneck_chained(generated):
    """The device walk over the colour branch (ColourTail.backward, ColourDecoder.backward, NonLocalGrad.backward and
    BottleneckGrad.backward) on one forward at (32, 256), against the four statements chained on the device's own activations."""
    from blindshadowremoval_amd import objective
    import clr_decoder_grad_cases as dec_cases
    import nonlocal_grad_cases as nl_cases
    import test_clr_tail_grad_gpu as tail_gpu
    gen, w, outs, copies = generated
    _, _, g_con_a, g_gs_a = host.example_inputs(32, 256, 2, 9)
    g_con, g_gs = to_dev(g_con_a, g_gs_a)
    walked = objective.device_walk(objective.device_runners(objective.STAGES, w), gen, dict(gs=outs[0], grad_con=g_con, grad_gs=g_gs),
                                   keep=("tail", "bottleneck"))
    t, b = walked["tail"], to_host(walked["bottleneck"])
    torch.cuda.synchronize()
    f1, f2, f = (gen.probe(k).cpu().numpy() for k in ("f1", "f2", "f"))
    y3x, xin, out = (c.cpu().numpy() for c in copies)
    st_t = host.tail_grad(w, outs[0].cpu().numpy(), f, g_con_a, g_gs_a, acts={"a1": t["a1"].cpu().numpy(), "a2": t["a2"].cpu().numpy()})
    st_d = host.decoder_grad(w, out, st_t["d_f"], acts={"f1": f1, "f2": f2, "f": f})
    st_n = host.nonlocal_grad(w, (y3x[..., :257] - xin[..., :257]).astype(f32), xin, st_d["d_x"], acts={"out": out})
    st_b = host.bottleneck_grad(w, xin, st_n["d_y3"], st_n["d_skip"], acts={"a1": b["a1"], "a2": b["a2"]})
    worst, at = cases.worst_scaled_diff(b, st_b)
    bound = tail_gpu.E2E_BOUND + dec_cases.E2E_BOUND + nl_cases.E2E_BOUND + cases.E2E_BOUND
    print("colour tail, decoder, non-local block and bottleneck chained: worst scaled error %.3g at %s (bound %.3g)" % (worst, at, bound))
    assert worst <= bound, (worst, at)


# ---- the command
def test_command_bottleneck_device_route_matches_the_host_route(tmp_path_factory, capsys):
    """--grad-total --tail --decoder --nonlocal --bottleneck on one item at 256 x 256: both routes print the same fields, the bottleneck's
    26 norms after the non-local block's, and each agrees within 1e-3 of its own magnitude, the ceiling of every end-to-end bound of the
    project (the routes feed the stage gradients that already differ by the chains' own end-to-end errors above it).  Without --nonlocal
    the flag is refused, and without the flag the line is the one --nonlocal prints."""
    import pairs_cases
    from blindshadowremoval_amd import objective
    from blindshadowremoval_amd.weights import init_vgg_weights, save_vgg_weights
    folder = pairs_cases.write_pairs(tmp_path_factory.mktemp("bottleneck_pairs"))
    vgg = str(tmp_path_factory.mktemp("bottleneck_vgg") / "vgg.npz")
    save_vgg_weights(vgg, init_vgg_weights(21))
    names = objective.bottleneck_grad_names()
    above = (objective.ALL_NAMES + objective.TOTAL_GRAD_NAMES + tuple(objective.tail_grad_names()) + tuple(objective.decoder_grad_names())
             + tuple(objective.nonlocal_grad_names()))
    printed = []
    for extra in ([], ["--host"]):
        assert objective.main([folder, "--vgg", vgg, "--batch", "1", "--grad-total", "--tail", "--decoder", "--nonlocal", "--bottleneck"] + extra) == 0
        lines = capsys.readouterr().out.strip().split("\n")
        assert len(lines) == 2 and lines[0].startswith("1/1 ")
        fields = dict(f.rsplit(":", 1) for f in lines[0][4:].split(", "))
        assert tuple(fields) == above + tuple(names)
        printed.append((lines[0], {k: float(v) for k, v in fields.items()}))
    (dev_line, dev_route), (_, host_route) = printed
    for k in names:
        scale = host_route[k]
        d = abs(dev_route[k] - host_route[k])
        print("objective command --bottleneck %s: device %.9g host %.9g, difference over scale %.3g" % (k, dev_route[k], host_route[k], d / scale))
        assert scale > 0 and d <= 1e-3 * scale, k
    capsys.readouterr()
    assert objective.main([folder, "--vgg", vgg, "--batch", "1", "--grad-total", "--tail", "--decoder", "--nonlocal"]) == 0
    without = capsys.readouterr().out.strip().split("\n")[0]
    assert dev_line.startswith(without + ", ") and len(dev_line[len(without) + 2:].split(", ")) == 26
    with pytest.raises(SystemExit):
        objective.main([folder, "--vgg", vgg, "--grad-total", "--tail", "--decoder", "--bottleneck"])
    capsys.readouterr()
