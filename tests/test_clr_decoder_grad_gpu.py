"""bsr_clr_decoder_grad (csrc/clr_up_grad_kernels.h) against the host statement blindshadowremoval_amd/generator_grad.py: decoder_grad.

Stage by stage: each of the chain's launches, fed the DEVICE's own inputs, against the float64 statement of that launch alone within
max|got - ref| / max|ref| <= 1e-5, the project's fp32-class stage budget.  End to end: the thirteen outputs against decoder_grad(acts =
the device's own f1, f2, f), each on the scale of its own largest reference magnitude, within cases.E2E_BOUND = 4 x the largest figure
measured on the MI355X over these shapes (tools/clr_decoder_bench.py --parity, profiles/clr_decoder_grad_bench.json).

Image sizes (H, W, B): (32, 256, 1) is the smallest the generator takes (clr_up1's grid is one dgrad tile and two wgrad tiles);
(64, 256, 2) has tile seams both ways at every level and 8, 32, 128 tiles for P = 3, 11, 43 partials, none of which divides its
count; (96, 256, 3) has tile counts that are multiples of 3 (P = ceil(tiles / 3) divides those, so it is not the odd shape); (32, 512, 1)
is wide."""
import ctypes

import numpy as np
import pytest

from blindshadowremoval_amd import generator_grad as host

import clr_decoder_grad_cases as cases

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
f32 = np.float32
SIZES = ((32, 256, 1), (64, 256, 2), (96, 256, 3), (32, 512, 1))
ACTS = ("x", "f1", "f2", "f")


@pytest.fixture(scope="module")
def runner():
    from blindshadowremoval_amd import ColourDecoder
    r = ColourDecoder(0)
    r.load_weights(cases.decoder_weights())
    return r


def to_dev(*arrays):
    dev = torch.device("cuda", 0)
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def to_host(res):
    return {k: v.cpu().numpy() for k, v in res.items()}


def forward32(w, x):
    """x, f1, f2, f float32: decoder_forward in float32."""
    return (x,) + tuple(np.ascontiguousarray(a, f32) for a in host.decoder_forward(w, x, f32))


def device_run(runner, w, x, d_f, acts=None):
    """The `run` of cases.check_*: the runner's own forward is decoder_forward in float32."""
    runner.load_weights(w)
    fs = forward32(w, x)[1:] if acts is None else tuple(np.asarray(acts[k], f32) for k in ("f1", "f2", "f"))
    res = runner.decoder_grad(*to_dev(x, *fs, d_f), keep=True)
    torch.cuda.synchronize()
    out = to_host(res)
    out.update(zip(("f1", "f2", "f"), fs))
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
        w, x, d_f = cases.case(H // 8, W // 8, B, 1)
        arrays = forward32(w, x) + (d_f,)
        res = runner.decoder_grad(*to_dev(*arrays), keep=True)
        torch.cuda.synchronize()
        out[(H, W, B)] = (w, arrays, to_host(res), to_host(runner.maps(B, H, W)))
    return out


@pytest.mark.parametrize("check", cases.CONSTRUCTED, ids=lambda c: c.__name__)
def test_constructed_case(runner, check):
    check(lambda *a: device_run(runner, *a))
    runner.load_weights(cases.decoder_weights())


@pytest.mark.parametrize("H,W,B", SIZES)
def test_stage_by_stage(device_results, H, W, B):
    w, (x, f1, f2, f, d_f), res, maps = device_results[(H, W, B)]

    def hold(what, got, want):
        got, want = np.asarray(got), np.asarray(want)
        assert got.shape == want.shape, what
        e = scaled_error(got, want)
        print("colour decoder grad H=%d W=%d B=%d %s fed the device's input: scaled error %.3g" % (H, W, B, what, e))
        assert e <= cases.STAGE_BUDGET, (what, e)

    # launch 1: the entry mask, exact
    assert maps["gz3"].tobytes() == host.leaky_grad(d_f, f).astype(f32).tobytes()
    below = {3: (f2, f2), 2: (f1, f1), 1: (x, None)}                  # layer -> (its input, the activation whose sign masks its dx)
    for n, i in ((2, 3), (4, 2), (6, 1)):
        stem = "clr_up%d" % i
        a_in, mask = below[i]
        gz = maps["gz%d" % i].astype(np.float64)
        K = np.asarray(w[stem + "/conv/kernel"], np.float64)
        bias, inv, mean, rstd, _ = host.bn_vectors(w, stem)
        # the kernel gradient before the BN factor and S, from the device's gz
        Wg, S = maps["Wg%d" % i], maps["S%d" % i]
        hold("launch %d Wg%d" % (n, i), Wg, host.convt3x3_same_wgrad(a_in, gz))
        hold("launch %d S%d" % (n, i), S, gz.sum(axis=(0, 1, 2)))
        # the data gradient from the device's gz
        dx = host.convt3x3_same_dgrad(gz * inv, K)
        if mask is None:
            hold("launch %d d_x" % (n + 1), res["d_x"], dx)
        else:
            hold("launch %d gz%d" % (n + 1, i - 1), maps["gz%d" % (i - 1)], host.leaky_grad(dx, mask))
        # launches 8 and 9 from the device's Wg and S
        hold("launch 8 d K%d" % i, res[stem + "/conv/kernel"], Wg * inv[:, None])
        hold("launch 9 d beta%d" % i, res[stem + "/bnorm/beta"], S)
        hold("launch 9 d bias%d" % i, res[stem + "/conv/bias"], inv * S)
        hold("launch 9 d gamma%d" % i, res[stem + "/bnorm/gamma"], (((K * Wg).sum(axis=(0, 1, 3)) + bias * S) - mean * S) * rstd)


@pytest.mark.parametrize("H,W,B", SIZES)
def test_end_to_end(device_results, H, W, B):
    w, (x, f1, f2, f, d_f), res, maps = device_results[(H, W, B)]
    st = host.decoder_grad(w, x, d_f, acts={"f1": f1, "f2": f2, "f": f})
    for name in cases.OUTPUTS:
        print("colour decoder grad H=%d W=%d B=%d %s against the statement on the device's activations: scaled error %.3g (bound %.3g)"
              % (H, W, B, name, scaled_error(res[name], st[name]), cases.E2E_BOUND))
    d, at = cases.worst_scaled_diff(res, st)
    print("colour decoder grad H=%d W=%d B=%d: worst %.3g at %s" % (H, W, B, d, at))
    assert d <= cases.E2E_BOUND, (d, at)


def test_some_shape_has_a_tile_count_its_partials_do_not_divide():
    from blindshadowremoval_amd import _lib
    lib = _lib.load()
    odd = []
    for H, W, B in SIZES:
        for layer in (1, 2, 3):
            P = int(lib.bsr_clr_decoder_grad_partials(B, H, W, layer))
            tiles = B * ((H >> (4 - layer)) // 4) * ((W >> (4 - layer)) // 16)
            assert 1 <= P <= tiles
            if P > 1 and tiles % P:
                odd.append((H, W, B, layer, tiles, P))
    print("colour decoder grad: (H, W, B, layer, tiles, P) with tiles % P != 0:", odd)
    assert {o[3] for o in odd if o[:3] == (64, 256, 2)} == {1, 2, 3}


def flat_bytes(res):
    return [res[k].cpu().numpy().tobytes() for k in ("", "d_x")]


def test_a_repeated_call_and_two_sizes_on_one_scratch(runner, device_results):
    w, arrays3, _, _ = device_results[(96, 256, 3)]
    _, arrays1, _, _ = device_results[(32, 256, 1)]
    t3, t1 = to_dev(*arrays3), to_dev(*arrays1)
    first3 = flat_bytes(runner.decoder_grad(*t3))
    first1 = flat_bytes(runner.decoder_grad(*t1))             # B = 3 then B = 1 on the larger call's scratch
    assert flat_bytes(runner.decoder_grad(*t3)) == first3
    assert flat_bytes(runner.decoder_grad(*t1)) == first1
    assert flat_bytes(runner.decoder_grad(*t1, keep=True)) == first1      # keeping the maps changes no output
    assert t1[4].cpu().numpy().tobytes() == arrays1[4].tobytes()         # d_f is never written
    fresh = type(runner)(0)
    fresh.load_weights(w)
    assert flat_bytes(fresh.decoder_grad(*t1)) == first1       # a scratch of its own size gives the same bytes


def test_debug_stops(runner, device_results):
    from blindshadowremoval_amd.clr_decoder_gpu import LAUNCHES
    _, arrays, res, _ = device_results[(64, 256, 2)]
    t = to_dev(*arrays)
    assert len(LAUNCHES) == 9
    for stop in range(10):
        got = to_host(runner.stages(*t, stop))
        assert (got["d_x"].tobytes() == res["d_x"].tobytes()) if stop >= 7 else not got["d_x"].any(), stop
        views = type(runner).split_grads(torch.from_numpy(got[""]))
        for name in cases.NAMES:
            v = views[name].numpy()
            done = stop >= 8 if name.endswith("/kernel") else stop >= 9
            assert (v.tobytes() == res[name].tobytes()) if done else not v.any(), (stop, name)
        for name, first in (("gz3", 1), ("gz2", 3), ("gz1", 5)):
            if stop >= first:
                assert got[name].tobytes() == res[name].tobytes(), (stop, name)
    with pytest.raises(ValueError, match="stop_after"):
        runner.stages(*t, 10)


def test_the_chain_is_captured_into_a_graph_and_replays_the_same_bytes(runner, device_results):
    """Stream capture refuses a host synchronisation and work on another stream that is not joined: a call that is captured, replayed
    and gives the eager call's bytes has neither.  The chain is a line of launches: the captured graph has no branches."""
    _, arrays, _, _ = device_results[(32, 256, 1)]
    t = to_dev(*arrays)
    eager = flat_bytes(runner.decoder_grad(*t))
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        runner.decoder_grad(*t)
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=side):
            res = runner.decoder_grad(*t)
    torch.cuda.current_stream().wait_stream(side)
    for k in ("", "d_x"):
        res[k].zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert flat_bytes(res) == eager


def test_argument_errors_raise_before_any_launch(runner, device_results):
    from blindshadowremoval_amd import ColourDecoder, _lib
    from blindshadowremoval_amd.clr_decoder_gpu import NO_WEIGHTS_TEXT, SIZE_TEXT
    dev = torch.device("cuda", 0)
    _, arrays, _, _ = device_results[(32, 256, 1)]
    x, f1, f2, f, d_f = to_dev(*arrays)
    with pytest.raises(ValueError) as e:
        ColourDecoder(0).decoder_grad(x, f1, f2, f, d_f)
    assert str(e.value) == NO_WEIGHTS_TEXT
    with pytest.raises(TypeError) as e:
        runner.decoder_grad(x, f1.cpu(), f2, f, d_f)
    assert str(e.value) == "f1 must be a float32 tensor [B,.,.,128] on %s" % dev
    with pytest.raises(ValueError) as e:
        runner.decoder_grad(x[..., :260].contiguous(), f1, f2, f, d_f)
    assert str(e.value) == "x must be [1,4,32,261] for this d_f, got (1, 4, 32, 260)"
    with pytest.raises(ValueError) as e:
        runner.decoder_grad(*[torch.zeros((1, 48 // d, 256 // d, c), device=dev) for d, c in ((8, 261), (4, 128), (2, 96), (1, 64), (1, 64))])
    assert str(e.value) == SIZE_TEXT % (1, 48, 256)
    # the entry point itself: nothing is launched, the outputs keep their bytes
    lib = _lib.load()
    d_x = torch.full((1, 4, 32, 261), 7.0, device=dev)
    flat = torch.full((int(lib.bsr_clr_decoder_grad_floats()),), 7.0, device=dev)
    scratch = runner.scratch4(1, 32, 256, False)
    p = lambda t: ctypes.c_void_p(t.data_ptr())                                      # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(h=32, w=256, x_cs=261, f1_cs=128, nbytes=runner._blob.numel(), scr=scratch):
        return lib.bsr_clr_decoder_grad(0, p(runner._blob), nbytes, p(x), x_cs, p(f1), f1_cs, p(f2), 96, p(f), 64, p(d_f), 1, h, w, p(d_x), p(flat), 0,
                                        ctypes.c_void_p(scr), stream), lib.bsr_last_error().decode()

    size = "B must be positive, H a multiple of 32 and W a multiple of 256 (the generator's rule), at most 2^26 pixels in all"
    for kw, text in ((dict(h=48), size), (dict(w=128), size), (dict(x_cs=260), "x_cs must be at least 261"),
                     (dict(f1_cs=130), "f1_cs, f2_cs, f_cs must be multiples of 4 and at least 128, 96, 64"),
                     (dict(nbytes=16), "blob_bytes must be bsr_clr_decoder_grad_blob_bytes() (pack.pack_clr_decoder_grad; the GSC width 261 only, not TSM's 877)"),
                     (dict(scr=scratch + 8), "scratch must be 256-byte aligned")):
        assert call(**kw) == (1, "bsr_clr_decoder_grad: " + text), kw
    torch.cuda.synchronize()
    for t in (d_x, flat):
        assert bool((t == 7.0).all())


# ---- the generator's own tensors, in place
@pytest.fixture(scope="module")
def generated():
    """A seeded generator's forward at (32, 256), B = 2, its outputs and copies of the decoder's four tensors."""
    from blindshadowremoval_amd import Generator
    w = cases.decoder_weights()
    gen = Generator(device=0)
    gen.load_weights(w)
    with pytest.raises(RuntimeError, match="no forward has run"):
        gen.last_decoder()
    rng = np.random.default_rng(21)
    inputs, uv = to_dev(rng.uniform(0, 1, (2, 32, 256, 3)).astype(f32), rng.uniform(0, 1, (2, 32, 256, 3)).astype(f32))
    outs = gen(inputs, uv)
    torch.cuda.synchronize()
    return gen, w, outs, [gen.probe(k).clone() for k in ("res5", "f1", "f2", "f")]


def test_backward_reads_the_generators_tensors_in_place(runner, generated):
    gen, w, outs, copies = generated
    runner.load_weights(w)
    before = [o.cpu().numpy().tobytes() for o in outs]
    d_f, = to_dev(host.decoder_example_inputs(4, 32, 2, 9)[1])
    ptrs, x_cs, shape = gen.last_decoder()
    assert shape == (2, 32, 256, 64) and x_cs >= 261 and all(p % 16 == 0 for p in ptrs)
    assert tuple(copies[0].shape) == (2, 4, 32, 261)
    in_place = runner.backward(gen, d_f)
    copied = runner.decoder_grad(*copies, d_f)
    torch.cuda.synchronize()
    assert flat_bytes(in_place) == flat_bytes(copied)
    assert [o.cpu().numpy().tobytes() for o in outs] == before                 # the generator's four outputs are untouched
    for k, c in zip(("res5", "f1", "f2", "f"), copies):
        assert gen.probe(k).cpu().numpy().tobytes() == c.cpu().numpy().tobytes(), k
    # the chain differentiates the function the forward computed
    fs = host.decoder_forward(w, copies[0].cpu().numpy())
    for k, c, want in zip(("f1", "f2", "f"), copies[1:], fs):
        e = scaled_error(c.cpu().numpy(), want)
        print("colour decoder: the generator's %s against decoder_forward on its own res5 in float64: scaled error %.3g" % (k, e))
        assert e <= 1e-5
    with pytest.raises(ValueError, match="last forward was"):
        runner.backward(gen, d_f[:1].contiguous())


def test_tail_and_decoder_chained(generated):
    """The device walk over the tail and the decoder (ColourTail.backward then ColourDecoder.backward) on one forward at (32, 256),
    against the two statements chained on the device's own activations (the tail's a1, a2 and the decoder's f1, f2, f)."""
    from blindshadowremoval_amd import objective
    gen, w, outs, copies = generated
    _, _, g_con_a, g_gs_a = host.example_inputs(32, 256, 2, 9)
    g_con, g_gs = to_dev(g_con_a, g_gs_a)
    walked = objective.device_walk(objective.device_runners(("tail", "decoder"), w), gen, dict(gs=outs[0], grad_con=g_con, grad_gs=g_gs), keep=("tail",))
    t, d = walked["tail"], to_host(walked["decoder"])
    torch.cuda.synchronize()
    x, f1, f2, f = (c.cpu().numpy() for c in copies)
    st_t = host.tail_grad(w, outs[0].cpu().numpy(), f, g_con_a, g_gs_a, acts={"a1": t["a1"].cpu().numpy(), "a2": t["a2"].cpu().numpy()})
    st_d = host.decoder_grad(w, x, st_t["d_f"], acts={"f1": f1, "f2": f2, "f": f})
    import clr_tail_grad_cases as tail_cases
    import test_clr_tail_grad_gpu as tail_gpu
    worst, at = cases.worst_scaled_diff(d, st_d)
    print("colour tail and decoder chained: worst scaled error %.3g at %s (bound %.3g + %.3g)" % (worst, at, tail_gpu.E2E_BOUND, cases.E2E_BOUND))
    assert tail_cases.worst_scaled_diff(to_host(t), st_t)[0] <= tail_gpu.E2E_BOUND
    assert worst <= tail_gpu.E2E_BOUND + cases.E2E_BOUND, (worst, at)


def test_last_decoder_is_refused_for_a_sixteen_bit_generator():
    from blindshadowremoval_amd import Generator
    gen = Generator(device=0, dtype="f16")
    gen.load_weights(cases.decoder_weights())
    rng = np.random.default_rng(22)
    inputs, uv = to_dev(rng.uniform(0, 1, (1, 32, 256, 3)).astype(f32), rng.uniform(0, 1, (1, 32, 256, 3)).astype(f32))
    gen(inputs, uv)
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="BSR_DTYPE_F32 handles only"):
        gen.last_decoder()


# ---- the command
def test_command_decoder_device_route_matches_the_host_route(tmp_path_factory, capsys):
    """--grad-total --tail --decoder on one item at 256 x 256: both routes print the same fields, the decoder's 26 norms after the
    tail's, and each agrees within 1e-3 of its own magnitude, the ceiling of every end-to-end bound of the project (the routes feed the
    decoder d_f's that already differ by the terms' and the tail's own end-to-end errors, tests/test_objective_gpu.py).  Without --tail
    the flag is refused."""
    import pairs_cases
    from blindshadowremoval_amd import objective
    from blindshadowremoval_amd.weights import init_vgg_weights, save_vgg_weights
    folder = pairs_cases.write_pairs(tmp_path_factory.mktemp("decoder_pairs"))
    vgg = str(tmp_path_factory.mktemp("decoder_vgg") / "vgg.npz")
    save_vgg_weights(vgg, init_vgg_weights(21))
    names = objective.decoder_grad_names()
    assert len(names) == 26 and names[:2] == ["d_x_l1", "d_x_linf"]
    printed = []
    for extra in ([], ["--host"]):
        assert objective.main([folder, "--vgg", vgg, "--batch", "1", "--grad-total", "--tail", "--decoder"] + extra) == 0
        lines = capsys.readouterr().out.strip().split("\n")
        assert len(lines) == 2 and lines[0].startswith("1/1 ")
        fields = dict(f.rsplit(":", 1) for f in lines[0][4:].split(", "))
        assert tuple(fields) == objective.ALL_NAMES + objective.TOTAL_GRAD_NAMES + tuple(objective.tail_grad_names()) + tuple(names)
        printed.append({k: float(v) for k, v in fields.items()})
    dev_route, host_route = printed
    for k in names:
        d = abs(dev_route[k] - host_route[k])
        print("objective command --decoder %s: device %.9g host %.9g, relative difference %.3g" % (k, dev_route[k], host_route[k], d / host_route[k]))
        assert host_route[k] > 0 and d <= 1e-3 * host_route[k], k
    with pytest.raises(SystemExit):
        objective.main([folder, "--vgg", vgg, "--grad-total", "--decoder"])
    capsys.readouterr()
