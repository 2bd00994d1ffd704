"""bsr_grey_decoder_grad (csrc/grey_up_grad_kernels.h) against the host statement blindshadowremoval_amd/generator_grad.py:
grey_decoder_grad.

Stage by stage: each of the chain's launches, fed the DEVICE's own inputs, against the float64 statement of that launch alone within
max|got - ref| / max|ref| <= 1e-5, the project's fp32-class stage budget.  End to end: the fifteen outputs against grey_decoder_grad(acts
= the device's own up1, up2, y), each on the scale of its own largest reference magnitude, within cases.E2E_BOUND = 4 x the largest
figure measured on the MI355X over these shapes (tools/grey_decoder_bench.py --parity, profiles/grey_decoder_grad_bench.json, DESIGN
section 25), never above 1e-5.

Image sizes (H, W, B): (32, 256, 1) is the smallest the generator takes (up1's grid is one dgrad tile and two wgrad tiles); (64, 256, 2)
has tile seams both ways at every level, an image seam and 8, 32, 128 tiles for P = 3, 11, 43 partials, none of which divides its count;
(96, 256, 3) has 18, 72, 288 tiles: with B = 3 every count is a multiple of 3, so P = ceil(tiles / 3) = 6, 24, 96 divides it at every
level whatever the caps (85, 51, 128) — the size whose slice counts do not divide is (64, 256, 2), asserted below from
bsr_grey_decoder_grad_partials; (32, 512, 1) is wide."""
import ctypes

import numpy as np
import pytest

from blindshadowremoval_amd import generator_grad as host

import grey_decoder_grad_cases as cases

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
f32 = np.float32
SIZES = ((32, 256, 1), (64, 256, 2), (96, 256, 3), (32, 512, 1))
DATA = cases.DATA


@pytest.fixture(scope="module")
def runner():
    from blindshadowremoval_amd import GreyDecoder
    r = GreyDecoder(0)
    r.load_weights(cases.decoder_weights())
    return r


def to_dev(*arrays):
    dev = torch.device("cuda", 0)
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def to_host(res):
    return {k: v.cpu().numpy() for k, v in res.items()}


def entry_arrays(x, x3, x2, acts, d_y):
    """(x, c2 = cat[up1, x3], c3 = cat[up2, x2], y, d_y) float32: the entry point's five inputs, the concatenations as the forward lays
    them out."""
    up1, up2, y = (np.asarray(acts[k], f32) for k in ("up1", "up2", "y"))
    return (x, np.concatenate([up1, x3], axis=3), np.concatenate([up2, x2], axis=3), np.ascontiguousarray(y), d_y)


def device_run(runner, w, x, x3, x2, d_y, acts=None):
    """The `run` of cases.check_*: the runner's own forward is grey_decoder_forward in float32."""
    runner.load_weights(w)
    if acts is None:
        acts = dict(zip(("up1", "up2", "y"), cases.forward32(w, x, x3, x2)))
    res = runner.grey_decoder_grad(*to_dev(*entry_arrays(x, x3, x2, acts, d_y)), keep=True)
    torch.cuda.synchronize()
    out = to_host(res)
    out.update((k, np.asarray(acts[k], f32)) for k in ("up1", "up2", "y"))
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
        w, x, x3, x2, d_y = cases.case(H // 8, W // 8, B, 1)
        acts = dict(zip(("up1", "up2", "y"), cases.forward32(w, x, x3, x2)))
        arrays = entry_arrays(x, x3, x2, acts, d_y)
        res = runner.grey_decoder_grad(*to_dev(*arrays), keep=True)
        torch.cuda.synchronize()
        out[(H, W, B)] = (w, (x, x3, x2, acts, d_y), arrays, to_host(res), to_host(runner.maps(B, H, W)))
    return out


@pytest.mark.parametrize("check", cases.CONSTRUCTED, ids=lambda c: c.__name__)
def test_constructed_case(runner, check):
    check(lambda *a: device_run(runner, *a))
    runner.load_weights(cases.decoder_weights())


@pytest.mark.parametrize("H,W,B", SIZES)
def test_stage_by_stage(device_results, H, W, B):
    w, (x, x3, x2, acts, d_y), (_, c2, c3, y, _), res, maps = device_results[(H, W, B)]

    def hold(what, got, want):
        got, want = np.asarray(got), np.asarray(want)
        assert got.shape == want.shape, what
        e = scaled_error(got, want)
        print("grey decoder grad H=%d W=%d B=%d %s fed the device's input: scaled error %.3g" % (H, W, B, what, e))
        assert e <= cases.STAGE_BUDGET, (what, e)

    # launch 1: the entry mask, exact
    assert maps["gz3"].tobytes() == host.leaky_grad(d_y, y).astype(f32).tobytes()
    # layer -> (its input, the channels of its dx that stay in the decoder, the activation whose sign masks those, the skip's output)
    below = {3: (c3, 64, acts["up2"], "d_x2"), 2: (c2, 96, acts["up1"], "d_x3"), 1: (x, 257, None, None)}
    for n, i in ((2, 3), (4, 2), (6, 1)):
        stem = "up%d" % i
        a_in, own, mask, skip = below[i]
        gz = maps["gz%d" % i].astype(np.float64)
        K = np.asarray(w[stem + "/conv/kernel"], np.float64)
        bias, inv, mean, rstd, _ = host.bn_vectors(w, stem)
        # the kernel gradient before the BN factor and S, from the device's gz
        Wg, S = maps["Wg%d" % i], maps["S%d" % i]
        hold("launch %d Wg%d" % (n, i), Wg, host.convt3x3_same_wgrad(a_in, gz))
        hold("launch %d S%d" % (n, i), S, gz.sum(axis=(0, 1, 2)))
        # the data gradient from the device's gz: the decoder's half masked, the skip's half plain
        dx = host.convt3x3_same_dgrad(gz * inv, K)
        if mask is None:
            hold("launch %d d_x" % (n + 1), res["d_x"], dx)
        else:
            hold("launch %d gz%d" % (n + 1, i - 1), maps["gz%d" % (i - 1)], host.leaky_grad(dx[..., :own], mask))
            hold("launch %d %s" % (n + 1, skip), res[skip], dx[..., own:])
        # launches 8 and 9 from the device's Wg and S
        hold("launch 8 d K%d" % i, res[stem + "/conv/kernel"], Wg * inv[:, None])
        hold("launch 9 d beta%d" % i, res[stem + "/bnorm/beta"], S)
        hold("launch 9 d bias%d" % i, res[stem + "/conv/bias"], inv * S)
        hold("launch 9 d gamma%d" % i, res[stem + "/bnorm/gamma"], (((K * Wg).sum(axis=(0, 1, 3)) + bias * S) - mean * S) * rstd)


@pytest.mark.parametrize("H,W,B", SIZES)
def test_end_to_end(device_results, H, W, B):
    w, (x, x3, x2, acts, d_y), _, res, maps = device_results[(H, W, B)]
    st = host.grey_decoder_grad(w, x, x3, x2, d_y, acts=acts)
    for name in cases.OUTPUTS:
        print("grey decoder grad H=%d W=%d B=%d %s against the statement on the device's activations: scaled error %.3g (bound %.3g)"
              % (H, W, B, name, scaled_error(res[name], st[name]), cases.E2E_BOUND))
    d, at = cases.worst_scaled_diff(res, st)
    print("grey decoder grad H=%d W=%d B=%d: worst %.3g at %s" % (H, W, B, d, at))
    assert d <= cases.E2E_BOUND <= cases.STAGE_BUDGET, (d, at)


def test_some_shape_has_slice_counts_that_do_not_divide_its_tiles():
    from blindshadowremoval_amd import _lib
    lib = _lib.load()
    odd = []
    for H, W, B in SIZES:
        for layer in (1, 2, 3):
            P = int(lib.bsr_grey_decoder_grad_partials(B, H, W, layer))
            tiles = B * ((H >> (4 - layer)) // 4) * ((W >> (4 - layer)) // 16)
            assert 1 <= P <= tiles
            if P > 1 and tiles % P:
                odd.append((H, W, B, layer, tiles, P))
    print("grey decoder grad: (H, W, B, layer, tiles, P) with tiles % P != 0:", odd)
    assert {o[3] for o in odd if o[:3] == (64, 256, 2)} == {1, 2, 3}
    assert not [o for o in odd if o[:3] == (96, 256, 3)]          # multiples of 3 at every level: see the module's text


def flat_bytes(res):
    return [res[k].cpu().numpy().tobytes() for k in ("",) + DATA]


def test_a_repeated_call_and_two_sizes_on_one_scratch(runner, device_results):
    w, _, arrays3, _, _ = device_results[(96, 256, 3)]
    _, _, arrays1, _, _ = device_results[(32, 256, 1)]
    t3, t1 = to_dev(*arrays3), to_dev(*arrays1)
    first3 = flat_bytes(runner.grey_decoder_grad(*t3))
    first1 = flat_bytes(runner.grey_decoder_grad(*t1))             # B = 3 then B = 1 on the larger call's scratch
    assert flat_bytes(runner.grey_decoder_grad(*t3)) == first3
    assert flat_bytes(runner.grey_decoder_grad(*t1)) == first1
    assert flat_bytes(runner.grey_decoder_grad(*t1, keep=True)) == first1      # keeping the maps changes no output
    for t, a in zip(t1, arrays1):
        assert t.cpu().numpy().tobytes() == np.ascontiguousarray(a).tobytes()  # no input is ever written
    fresh = type(runner)(0)
    fresh.load_weights(w)
    assert flat_bytes(fresh.grey_decoder_grad(*t1)) == first1       # a scratch of its own size gives the same bytes


def test_debug_stops(runner, device_results):
    from blindshadowremoval_amd.grey_decoder_gpu import LAUNCHES
    _, _, arrays, res, _ = device_results[(64, 256, 2)]
    t = to_dev(*arrays)
    assert len(LAUNCHES) == 9
    for stop in range(10):
        got = to_host(runner.stages(*t, stop))
        for name, first in (("d_x2", 3), ("d_x3", 5), ("d_x", 7)):
            assert (got[name].tobytes() == res[name].tobytes()) if stop >= first else not got[name].any(), (stop, name)
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
    _, _, arrays, _, _ = device_results[(32, 256, 1)]
    t = to_dev(*arrays)
    eager = flat_bytes(runner.grey_decoder_grad(*t))
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        runner.grey_decoder_grad(*t)
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=side):
            res = runner.grey_decoder_grad(*t)
    torch.cuda.current_stream().wait_stream(side)
    for k in ("",) + DATA:
        res[k].zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert flat_bytes(res) == eager


def _entry_call(runner, lib, t, outs, scratch, **over):
    """bsr_grey_decoder_grad on the tensors t = (x, c2, c3, y, d_y) of (32, 256, 1) with the named arguments replaced -> (code, text)."""
    p = lambda v: ctypes.c_void_p(v.data_ptr())                                      # noqa: E731
    x, c2, c3, y, d_y = t
    a = dict(h=32, w=256, x=x, x_cs=257, c2_cs=160, nbytes=runner._blob.numel(), scr=scratch)
    a.update(over)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    return lib.bsr_grey_decoder_grad(0, p(runner._blob), a["nbytes"], p(a["x"]), a["x_cs"], p(c2), a["c2_cs"], p(c3), 128, p(y), 64, p(d_y), 1, a["h"], a["w"],
                                     *(p(o) for o in outs), 0, ctypes.c_void_p(a["scr"]), stream), lib.bsr_last_error().decode()


def _entry_outputs(lib, fill):
    dev = torch.device("cuda", 0)
    return [torch.full(s, fill, device=dev) for s in ((1, 4, 32, 257), (1, 8, 64, 64), (1, 16, 128, 64), (int(lib.bsr_grey_decoder_grad_floats()),))]


def test_a_strided_x_with_other_pad_lanes_gives_the_dense_bytes(runner, device_results):
    """x with 264 floats between pixels and lanes 257..263 full of large values, as a caller's tensor may hold: the chain stages the
    channels past 256 as zeros itself and reads no pad lane, so every output has the dense x's bytes."""
    from blindshadowremoval_amd import _lib
    lib = _lib.load()
    _, _, arrays, res, _ = device_results[(32, 256, 1)]
    t = to_dev(*arrays)
    wide = torch.full((1, 4, 32, 264), 1.0e6, device=t[0].device)
    wide[..., :257] = t[0]
    outs = _entry_outputs(lib, 7.0)
    scratch = runner.scratch4(1, 32, 256, False)
    assert _entry_call(runner, lib, t, outs, scratch, x=wide, x_cs=264)[0] == 0
    torch.cuda.synchronize()
    for name, o in zip(DATA + ("",), outs):
        assert o.cpu().numpy().tobytes() == res[name].tobytes(), name


def test_argument_errors_raise_before_any_launch(runner, device_results):
    from blindshadowremoval_amd import GreyDecoder, _lib
    from blindshadowremoval_amd.grey_decoder_gpu import NO_WEIGHTS_TEXT, SIZE_TEXT
    dev = torch.device("cuda", 0)
    _, _, arrays, _, _ = device_results[(32, 256, 1)]
    t = to_dev(*arrays)
    x, c2, c3, y, d_y = t
    with pytest.raises(ValueError) as e:
        GreyDecoder(0).grey_decoder_grad(*t)
    assert str(e.value) == NO_WEIGHTS_TEXT
    with pytest.raises(TypeError) as e:
        runner.grey_decoder_grad(x, c2.cpu(), c3, y, d_y)
    assert str(e.value) == "c2 must be a float32 tensor [B,.,.,160] on %s" % dev
    with pytest.raises(ValueError) as e:
        runner.grey_decoder_grad(x[..., :256].contiguous(), c2, c3, y, d_y)
    assert str(e.value) == "x must be [1,4,32,257] for this d_y, got (1, 4, 32, 256)"
    with pytest.raises(ValueError) as e:
        runner.grey_decoder_grad(*[torch.zeros((1, 48 // d, 256 // d, c), device=dev) for d, c in ((8, 257), (4, 160), (2, 128), (1, 64), (1, 64))])
    assert str(e.value) == SIZE_TEXT % (1, 48, 256)
    # the entry point itself: nothing is launched, the outputs keep their bytes
    lib = _lib.load()
    outs = _entry_outputs(lib, 7.0)
    scratch = runner.scratch4(1, 32, 256, False)
    size = "B must be positive, H a multiple of 32 and W a multiple of 256 (the generator's rule), at most 2^26 pixels in all"
    for kw, text in ((dict(h=48), size), (dict(w=128), size), (dict(x_cs=256), "x_cs must be at least 257"),
                     (dict(c2_cs=162), "c2_cs, c3_cs, y_cs must be multiples of 4 and at least 160, 128, 64"),
                     (dict(nbytes=16), "blob_bytes must be bsr_grey_decoder_grad_blob_bytes() (pack.pack_grey_decoder_grad; the GSC width 257 only, not TSM's 291)"),
                     (dict(scr=scratch + 8), "scratch must be 256-byte aligned")):
        assert _entry_call(runner, lib, t, outs, scratch, **kw) == (1, "bsr_grey_decoder_grad: " + text), kw
    torch.cuda.synchronize()
    for o in outs:
        assert bool((o == 7.0).all())


# ---- the generator's own tensors, in place
PROBES = ("res2", "up1", "x3", "up2", "x2", "y")


@pytest.fixture(scope="module")
def generated():
    """A seeded generator's forward at 256 x 256, B = 1, its inputs, outputs and copies of the six probes the grey decoder reads."""
    from blindshadowremoval_amd import Generator
    w = cases.decoder_weights()
    gen = Generator(device=0)
    gen.load_weights(w)
    with pytest.raises(RuntimeError, match="no forward has run"):
        gen.last_grey_decoder()
    rng = np.random.default_rng(21)
    inputs, uv = to_dev(rng.uniform(0, 1, (1, 256, 256, 3)).astype(f32), rng.uniform(0, 1, (1, 256, 256, 3)).astype(f32))
    outs = gen(inputs, uv)
    torch.cuda.synchronize()
    return gen, w, inputs, outs, {k: gen.probe(k).clone() for k in PROBES}


def test_backward_reads_the_generators_tensors_in_place(runner, generated):
    gen, w, inputs, outs, probes = generated
    runner.load_weights(w)
    before = [o.cpu().numpy().tobytes() for o in outs]
    d_y, = to_dev(host.grey_decoder_example_inputs(32, 32, 1, 9)[3])
    ptrs, strides, shape = gen.last_grey_decoder()
    assert shape == (1, 256, 256, 64) and strides[0] >= 257 and strides[1:] == (160, 128, 64) and all(p % 16 == 0 for p in ptrs)
    assert tuple(probes["res2"].shape) == (1, 32, 32, 257)
    copies = (probes["res2"], torch.cat([probes["up1"], probes["x3"]], dim=3), torch.cat([probes["up2"], probes["x2"]], dim=3), probes["y"])
    in_place = runner.backward(gen, d_y)
    copied = runner.grey_decoder_grad(*copies, d_y)
    torch.cuda.synchronize()
    assert flat_bytes(in_place) == flat_bytes(copied)
    kept = runner.backward(gen, d_y, keep=True)
    assert flat_bytes(kept) == flat_bytes(in_place) and all(k in kept for k in ("gz1", "gz2", "gz3"))
    assert [o.cpu().numpy().tobytes() for o in outs] == before                 # the generator's four outputs are untouched
    for k in PROBES:
        assert gen.probe(k).cpu().numpy().tobytes() == probes[k].cpu().numpy().tobytes(), k
    # the chain differentiates the function the forward computed
    ups = host.grey_decoder_forward(w, *(probes[k].cpu().numpy() for k in ("res2", "x3", "x2")))
    for k, want in zip(("up1", "up2", "y"), ups):
        e = scaled_error(probes[k].cpu().numpy(), want)
        print("grey decoder: the generator's %s against grey_decoder_forward on its own res2, x3, x2 in float64: scaled error %.3g" % (k, e))
        assert e <= 1e-5
    with pytest.raises(ValueError, match="last forward was"):
        runner.backward(gen, d_y[:, :128].contiguous())


def test_last_grey_decoder_is_refused_for_a_sixteen_bit_generator():
    from blindshadowremoval_amd import Generator
    gen = Generator(device=0, dtype="f16")
    gen.load_weights(cases.decoder_weights())
    rng = np.random.default_rng(22)
    inputs, uv = to_dev(rng.uniform(0, 1, (1, 32, 256, 3)).astype(f32), rng.uniform(0, 1, (1, 32, 256, 3)).astype(f32))
    gen(inputs, uv)
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="BSR_DTYPE_F32 handles only"):
        gen.last_grey_decoder()
    gen.close()


def test_total_gradient_tail_heads_and_grey_decoder_chained(runner, generated):
    """Forward -> DeviceRoute.total_grad -> the device walk over the tail and the heads -> GreyDecoder.backward(generator, d_y) on one
    forward at 256 x 256, against the three statements chained by hand on the device's own activations; the allowance is the three
    stages' added."""
    from blindshadowremoval_amd import objective
    from blindshadowremoval_amd.weights import init_discriminator_weights, init_vgg_weights
    import heads_grad_cases
    import test_clr_tail_grad_gpu as tail_gpu
    gen, w, inputs, outs, probes = generated
    runner.load_weights(w)
    route = objective.DeviceRoute(init_discriminator_weights(1), init_vgg_weights(21), w, wanted=("tail", "heads"))
    rng = np.random.default_rng(23)
    gt, mask_sv = to_dev(rng.uniform(0, 1, (1, 256, 256, 3)).astype(f32), rng.uniform(0, 1, (1, 256, 256, 3)).astype(f32))
    gs, con_rgb, mask22, _ = outs
    _, _, _, grad_con, grad_gs = route.total_grad(inputs, gt, mask_sv, gs, con_rgb)
    walked = objective.device_walk(route.runners, gen, dict(img=inputs, gs=gs, mask22=mask22, grad_con=grad_con, grad_gs=grad_gs), keep=("tail", "heads"))
    t, h = walked["tail"], walked["heads"]
    g = to_host(runner.backward(gen, h["d_y"]))
    torch.cuda.synchronize()
    f = gen.probe("f").cpu().numpy()
    st_t = host.tail_grad(w, gs.cpu().numpy(), f, grad_con.cpu().numpy(), grad_gs.cpu().numpy(),
                          acts={"a1": t["a1"].cpu().numpy(), "a2": t["a2"].cpu().numpy()})
    p = {k: v.cpu().numpy() for k, v in probes.items()}
    st_h = host.heads_grad(w, inputs.cpu().numpy(), p["y"], st_t["d_gs"], acts={"mask": h["mask"].cpu().numpy()})
    st_g = host.grey_decoder_grad(w, p["res2"], p["x3"], p["x2"], st_h["d_y"], acts={"up1": p["up1"], "up2": p["up2"], "y": p["y"]})
    worst, at = cases.worst_scaled_diff(g, st_g)
    bound = tail_gpu.E2E_BOUND + heads_grad_cases.E2E_BOUND + cases.E2E_BOUND
    print("total gradient, colour tail, heads and grey decoder chained: worst scaled error %.3g at %s (bound %.3g)" % (worst, at, bound))
    assert worst <= bound, (worst, at)
