"""bsr_heads_grad (csrc/heads_grad_kernels.h) against the host statement blindshadowremoval_amd/generator_grad.py: heads_grad.

Stage by stage: each of the chain's launches, fed the DEVICE's own inputs, against the float64 statement of that launch alone within
max|got - ref| / max|ref| <= 1e-5, the project's fp32-class stage budget (the entry's g_m, whose float32 order is declared, bit for
bit).  End to end: the five outputs against heads_grad(acts = the device's own mask), each on the scale of its own largest reference
magnitude, within cases.E2E_BOUND = 4 x the largest figure measured on the MI355X over these sizes.

Sizes (H, W, B): (8, 32, 1) one tile, whose 3-pixel halo meets both borders at once; (16, 32, 2) tile seams, and the seam between the
images inside one slice's pixel range; (8, 64, 1) two tiles across; (24, 96, 3) more than one tile each way, 27 tiles in 14 slices;
(40, 32, 1) 5 tiles in 3 slices: the last two run the kernel gradient on more than one slice with a tile count that is no multiple of
the slice count (test_heads_bindings_cpu.py holds bsr_heads_grad_partials to cases.SLICES)."""
import ctypes

import numpy as np
import pytest

from blindshadowremoval_amd import generator_grad as host
from blindshadowremoval_amd import pack
from blindshadowremoval_amd.train_losses import gray

import heads_grad_cases as cases

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
f32 = np.float32
SIZES = cases.GPU_SIZES
OUT_KEYS = ("", "d_y")


@pytest.fixture(scope="module")
def runner():
    from blindshadowremoval_amd import HeadsGrad
    r = HeadsGrad(0)
    r.load_weights(cases.heads_weights())
    return r


def to_dev(*arrays):
    dev = torch.device("cuda", 0)
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def to_host(res):
    return {k: v.cpu().numpy() for k, v in res.items()}


def device_run(runner, w, inputs, y, d_gs):
    """The `run` of cases.check_*: the chain is handed the mask22 of the statement's own forward."""
    runner.load_weights(w)
    res = runner.heads_grad(*to_dev(inputs, cases.mask22_of(w, inputs, y), y, d_gs), keep=True)
    torch.cuda.synchronize()
    out = to_host(res)
    out["g_con"] = runner.maps(*d_gs.shape[:3])["g_con"].cpu().numpy()
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
        wt, inputs, y, d_gs = cases.case(H, W, B, 1)
        arrays = (inputs, cases.mask22_of(wt, inputs, y), y, d_gs)
        res = runner.heads_grad(*to_dev(*arrays), keep=True)
        torch.cuda.synchronize()
        out[(H, W, B)] = (wt, arrays, to_host(res), to_host(runner.maps(B, H, W)))
    return out


@pytest.mark.parametrize("check", cases.CONSTRUCTED, ids=lambda c: c.__name__)
def test_constructed_case(runner, check):
    check(lambda *a: device_run(runner, *a))
    runner.load_weights(cases.heads_weights())


@pytest.mark.parametrize("H,W,B", SIZES)
def test_stage_by_stage(device_results, H, W, B):
    wt, (inputs, mask22, y, d_gs), res, maps = device_results[(H, W, B)]

    def hold(what, got, want):
        got, want = np.asarray(got), np.asarray(want)
        assert got.shape == want.shape, what
        e = scaled_error(got, want)
        print("heads grad H=%d W=%d B=%d %s fed the device's input: scaled error %.3g" % (H, W, B, what, e))
        assert e <= cases.STAGE_BUDGET, (what, e)

    m = {k: v.astype(np.float64) for k, v in maps.items()}
    K2, K3 = (np.asarray(wt[n], np.float64) for n in (cases.K2, cases.K3))
    # launch 1: the mask is the forward's, g_con is d_gs, and g_m is its declared float32 order bit for bit
    mask = mask22[..., 0:1] - mask22[..., 2:3]
    assert maps["mask"].tobytes() == mask.tobytes() and maps["g_con"].tobytes() == d_gs.tobytes()
    g32 = gray(inputs)[..., None]
    assert g32.dtype == f32
    want = (d_gs * g32) * (f32(1) - mask * mask)
    assert want.dtype == f32 and maps["g_m"].tobytes() == want.tobytes()
    hold("launch 1 g_m", maps["g_m"], (d_gs.astype(np.float64) * g32) * (1 - mask.astype(np.float64) ** 2))
    # launch 2: d_y from the device's g2
    hold("launch 2 d_y", res["d_y"], host.convk_same_dgrad(m["g_m"], K2) + host.convk_same_dgrad(m["g_con"], K3))
    # launches 3, 4: the kernel gradients from the device's g2
    hold("launches 3, 4 Wg mask head", maps["Wg"][0], host.convk_same_wgrad(y, m["g_m"])[..., 0])
    hold("launches 3, 4 Wg con head", maps["Wg"][1], host.convk_same_wgrad(y, m["g_con"])[..., 0])
    for j, name in enumerate((cases.K2, cases.K3)):
        assert res[name].tobytes() == maps["Wg"][j].astype(f32).reshape(7, 7, 64, 1).tobytes(), name        # rounded once
    # launches 1, 5: the sums and the biases from the device's g2
    hold("launch 5 S", maps["S"], [m["g_m"].sum(), m["g_con"].sum()])
    assert res[cases.B2].tobytes() == maps["S"][0:1].astype(f32).tobytes() and res[cases.B3].tobytes() == maps["S"][1:2].astype(f32).tobytes()


@pytest.mark.parametrize("H,W,B", SIZES)
def test_end_to_end(device_results, H, W, B):
    wt, (inputs, mask22, y, d_gs), res, maps = device_results[(H, W, B)]
    for k in ("g_m", "mask"):
        assert res[k].tobytes() == maps[k].tobytes(), k                    # what keep=True returns is what the scratch holds
    st = host.heads_grad(wt, inputs, y, d_gs, acts={"mask": res["mask"]})
    for name in cases.OUTPUTS:
        print("heads grad H=%d W=%d B=%d %s against the statement on the device's mask: scaled error %.3g (bound %.3g)"
              % (H, W, B, name, cases.worst_scaled_diff(res, st, (name,))[0], cases.E2E_BOUND))
    d, at = cases.worst_scaled_diff(res, st)
    print("heads grad H=%d W=%d B=%d: worst %.3g at %s" % (H, W, B, d, at))
    assert d <= cases.E2E_BOUND, (d, at)
    # the mask handed in is the statement's own within float32's rounding, and both signs are present
    fw = host.heads_forward(wt, inputs, y)
    assert np.abs(res["mask"] - fw["mask"]).max() <= 2.0 ** -24
    assert (res["mask"] > 0).any() and (res["mask"] < 0).any()


def flat_bytes(res):
    return [res[k].cpu().numpy().tobytes() for k in OUT_KEYS]


def test_a_repeated_call_and_two_sizes_on_one_scratch(runner, device_results):
    w, arrays3, _, _ = device_results[(24, 96, 3)]
    _, arrays1, _, _ = device_results[(8, 32, 1)]
    t3, t1 = to_dev(*arrays3), to_dev(*arrays1)
    first3 = flat_bytes(runner.heads_grad(*t3))
    first1 = flat_bytes(runner.heads_grad(*t1))            # B = 3 then B = 1 on the larger call's scratch
    assert flat_bytes(runner.heads_grad(*t3)) == first3
    assert flat_bytes(runner.heads_grad(*t1)) == first1
    assert flat_bytes(runner.heads_grad(*t1, keep=True)) == first1     # keeping the maps changes no output
    for t, a in zip(t1, arrays1):
        assert t.cpu().numpy().tobytes() == a.tobytes()                 # no input is ever written
    fresh = type(runner)(0)
    fresh.load_weights(w)
    assert flat_bytes(fresh.heads_grad(*t1)) == first1      # a scratch of its own size gives the same bytes


def test_a_strided_y_is_read_like_a_dense_one(runner, device_results):
    """y with 96 floats between pixels, as a workspace slot may hold it, through the entry point: the bytes of the dense call."""
    from blindshadowremoval_amd import _lib
    _, arrays, res, _ = device_results[(16, 32, 2)]
    inputs, mask22, y, d_gs = to_dev(*arrays)
    wide = torch.full((2, 16, 32, 96), float("nan"), device=y.device)
    wide[..., :64] = y
    d_y, flat = torch.zeros_like(y), torch.zeros(6274, device=y.device)
    lib = _lib.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr())                                      # noqa: E731
    rc = lib.bsr_heads_grad(0, p(runner._blob), runner._blob.numel(), p(inputs), p(mask22), p(wide), 96, p(d_gs), 2, 16, 32, p(d_y), p(flat),
                            ctypes.c_void_p(runner.scratch3(2, 16, 32)), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0 and d_y.cpu().numpy().tobytes() == res["d_y"].tobytes() and flat.cpu().numpy().tobytes() == res[""].tobytes()


def test_debug_stops(runner, device_results):
    from blindshadowremoval_amd.heads_grad_gpu import LAUNCHES
    _, arrays, res, maps = device_results[(16, 32, 2)]
    t = to_dev(*arrays)
    assert len(LAUNCHES) == 5
    runner.stages(*t, 0)
    first = {"g_m": 1, "g_con": 1, "mask": 1, "Wg": 4, "S": 5}
    kernels = (cases.K2, cases.K3)
    for stop in range(6):
        got = to_host(runner.stages(*t, stop))
        assert (got["d_y"].tobytes() == res["d_y"].tobytes()) if stop >= 2 else not got["d_y"].any(), stop
        views = type(runner).split_grads(torch.from_numpy(got[""]))
        for name in cases.NAMES:
            v = views[name].numpy()
            done = stop >= 4 if name in kernels else stop >= 5
            assert (v.tobytes() == res[name].tobytes()) if done else not v.any(), (stop, name)
        for name, at in first.items():
            if stop >= at:
                assert got[name].tobytes() == maps[name].tobytes(), (stop, name)
    with pytest.raises(ValueError, match="stop_after"):
        runner.stages(*t, 6)


def test_the_chain_is_captured_into_a_graph_and_replays_the_same_bytes(runner, device_results):
    """Stream capture refuses a host synchronisation and work on another stream that is not joined: a call that is captured, replayed
    and gives the eager call's bytes has neither.  The chain is a line of launches: the captured graph has no branches."""
    _, arrays, _, _ = device_results[(8, 32, 1)]
    t = to_dev(*arrays)
    eager = flat_bytes(runner.heads_grad(*t))
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        runner.heads_grad(*t)
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=side):
            res = runner.heads_grad(*t)
    torch.cuda.current_stream().wait_stream(side)
    for k in OUT_KEYS:
        res[k].zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert flat_bytes(res) == eager


def test_argument_errors_raise_before_any_launch(runner, device_results):
    from blindshadowremoval_amd import HeadsGrad, _lib
    from blindshadowremoval_amd.heads_grad_gpu import NO_WEIGHTS_TEXT, SIZE_TEXT
    from blindshadowremoval_amd.weights import init_weights
    dev = torch.device("cuda", 0)
    _, arrays, _, _ = device_results[(8, 32, 1)]
    inputs, mask22, y, d_gs = to_dev(*arrays)
    with pytest.raises(ValueError) as e:
        HeadsGrad(0).heads_grad(inputs, mask22, y, d_gs)
    assert str(e.value) == NO_WEIGHTS_TEXT
    with pytest.raises(TypeError) as e:
        runner.heads_grad(inputs, mask22, y.cpu(), d_gs)
    assert str(e.value) == "y must be a float32 tensor [B,H,W,64] on %s" % dev
    with pytest.raises(ValueError) as e:
        runner.heads_grad(inputs, mask22, y[..., :63].contiguous(), d_gs)
    assert str(e.value) == "y must be [1,8,32,64] like d_gs, got (1, 8, 32, 63)"
    with pytest.raises(ValueError) as e:
        runner.heads_grad(*[torch.zeros((1, 12, 32, c), device=dev) for c in (3, 3, 64, 1)])
    assert str(e.value) == SIZE_TEXT % (1, 12, 32)
    with pytest.raises(ValueError) as e:
        HeadsGrad(0).load_weights(init_weights(1, variant="rgb"))
    assert str(e.value) == pack.HEADS_RGB_TEXT
    # the entry point itself: nothing is launched, the outputs keep their bytes
    lib = _lib.load()
    d_y = torch.full((1, 8, 32, 64), 7.0, device=dev)
    flat = torch.full((int(lib.bsr_heads_grad_floats()),), 7.0, device=dev)
    scratch = runner.scratch3(1, 8, 32)
    p = lambda t: ctypes.c_void_p(t.data_ptr())                                      # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(H=8, W=32, y_cs=64, nbytes=runner._blob.numel(), scr=scratch):
        return lib.bsr_heads_grad(0, p(runner._blob), nbytes, p(inputs), p(mask22), p(y), y_cs, p(d_gs), 1, H, W, p(d_y), p(flat),
                                  ctypes.c_void_p(scr), stream), lib.bsr_last_error().decode()

    size = "B must be positive, H a multiple of 8 and W a multiple of 32 (the forward heads' tile), at most 2^26 pixels in all"
    for kw, text in ((dict(H=12), size), (dict(W=16), size), (dict(y_cs=62), "y_cs must be a multiple of 4 and at least 64"),
                     (dict(nbytes=16), "blob_bytes must be bsr_heads_grad_blob_bytes() (pack.pack_heads_grad)"),
                     (dict(scr=scratch + 8), "scratch must be 256-byte aligned")):
        assert call(**kw) == (1, "bsr_heads_grad: " + text), kw
    torch.cuda.synchronize()
    for t in (d_y, flat):
        assert bool((t == 7.0).all())


# ---- the generator's own tensors, in place
@pytest.fixture(scope="module")
def generated():
    """A seeded generator's forward at 256 x 256, B = 1, its inputs, outputs and a copy of y."""
    from blindshadowremoval_amd import Generator
    w = cases.heads_weights()
    gen = Generator(device=0)
    gen.load_weights(w)
    with pytest.raises(RuntimeError, match="no forward has run"):
        gen.last_y()
    rng = np.random.default_rng(21)
    inputs, uv = to_dev(rng.uniform(0, 1, (1, 256, 256, 3)).astype(f32), rng.uniform(0, 1, (1, 256, 256, 3)).astype(f32))
    outs = gen(inputs, uv)
    torch.cuda.synchronize()
    return gen, w, inputs, outs, gen.probe("y").clone()


def test_backward_reads_the_generators_y_in_place(runner, generated):
    gen, w, inputs, outs, y_copy = generated
    runner.load_weights(w)
    before = [o.cpu().numpy().tobytes() for o in outs]
    d_gs, = to_dev(host.heads_example_inputs(256, 256, 1, 9)[2])
    ptr, stride, shape = gen.last_y()
    assert shape == (1, 256, 256, 64) and stride >= 64 and stride % 4 == 0 and ptr % 16 == 0
    in_place = runner.backward(gen, inputs, outs[2], d_gs)
    copied = runner.heads_grad(inputs, outs[2], y_copy, d_gs)
    torch.cuda.synchronize()
    assert flat_bytes(in_place) == flat_bytes(copied)
    kept = runner.backward(gen, inputs, outs[2], d_gs, keep=True)
    assert flat_bytes(kept) == flat_bytes(in_place) and all(k in kept for k in ("g_m", "mask"))
    assert [o.cpu().numpy().tobytes() for o in outs] == before                 # the generator's four outputs are untouched
    assert gen.probe("y").cpu().numpy().tobytes() == y_copy.cpu().numpy().tobytes()
    # the chain differentiates the function the forward computed: mask22[.., 0] - mask22[.., 2] and gs against heads_forward on its own y
    fw = host.heads_forward(w, inputs.cpu().numpy(), y_copy.cpu().numpy())
    mask22 = outs[2].cpu().numpy()
    e_mask = float(np.abs((mask22[..., 0:1] - mask22[..., 2:3]) - fw["mask"]).max())
    e_gs = scaled_error(outs[0].cpu().numpy(), fw["gs"])
    print("heads grad: the generator's mask against tanh(m) on its own y in float64: error %.3g; its gs: scaled error %.3g" % (e_mask, e_gs))
    assert e_mask <= 1e-5 and e_gs <= 1e-5
    assert kept["mask"].cpu().numpy().tobytes() == (mask22[..., 0:1] - mask22[..., 2:3]).tobytes()
    with pytest.raises(ValueError, match="last forward was"):
        runner.backward(gen, inputs[:, :128].contiguous(), outs[2][:, :128].contiguous(), d_gs[:, :128].contiguous())


def test_backward_is_refused_before_a_forward_and_for_a_sixteen_bit_generator(runner):
    from blindshadowremoval_amd import Generator
    rng = np.random.default_rng(22)
    inputs, uv, mask22 = to_dev(*(rng.uniform(0, 1, (1, 32, 256, 3)).astype(f32) for _ in range(3)))
    d_gs, = to_dev(host.heads_example_inputs(32, 256, 1, 9)[2])
    gen = Generator(device=0)
    gen.load_weights(cases.heads_weights())
    with pytest.raises(RuntimeError, match="no forward has run"):
        runner.backward(gen, inputs, mask22, d_gs)
    gen.close()
    gen = Generator(device=0, dtype="f16")
    gen.load_weights(cases.heads_weights())
    gen(inputs, uv)
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="BSR_DTYPE_F32 handles only"):
        runner.backward(gen, inputs, mask22, d_gs)
    gen.close()


def test_total_gradient_tail_and_heads_chained(generated):
    """Forward -> DeviceRoute.total_grad -> the device walk over the tail and the heads (ColourTail.backward -> HeadsGrad.backward) on one
    forward at 256 x 256, against the tail's and the heads' statements chained on the device's own activations; the allowance is the two
    stages' added."""
    from blindshadowremoval_amd import objective
    from blindshadowremoval_amd.weights import init_discriminator_weights, init_vgg_weights
    import test_clr_tail_grad_gpu as tail_gpu
    gen, w, inputs, outs, y_copy = generated
    route = objective.DeviceRoute(init_discriminator_weights(1), init_vgg_weights(21), w, wanted=("tail", "heads"))
    rng = np.random.default_rng(23)
    gt, mask_sv = to_dev(rng.uniform(0, 1, (1, 256, 256, 3)).astype(f32), rng.uniform(0, 1, (1, 256, 256, 3)).astype(f32))
    gs, con_rgb, mask22, _ = outs
    _, _, _, grad_con, grad_gs = route.total_grad(inputs, gt, mask_sv, gs, con_rgb)
    walked = objective.device_walk(route.runners, gen, dict(img=inputs, gs=gs, mask22=mask22, grad_con=grad_con, grad_gs=grad_gs), keep=("tail", "heads"))
    t, h = walked["tail"], to_host(walked["heads"])
    torch.cuda.synchronize()
    f = gen.probe("f").cpu().numpy()
    st_t = host.tail_grad(w, gs.cpu().numpy(), f, grad_con.cpu().numpy(), grad_gs.cpu().numpy(),
                          acts={"a1": t["a1"].cpu().numpy(), "a2": t["a2"].cpu().numpy()})
    st_h = host.heads_grad(w, inputs.cpu().numpy(), y_copy.cpu().numpy(), st_t["d_gs"], acts={"mask": h["mask"]})
    worst, at = cases.worst_scaled_diff(h, st_h)
    bound = tail_gpu.E2E_BOUND + cases.E2E_BOUND
    print("total gradient, colour tail and heads chained: worst scaled error %.3g at %s (bound %.3g)" % (worst, at, bound))
    assert worst <= bound, (worst, at)


# ---- the command
def test_command_heads_device_route_matches_the_host_route(tmp_path_factory, capsys):
    """--grad-total --tail --heads on one item at 256 x 256: both routes print the same fields, the heads' 10 norms after the tail's, and
    each agrees within 1e-3 of its own magnitude, the ceiling of every end-to-end bound of the project (the routes feed the stage a d_gs
    that already differs by the terms' and the tail's own end-to-end errors).  With the colour branch's flags the heads' columns still
    come last; without --tail the flag is refused, and without the flag the line is the one --tail prints."""
    import pairs_cases
    from blindshadowremoval_amd import objective
    from blindshadowremoval_amd.weights import init_vgg_weights, save_vgg_weights
    folder = pairs_cases.write_pairs(tmp_path_factory.mktemp("heads_pairs"))
    vgg = str(tmp_path_factory.mktemp("heads_vgg") / "vgg.npz")
    save_vgg_weights(vgg, init_vgg_weights(21))
    names = objective.heads_grad_names()
    above = objective.ALL_NAMES + objective.TOTAL_GRAD_NAMES + tuple(objective.tail_grad_names())
    printed = []
    for extra in ([], ["--host"]):
        assert objective.main([folder, "--vgg", vgg, "--batch", "1", "--grad-total", "--tail", "--heads"] + extra) == 0
        lines = capsys.readouterr().out.strip().split("\n")
        assert len(lines) == 2 and lines[0].startswith("1/1 ")
        fields = dict(f.rsplit(":", 1) for f in lines[0][4:].split(", "))
        assert tuple(fields) == above + tuple(names)
        printed.append((lines[0], {k: float(v) for k, v in fields.items()}))
    (dev_line, dev_route), (_, host_route) = printed
    for k in names:
        scale = host_route[k]
        d = abs(dev_route[k] - host_route[k])
        print("objective command --heads %s: device %.9g host %.9g, difference over scale %.3g" % (k, dev_route[k], host_route[k], d / scale))
        assert scale > 0 and d <= 1e-3 * scale, k
    capsys.readouterr()
    assert objective.main([folder, "--vgg", vgg, "--batch", "1", "--grad-total", "--tail"]) == 0
    without = capsys.readouterr().out.strip().split("\n")[0]
    assert dev_line.startswith(without + ", ") and len(dev_line[len(without) + 2:].split(", ")) == 10
    assert objective.main([folder, "--vgg", vgg, "--batch", "1", "--grad-total", "--tail", "--decoder", "--heads"]) == 0
    fields = [f.rsplit(":", 1)[0] for f in capsys.readouterr().out.strip().split("\n")[0][4:].split(", ")]
    assert tuple(fields) == above + tuple(objective.decoder_grad_names()) + tuple(names)
    with pytest.raises(SystemExit):
        objective.main([folder, "--vgg", vgg, "--grad-total", "--heads"])
    capsys.readouterr()
