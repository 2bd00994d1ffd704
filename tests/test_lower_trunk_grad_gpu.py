"""bsr_lower_trunk_grad (csrc/block_chain_grad.h) against the host statement blindshadowremoval_amd/generator_grad.py:
lower_trunk_grad.

Stage by stage: the chain is stopped after each of its 72 launches and what the launch wrote is the complete call's, byte for byte; each
launch, fed the DEVICE's own inputs, is then held to the float64 statement of that launch alone within max|got - ref| / max|ref| <=
1e-5, the project's fp32-class stage budget, by the per-launch statements of test_nonlocal_grad_gpu.py and test_bottleneck_grad_gpu.py
with the block's variables in block 5's names (both read the widths off the tensors; the one place that does not, the entry's d_skip at
block 0's 99 channels, is held here bit for bit).  End to end: the 67 outputs against lower_trunk_grad(acts = the device's own a1, a2 of
the three blocks), each on the scale of its own largest reference magnitude, within cases.E2E_BOUND = 4 x the largest figure measured on
the MI355X over these sizes.

Grids (h, w, B): (4, 32, 1) one tile row; (8, 32, 2) seams between tiles and between items; (12, 32, 3) an odd tile count; (4, 64, 1)
wide.  The workload's own grid belongs to tools/lower_trunk_bench.py."""
import ctypes

import numpy as np
import pytest

from blindshadowremoval_amd import generator_grad as host

import block_chain_cases as chain
import lower_trunk_grad_cases as cases
from block_chain_cases import scaled_error, to_dev, to_host

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
f32 = np.float32
SIZES = cases.GPU_SIZES
OUT_KEYS = ("", "d_x0")
N = 72
FIRST = chain.first_table(cases.BLOCKS, "d_x0", tail=False)        # the launch (1..72) that first writes each map and output


@pytest.fixture(scope="module")
def runner():
    from blindshadowremoval_amd import LowerTrunk
    r = LowerTrunk(0)
    r.load_weights(cases.lt_weights())
    return r


def strided_call(runner, tensors, strides, d_res2, keep=True):
    """lower_trunk_grad on the seven input tensors at the given floats between pixels: what backward does with the generator's own."""
    b, h, w = (int(d) for d in d_res2.shape[:3])
    given = {"d_res2": d_res2}
    names = [name for name, _, _, _ in runner.INPUTS[:7]]
    strided = {name: (t.data_ptr(), cs) for name, t, cs in zip(names, tensors, strides)}
    runner._check(given, in_place=True)
    return runner._result(runner._run(given, strided, b, h, w, keep), b, h, w, keep)


def device_run(runner, wt, x0, d_res2):
    """The `run` of cases.check_*.  An x0 that is a view of wider rows goes to the device with its rows, pad lanes included, and the
    chain reads it in place at that stride."""
    runner.load_weights(wt)
    six, y3s = cases.device_inputs(wt, np.ascontiguousarray(x0))
    t = to_dev(*six, np.ascontiguousarray(x0), d_res2)
    if x0.flags["C_CONTIGUOUS"]:
        res = runner.lower_trunk_grad(*t, keep=True)
    else:
        stride = x0.strides[2] // 4
        wide, = to_dev(np.lib.stride_tricks.as_strided(x0, x0.shape[:3] + (stride,), x0.strides))     # the whole rows behind the view
        assert tuple(wide.shape[:3]) == x0.shape[:3] and bool(torch.isnan(wide[..., 99:]).all())
        res = strided_call(runner, t[:6] + [wide], [257] * 6 + [stride], t[7])
    torch.cuda.synchronize()
    out = to_host(res)
    out.update({"res2": six[1], "res1": six[3], "res0": six[5], "y3_2": y3s[2], "y3_1": y3s[1], "y3_0": y3s[0], "dtype": f32})
    return out


@pytest.fixture(scope="module")
def device_results(runner):
    """Inputs, the device's result, what it left in the scratch and the statement on the device's activations, once per size."""
    out = {}
    for h, w, B in SIZES:
        wt, arrays, y3s, res, worst, at, st = cases.device_parity(runner, h, w, B)
        out[(h, w, B)] = (wt, arrays, y3s, res, to_host(runner.maps(B, h, w)), (worst, at, st))
    return out


@pytest.mark.parametrize("check", cases.CONSTRUCTED, ids=lambda c: c.__name__)
def test_constructed_case(runner, check):
    check(lambda *a: device_run(runner, *a))
    runner.load_weights(cases.lt_weights())


@pytest.mark.parametrize("h,w,B", SIZES)
def test_every_stop_leaves_what_the_complete_call_leaves(runner, device_results, h, w, B):
    """stages(..., n) for n = 1..72: what launches 1..n write is the complete call's, byte for byte, and the outputs of the launches
    that did not run are zero.  So every launch of the complete call ran on the inputs the per-launch statements below read."""
    _, arrays, _, _, _, _ = device_results[(h, w, B)]
    assert len(runner.LAUNCHES) == N and len(FIRST) == 3 * (15 + 12 + 3 + 22)
    chain.check_every_stop(runner, arrays, FIRST, "d_x0")


_as_block5 = chain.as_block5


@pytest.mark.parametrize("h,w,B", SIZES)
def test_stage_by_stage(device_results, h, w, B):
    import test_bottleneck_grad_gpu as bn_gpu
    import test_nonlocal_grad_gpu as nl_gpu
    wt, (y3x2, out2, y3x1, out1, y3x0, out0, x0, d_res2), _, res, maps, _ = device_results[(h, w, B)]
    feeds = {2: (y3x2, out1, out2, d_res2), 1: (y3x1, out0, out1, maps["d_xin2"]), 0: (y3x0, x0, out0, maps["d_xin1"])}
    for b in cases.BLOCKS:
        y3x, xin, out, d_out = feeds[b]
        X = cases.WIDTHS[b]
        assert xin.shape[3] == X and maps["bn%d.xp" % b].shape[3] == X and maps["bn%d.Wg1" % b].shape == (X, 128)
        moved, res5 = _as_block5(wt, res, b)
        y3_used = (y3x - cases.pad257(xin)).astype(f32)
        # the entry's d_skip, bit for bit at the block's own width: gz's first X channels
        gz = host.leaky_grad(d_out, out).astype(f32)
        assert maps["d_skip_%d" % b].shape[3] == X and maps["d_skip_%d" % b].tobytes() == np.ascontiguousarray(gz[..., :X]).tobytes()
        # launches 1..12 of the block: the non-local chain's statements on the device's own inputs.  They compare d_skip with all of gz:
        # block 0's stands in front of the device's own dz beyond channel 98, which the same statements hold to gz bit for bit
        d_skip = np.concatenate([maps["d_skip_%d" % b], maps["nl%d.dz" % b].reshape(B, h, w, 257)[..., X:]], axis=3)
        nl_res = dict(res5, d_y3=maps["d_y3_%d" % b], d_skip=d_skip)
        nl_maps = {k.split(".", 1)[1]: v for k, v in maps.items() if k.startswith("nl%d." % b)}
        nl_gpu.test_stage_by_stage({(8 * h, 8 * w, B): (moved, (y3x, xin, out, d_out), y3_used, nl_res, nl_maps)}, 8 * h, 8 * w, B)
        # launches 13..24 of the block: the bottleneck chain's statements on the device's own d_y3 and d_skip, at the block's width
        bn_res = dict(res5, d_xin=res["d_x0"] if b == 0 else maps["d_xin%d" % b])
        bn_maps = {k.split(".", 1)[1]: v for k, v in maps.items() if k.startswith("bn%d." % b)}
        bn_gpu.test_stage_by_stage({(h, w, B): (moved, (xin, maps["d_y3_%d" % b], maps["d_skip_%d" % b]), bn_res, bn_maps)}, h, w, B)
    for k in host.LOWER_TRUNK_DATA:
        assert res[k].tobytes() == maps[k].tobytes(), k


@pytest.mark.parametrize("h,w,B", SIZES)
def test_end_to_end(device_results, h, w, B):
    import bottleneck_grad_cases
    import nonlocal_grad_cases
    wt, arrays, _, res, maps, (d, at, st) = device_results[(h, w, B)]
    for k in res:
        if k in maps:
            assert res[k].tobytes() == maps[k].tobytes(), k                # what keep=True returns is what the scratch holds
    assert all(k in res for k in tuple("a%d_%d" % (j, b) for b in (0, 1, 2) for j in (1, 2)) + host.LOWER_TRUNK_DATA)
    for name in cases.OUTPUTS:
        print("lower trunk grad h=%d w=%d B=%d %s against the statement on the device's a1, a2: scaled error %.3g (bound %.3g)"
              % (h, w, B, name, cases.worst_scaled_diff(res, st, (name,))[0], cases.E2E_BOUND))
    print("lower trunk grad h=%d w=%d B=%d: worst %.3g at %s; three times the two single-block bounds added: %.3g"
          % (h, w, B, d, at, 3 * (nonlocal_grad_cases.E2E_BOUND + bottleneck_grad_cases.E2E_BOUND)))
    assert d <= cases.E2E_BOUND, (d, at)
    # the device's activations are the statement's own within the stage budget, and both signs are present
    fw = host.lower_trunk_forward(wt, arrays[6])
    for b in (0, 1, 2):
        for k in ("a1_%d" % b, "a2_%d" % b):
            assert scaled_error(res[k], fw[k]) <= cases.STAGE_BUDGET, k
            assert (res[k] > 0).any() and (res[k] < 0).any(), k


@pytest.mark.parametrize("h,w,B", ((4, 32, 1), (8, 32, 2), (4, 64, 3)))
def test_the_width_specific_kernels_alone_on_random_tensors(runner, h, w, B):
    """nl_entry_kernel<257> (launch 1), nl_entry_kernel<99> (launch 49), bn_entry_kernel<99> (launch 61) and launch 9 of block 0's
    bottleneck chain at n_store = 99 (launch 69) on random tensors, x0 at the generator's 120 floats between pixels with its pad lanes
    NaN: the entries against float32 numpy bit for bit (a select, a subtraction, copies), launch 69 against float64 on the device's own
    gz1 within the stage budget.  The tensors between them are whatever the chain made of the random inputs."""
    rng = np.random.default_rng(51 + h + w + B)
    normal = lambda c, s=1.0: (s * rng.standard_normal((B, h, w, c))).astype(f32)     # noqa: E731
    y3x2, out2, y3x1, out1, y3x0, out0 = normal(257, 0.25), normal(257), normal(257, 0.25), normal(257), normal(257, 0.25), normal(257)
    out2[0, 0, :3, :5] = [[0.0, -0.0, 1.0, -1.0, 0.0]] * 3                            # an activation of exactly +-0 takes the slope
    out0[0, 1, :3, 96:101] = [[-0.0, 0.0, 2.0, -2.0, -0.0]] * 3
    d_res2 = normal(257, 1e-3)
    wide = np.full((B, h, w, 120), np.nan, f32)
    wide[..., :99] = normal(99)
    x0 = np.ascontiguousarray(wide[..., :99])
    t = to_dev(y3x2, out2, y3x1, out1, y3x0, out0, wide, d_res2)
    res = to_host(strided_call(runner, t[:7], [257] * 6 + [120], t[7]))
    torch.cuda.synchronize()
    maps = to_host(runner.maps(B, h, w))
    wt = cases.lt_weights()
    # launch 1: nl_entry_kernel<257>
    gz = host.leaky_grad(d_res2, out2).astype(f32)
    assert gz[0, 0, 0, 0] == f32(0.3) * d_res2[0, 0, 0, 0] and gz[0, 0, 0, 2] == d_res2[0, 0, 0, 2]
    assert maps["d_skip_2"].tobytes() == gz.tobytes() and maps["nl2.dz"].tobytes() == gz.tobytes()
    assert maps["nl2.y3"].tobytes() == (y3x2 - out1).astype(f32).tobytes()
    # launch 49: nl_entry_kernel<99> on the device's own d_xin1
    assert np.isfinite(maps["d_xin1"]).all()
    gz = host.leaky_grad(maps["d_xin1"], out0).astype(f32)
    assert maps["nl0.dz"].tobytes() == gz.tobytes()
    assert maps["d_skip_0"].shape == (B, h, w, 99) and maps["d_skip_0"].tobytes() == np.ascontiguousarray(gz[..., :99]).tobytes()
    assert maps["nl0.y3"].tobytes() == (y3x0 - cases.pad257(x0)).astype(f32).tobytes()
    # launch 61: bn_entry_kernel<99>: the copies, the pad lanes of xp exact zeros
    lib = __import__("blindshadowremoval_amd")._lib.load()
    xp = runner.view(int(lib.bsr_lower_trunk_grad_offset(B, h, w, 46)), (B, h, w, 112)).cpu().numpy()
    assert xp[..., :99].tobytes() == x0.tobytes() and not xp[..., 99:].any() and not np.signbit(xp[..., 99:]).any()
    assert maps["bn0.xp"].tobytes() == x0.tobytes() and maps["bn0.dyp"].tobytes() == maps["d_y3_0"].tobytes()
    # launch 69: d_x0 = d_skip_0 + (gz1 inv1) W1^T, 99 columns of one 128-column tile
    K1 = np.asarray(wt["res_stack/0/conv1/kernel"], np.float64)[0, 0]
    inv1 = host.bottleneck_bn_vectors(wt, 1, 0)[1]
    want = maps["d_skip_0"].astype(np.float64) + (maps["bn0.gz1"].astype(np.float64) * inv1) @ K1.T
    e = scaled_error(res["d_x0"], want)
    print("lower trunk h=%d w=%d B=%d launch 69 (d_x0, n_store = 99) on random tensors: scaled error %.3g" % (h, w, B, e))
    assert res["d_x0"].shape == (B, h, w, 99) and e <= cases.STAGE_BUDGET
    assert all(np.isfinite(res[k]).all() for k in cases.OUTPUTS)


def test_the_device_keeps_the_bits_of_the_commit_before_the_shared_chain(device_results):
    """The flat gradient buffer, d_x0 and every kept entry at (4, 32, 1) and (12, 32, 3) hash to what the parent commit left on the MI355X
    (cases.PARENT_DEVICE_DIGESTS).  No further launch."""
    from blindshadowremoval_amd import LowerTrunk
    for size, want in cases.PARENT_DEVICE_DIGESTS.items():
        assert chain.device_digest(device_results[size][3], "d_x0", LowerTrunk.KEPT) == want, size


def flat_bytes(res):
    return chain.flat_bytes(res, OUT_KEYS)


def test_a_repeated_call_and_two_sizes_on_one_scratch(runner, device_results):
    wt, arrays3, _, res3, _, _ = device_results[(12, 32, 3)]
    _, arrays1, _, res1, _, _ = device_results[(4, 32, 1)]
    chain.check_a_repeated_call_and_two_sizes_on_one_scratch(runner, "lower_trunk_grad", wt, (arrays3, res3), (arrays1, res1), OUT_KEYS)


def test_the_chain_is_captured_into_a_graph_and_replays_the_same_bytes(runner, device_results):
    """Stream capture refuses a host synchronisation and work on another stream that is not joined: a call that is captured, replayed
    and gives the eager call's bytes has neither.  The chain is a line of launches: the captured graph has no branches."""
    chain.check_graph_capture(runner, "lower_trunk_grad", device_results[(4, 32, 1)][1], OUT_KEYS)


def test_argument_errors_raise_before_any_launch(runner, device_results):
    from blindshadowremoval_amd import LowerTrunk, _lib, pack
    from blindshadowremoval_amd.lower_trunk_gpu import NO_WEIGHTS_TEXT, SIZE_TEXT
    dev = torch.device("cuda", 0)
    _, arrays, _, _, _, _ = device_results[(4, 32, 1)]
    t = to_dev(*arrays)
    with pytest.raises(ValueError) as e:
        LowerTrunk(0).lower_trunk_grad(*t)
    assert str(e.value) == NO_WEIGHTS_TEXT
    with pytest.raises(TypeError) as e:
        runner.lower_trunk_grad(*t[:6], t[6].cpu(), t[7])
    assert str(e.value) == "x0 must be a float32 tensor [B,h,w,99] on %s" % dev
    with pytest.raises(ValueError) as e:
        runner.lower_trunk_grad(*t[:6], t[6][..., :98].contiguous(), t[7])
    assert str(e.value) == "x0 must be [1,4,32,99] for this d_res2, got (1, 4, 32, 98)"
    with pytest.raises(ValueError) as e:
        runner.lower_trunk_grad(*[torch.zeros((1, 6, 32, c), device=dev) for c in (257,) * 6 + (99, 257)])
    assert str(e.value) == SIZE_TEXT % (1, 6, 32)
    with pytest.raises(ValueError) as e:
        runner.load_weights(cases.lt_weights(variant="tsm"))
    assert str(e.value) == pack.LOWER_TRUNK_TEXT % (2, 257, (1, 1, 291, 128))
    # the entry point itself: nothing is launched, the outputs keep their bytes
    lib = _lib.load()
    d_x0 = torch.full((1, 4, 32, 99), 7.0, device=dev)
    flat = torch.full((int(lib.bsr_lower_trunk_grad_floats()),), 7.0, device=dev)
    scratch = runner.scratch3(1, 4, 32)
    p = lambda x: ctypes.c_void_p(x.data_ptr())                                      # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(h=4, w=32, x0_cs=99, out0_cs=257, nbytes=runner._blob.numel(), scr=scratch):
        return lib.bsr_lower_trunk_grad(0, p(runner._blob), nbytes, p(t[0]), 257, p(t[1]), 257, p(t[2]), 257, p(t[3]), 257, p(t[4]), 257, p(t[5]), out0_cs,
                                        p(t[6]), x0_cs, p(t[7]), 1, h, w, p(d_x0), p(flat), ctypes.c_void_p(scr), stream), lib.bsr_last_error().decode()

    size = "B must be positive, h a multiple of 4 and w a multiple of 32 (the generator's rule at 1/8 resolution), at most 2^21 pixels in all"
    strides = "y3x2_cs, y3x1_cs, y3x0_cs, out2_cs, out1_cs and out0_cs must be at least 257, x0_cs at least 99"
    for kw, text in ((dict(h=6), size), (dict(w=16), size), (dict(x0_cs=98), strides), (dict(out0_cs=256), strides),
                     (dict(nbytes=16), "blob_bytes must be bsr_lower_trunk_grad_blob_bytes() (pack.pack_lower_trunk_grad; the GSC widths 99 and 257 only, "
                                       "not TSM's 291 or RGB's 513)"),
                     (dict(scr=scratch + 8), "scratch must be 256-byte aligned")):
        assert call(**kw) == (1, "bsr_lower_trunk_grad: " + text), kw
    torch.cuda.synchronize()
    for o in (d_x0, flat):
        assert bool((o == 7.0).all())


# ---- the generator's own tensors, in place
@pytest.fixture(scope="module")
def generated():
    """cases.generated_forward: a forward at (32, 256), B = 2, with init_weights(1), under which about half of the pixels lie in the hole."""
    from blindshadowremoval_amd import Generator
    from blindshadowremoval_amd.weights import init_weights
    gen = Generator(device=0)
    gen.load_weights(init_weights(1))
    with pytest.raises(RuntimeError, match="no forward has run"):
        gen.last_lower_trunk()
    gen.close()
    return cases.generated_forward()


def test_backward_reads_the_generators_tensors_in_place(runner, generated):
    gen, w, inputs, outs, probes = generated
    runner.load_weights(w)
    before = [o.cpu().numpy().tobytes() for o in outs]
    d_res2, = to_dev(host.lower_trunk_example_inputs(4, 32, 2, 9)[1])
    ptrs, strides, shape = gen.last_lower_trunk()
    assert shape == (2, 4, 32, 257) and len(ptrs) == len(strides) == 7 and len(set(ptrs)) == 7 and all(p % 4 == 0 for p in ptrs)
    assert strides == (288, 264, 288, 264, 288, 264, 120)
    assert gen.last_grey_decoder()[0][0] == ptrs[1]                         # res_stack/2's output is the grey decoder's x
    for block in (2, 1, 0):
        with pytest.raises(RuntimeError, match="block must be 3, 4 or 5"):
            gen.last_block(block)
    copies = cases.probe_copies(probes)
    assert [tuple(c.shape) for c in copies] == [(2, 4, 32, 257)] * 6 + [(2, 4, 32, 99)]
    in_place = runner.backward(gen, d_res2)
    copied = runner.lower_trunk_grad(*copies, d_res2)
    torch.cuda.synchronize()
    assert flat_bytes(in_place) == flat_bytes(copied)
    kept = runner.backward(gen, d_res2, keep=True)
    assert flat_bytes(kept) == flat_bytes(in_place) and all(k in kept for k in type(runner).KEPT)
    assert [o.cpu().numpy().tobytes() for o in outs] == before                 # the generator's four outputs are untouched
    for k in probes:
        assert gen.probe(k).cpu().numpy().tobytes() == probes[k].cpu().numpy().tobytes(), k
    # the chain differentiates the function the forward computed: y3 = y3x<b> - pad(xin_b) against bottleneck_forward on xin_b
    p = {k: probes[k].cpu().numpy() for k in cases.PROBES}
    for b, xin in ((0, p["x0"]), (1, p["res0"]), (2, p["res1"])):
        y3 = (p["y3x%d" % b][..., :257] - cases.pad257(xin)).astype(f32)
        e = scaled_error(y3, host.bottleneck_forward(w, xin, block=b)["y3"])
        print("lower trunk: the generator's y3x%d - pad(xin) against bottleneck_forward(block=%d) on its own xin in float64: scaled error %.3g" % (b, b, e))
        assert e <= 1e-5
    with pytest.raises(ValueError, match="last forward was"):
        runner.backward(gen, d_res2[:1].contiguous())
    runner.load_weights(cases.lt_weights())


def test_backward_is_refused_before_a_forward_for_a_sixteen_bit_generator_and_for_tsm_weights(runner):
    from blindshadowremoval_amd import Generator, GeneratorTSM, pack
    d_res2, = to_dev(host.lower_trunk_example_inputs(4, 32, 1, 9)[1])
    gen = Generator(device=0)
    gen.load_weights(cases.lt_weights())
    with pytest.raises(RuntimeError, match="no forward has run"):
        runner.backward(gen, d_res2)
    gen.close()
    gen = Generator(device=0, dtype="f16")
    gen.load_weights(cases.lt_weights())
    rng = np.random.default_rng(22)
    inputs, uv = to_dev(rng.uniform(0, 1, (1, 32, 256, 3)).astype(f32), rng.uniform(0, 1, (1, 32, 256, 3)).astype(f32))
    gen(inputs, uv)
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="BSR_DTYPE_F32 handles only"):
        runner.backward(gen, d_res2)
    gen.close()
    tsm = cases.lt_weights(variant="tsm")
    with pytest.raises(ValueError) as e:
        type(runner)(0).load_weights(tsm)
    assert str(e.value) == pack.LOWER_TRUNK_TEXT % (2, 257, (1, 1, 291, 128))
    gen = GeneratorTSM(device=0)
    gen.load_weights(tsm)
    with pytest.raises(RuntimeError, match="not a TSM handle's 291"):
        runner.backward(gen, d_res2)
    gen.close()


def test_the_whole_backward_chained(generated):
    """On that forward: the device walk over the five table stages, then GreyDecoder.backward, ColourTrunk.backward and
    LowerTrunk.backward(generator, d_res2), against the eight host statements chained on the device's own activations: d_x0 is the
    gradient at the trunk's input."""
    gen, w, inputs, outs, probes = generated
    res, st, share = cases.whole_backward_chained(gen, w, inputs, outs, probes)
    assert 0.25 <= share <= 0.75, share
    worst, at = cases.worst_scaled_diff(res, st)
    print("the whole backward chained down to the trunk's input: worst scaled error %.3g at %s (bound %.3g); d_x0 %.3g; hole share %.3f"
          % (worst, at, cases.CHAINED_BOUND, cases.worst_scaled_diff(res, st, ("d_x0",))[0], share))
    assert worst <= cases.CHAINED_BOUND, (worst, at)
    assert np.abs(res["d_x0"][..., :96]).max() > 0 and np.abs(res["d_x0"][..., 96:]).max() > 0
