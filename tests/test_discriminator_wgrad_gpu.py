"""bsr_disc_wgrad (csrc/disc_wgrad_kernels.h) against the host statement blindshadowremoval_amd/discriminator.py: disc_grad.

Stage by stage: each of the chain's launches, fed the DEVICE's own incoming gradient, kept activations and logits, against the float64
statement of that launch alone within max|got - ref| / max|ref| <= 1e-5, the project's fp32-class stage budget (tests/stage_parity.py);
the seed bit for bit.  End to end: all 54 gradients against disc_grad(acts = the device's, logits = the device's), each variable on
the scale of its own largest reference magnitude, within 4 x E2E_MEASURED, the largest figure measured on the MI355X over these sizes
(profiles/discriminator_wgrad_bench.json), never above 1e-3; the difference from the statement on its own float64
forward is printed and not asserted, since masks flip at pre-activations that round across 0.  The sizes are
discriminator_grad_cases.GPU_SIZES and the hinge case (S = 128, B = 2): S = 32 has maps smaller than a tile, down to 1 x 1 with pad
(1, 2), and reductions of 1 to 4 pixels; 64 and 128 add interior tile edges and more than one partial per layer; at S = 128, B = 2
discriminator 1's conv0 has 128 tiles of its 16384 output pixels for 43 partials (a workgroup walks at least three tiles where there
are three) and its conv1 32 for 11, so the partial count divides neither the tile count nor the pixel count.

The command runs at S = 256, the only size objective.folder_steps' generator takes, on one item."""
import numpy as np
import pytest

from blindshadowremoval_amd import discriminator as host
from blindshadowremoval_amd.weights import BN_EPS, N_LAYER_D, init_discriminator_weights

import discriminator_cases as dcases
import discriminator_grad_cases as gcases
import discriminator_wgrad_cases as cases
import pairs_cases

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
f32 = np.float32
STAGE_BUDGET = 1e-5
E2E_MEASURED = 7.9e-6          # the largest scaled error of a variable's gradient measured on SIZES: S = 128, B = 1 (tools/discriminator_bench.py --wgrad --parity)
E2E_BOUND = min(4 * E2E_MEASURED, 1e-3)
HINGE = (128, 2)
SIZES = gcases.GPU_SIZES + (HINGE,)


@pytest.fixture(scope="module")
def runner():
    from blindshadowremoval_amd import Discriminators
    return Discriminators(0)


@pytest.fixture(scope="module")
def weights():
    return init_discriminator_weights(3)


def to_dev(*arrays):
    dev = torch.device("cuda", 0)
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def device_run(runner, w, gt, con_rgb, mask_sv, raw=False):
    if w is not None:
        runner.load_weights(w)
    res = runner.disc_grad(*to_dev(gt, con_rgb, mask_sv), keep=True, logits=True)
    torch.cuda.synchronize()
    if raw:
        return res
    grads = {k: v.cpu().numpy() for k, v in res[2].items()}
    return {"losses": res[0].cpu().numpy(), "sums": res[1].cpu().numpy(), "grads": grads, "logits": [y.cpu().numpy() for y in res[3]],
            "acts": {k: v.cpu().numpy() for k, v in res[4].items()}, "dtype": f32}


def flat_bytes(res):
    parts = []
    for r in res:
        if isinstance(r, dict):
            r = [r[""]] if "" in r else list(r.values())
        for t in (r if isinstance(r, list) else [r]):
            parts.append(t.cpu().numpy().tobytes())
    return parts


def scaled_error(got, ref):
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / np.abs(ref).max())


@pytest.fixture(scope="module")
def device_results(runner, weights):
    """Inputs, weights, the device's result and its gradient maps, once per size: {(S, B): (arrays, weights, result, maps)}."""
    out = {}
    for S, B in SIZES:
        if (S, B) == HINGE:
            w, *arrays = dcases.hinge_case()
        else:
            w, arrays = weights, host.example_inputs(S, B, 1)
        res = device_run(runner, w, *arrays)
        maps = {k: v.cpu().numpy() for k, v in runner.wgrad_maps(B, S).items()}
        out[(S, B)] = (arrays, w, res, maps)
    return out


@pytest.mark.parametrize("check", cases.CONSTRUCTED, ids=lambda c: c.__name__)
def test_constructed_case(runner, check):
    check(lambda *a: device_run(runner, *a))


@pytest.mark.parametrize("S,B", SIZES)
def test_stage_by_stage(device_results, S, B):
    arrays, w, res, maps = device_results[(S, B)]
    acts, grads = res["acts"], res["grads"]
    worst = {}

    def hold(what, got, want):
        got, want = np.asarray(got), np.asarray(want)
        assert got.shape == want.shape, what
        e = scaled_error(got, want)
        kind = what.split(" ")[-1]
        worst[kind] = max(worst.get(kind, 0.0), e)
        print("discriminator wgrad S=%d B=%d %s fed the device's input: scaled error %.3g" % (S, B, what, e))
        assert e <= STAGE_BUDGET, (what, e)

    for k, w_k in zip((1, 2, 3), host.seed_weights(B, S)):
        sides = host.map_sides(S, k)
        head_st = "discriminator_%d/conv2/conv/" % k
        # launch 1: the seed from the device's logits, bit for bit; the head's input gradient and conv3's slope
        seed = host.hinge_seed(res["logits"][k - 1], B, w_k)
        assert maps["d%d/out" % k].tobytes() == seed.astype(f32).tobytes()
        assert acts["d%d/out" % k][..., 0].tobytes() == res["logits"][k - 1].tobytes()
        seed_dev = maps["d%d/out" % k]
        want = host.leaky_grad(host.conv2d_same_dgrad(seed_dev, w[head_st + "kernel"], 1, sides[N_LAYER_D]), acts["d%d/conv3" % k])
        hold("d%d launch 1 head dgrad" % k, maps["d%d/conv3" % k], want)
        # launches 2 and 11: the head's kernel and bias gradients
        hold("d%d launches 2, 11 head kernel" % k, grads[head_st + "kernel"], host.conv2d_same_wgrad(acts["d%d/conv3" % k], seed_dev, 1))
        assert grads[head_st + "bias"].tobytes() == np.asarray(seed_dev, np.float64).sum(axis=(0, 1, 2)).astype(f32).tobytes()
        for i in reversed(range(N_LAYER_D)):
            st = "discriminator_%d/conv_stack/%d/" % (k, i)
            gz = maps["d%d/conv%d" % (k, i)].astype(np.float64)
            inv = host.bn_inv(w, k, i)
            x = acts["d%d/in" % k] if i == 0 else acts["d%d/conv%d" % (k, i - 1)]
            # the kernel-gradient launch of the layer and the fold
            hold("d%d conv%d kernel" % (k, i), grads[st + "conv/kernel"], host.conv2d_same_wgrad(x, gz, 2) * inv)
            # the finishing launch
            total = gz.sum(axis=(0, 1, 2))
            mean, var = (np.asarray(w[st + "bnorm/" + p], np.float64) for p in ("moving_mean", "moving_variance"))
            c = host.conv2d_same(x, w[st + "conv/kernel"], w[st + "conv/bias"], 2)
            hold("d%d conv%d beta" % (k, i), grads[st + "bnorm/beta"], total)
            hold("d%d conv%d bias" % (k, i), grads[st + "conv/bias"], inv * total)
            hold("d%d conv%d gamma" % (k, i), grads[st + "bnorm/gamma"], (gz * ((c - mean) / np.sqrt(var + BN_EPS))).sum(axis=(0, 1, 2)))
            # the data-gradient launch to the layer below
            if i > 0:
                want = host.leaky_grad(host.conv2d_same_dgrad(gz * inv, w[st + "conv/kernel"], 2, sides[i]), acts["d%d/conv%d" % (k, i - 1)])
                hold("d%d conv%d dgrad" % (k, i), maps["d%d/conv%d" % (k, i - 1)], want)
    print("discriminator wgrad S=%d B=%d: worst stage figures %s" % (S, B, ", ".join("%s %.3g" % kv for kv in sorted(worst.items()))))


@pytest.mark.parametrize("S,B", SIZES)
def test_end_to_end(device_results, S, B):
    arrays, w, res, _ = device_results[(S, B)]
    ref = host.disc_grad(w, *arrays, acts=res["acts"], logits=res["logits"])
    e, at = cases.worst_scaled_diff(res["grads"], ref)
    own, own_at = cases.worst_scaled_diff(res["grads"], host.disc_grad(w, *arrays))
    print("discriminator wgrad S=%d B=%d end to end: worst scaled error %.3g at %s on the device's masks (bound %.3g); %.3g at %s against the statement's own float64 forward"
          % (S, B, e, at, E2E_BOUND, own, own_at))
    assert all(res["grads"][n].dtype == np.float32 for n in cases.NAMES) and e <= E2E_BOUND


def test_the_hinge_case_clips_on_the_device(device_results):
    arrays, w, res, maps = device_results[HINGE]
    B = HINGE[1]
    assert dcases.hinge_condition(res["logits"], B)
    for k in (1, 2, 3):
        seed = maps["d%d/out" % k]
        assert (seed[:B] < 0).any() and (seed[:B] == 0).any() and (seed[B:] > 0).any() and (seed[B:] == 0).any()


def test_forward_outputs_are_gan_losses_bytes_and_gen_grad_is_untouched(runner, weights, device_results):
    arrays, _, _, _ = device_results[(64, 2)]
    fresh = type(runner)(0)
    fresh.load_weights(weights)
    t = to_dev(*arrays)
    before = fresh.gen_grad(*t)[2].cpu().numpy().tobytes()                     # before any disc_grad call of this runner
    plain = fresh.gan_losses(*t, logits=True, keep=True)
    torch.cuda.synchronize()
    both = fresh.disc_grad(*t, keep=True, logits=True)
    torch.cuda.synchronize()
    assert flat_bytes(plain) == flat_bytes((both[0], both[1], both[3], both[4])) and len(flat_bytes(plain)) == 2 + 3 + 18
    assert fresh.gen_grad(*t)[2].cpu().numpy().tobytes() == before


def test_repeated_calls_give_identical_bytes_and_a_second_batch_size_is_correct(runner, weights, device_results):
    arrays3, _, res3, _ = device_results[(32, 3)]
    first = flat_bytes(device_run(runner, weights, *arrays3, raw=True)[:3])
    second = flat_bytes(device_run(runner, None, *arrays3, raw=True)[:3])      # the same object: the same scratch, the same blobs
    assert first == second and len(first) == 3 and first[2] == res3["grads"][""].tobytes()
    arrays1, _, res1, _ = device_results[(32, 1)]
    got = device_run(runner, None, *arrays1)                                   # B = 1 after B = 3 on the same scratch
    assert got["grads"][""].tobytes() == res1["grads"][""].tobytes() and got["losses"].tobytes() == res1["losses"].tobytes()
    assert flat_bytes(device_run(runner, None, *arrays3, raw=True)[:3]) == first


def test_the_views_are_the_flat_buffer(runner, weights, device_results):
    from blindshadowremoval_amd import _lib
    from blindshadowremoval_amd.weights import discriminator_variable_shapes
    arrays, _, _, _ = device_results[(32, 1)]
    runner.load_weights(weights)
    grads = runner.disc_grad(*to_dev(*arrays))[2]
    lib, shapes = _lib.load(), discriminator_variable_shapes()
    assert grads[""].numel() == lib.bsr_disc_wgrad_floats() == sum(int(np.prod(shapes[n])) for n in cases.NAMES) and len(grads) == 55
    for index, name in enumerate(cases.NAMES):
        assert tuple(grads[name].shape) == shapes[name]
        assert grads[name].data_ptr() == grads[""].data_ptr() + 4 * lib.bsr_disc_wgrad_var_offset(index)


def test_the_debug_entry_stops_after_the_given_launches(runner, weights, device_results):
    from blindshadowremoval_amd import _lib
    from blindshadowremoval_amd.discriminator_gpu import WGRAD_LAUNCHES
    arrays, _, res, maps = device_results[(32, 1)]
    assert len(WGRAD_LAUNCHES) == 11
    runner.load_weights(weights)
    t = to_dev(*arrays)
    base = runner.scratch(1, 32, runner.WGRAD_SCRATCH_QUERY) - runner._scratch.data_ptr()
    written = {1: ("out", "conv3"), 4: ("conv2",), 6: ("conv1",), 8: ("conv0",)}                 # launch -> the maps it writes
    for stop in (0, 1, 5, 10, 11):
        runner._scratch[base + int(_lib.load().bsr_disc_losses_scratch_bytes(1, 32)):].zero_()
        got = {n: v.cpu().numpy() for n, v in runner.wgrad_stages(*t, stop_after=stop).items()}
        for launch, names in written.items():
            for k in (1, 2, 3):
                for name in names:
                    n = "d%d/%s" % (k, name)
                    if launch <= stop:
                        assert got[n].tobytes() == maps[n].tobytes(), (stop, n)
                    else:
                        assert not got[n].any(), (stop, n)
        views = {n: v.cpu().numpy() for n, v in runner.split_grads(torch.from_numpy(got[""])).items()}
        for n in cases.NAMES:                                                   # the fold writes the twelve kernels, the finish the rest
            if stop >= (10 if n.endswith("/kernel") and "/conv_stack/" in n else 11):
                assert views[n].tobytes() == res["grads"][n].tobytes(), (stop, n)
            else:
                assert not views[n].any(), (stop, n)
    with pytest.raises(ValueError, match="stop_after"):
        runner.wgrad_stages(*t, stop_after=12)


def test_the_chain_is_captured_into_a_graph_and_replays_the_same_bytes(runner, weights, device_results):
    """Stream capture refuses a host synchronisation and work on another stream that is not joined: a call that is captured, replayed
    and gives the eager call's bytes has neither.  The chain is a line of launches: the captured graph has no branches."""
    arrays, _, _, _ = device_results[(64, 2)]
    eager = flat_bytes(device_run(runner, weights, *arrays, raw=True)[:3])
    t = to_dev(*arrays)
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        runner.disc_grad(*t)
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=side):
            res = runner.disc_grad(*t)
    torch.cuda.current_stream().wait_stream(side)
    res[0].zero_(), res[1].zero_(), res[2][""].zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert flat_bytes(res) == eager


def test_argument_errors_raise_before_any_launch(runner, weights):
    from blindshadowremoval_amd import Discriminators, _lib, pack
    dev = torch.device("cuda", 0)
    runner.load_weights(weights)
    ok = [torch.from_numpy(a).to(dev) for a in host.example_inputs(32, 1, 0)]
    with pytest.raises(ValueError, match="32, 64, 128 or 256"):
        runner.disc_grad(*(torch.zeros((1, 48, 48, 3), device=dev) for _ in range(3)))
    with pytest.raises(ValueError, match="1..32767"):
        runner.disc_grad(*(torch.zeros((0, 32, 32, 3), device=dev) for _ in range(3)))
    with pytest.raises(ValueError, match="contiguous"):
        runner.disc_grad(ok[0], torch.zeros((1, 32, 32, 6), device=dev)[..., ::2], ok[2])
    with pytest.raises(ValueError, match="mask_sv must be"):
        runner.disc_grad(ok[0], ok[1], ok[2][:, :16].contiguous())
    with pytest.raises(TypeError):
        runner.disc_grad(ok[0].double(), ok[1], ok[2])
    with pytest.raises(TypeError):
        runner.disc_grad(ok[0].cpu(), ok[1], ok[2])
    with pytest.raises(ValueError, match="no weights"):
        Discriminators(0).disc_grad(*ok)
    forward_only = Discriminators(0)
    forward_only.load_weights(weights)
    forward_only.load_blob(pack.pack_discriminators(weights))
    forward_only.gan_losses(*ok)                                               # load_blob keeps its meaning: the forward's weights alone
    for call in (forward_only.disc_grad, forward_only.gen_grad):
        with pytest.raises(ValueError, match="no weights"):
            call(*ok)
    lib = _lib.load()
    assert lib.bsr_disc_wgrad_scratch_bytes(1, 48) == 0 and lib.bsr_disc_wgrad_scratch_bytes(32768, 32) == 0 and lib.bsr_disc_wgrad_scratch_bytes(0, 32) == 0
    assert lib.bsr_disc_wgrad_offset(1, 32, 1, 1) == lib.bsr_disc_losses_scratch_bytes(1, 32)
    assert lib.bsr_disc_wgrad_offset(1, 32, 0, 1) == lib.bsr_disc_wgrad_offset(1, 32, 4, 1) == lib.bsr_disc_wgrad_offset(1, 32, 1, 0) == 2 ** 64 - 1
    assert lib.bsr_disc_wgrad_offset(1, 32, 1, 6) == lib.bsr_disc_wgrad_var_offset(-1) == lib.bsr_disc_wgrad_var_offset(54) == 2 ** 64 - 1
    assert lib.bsr_disc_wgrad_var_offset(0) == 0 and lib.bsr_disc_wgrad_var_offset(1) == 16 * 6 * 32
    assert lib.bsr_disc_wgrad_scratch_bytes(2, 64) > lib.bsr_disc_grad_scratch_bytes(2, 64)
    nbytes, dbytes, wbytes = lib.bsr_disc_blob_bytes(), lib.bsr_disc_dgrad_blob_bytes(), lib.bsr_disc_wgrad_blob_bytes()
    assert wbytes == len(pack.pack_discriminators_wgrad(weights))
    n_grads = lib.bsr_disc_wgrad_floats()
    assert lib.bsr_disc_wgrad(0, None, nbytes, None, dbytes, None, wbytes, None, None, None, 1, 32, None, None, None, None, None, None) == 1
    assert b"bsr_disc_wgrad" in lib.bsr_last_error()
    blobs = [torch.zeros(n, dtype=torch.uint8, device=dev) for n in (nbytes, dbytes, wbytes)]
    b0, b1, b2 = (b.data_ptr() for b in blobs)
    p = [t.data_ptr() for t in ok]
    sums, losses, grads = torch.zeros((1, host.K), dtype=torch.float64, device=dev), torch.zeros(3, device=dev), torch.zeros(n_grads, device=dev)
    scratch = torch.zeros(lib.bsr_disc_wgrad_scratch_bytes(1, 32) + 512, dtype=torch.uint8, device=dev)
    base = scratch.data_ptr() + (-scratch.data_ptr()) % 256
    for nb, db, wb, b, s, sc in ((nbytes, dbytes, wbytes, 1, 48, base), (nbytes, dbytes, wbytes, 0, 32, base), (nbytes, dbytes, wbytes, 32768, 32, base),
                                 (nbytes, dbytes, wbytes, 1, 32, base + 8), (nbytes - 4, dbytes, wbytes, 1, 32, base), (nbytes, dbytes - 4, wbytes, 1, 32, base),
                                 (nbytes, dbytes, wbytes - 4, 1, 32, base)):
        assert lib.bsr_disc_wgrad(0, b0, nb, b1, db, b2, wb, *p, b, s, sums.data_ptr(), losses.data_ptr(), None, grads.data_ptr(), sc, None) == 1
    assert lib.bsr_disc_wgrad(0, b0, nbytes, b1, dbytes, b2 + 4, wbytes, *p, 1, 32, sums.data_ptr(), losses.data_ptr(), None, grads.data_ptr(), base, None) == 1
    assert lib.bsr_debug_disc_wgrad(0, b0, nbytes, b1, dbytes, b2, wbytes, *p, 1, 32, sums.data_ptr(), losses.data_ptr(), None, grads.data_ptr(), base, 12,
                                    None) == 1
    assert b"stop_after must be 0..11" in lib.bsr_last_error()
    torch.cuda.synchronize()
    assert not sums.any() and not losses.any() and not grads.any() and not scratch.any()          # nothing was launched


def test_command_wgrad_device_route_matches_the_host_route(tmp_path, capsys):
    folder = pairs_cases.write_pairs(tmp_path)
    printed = []
    for extra in ([], ["--host"]):
        assert host.main([folder, "--batch", "1", "--wgrad"] + extra) == 0
        lines = capsys.readouterr().out.strip().split("\n")
        assert len(lines) == 2 and lines[0].startswith("Testing 1/1: ")
        fields = dict(f.split(":") for f in lines[1].split(", "))
        assert tuple(fields) == host.LOSS_NAMES + host.WGRAD_NAMES
        printed.append({k: float(v) for k, v in fields.items()})
    dev_route, host_route = printed
    print("discriminator command --wgrad: device %s\ndiscriminator command --wgrad: host %s" % (dev_route, host_route))
    # the end-to-end tolerance, E2E_BOUND of a variable's largest magnitude per element and so at most of the L-infinity norm over all 54:
    # the L-infinity norm moves by at most that, the L1 norm by at most that for each of its elements
    from blindshadowremoval_amd import _lib
    n, linf = int(_lib.load().bsr_disc_wgrad_floats()), host_route["d_grad_linf"]
    d_linf, d_l1 = abs(dev_route["d_grad_linf"] - linf), abs(dev_route["d_grad_l1"] - host_route["d_grad_l1"])
    print("discriminator command --wgrad: |device - host| linf %.3g (bound %.3g), l1 %.3g (bound %.3g)" % (d_linf, E2E_BOUND * linf, d_l1, E2E_BOUND * n * linf))
    assert linf > 0 and host_route["d_grad_l1"] > linf
    assert d_linf <= E2E_BOUND * linf and d_l1 <= E2E_BOUND * n * linf
