"""bsr_disc_gen_grad (csrc/disc_grad_kernels.h) against the host statement blindshadowremoval_amd/discriminator.py: gen_grad.

The constructed cases bit for bit (discriminator_grad_cases: every sum has at most one term that is not 0, so the closed forms hold in
float32 as in float64).  Stage by stage: each of the chain's six backward launches, fed the DEVICE's own incoming gradient and the
device's own kept activations, against the float64 statement of that launch alone — the head kernel's tap sums and slopes and the four
gradient convolutions within max|got - ref| / max|ref| <= 1e-5, the project's fp32-class stage budget (tests/stage_parity.py), positions
that receive no head tap exactly 0, the gather bit for bit against its float32 statement.  End to end: grad against gen_grad(acts =
the device's activations) within 4 x E2E_MEASURED on the scale of the largest magnitude, the largest figure measured on the MI355X
over these sizes (profiles/discriminator_grad_bench.json), never above 1e-3; the difference from the statement on
its own float64 forward is printed and not asserted, since masks flip at pre-activations that round across 0.

The command runs at S = 256, the only size objective.folder_steps' generator takes, on one item."""
import numpy as np
import pytest

from blindshadowremoval_amd import discriminator as host
from blindshadowremoval_amd.weights import N_LAYER_D, init_discriminator_weights

import discriminator_grad_cases as gcases
import pairs_cases

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
f32 = np.float32
STAGE_BUDGET = 1e-5
E2E_BOUND = gcases.E2E_BOUND


@pytest.fixture(scope="module")
def runner():
    from blindshadowremoval_amd import Discriminators
    return Discriminators(0)


@pytest.fixture(scope="module")
def weights():
    return init_discriminator_weights(3)


def to_dev(*arrays):
    dev = torch.device("cuda", 0)
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def device_run(runner, w, gt, con_rgb, mask_sv, upstream=None, keep=True, raw=False):
    if w is not None:
        runner.load_weights(w)
    up = None if upstream is None else np.asarray(upstream, f32).reshape(1)
    res = runner.gen_grad(*to_dev(gt, con_rgb, mask_sv, up), keep=keep)
    torch.cuda.synchronize()
    if raw:
        return res
    out = {"losses": res[0].cpu().numpy(), "sums": res[1].cpu().numpy(), "grad": res[2].cpu().numpy(), "dtype": f32}
    if keep:
        out["acts"] = {k: v.cpu().numpy() for k, v in res[3].items()}
    return out


def flat_bytes(res):
    parts = []
    for r in res:
        for t in (r.values() if isinstance(r, dict) else [r]):
            parts.append(t.cpu().numpy().tobytes())
    return parts


def scaled_error(got, ref):
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / np.abs(ref).max())


@pytest.fixture(scope="module")
def device_results(runner, weights):
    """Inputs, the device's result with its activations and its gradient maps, once per size: {(S, B): (arrays, result, maps)}."""
    out = {}
    for S, B in gcases.GPU_SIZES:
        arrays = host.example_inputs(S, B, 1)
        res = device_run(runner, weights, *arrays)
        maps = {k: v.cpu().numpy() for k, v in runner.gradients(B, S).items()}
        out[(S, B)] = (arrays, res, maps)
    return out


@pytest.mark.parametrize("check", gcases.CONSTRUCTED, ids=lambda c: c.__name__)
def test_constructed_case(runner, check):
    check(lambda *a, **k: device_run(runner, *a, **k))


def gather_f32(maps, S, upstream=None):
    """The gather's float32 statement: ((g_1 + 0.25 g_2) + t_3) * upstream."""
    g1, g2, g3 = (np.asarray(maps["d%d/in" % k], f32) for k in (1, 2, 3))
    up2 = f32(0.25) * np.repeat(np.repeat(g2, 2, axis=1), 2, axis=2)
    t3 = f32(0.25) * np.repeat(np.repeat(g3, 4, axis=1), 4, axis=2)
    mid = np.isin(np.arange(S) % 4, (1, 2))
    t3 = np.where((mid[:, None] & mid[None, :])[None, :, :, None], t3, f32(0))
    return ((g1 + up2) + t3) * (f32(1) if upstream is None else f32(upstream))


@pytest.mark.parametrize("S,B", gcases.GPU_SIZES)
def test_stage_by_stage(weights, device_results, S, B):
    arrays, res, maps = device_results[(S, B)]
    acts = res["acts"]
    worst = 0.0
    for k, w_k in zip((1, 2, 3), host.seed_weights(B, S)):
        sides = host.map_sides(S, k)
        # launch 1: the head's gradient and conv3's slope, from the constant seed
        seed = np.full((B, sides[-1], sides[-1], 1), -float(w_k))
        taps = host.conv2d_same_dgrad(seed, weights["discriminator_%d/conv2/conv/kernel" % k], 1, sides[N_LAYER_D])
        want = host.leaky_grad(taps, acts["d%d/conv3" % k][B:])
        got = maps["d%d/conv3" % k]
        e = scaled_error(got, want)
        ones = host.conv2d_same_dgrad(np.ones_like(seed), np.ones((4, 4, 1, 1)), 1, sides[N_LAYER_D])[..., 0]       # taps received per position
        assert (ones > 0).all() or not got[ones == 0].any()
        print("discriminator grad S=%d B=%d d%d launch 1 head: scaled error %.3g" % (S, B, k, e))
        assert e <= STAGE_BUDGET
        # launches 2..4: the gradient convolutions with the slope of the layer below; launch 5: conv0's, no slope
        for i in reversed(range(N_LAYER_D)):
            g_in = maps["d%d/conv%d" % (k, i)]
            want = host.conv2d_same_dgrad(g_in * host.bn_inv(weights, k, i), weights["discriminator_%d/conv_stack/%d/conv/kernel" % (k, i)], 2, sides[i])
            if i > 0:
                want = host.leaky_grad(want, acts["d%d/conv%d" % (k, i - 1)][B:])
                got = maps["d%d/conv%d" % (k, i - 1)]
            else:
                want, got = want[..., :3], maps["d%d/in" % k]
            assert got.shape == want.shape
            e = scaled_error(got, want)
            worst = max(worst, e)
            print("discriminator grad S=%d B=%d d%d launch %d conv%d fed the device's input: scaled error %.3g" % (S, B, k, 5 - i, i, e))
            assert e <= STAGE_BUDGET, (k, i, e)
    # launch 6: the gather
    assert res["grad"].tobytes() == gather_f32(maps, S).tobytes()
    print("discriminator grad S=%d B=%d: worst gradient convolution %.3g" % (S, B, worst))
    assert np.abs(res["grad"]).max() > 0


def test_the_head_kernel_leaves_exact_zeros_where_no_tap_arrives(runner, weights):
    """A head kernel with the one tap (0, 0): it is read by the output one down and one right, so the last row and column of conv3's
    map receive nothing."""
    w = {n: v.copy() for n, v in weights.items()}
    for k in (1, 2, 3):
        kern = w["discriminator_%d/conv2/conv/kernel" % k]
        kern[1:] = 0
        kern[:, 1:] = 0
    arrays = host.example_inputs(64, 1, 2)
    runner.load_weights(w)
    maps = {n: v.cpu().numpy() for n, v in runner.grad_stages(*to_dev(*arrays), stop_after=1).items()}
    for k in (1, 2):
        g = maps["d%d/conv3" % k]
        assert not g[:, -1].any() and not g[:, :, -1].any() and np.abs(g[:, :-1, :-1]).min() > 0
    assert not maps["d3/conv3"].any()                                       # 1 x 1: no output reads it at tap (0, 0)


@pytest.mark.parametrize("S,B", gcases.GPU_SIZES)
def test_end_to_end(weights, device_results, S, B):
    arrays, res, _ = device_results[(S, B)]
    ref = host.gen_grad(weights, *arrays, acts=res["acts"])
    e = scaled_error(res["grad"], ref["grad"])
    own = host.gen_grad(weights, *arrays)
    print("discriminator grad S=%d B=%d end to end: scaled error %.3g on the device's masks (bound %.3g); %.3g against the statement's own float64 forward; largest |grad| %.3g"
          % (S, B, e, E2E_BOUND, scaled_error(res["grad"], own["grad"]), np.abs(ref["grad"]).max()))
    assert res["grad"].shape == (B, S, S, 3) and res["grad"].dtype == np.float32 and e <= E2E_BOUND


def test_forward_outputs_are_gan_losses_bytes(runner, weights, device_results):
    arrays, _, _ = device_results[(64, 2)]
    runner.load_weights(weights)
    t = to_dev(*arrays)
    plain = runner.gan_losses(*t, keep=True)
    torch.cuda.synchronize()
    both = runner.gen_grad(*t, keep=True)
    torch.cuda.synchronize()
    assert flat_bytes(plain) == flat_bytes((both[0], both[1], both[3])) and len(flat_bytes(plain)) == 2 + 18


def test_repeated_calls_give_identical_bytes_and_a_second_batch_size_is_correct(runner, weights, device_results):
    arrays3, res3, _ = device_results[(32, 3)]
    first = flat_bytes(device_run(runner, weights, *arrays3, keep=False, raw=True))
    second = flat_bytes(device_run(runner, None, *arrays3, keep=False, raw=True))          # the same object: the same scratch, the same blobs
    assert first == second and len(first) == 3 and first[2] == res3["grad"].tobytes()
    arrays1, res1, _ = device_results[(32, 1)]
    got = device_run(runner, None, *arrays1, keep=False)                                    # B = 1 after B = 3 on the same scratch
    assert got["grad"].tobytes() == res1["grad"].tobytes() and got["losses"].tobytes() == res1["losses"].tobytes()
    assert flat_bytes(device_run(runner, None, *arrays3, keep=False, raw=True)) == first


def test_upstream_none_is_a_tensor_of_one(runner, weights, device_results):
    arrays, res, maps = device_results[(32, 3)]
    got = device_run(runner, weights, *arrays, upstream=np.ones(1, f32), keep=False)["grad"]
    assert got.tobytes() == res["grad"].tobytes()
    scaled = device_run(runner, None, *arrays, upstream=np.array([0.005], f32), keep=False)["grad"]
    assert scaled.tobytes() == gather_f32(maps, 32, upstream=0.005).tobytes()


def test_the_debug_entry_stops_after_the_given_launches(runner, weights, device_results):
    from blindshadowremoval_amd import _lib
    from blindshadowremoval_amd.discriminator_gpu import GRAD_LAUNCHES
    arrays, res, maps = device_results[(32, 1)]
    assert len(GRAD_LAUNCHES) == 6
    runner.load_weights(weights)
    t = to_dev(*arrays)
    base = runner.scratch(1, 32, grad=True) - runner._scratch.data_ptr()
    for stop in (0, 3, 6):
        runner._scratch[base + int(_lib.load().bsr_disc_losses_scratch_bytes(1, 32)):].zero_()
        got = {n: v.cpu().numpy() for n, v in runner.grad_stages(*t, stop_after=stop).items()}
        for j, (_, name) in enumerate(GRAD_LAUNCHES[:5]):
            for k in (1, 2, 3):
                n = "d%d/%s" % (k, name)
                if j < stop:
                    assert got[n].tobytes() == maps[n].tobytes(), (stop, n)
                else:
                    assert not got[n].any(), (stop, n)
    with pytest.raises(ValueError, match="stop_after"):
        runner.grad_stages(*t, stop_after=7)


def test_the_chain_is_captured_into_a_graph_and_replays_the_same_bytes(runner, weights, device_results):
    """Stream capture refuses a host synchronisation and work on another stream that is not joined: a call that is captured, replayed
    and gives the eager call's bytes has neither.  The chain is a line of launches: the captured graph has no branches."""
    arrays, _, _ = device_results[(64, 2)]
    eager = flat_bytes(device_run(runner, weights, *arrays, keep=False, raw=True))
    t = to_dev(*arrays)
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        runner.gen_grad(*t)
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=side):
            res = runner.gen_grad(*t)
    torch.cuda.current_stream().wait_stream(side)
    for r in res:
        r.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert flat_bytes(res) == eager


def test_autograd_door(runner, weights, device_results):
    arrays, res, _ = device_results[(32, 3)]
    runner.load_weights(weights)
    gt, con, mask = to_dev(*arrays)
    con.requires_grad_()
    loss = runner.gen_loss(gt, con, mask)
    assert loss.shape == () and loss.grad_fn is not None and loss.detach().cpu().numpy().tobytes() == res["losses"][:1].tobytes()
    loss.backward()
    assert gt.grad is None and mask.grad is None and con.grad.cpu().numpy().tobytes() == res["grad"].tobytes()
    con.grad = None
    (2 * runner.gen_loss(gt, con, mask)).backward()
    scaled = device_run(runner, None, *arrays, upstream=np.array([2.0], f32), keep=False)["grad"]
    assert con.grad.cpu().numpy().tobytes() == scaled.tobytes()
    plain = runner.gen_loss(gt, con.detach(), mask)                                        # nothing to differentiate: the forward alone
    assert not plain.requires_grad and plain.cpu().numpy().tobytes() == res["losses"][:1].tobytes()


def test_argument_errors_raise_before_any_launch(runner, weights):
    from blindshadowremoval_amd import Discriminators, _lib, pack
    dev = torch.device("cuda", 0)
    runner.load_weights(weights)
    ok = [torch.from_numpy(a).to(dev) for a in host.example_inputs(32, 1, 0)]
    with pytest.raises(ValueError, match="32, 64, 128 or 256"):
        runner.gen_grad(*(torch.zeros((1, 48, 48, 3), device=dev) for _ in range(3)))
    with pytest.raises(ValueError, match="1..32767"):
        runner.gen_grad(*(torch.zeros((0, 32, 32, 3), device=dev) for _ in range(3)))
    with pytest.raises(ValueError, match="contiguous"):
        runner.gen_grad(ok[0], torch.zeros((1, 32, 32, 6), device=dev)[..., ::2], ok[2])
    with pytest.raises(ValueError, match="mask_sv must be"):
        runner.gen_grad(ok[0], ok[1], ok[2][:, :16].contiguous())
    with pytest.raises(TypeError):
        runner.gen_grad(ok[0].double(), ok[1], ok[2])
    with pytest.raises(TypeError):
        runner.gen_grad(ok[0].cpu(), ok[1], ok[2])
    for bad in (torch.ones(1, dtype=torch.float64, device=dev), torch.ones(2, device=dev), torch.ones(1), 0.005):
        with pytest.raises(TypeError, match="upstream"):
            runner.gen_grad(*ok, upstream=bad)
    with pytest.raises(ValueError, match="no weights"):
        Discriminators(0).gen_grad(*ok)
    forward_only = Discriminators(0)
    forward_only.load_blob(pack.pack_discriminators(weights))
    forward_only.gan_losses(*ok)                                               # load_blob keeps its meaning
    with pytest.raises(ValueError, match="no weights"):
        forward_only.gen_grad(*ok)
    lib = _lib.load()
    assert lib.bsr_disc_grad_scratch_bytes(1, 48) == 0 and lib.bsr_disc_grad_scratch_bytes(32768, 32) == 0 and lib.bsr_disc_grad_scratch_bytes(0, 32) == 0
    assert lib.bsr_disc_grad_offset(1, 32, 1, 0) == lib.bsr_disc_losses_scratch_bytes(1, 32)
    assert lib.bsr_disc_grad_offset(1, 32, 0, 0) == lib.bsr_disc_grad_offset(1, 32, 4, 0) == lib.bsr_disc_grad_offset(1, 32, 1, 5) == 2 ** 64 - 1
    assert lib.bsr_disc_grad_scratch_bytes(2, 64) > lib.bsr_disc_losses_scratch_bytes(2, 64)
    nbytes, dbytes = lib.bsr_disc_blob_bytes(), lib.bsr_disc_dgrad_blob_bytes()
    assert dbytes == 1_394_688 == len(pack.pack_discriminators_dgrad(weights))
    assert lib.bsr_disc_gen_grad(0, None, nbytes, None, dbytes, None, None, None, None, 1, 32, None, None, None, None, None, None) == 1
    assert b"bsr_disc_gen_grad" in lib.bsr_last_error()
    blob, dblob = torch.zeros(nbytes, dtype=torch.uint8, device=dev), torch.zeros(dbytes, dtype=torch.uint8, device=dev)
    p = [t.data_ptr() for t in ok]
    sums, losses, grad = torch.zeros((1, host.K), dtype=torch.float64, device=dev), torch.zeros(3, device=dev), torch.zeros((1, 32, 32, 3), device=dev)
    scratch = torch.zeros(lib.bsr_disc_grad_scratch_bytes(1, 32) + 512, dtype=torch.uint8, device=dev)
    base = scratch.data_ptr() + (-scratch.data_ptr()) % 256
    for nb, db, b, s, sc in ((nbytes, dbytes, 1, 48, base), (nbytes, dbytes, 0, 32, base), (nbytes, dbytes, 32768, 32, base), (nbytes, dbytes, 1, 32, base + 8),
                             (nbytes - 4, dbytes, 1, 32, base), (nbytes, dbytes - 4, 1, 32, base)):
        assert lib.bsr_disc_gen_grad(0, blob.data_ptr(), nb, dblob.data_ptr(), db, *p, None, b, s, sums.data_ptr(), losses.data_ptr(), None, grad.data_ptr(), sc,
                                     None) == 1
    assert lib.bsr_debug_disc_gen_grad(0, blob.data_ptr(), nbytes, dblob.data_ptr(), dbytes, *p, None, 1, 32, sums.data_ptr(), losses.data_ptr(), None,
                                       grad.data_ptr(), base, 7, None) == 1
    torch.cuda.synchronize()
    assert not sums.any() and not losses.any() and not grad.any() and not scratch.any()          # nothing was launched


def test_command_grad_device_route_matches_the_host_route(tmp_path, capsys):
    folder = pairs_cases.write_pairs(tmp_path)
    printed = []
    for extra in ([], ["--host"]):
        assert host.main([folder, "--batch", "1", "--grad"] + extra) == 0
        lines = capsys.readouterr().out.strip().split("\n")
        assert len(lines) == 2 and lines[0].startswith("Testing 1/1: ")
        names = tuple(f.split(":")[0] for f in lines[0][len("Testing 1/1: "):].split(", ") if ":" in f)
        fields = dict(f.split(":") for f in lines[1].split(", "))                 # one step: its means are the step's values, at nine digits
        assert names == tuple(fields) == host.LOSS_NAMES + host.GRAD_NAMES
        printed.append({k: float(v) for k, v in fields.items()})
    assert host.main([folder, "--batch", "1"]) == 0                              # without --grad the lines are what they were
    lines = capsys.readouterr().out.strip().split("\n")
    assert tuple(dict(f.split(":") for f in lines[1].split(", "))) == host.LOSS_NAMES
    dev_route, host_route = printed
    print("discriminator command --grad: device %s\ndiscriminator command --grad: host %s" % (dev_route, host_route))
    # the end-to-end tolerance, E2E_BOUND of the largest magnitude per element: the L-infinity norm moves by at most that, the L1 norm
    # by at most that for each of its S * S * 3 elements
    n, linf = pairs_cases.S * pairs_cases.S * 3, host_route["gen_grad_linf"]
    d_linf, d_l1 = abs(dev_route["gen_grad_linf"] - linf), abs(dev_route["gen_grad_l1"] - host_route["gen_grad_l1"])
    print("discriminator command --grad: |device - host| linf %.3g (bound %.3g), l1 %.3g (bound %.3g)" % (d_linf, E2E_BOUND * linf, d_l1, E2E_BOUND * n * linf))
    assert linf > 0 and host_route["gen_grad_l1"] > linf
    assert d_linf <= E2E_BOUND * linf and d_l1 <= E2E_BOUND * n * linf
