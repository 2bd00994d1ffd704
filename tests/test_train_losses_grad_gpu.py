"""bsr_train_losses_grad (csrc/train_losses_kernels.h) against the host statement train_losses.step_losses_grad.

losses and sums are step_losses' bytes.  grad_gs and d_recon_c are formed in float64 in the statement's order from signs of the same
float32 differences: bit for bit.  Stage by stage: each map g_l left in the scratch against the statement's g_l, and d_grad against the
statement's last two steps fed the DEVICE's own maps, within max|got - ref| / max|ref| <= 1e-5, the project's fp32-class stage budget
(tests/stage_parity.py), with no position excluded.  End to end: grad_con against the statement within min(4 x E2E_MEASURED, 1e-4),
E2E_MEASURED the largest scaled error seen on the MI355X over these sizes (profiles/train_losses_grad_bench.json).

Figures of the MI355X (scaled errors): g_l at most 4.9e-8 (the float32 rounding of a float64 sum), d_grad fed the device's maps at most
5.2e-8, grad_con end to end at most 8.3e-8 (S = 32, B = 3), so the bound is 3.3e-7.

The commands run at S = 256, the only size objective.folder_steps' generator takes, on one item."""
import numpy as np
import pytest

from blindshadowremoval_amd import train_losses as host

import train_losses_grad_cases as cases
import pairs_cases

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
f32 = np.float32
STAGE_BUDGET = 1e-5
E2E_BOUND = cases.E2E_BOUND
NAMES = ("losses", "sums", "grad_gs", "grad_con", "d_recon_c", "d_grad")


@pytest.fixture(scope="module")
def runner():
    from blindshadowremoval_amd import TrainLosses
    return TrainLosses(0)


def to_dev(*arrays):
    dev = torch.device("cuda", 0)
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def device_run(runner, img, gt, mask_sv, gs, con_rgb, upstream=None, parts=True, maps=True):
    up = None if upstream is None else np.asarray(upstream, f32)
    res = runner.step_losses_grad(*to_dev(img, gt, mask_sv, gs, con_rgb, up), parts=parts)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in zip(NAMES, res)}
    if maps:
        out.update({k: v.cpu().numpy() for k, v in runner.gradients(gt.shape[0], gt.shape[1]).items()})
    return out


def scaled_error(got, ref):
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / np.abs(ref).max())


@pytest.fixture(scope="module")
def results(runner):
    """Inputs, the device's result with its maps and the statement's, once per size: {(S, B): (arrays, device, statement)}."""
    out = {}
    for S, B in cases.GPU_SIZES:
        arrays = host.example_inputs(S, B, 1)
        up = np.array(host.G_TOTAL_WEIGHTS, f32)
        out[(S, B)] = (arrays, device_run(runner, *arrays, upstream=up), host.step_losses_grad(*arrays, upstream=up))
    return out


@pytest.mark.parametrize("S,B", cases.GPU_SIZES)
def test_forward_outputs_are_step_losses_bytes(runner, results, S, B):
    arrays, dev, ref = results[(S, B)]
    plain = runner.step_losses(*to_dev(*arrays))
    torch.cuda.synchronize()
    assert plain[0].cpu().numpy().tobytes() == dev["losses"].tobytes() and plain[1].cpu().numpy().tobytes() == dev["sums"].tobytes()
    assert dev["sums"].shape == (B, host.K) and dev["losses"].tobytes() == host.losses_from_sums(dev["sums"], S).tobytes()


@pytest.mark.parametrize("S,B", cases.GPU_SIZES)
def test_pointwise_gradients_bit_for_bit(results, S, B):
    arrays, dev, ref = results[(S, B)]
    assert dev["sums"][:, [host.IDX["n_bi"], host.IDX["n_edge"]]].tobytes() == ref["sums"][:, [host.IDX["n_bi"], host.IDX["n_edge"]]].tobytes()
    for name in ("grad_gs", "d_recon_c"):
        assert dev[name].dtype == f32 and dev[name].shape == ref[name].shape and np.abs(ref[name]).max() > 0
        assert dev[name].tobytes() == ref[name].tobytes(), name


@pytest.mark.parametrize("S,B", cases.GPU_SIZES)
def test_stage_by_stage(results, S, B):
    arrays, dev, ref = results[(S, B)]
    for l in range(5):
        got, want = dev["g%d" % l], ref["g%d" % l]
        assert got.shape == want.shape == (B, S >> l, S >> l, 3)
        e = scaled_error(got, want)
        print("train_losses grad S=%d B=%d g%d: scaled error %.3g over all %d positions (0 excluded), largest %.3g" % (S, B, l, e, got.size, np.abs(want).max()))
        assert e <= STAGE_BUDGET, (l, e)
    want = host.d_grad_from_maps([dev["g%d" % l] for l in range(5)], host.G_TOTAL_WEIGHTS[2])
    e = scaled_error(dev["d_grad"], want)
    print("train_losses grad S=%d B=%d d_grad fed the device's maps: scaled error %.3g over all %d positions (0 excluded)" % (S, B, e, want.size))
    assert e <= STAGE_BUDGET


@pytest.mark.parametrize("S,B", cases.GPU_SIZES)
def test_end_to_end(results, S, B):
    arrays, dev, ref = results[(S, B)]
    e = scaled_error(dev["grad_con"], ref["grad_con"])
    print("train_losses grad S=%d B=%d end to end: grad_con scaled error %.3g (bound %.3g), d_grad %.3g; largest |grad_con| %.3g"
          % (S, B, e, E2E_BOUND, scaled_error(dev["d_grad"], ref["d_grad"]), np.abs(ref["grad_con"]).max()))
    assert dev["grad_con"].shape == (B, S, S, 3) and dev["grad_con"].dtype == f32 and e <= E2E_BOUND


@pytest.mark.parametrize("check", cases.CONSTRUCTED, ids=lambda c: c.__name__)
def test_constructed_case(runner, check):
    check(lambda *a, **k: device_run(runner, *a, **k))


def test_repeated_calls_and_changing_sizes_on_one_runner(runner, results):
    """Two calls give the same bytes; one runner across (B, S) growing and shrinking gives each size's bytes again."""
    def raw(key):
        arrays = results[key][0]
        d = device_run(runner, *arrays, upstream=np.array(host.G_TOTAL_WEIGHTS, f32))
        return [d[k].tobytes() for k in NAMES + tuple("g%d" % l for l in range(5))]
    first = raw((32, 3))
    assert raw((32, 3)) == first
    for key in ((32, 1), (64, 2), (256, 1), (32, 3), (64, 2), (32, 1)):
        got, (_, dev, _) = raw(key), results[key]
        assert got == [dev[k].tobytes() for k in NAMES + tuple("g%d" % l for l in range(5))], key


def test_parts_false_gives_the_same_tensors(runner, results):
    arrays, dev, _ = results[(64, 2)]
    res = runner.step_losses_grad(*to_dev(*arrays, np.array(host.G_TOTAL_WEIGHTS, f32)))
    torch.cuda.synchronize()
    assert len(res) == 4 and [r.cpu().numpy().tobytes() for r in res] == [dev[k].tobytes() for k in NAMES[:4]]


def test_upstream_none_is_ones(runner, results):
    arrays = results[(32, 3)][0]
    a, b = device_run(runner, *arrays), device_run(runner, *arrays, upstream=np.ones(3, f32))
    ref = host.step_losses_grad(*arrays)
    assert all(a[k].tobytes() == b[k].tobytes() for k in NAMES)
    assert a["grad_gs"].tobytes() == ref["grad_gs"].tobytes() and scaled_error(a["grad_con"], ref["grad_con"]) <= E2E_BOUND


def test_autograd_door(runner, results):
    arrays, dev, _ = results[(32, 3)]
    t = to_dev(*arrays)
    t[3].requires_grad_()
    t[4].requires_grad_()
    loss = runner.loss(*t)
    w = [f32(x) for x in host.G_TOTAL_WEIGHTS]
    assert loss.shape == () and loss.dtype == torch.float32 and loss.grad_fn is not None
    assert loss.detach().cpu().numpy().tobytes() == f32((w[0] * dev["losses"][0] + w[1] * dev["losses"][1]) + w[2] * dev["losses"][2]).tobytes()
    loss.backward()
    assert t[0].grad is None and t[1].grad is None and t[2].grad is None
    assert t[3].grad.cpu().numpy().tobytes() == dev["grad_gs"].tobytes() and t[4].grad.cpu().numpy().tobytes() == dev["grad_con"].tobytes()
    t[3].grad = t[4].grad = None
    (2 * runner.loss(*t, weights=(1.0, 0.5, 3.0))).backward()
    other = device_run(runner, *arrays, upstream=np.array([1.0, 0.5, 3.0], f32), maps=False)
    assert t[3].grad.cpu().numpy().tobytes() == (other["grad_gs"] * f32(2)).tobytes() and t[4].grad.cpu().numpy().tobytes() == (other["grad_con"] * f32(2)).tobytes()
    only = to_dev(*arrays)
    only[4].requires_grad_()                                                  # gs needs none: it gets none
    runner.loss(*only).backward()
    assert only[3].grad is None and only[4].grad.cpu().numpy().tobytes() == dev["grad_con"].tobytes()
    plain = runner.loss(*to_dev(*arrays))                                     # nothing to differentiate: the forward alone
    assert not plain.requires_grad and plain.cpu().numpy().tobytes() == loss.detach().cpu().numpy().tobytes()


def test_the_chain_is_captured_into_a_graph_and_replays_the_same_bytes(runner, results):
    """Stream capture refuses a host synchronisation and work on another stream that is not joined: a call that is captured, replayed
    and gives the eager call's bytes has neither.  The chain is a line of launches: the captured graph has no branches."""
    arrays, dev, _ = results[(64, 2)]
    t = to_dev(*arrays, np.array(host.G_TOTAL_WEIGHTS, f32))
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        runner.step_losses_grad(*t, parts=True)
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=side):
            res = runner.step_losses_grad(*t, parts=True)
    torch.cuda.current_stream().wait_stream(side)
    for r in res:
        r.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert [r.cpu().numpy().tobytes() for r in res] == [dev[k].tobytes() for k in NAMES]


def test_argument_errors_raise_before_any_launch(runner):
    from blindshadowremoval_amd import _lib
    dev = torch.device("cuda", 0)
    ok = to_dev(*host.example_inputs(32, 1, 0))
    with pytest.raises(ValueError, match="32, 64, 128 or 256"):
        runner.step_losses_grad(*(torch.zeros((1, 48, 48, c), device=dev) for c in (3, 3, 3, 1, 3)))
    with pytest.raises(ValueError, match="1..65535"):
        runner.step_losses_grad(*(torch.zeros((0, 32, 32, c), device=dev) for c in (3, 3, 3, 1, 3)))
    with pytest.raises(ValueError, match="contiguous"):
        runner.step_losses_grad(ok[0], torch.zeros((1, 32, 32, 6), device=dev)[..., ::2], *ok[2:])
    with pytest.raises(ValueError, match="gs must be"):
        runner.step_losses_grad(*ok[:3], ok[4], ok[4])
    with pytest.raises(TypeError):
        runner.step_losses_grad(ok[0].double(), *ok[1:])
    with pytest.raises(TypeError):
        runner.step_losses_grad(ok[0].cpu(), *ok[1:])
    for bad in (torch.ones(3, dtype=torch.float64, device=dev), torch.ones(1, device=dev), torch.ones(3), (200.0, 200.0, 2.0)):
        with pytest.raises(TypeError, match="upstream"):
            runner.step_losses_grad(*ok, upstream=bad)
    lib = _lib.load()
    p = [t.data_ptr() for t in ok]
    sums, losses = torch.zeros((1, host.K), dtype=torch.float64, device=dev), torch.zeros(3, device=dev)
    g_gs, g_con = torch.zeros((1, 32, 32, 1), device=dev), torch.zeros((1, 32, 32, 3), device=dev)
    scratch = torch.zeros(lib.bsr_train_losses_grad_scratch_bytes(1, 32) + 512, dtype=torch.uint8, device=dev)
    base = scratch.data_ptr() + (-scratch.data_ptr()) % 256
    for b, s, sc in ((1, 48, base), (0, 32, base), (65536, 32, base), (1, 32, base + 8)):
        assert lib.bsr_train_losses_grad(0, *p, None, b, s, sums.data_ptr(), losses.data_ptr(), g_gs.data_ptr(), g_con.data_ptr(), None, None, sc, None) == 1
    assert lib.bsr_train_losses_grad(0, *p, None, 1, 32, sums.data_ptr(), losses.data_ptr(), None, g_con.data_ptr(), None, None, base, None) == 1
    assert b"bsr_train_losses_grad" in lib.bsr_last_error()
    torch.cuda.synchronize()
    assert not sums.any() and not losses.any() and not g_gs.any() and not g_con.any() and not scratch.any()          # nothing was launched


@pytest.fixture(scope="module")
def pairs_folder(tmp_path_factory):
    """One synthesised pair of side 256, as the shadow_synth command writes it."""
    return pairs_cases.write_pairs(tmp_path_factory.mktemp("grad_pairs"))


def test_command_grad_device_route_matches_the_host_route(pairs_folder, capsys):
    S = 256
    printed = []
    for extra in ([], ["--host"]):
        assert host.main([pairs_folder, "--batch", "1", "--grad"] + extra) == 0
        lines = capsys.readouterr().out.strip().split("\n")
        assert len(lines) == 2 and lines[0].startswith("Testing 1/1: ")
        fields = dict(f.split(":") for f in lines[1].split(", "))                 # one step: its means are the step's values, at nine digits
        assert tuple(fields) == host.LOSS_NAMES + host.GRAD_NAMES
        printed.append({k: float(v) for k, v in fields.items()})
    assert host.main([pairs_folder, "--batch", "1"]) == 0                          # without --grad the lines are what they were
    lines = capsys.readouterr().out.strip().split("\n")
    assert tuple(dict(f.split(":") for f in lines[1].split(", "))) == host.LOSS_NAMES
    dev_route, host_route = printed
    print("train_losses command --grad: device %s\ntrain_losses command --grad: host %s" % (dev_route, host_route))
    for k in host.LOSS_NAMES + ("grad_gs_l1", "grad_gs_linf"):                    # bit-identical tensors, the same float64 norms, printed at nine digits
        assert dev_route[k] == host_route[k], k
    # the end-to-end tolerance, E2E_BOUND of the largest magnitude per element: the L-infinity norm moves by at most that, the L1 norm
    # by at most that for each of its S * S * 3 elements
    n, linf = S * S * 3, host_route["grad_con_linf"]
    assert linf > 0 and host_route["grad_con_l1"] > linf and host_route["grad_gs_linf"] > 0
    assert abs(dev_route["grad_con_linf"] - linf) <= E2E_BOUND * linf + 1e-9 * linf          # and the nine printed digits
    assert abs(dev_route["grad_con_l1"] - host_route["grad_con_l1"]) <= E2E_BOUND * n * linf + 1e-9 * host_route["grad_con_l1"]
