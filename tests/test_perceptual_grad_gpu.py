"""bsr_vgg_per_loss_grad (csrc/vgg_grad_kernels.h) against the host statement blindshadowremoval_amd/perceptual.py: per_loss_grad.

The constructed cases bit for bit (perceptual_grad_cases: powers of two through kernels of ones and zeros are exact in float32 and float64
alike).  Stage by stage: each of the chain's 18 backward launches, fed the DEVICE's own incoming gradient and the device's own kept
activations, against the float64 statement of that launch alone — the seed and the four un-pools exactly, the thirteen gradient
convolutions within max|got - ref| / max|ref| <= 1e-5, the project's fp32-class stage budget (tests/stage_parity.py); where the
epilogue adds a seed and masks, the reference does so too, from the same activations.  End to end: grad against
per_loss_grad(acts = the device's activations) within 4 x E2E_MEASURED on the scale of the largest magnitude, the largest figure
measured on the MI355X over these sizes (profiles/perceptual_grad_bench.json), never above 1e-3; the difference from
the statement on its own float64 forward is printed and not asserted, since masks can flip at values that round across 0."""
import numpy as np
import pytest

from blindshadowremoval_amd import perceptual as host
from blindshadowremoval_amd.weights import VGG_LAYERS, VGG_TAPS, init_vgg_weights

import perceptual_cases as cases
import perceptual_grad_cases as gcases

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
f32 = np.float32
STAGE_BUDGET = 1e-5
E2E_BOUND = gcases.E2E_BOUND


@pytest.fixture(scope="module")
def runner():
    from blindshadowremoval_amd import Perceptual
    return Perceptual(0)


@pytest.fixture(scope="module")
def vgg_weights():
    return init_vgg_weights(21)


def to_dev(*arrays):
    dev = torch.device("cuda", 0)
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def device_run(runner, weights, gt, con_rgb, upstream=None, keep=True, raw=False):
    if weights is not None:
        runner.load_weights(weights)
    res = runner.per_loss_grad(*to_dev(gt, con_rgb, upstream), keep=keep)
    torch.cuda.synchronize()
    if raw:
        return res
    out = {"loss": res[0].cpu().numpy(), "sums": res[1].cpu().numpy(), "grad": res[2].cpu().numpy()}
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
def device_results(runner, vgg_weights):
    """Inputs and the device's result with its activations, once per size: {(S, B): (arrays, result)}."""
    out = {}
    for S, B in gcases.GRAD_SIZES:
        arrays = gcases.inputs(S, B)
        out[(S, B)] = (arrays, device_run(runner, vgg_weights, *arrays))
    return out


@pytest.mark.parametrize("tap", range(9))
def test_one_tap_layers_at_32(runner, tap):
    args, r = gcases.check_one_tap_layers(lambda *a, **k: device_run(runner, *a, **k), tap)
    assert r["grad"].tobytes() == host.per_loss_grad(*args)["grad"].tobytes()


def test_tie_map_sends_the_gradient_to_the_first_maximum(runner):
    args, r = gcases.check_tie_map(lambda *a, **k: device_run(runner, *a, **k))
    assert r["grad"].tobytes() == host.per_loss_grad(*args)["grad"].tobytes()


def test_equal_images_give_a_zero_gradient(runner):
    gcases.check_equal_images(lambda *a, **k: device_run(runner, *a, **k))


def test_items_in_the_other_order_give_the_rows_in_the_other_order(runner, vgg_weights):
    gcases.check_item_order(lambda *a, **k: device_run(runner, *a, **k), vgg_weights)


def test_upstream_is_one_float32_multiply_and_none_is_one(runner, vgg_weights):
    run = lambda *a, **k: device_run(runner, *a, **k)
    gcases.check_upstream(run, vgg_weights)
    gt, con = gcases.inputs(32, 3)
    assert run(None, gt, con)["grad"].tobytes() == run(None, gt, con, upstream=np.ones(1, f32))["grad"].tobytes()


def stage_reference(weights, kind, name, g_in, acts, B, S):
    """The float64 statement of one backward launch from the device's incoming gradient and kept activations."""
    fake = lambda n: np.asarray(acts[n])[B:]
    if kind == "seed":
        return host.relu_mask(host.seeds(host.features_of(acts), B)[-1], fake(name))
    if kind == "unpool":
        return host.relu_mask(host.max_pool_grad(g_in, fake(name)), fake(name))
    g = host.conv_dgrad(weights, name, g_in)
    prev = cases.layer_input_name(name)
    if prev in VGG_LAYERS:                                   # a convolution's output: the seed where it is tapped, then its mask
        if prev in VGG_TAPS:
            g = g + host.seeds(host.features_of(acts), B)[VGG_TAPS.index(prev)]
        g = host.relu_mask(g, fake(prev))
    return g


@pytest.mark.parametrize("S,B", gcases.GRAD_SIZES)
def test_stage_by_stage(runner, vgg_weights, device_results, S, B):
    from blindshadowremoval_amd.perceptual_gpu import grad_stages
    arrays, res = device_results[(S, B)]
    acts = res["acts"]
    runner.load_weights(vgg_weights)
    t = to_dev(*arrays)
    stages = grad_stages()
    assert len(stages) == 18 and [k for k, _, _ in stages].count("dgrad") == 13 and [k for k, _, _ in stages].count("unpool") == 4
    g_in, worst = None, 0.0
    for j, (kind, name, (shift, ch)) in enumerate(stages):
        side = S >> shift
        if j < len(stages) - 1:
            got = runner.grad_stage(*t, stop_after=j + 1).cpu().numpy()[:B * side * side * ch].reshape(B, side, side, ch)
        else:
            got = None
        want = stage_reference(vgg_weights, kind, name, g_in, acts, B, S)
        if got is None:                                      # the last launch writes grad: 255, BGR reversed, in float32
            assert want.shape == (B, S, S, 3)
            e = scaled_error(res["grad"], 255.0 * want[..., ::-1])
            exact = False
        else:
            assert want.shape == got.shape, (kind, name)
            exact = kind != "dgrad"
            e = scaled_error(got, want) if np.abs(want).max() > 0 else float(np.abs(got).max())
        print("perceptual grad S=%d B=%d launch %d %s %s fed the device's input: scaled error %.3g" % (S, B, j + 1, kind, name, e))
        if exact:
            np.testing.assert_array_equal(got, want.astype(f32), err_msg="%s %s" % (kind, name))
        else:
            worst = max(worst, e)
            assert e <= STAGE_BUDGET, (kind, name, e)
        if kind == "dgrad" and got is not None and cases.layer_input_name(name) in VGG_LAYERS:
            assert not got[want == 0].any(), (kind, name)      # the masks are exact: what the mask closes is 0 on the device too
        g_in = got
    print("perceptual grad S=%d B=%d: worst gradient convolution %.3g" % (S, B, worst))
    assert np.abs(res["grad"]).max() > 0


@pytest.mark.parametrize("S,B", gcases.GRAD_SIZES)
def test_end_to_end(runner, vgg_weights, device_results, S, B):
    arrays, res = device_results[(S, B)]
    ref = host.per_loss_grad(vgg_weights, *arrays, acts=res["acts"])
    e = scaled_error(res["grad"], ref["grad"])
    own = host.per_loss_grad(vgg_weights, *arrays)
    print("perceptual grad S=%d B=%d end to end: scaled error %.3g on the device's masks (bound %.3g); %.3g against the statement's own float64 forward; largest |grad| %.3g"
          % (S, B, e, E2E_BOUND, scaled_error(res["grad"], own["grad"]), np.abs(ref["grad"]).max()))
    assert res["grad"].shape == (B, S, S, 3) and res["grad"].dtype == np.float32 and e <= E2E_BOUND


def test_forward_outputs_are_per_loss_bytes(runner, vgg_weights, device_results):
    arrays, _ = device_results[(64, 2)]
    runner.load_weights(vgg_weights)
    t = to_dev(*arrays)
    plain = runner.per_loss(*t, keep=True)
    torch.cuda.synchronize()
    both = runner.per_loss_grad(*t, keep=True)
    torch.cuda.synchronize()
    assert flat_bytes(plain) == flat_bytes((both[0], both[1], both[3])) and len(flat_bytes(plain)) == 2 + 18


def test_repeated_calls_give_identical_bytes_and_a_second_batch_size_is_correct(runner, vgg_weights, device_results):
    arrays3, res3 = device_results[(32, 3)]
    first = flat_bytes(device_run(runner, vgg_weights, *arrays3, keep=False, raw=True))
    second = flat_bytes(device_run(runner, None, *arrays3, keep=False, raw=True))          # the same object: the same scratch, the same blobs
    assert first == second and len(first) == 3 and first[2] == res3["grad"].tobytes()
    arrays1, res1 = device_results[(32, 1)]
    got = device_run(runner, None, *arrays1, keep=False)                                    # B = 1 after B = 3 on the same scratch
    assert got["grad"].tobytes() == res1["grad"].tobytes() and got["loss"].tobytes() == res1["loss"].tobytes()
    assert flat_bytes(device_run(runner, None, *arrays3, keep=False, raw=True)) == first


def test_the_chain_is_captured_into_a_graph_and_replays_the_same_bytes(runner, vgg_weights, device_results):
    """Stream capture refuses a host synchronisation and work on another stream that is not joined: a call that is captured, replayed
    and gives the eager call's bytes has neither.  The chain is a line of launches: the captured graph has no branches."""
    arrays, _ = device_results[(64, 2)]
    eager = flat_bytes(device_run(runner, vgg_weights, *arrays, keep=False, raw=True))
    t = to_dev(*arrays)
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        runner.per_loss_grad(*t)
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=side):
            res = runner.per_loss_grad(*t)
    torch.cuda.current_stream().wait_stream(side)
    for r in res:
        r.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert flat_bytes(res) == eager


def test_autograd_door(runner, vgg_weights, device_results):
    arrays, res = device_results[(32, 3)]
    runner.load_weights(vgg_weights)
    gt, con = to_dev(*arrays)
    con.requires_grad_()
    loss = runner.loss(gt, con)
    assert loss.shape == (1,) and loss.grad_fn is not None and loss.detach().cpu().numpy().tobytes() == res["loss"].tobytes()
    loss.backward()
    assert gt.grad is None and con.grad.cpu().numpy().tobytes() == res["grad"].tobytes()
    con.grad = None
    (0.005 * runner.loss(gt, con)).backward()
    scaled = device_run(runner, None, *arrays, upstream=np.array([0.005], f32), keep=False)["grad"]
    assert con.grad.cpu().numpy().tobytes() == scaled.tobytes()
    plain = runner.loss(gt, con.detach())                                                   # nothing to differentiate: the forward alone
    assert not plain.requires_grad and plain.cpu().numpy().tobytes() == res["loss"].tobytes()


def test_argument_errors_raise_before_any_launch(runner, vgg_weights):
    from blindshadowremoval_amd import Perceptual, _lib, pack
    dev = torch.device("cuda", 0)
    runner.load_weights(vgg_weights)
    ok = [torch.from_numpy(a).to(dev) for a in cases.inputs(32, 1, 0)]
    with pytest.raises(ValueError, match="32, 64, 128 or 256"):
        runner.per_loss_grad(*(torch.zeros((1, 48, 48, 3), device=dev) for _ in range(2)))
    with pytest.raises(ValueError, match="1..4096"):
        runner.per_loss_grad(*(torch.zeros((0, 32, 32, 3), device=dev) for _ in range(2)))
    with pytest.raises(ValueError, match="contiguous"):
        runner.per_loss_grad(ok[0], torch.zeros((1, 32, 32, 6), device=dev)[..., ::2])
    with pytest.raises(ValueError, match="con_rgb must be"):
        runner.per_loss_grad(ok[0], ok[1][:, :16].contiguous())
    with pytest.raises(TypeError):
        runner.per_loss_grad(ok[0].double(), ok[1])
    with pytest.raises(TypeError):
        runner.per_loss_grad(ok[0].cpu(), ok[1])
    for bad in (torch.ones(1, dtype=torch.float64, device=dev), torch.ones(2, device=dev), torch.ones(1), 0.005):
        with pytest.raises(TypeError, match="upstream"):
            runner.per_loss_grad(*ok, upstream=bad)
    with pytest.raises(ValueError, match="no weights"):
        Perceptual(0).per_loss_grad(*ok)
    forward_only = Perceptual(0)
    forward_only.load_blob(pack.pack_vgg(vgg_weights))
    with pytest.raises(ValueError, match="no weights"):
        forward_only.per_loss_grad(*ok)
    lib = _lib.load()
    assert lib.bsr_vgg_grad_scratch_bytes(1, 48) == 0 and lib.bsr_vgg_grad_scratch_bytes(4097, 32) == 0 and lib.bsr_vgg_grad_scratch_bytes(0, 32) == 0
    assert lib.bsr_vgg_grad_offset(1, 32, 0) == lib.bsr_vgg_scratch_bytes(1, 32) and lib.bsr_vgg_grad_offset(1, 32, 2) == 2 ** 64 - 1
    assert lib.bsr_vgg_grad_scratch_bytes(2, 64) == lib.bsr_vgg_scratch_bytes(2, 64) + 2 * 2 * 64 * 64 * 64 * 4
    nbytes, dbytes = lib.bsr_vgg_blob_bytes(), lib.bsr_vgg_dgrad_blob_bytes()
    assert dbytes == 51_904_512 == len(pack.pack_vgg_dgrad(vgg_weights))
    assert lib.bsr_vgg_per_loss_grad(0, None, nbytes, None, dbytes, None, None, None, 1, 32, None, None, None, None, None) == 1
    assert b"bsr_vgg_per_loss_grad" in lib.bsr_last_error()
    blob, dblob = torch.zeros(nbytes, dtype=torch.uint8, device=dev), torch.zeros(dbytes, dtype=torch.uint8, device=dev)
    p = [t.data_ptr() for t in ok]
    sums, loss, grad = torch.zeros((1, host.K), dtype=torch.float64, device=dev), torch.zeros(1, device=dev), torch.zeros((1, 32, 32, 3), device=dev)
    scratch = torch.zeros(lib.bsr_vgg_grad_scratch_bytes(1, 32) + 512, dtype=torch.uint8, device=dev)
    base = scratch.data_ptr() + (-scratch.data_ptr()) % 256
    for nb, db, b, s, sc in ((nbytes, dbytes, 1, 48, base), (nbytes, dbytes, 0, 32, base), (nbytes, dbytes, 4097, 32, base), (nbytes, dbytes, 1, 32, base + 8),
                             (nbytes - 4, dbytes, 1, 32, base), (nbytes, dbytes - 4, 1, 32, base)):
        assert lib.bsr_vgg_per_loss_grad(0, blob.data_ptr(), nb, dblob.data_ptr(), db, *p, None, b, s, sums.data_ptr(), loss.data_ptr(), grad.data_ptr(), sc, None) == 1
    assert lib.bsr_debug_vgg_per_loss_grad(0, blob.data_ptr(), nbytes, dblob.data_ptr(), dbytes, *p, None, 1, 32, sums.data_ptr(), loss.data_ptr(), grad.data_ptr(),
                                           base, 19, None) == 1
    torch.cuda.synchronize()
    assert not sums.any() and not loss.any() and not grad.any() and not scratch.any()          # nothing was launched
