"""bsr_vgg_per_loss (csrc/vgg_kernels.h) against the host statement blindshadowremoval_amd/perceptual.py.

Stage by stage: the preprocessed input bit for bit; each layer, fed the DEVICE's own preceding activation, against the float64 statement
within max|got - ref| / max|ref| <= 1e-5, the project's fp32-class stage budget (tests/stage_parity.py); the max pools exactly.  End to
end: the five tapped features against the float64 statement within 4 x cases.E2E_MEASURED on the same scale — thirteen stages compound
and the figure is the largest one measured on these very cases (profiles/perceptual_bench.json) — and never above
1e-3, the project's parity tolerance.  The float64 sums against sums_from_features of the device's own features within relative 1e-9
(cases.SUM_REL: the terms are non-negative and a sum has at most 2^22 of them); the float32 loss equal or one ulp apart."""
import numpy as np
import pytest

from blindshadowremoval_amd import perceptual as host
from blindshadowremoval_amd.weights import VGG_BLOCKS, VGG_LAYERS, VGG_TAPS, init_vgg_weights

import perceptual_cases as cases

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
f32 = np.float32
STAGE_BUDGET = 1e-5
E2E_BOUND = cases.E2E_BOUND


@pytest.fixture(scope="module")
def runner():
    from blindshadowremoval_amd import Perceptual
    return Perceptual(0)


def device_run(runner, weights, gt, con_rgb, keep=True, raw=False):
    dev = torch.device("cuda", 0)
    if weights is not None:
        runner.load_weights(weights)
    res = runner.per_loss(*(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (gt, con_rgb)), keep=keep)
    torch.cuda.synchronize()
    if raw:
        return res
    out = {"loss": res[0].cpu().numpy(), "sums": res[1].cpu().numpy()}
    if keep:
        out["acts"] = {k: v.cpu().numpy() for k, v in res[2].items()}
    return out


def flat_bytes(res):
    parts = []
    for r in res:
        for t in (r.values() if isinstance(r, dict) else [r]):
            parts.append(t.cpu().numpy().tobytes())
    return parts


@pytest.fixture(scope="module")
def vgg_weights():
    return init_vgg_weights(21)


@pytest.fixture(scope="module")
def references(vgg_weights):
    """Inputs and the float64 statement's result, computed once per size: {(S, B): (arrays, result)}."""
    out = {}
    for S, B in cases.GPU_SIZES:
        arrays = cases.inputs(S, B, seed=300 + S + B)
        out[(S, B)] = (arrays, host.per_loss(vgg_weights, *arrays))
    return out


def scaled_error(got, ref):
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / np.abs(ref).max())


def check_sums_and_loss(got, S, label):
    """The device's sums and loss against the host's sums of the device's own features."""
    want = host.sums_from_features([got["acts"][n] for n in VGG_TAPS])
    err = np.abs(got["sums"] - want)
    rel = float((err / np.maximum(want, 1e-300)).max()) if err.any() else 0.0
    want_loss = host.loss_from_sums(want, S)
    print("perceptual %s: sums max relative |device - host| %.3g, loss device %s host %s" % (label, rel, got["loss"], want_loss))
    assert got["sums"].shape == want.shape and got["sums"].dtype == np.float64 and (err <= cases.SUM_REL * want).all(), label
    assert got["loss"].shape == (1,) and cases.one_ulp_apart(got["loss"], want_loss), (label, got["loss"], want_loss)


@pytest.mark.parametrize("S,B", cases.GPU_SIZES)
def test_stage_by_stage(runner, vgg_weights, references, S, B):
    arrays, ref = references[(S, B)]
    got = device_run(runner, vgg_weights, *arrays)
    assert got["acts"]["input"].tobytes() == ref["acts"]["input"].tobytes()
    assert list(got["acts"]) == ["input"] + list(VGG_LAYERS) + ["block%d_pool" % b for b in range(1, 5)]
    worst = 0.0
    for name in VGG_LAYERS:
        want = host.conv_relu(vgg_weights, name, got["acts"][cases.layer_input_name(name)])
        e = scaled_error(got["acts"][name], want)
        worst = max(worst, e)
        print("perceptual S=%d B=%d %s fed the device's input: scaled error %.3g" % (S, B, name, e))
        assert got["acts"][name].shape == want.shape and e <= STAGE_BUDGET, (name, e)
    for blk in range(1, 5):
        last = "block%d_conv%d" % (blk, VGG_BLOCKS[blk - 1][1])
        np.testing.assert_array_equal(got["acts"]["block%d_pool" % blk], host.max_pool(got["acts"][last]))
    print("perceptual S=%d B=%d: worst stage %.3g" % (S, B, worst))


@pytest.mark.parametrize("S,B", cases.GPU_SIZES)
def test_end_to_end(runner, vgg_weights, references, S, B):
    arrays, ref = references[(S, B)]
    got = device_run(runner, vgg_weights, *arrays)
    moved = 0.0
    for k, name in enumerate(VGG_TAPS):
        e = scaled_error(got["acts"][name], ref["acts"][name])
        print("perceptual S=%d B=%d %s end to end: scaled error %.3g" % (S, B, name, e))
        assert got["acts"][name].shape == ref["acts"][name].shape and e <= E2E_BOUND, (name, e)
        moved += 2 * E2E_BOUND * float(np.abs(ref["acts"][name]).max())          # a mean of |real - fake| moves by at most twice the feature's budget
    check_sums_and_loss(got, S, "S=%d B=%d" % (S, B))
    print("perceptual S=%d B=%d: loss device %s host %s" % (S, B, got["loss"], ref["loss"]))
    np.testing.assert_allclose(got["loss"], ref["loss"], rtol=0, atol=moved + 2.0 ** -23 * float(ref["loss"][0]))


@pytest.mark.parametrize("tap", range(9))
def test_one_tap_layers_at_32(runner, tap):
    cases.check_one_tap_layers(lambda *a: device_run(runner, *a), tap)


@pytest.mark.parametrize("check", cases.CONSTRUCTED, ids=lambda c: c.__name__)
def test_constructed_case_at_32(runner, check):
    check(lambda *a: device_run(runner, *a))


def test_items_in_the_other_order_give_the_rows_in_the_other_order(runner, vgg_weights, references):
    (gt, con), _ = references[(32, 3)]
    a = device_run(runner, vgg_weights, gt, con, keep=False)
    b = device_run(runner, None, np.ascontiguousarray(gt[::-1]), np.ascontiguousarray(con[::-1]), keep=False)
    assert a["sums"][::-1].tobytes() == b["sums"].tobytes() and a["sums"][0].tobytes() != a["sums"][1].tobytes()
    assert cases.one_ulp_apart(a["loss"], b["loss"])


def test_repeated_calls_give_identical_bytes_and_a_second_batch_size_is_correct(runner, vgg_weights, references):
    arrays3, ref3 = references[(32, 3)]
    first = flat_bytes(device_run(runner, vgg_weights, *arrays3, raw=True))
    second = flat_bytes(device_run(runner, None, *arrays3, raw=True))          # the same object: the same scratch, the same blob
    assert first == second and len(first) == 2 + 18
    arrays1, ref1 = references[(32, 1)]
    got = device_run(runner, None, *arrays1)                                    # B = 1 after B = 3 on the same scratch
    for name in VGG_TAPS:
        assert scaled_error(got["acts"][name], ref1["acts"][name]) <= E2E_BOUND
    check_sums_and_loss(got, 32, "B=1 after B=3")
    got = device_run(runner, None, *arrays3, keep=False)
    assert [got["loss"].tobytes(), got["sums"].tobytes()] == first[:2]


def test_results_do_not_depend_on_keep(runner, vgg_weights, references):
    arrays, _ = references[(64, 2)]
    full = device_run(runner, vgg_weights, *arrays, raw=True)
    part = device_run(runner, None, *arrays, keep=False, raw=True)
    assert len(full) == 3 and len(part) == 2 and flat_bytes(part) == flat_bytes(full[:2])


def test_the_chain_is_captured_into_a_graph_and_replays_the_same_bytes(runner, vgg_weights, references):
    """Stream capture refuses a host synchronisation and work on another stream that is not joined: a call that is captured, replayed
    and gives the eager call's bytes has neither."""
    arrays, _ = references[(64, 2)]
    eager = flat_bytes(device_run(runner, vgg_weights, *arrays, keep=False, raw=True))
    dev = torch.device("cuda", 0)
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        runner.per_loss(*t)
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=side):
            res = runner.per_loss(*t)
    torch.cuda.current_stream().wait_stream(side)
    for r in res:
        r.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert flat_bytes(res) == eager


def test_argument_errors_raise_before_any_launch(runner, vgg_weights):
    from blindshadowremoval_amd import Perceptual, _lib
    dev = torch.device("cuda", 0)
    runner.load_weights(vgg_weights)
    ok = [torch.from_numpy(a).to(dev) for a in cases.inputs(32, 1, 0)]
    with pytest.raises(ValueError, match="32, 64, 128 or 256"):
        runner.per_loss(*(torch.zeros((1, 48, 48, 3), device=dev) for _ in range(2)))
    with pytest.raises(ValueError, match="1..4096"):
        runner.per_loss(*(torch.zeros((0, 32, 32, 3), device=dev) for _ in range(2)))
    with pytest.raises(ValueError, match="contiguous"):
        runner.per_loss(ok[0], torch.zeros((1, 32, 32, 6), device=dev)[..., ::2])
    with pytest.raises(ValueError, match="con_rgb must be"):
        runner.per_loss(ok[0], ok[1][:, :16].contiguous())
    with pytest.raises(TypeError):
        runner.per_loss(ok[0].double(), ok[1])
    with pytest.raises(TypeError):
        runner.per_loss(ok[0].cpu(), ok[1])
    with pytest.raises(ValueError, match="blob"):
        runner.load_blob(b"\0" * 1024)
    with pytest.raises(ValueError, match="no weights"):
        Perceptual(0).per_loss(*ok)
    lib = _lib.load()
    assert lib.bsr_vgg_scratch_bytes(1, 48) == 0 and lib.bsr_vgg_scratch_bytes(4097, 32) == 0 and lib.bsr_vgg_scratch_bytes(0, 32) == 0
    assert lib.bsr_vgg_act_offset(1, 32, 0) == 0 and lib.bsr_vgg_act_offset(1, 32, 18) == 2 ** 64 - 1 and lib.bsr_vgg_act_offset(1, 32, -1) == 2 ** 64 - 1
    assert lib.bsr_vgg_act_offset(1, 48, 0) == 2 ** 64 - 1
    offs = [lib.bsr_vgg_act_offset(2, 64, m) for m in range(18)]
    assert offs == sorted(offs) and all(o % 256 == 0 for o in offs) and offs[1] == 2 * 2 * 64 * 64 * 8 * 4 and offs[-1] < lib.bsr_vgg_scratch_bytes(2, 64)
    nbytes = lib.bsr_vgg_blob_bytes()
    assert nbytes == 51_791_360
    assert lib.bsr_vgg_per_loss(0, None, nbytes, None, None, 1, 32, None, None, None, None) == 1
    assert b"bsr_vgg_per_loss" in lib.bsr_last_error()
    blob = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    p = [t.data_ptr() for t in ok]
    sums, loss = torch.zeros((1, host.K), dtype=torch.float64, device=dev), torch.zeros(1, device=dev)
    scratch = torch.zeros(lib.bsr_vgg_scratch_bytes(1, 32) + 512, dtype=torch.uint8, device=dev)
    base = scratch.data_ptr() + (-scratch.data_ptr()) % 256
    for nb, b, s, sc in ((nbytes, 1, 48, base), (nbytes, 0, 32, base), (nbytes, 4097, 32, base), (nbytes, 1, 32, base + 8), (nbytes - 4, 1, 32, base)):
        assert lib.bsr_vgg_per_loss(0, blob.data_ptr(), nb, *p, b, s, sums.data_ptr(), loss.data_ptr(), sc, None) == 1      # bad S, bad B twice, misaligned scratch, a blob of the wrong size
    torch.cuda.synchronize()
    assert not sums.any() and not loss.any() and not scratch.any()          # nothing was launched
