"""bsr_disc_losses (csrc/disc_kernels.h) against the host statement blindshadowremoval_amd/discriminator.py.

Stage by stage: the 1/2 and 1/4 inputs bit for bit; each layer, fed the DEVICE's own preceding activation, against the float64
statement within max|got - ref| / max|ref| <= 1e-5, the project's fp32-class stage budget (tests/stage_parity.py).  End to end: the
logits within 5e-5 on the same scale (five stage budgets).  The float64 sums against losses_from_logits of the device's own logits
within relative 1e-9 — an a-priori bound: a sum has at most 2^8 float64 additions, each within 2^-53 of its result, and the hinge terms
are non-negative; the plain sum of the fake logits can cancel, so it is held on the scale of the sum of their magnitudes.  The three
float32 losses equal or one ulp apart."""
import numpy as np
import pytest

from blindshadowremoval_amd import discriminator as host
from blindshadowremoval_amd.weights import init_discriminator_weights

import discriminator_cases as cases
import pairs_cases

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
f32 = np.float32
STAGE_BUDGET = 1e-5


@pytest.fixture(scope="module")
def runner():
    from blindshadowremoval_amd import Discriminators
    return Discriminators(0)


def device_run(runner, weights, gt, con_rgb, mask_sv, logits=True, keep=True, raw=False):
    dev = torch.device("cuda", 0)
    if weights is not None:
        runner.load_weights(weights)
    res = runner.gan_losses(*(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (gt, con_rgb, mask_sv)), logits=logits, keep=keep)
    torch.cuda.synchronize()
    if raw:
        return res
    out = {"losses": res[0].cpu().numpy(), "sums": res[1].cpu().numpy()}
    if logits:
        out["logits"] = [y.cpu().numpy() for y in res[2]]
    if keep:
        out["acts"] = {k: v.cpu().numpy() for k, v in res[-1].items()}
    return out


def flat_bytes(res):
    """Every array of a raw result, as bytes."""
    parts = []
    for r in res:
        for t in (r if isinstance(r, list) else r.values() if isinstance(r, dict) else [r]):
            parts.append(t.cpu().numpy().tobytes())
    return parts


@pytest.fixture(scope="module")
def references():
    """Weights, inputs and the float64 statement's result, computed once per size: {(S, B): (weights, arrays, result)}."""
    out = {}
    for S, B in cases.GPU_SIZES:
        w = init_discriminator_weights(20 + S + B)
        arrays = cases.inputs(S, B, seed=200 + S + B)
        out[(S, B)] = (w, arrays, host.gan_losses(w, *arrays))
    return out


def scaled_error(got, ref):
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / np.abs(ref).max())


def loss_bound(ref):
    """Each loss is a sum over the three discriminators of a mean of logits or of hinge terms (1-Lipschitz in the logit): it moves by at
    most the sum of the three logit budgets, taken on the largest logit scale; plus a float32 rounding of the loss itself."""
    return 3 * 5 * STAGE_BUDGET * max(float(np.abs(y).max()) for y in ref["logits"]) + 2.0 ** -23 * float(np.abs(ref["losses"]).max())


def check_sums_and_losses(got, label):
    """The device's sums and losses against losses_from_logits of the device's own logits."""
    want = host.losses_from_logits(got["logits"])
    B = got["sums"].shape[0]
    scale = np.abs(want["sums"]).copy()
    for j, y in enumerate(got["logits"]):
        scale[:, 3 * j + 2] = np.abs(y[B:].astype(np.float64)).reshape(B, -1).sum(axis=1)
    err = np.abs(got["sums"] - want["sums"])
    rel = float((err / np.maximum(scale, 1e-300)).max()) if err.any() else 0.0
    print("discriminators %s: sums max relative |device - host| %.3g, losses device %s host %s" % (label, rel, got["losses"], want["losses"]))
    assert got["sums"].shape == want["sums"].shape and (err <= 1e-9 * scale).all(), label
    assert cases.one_ulp_apart(got["losses"], want["losses"]), (label, got["losses"], want["losses"])


@pytest.mark.parametrize("S,B", cases.GPU_SIZES)
def test_stage_by_stage(runner, references, S, B):
    w, arrays, ref = references[(S, B)]
    got = device_run(runner, w, *arrays)
    for k in (1, 2, 3):
        assert got["acts"]["d%d/in" % k].tobytes() == ref["acts"]["d%d/in" % k].tobytes(), "d%d/in" % k
        for i in range(4):
            prev = got["acts"]["d%d/in" % k] if i == 0 else got["acts"]["d%d/conv%d" % (k, i - 1)]
            want = host.layer(w, k, i, prev)
            e = scaled_error(got["acts"]["d%d/conv%d" % (k, i)], want)
            print("discriminators S=%d B=%d d%d/conv%d fed the device's input: scaled error %.3g" % (S, B, k, i, e))
            assert got["acts"]["d%d/conv%d" % (k, i)].shape == want.shape and e <= STAGE_BUDGET, (k, i, e)
        want = host.head(w, k, got["acts"]["d%d/conv3" % k])
        e = scaled_error(got["acts"]["d%d/out" % k], want)
        print("discriminators S=%d B=%d d%d/out fed the device's input: scaled error %.3g" % (S, B, k, e))
        assert e <= STAGE_BUDGET, (k, e)
        assert got["acts"]["d%d/out" % k][..., 0].tobytes() == got["logits"][k - 1].tobytes()


@pytest.mark.parametrize("S,B", cases.GPU_SIZES)
def test_end_to_end(runner, references, S, B):
    w, arrays, ref = references[(S, B)]
    got = device_run(runner, w, *arrays, keep=False)
    for k in range(3):
        e = scaled_error(got["logits"][k], ref["logits"][k])
        print("discriminators S=%d B=%d logits of d%d end to end: scaled error %.3g" % (S, B, k + 1, e))
        assert got["logits"][k].shape == ref["logits"][k].shape and e <= 5 * STAGE_BUDGET, (k, e)
    check_sums_and_losses(got, "S=%d B=%d" % (S, B))
    np.testing.assert_allclose(got["losses"], ref["losses"], rtol=0, atol=loss_bound(ref))


def test_one_tap_layers_at_32(runner):
    cases.check_one_tap_layers(lambda *a: device_run(runner, *a))


@pytest.mark.parametrize("check", cases.CONSTRUCTED, ids=lambda c: c.__name__)
def test_constructed_case_at_32(runner, check):
    check(lambda *a: device_run(runner, *a))


def test_hinge_case_at_128(runner):
    args = cases.hinge_case()
    ref = host.gan_losses(*args)
    assert cases.hinge_condition(ref["logits"], 2)
    got = device_run(runner, *args, keep=False)
    for k in range(3):
        assert scaled_error(got["logits"][k], ref["logits"][k]) <= 5 * STAGE_BUDGET
        y, z = got["logits"][k], ref["logits"][k]
        assert np.array_equal(1 - y[:2] > 0, 1 - z[:2] > 0) and np.array_equal(1 + y[2:] > 0, 1 + z[2:] > 0)          # the same active sets
    check_sums_and_losses(got, "hinge case")
    print("discriminators hinge case: losses device %s host %s" % (got["losses"], ref["losses"]))
    np.testing.assert_allclose(got["losses"], ref["losses"], rtol=0, atol=loss_bound(ref))


def test_repeated_calls_give_identical_bytes_and_a_second_batch_size_is_correct(runner, references):
    w3, arrays3, ref3 = references[(32, 3)]
    first = flat_bytes(device_run(runner, w3, *arrays3, raw=True))
    second = flat_bytes(device_run(runner, None, *arrays3, raw=True))          # the same object: the same scratch, the same blob
    assert first == second and len(first) == 2 + 3 + 18
    w1, arrays1, ref1 = references[(32, 1)]
    got = device_run(runner, w1, *arrays1)                                       # B = 1 after B = 3 on the same scratch
    for k in range(3):
        assert scaled_error(got["logits"][k], ref1["logits"][k]) <= 5 * STAGE_BUDGET
    check_sums_and_losses(got, "B=1 after B=3")
    got = device_run(runner, w3, *arrays3)
    assert flat_bytes([torch.from_numpy(got["losses"]), torch.from_numpy(got["sums"])]) == first[:2]


def test_the_chain_is_captured_into_a_graph_and_replays_the_same_bytes(runner, references):
    """Stream capture refuses a host synchronisation and work on another stream that is not joined: a call that is captured, replayed
    and gives the eager call's bytes has neither."""
    w, arrays, _ = references[(64, 2)]
    eager = flat_bytes(device_run(runner, w, *arrays, keep=False, raw=True))
    dev = torch.device("cuda", 0)
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        runner.gan_losses(*t, logits=True)
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=side):
            res = runner.gan_losses(*t, logits=True)
    torch.cuda.current_stream().wait_stream(side)
    for r in (res[0], res[1], *res[2]):
        r.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert flat_bytes(res) == eager


def test_results_do_not_depend_on_logits_or_keep(runner, references):
    w, arrays, _ = references[(64, 2)]
    full = device_run(runner, w, *arrays, raw=True)
    assert len(full) == 4
    for logits, keep in ((False, False), (True, False), (False, True)):
        part = device_run(runner, None, *arrays, logits=logits, keep=keep, raw=True)
        assert len(part) == 2 + int(logits) + int(keep)
        assert flat_bytes(part[:2]) == flat_bytes(full[:2])
        if logits:
            assert flat_bytes(part[2:3]) == flat_bytes(full[2:3])
        if keep:
            assert flat_bytes(part[-1:]) == flat_bytes(full[-1:])


def test_argument_errors_raise_before_any_launch(runner):
    from blindshadowremoval_amd import Discriminators, _lib
    dev = torch.device("cuda", 0)
    runner.load_weights(init_discriminator_weights(1))
    ok = [torch.from_numpy(a).to(dev) for a in cases.inputs(32, 1, 0)]
    with pytest.raises(ValueError, match="32, 64, 128 or 256"):
        runner.gan_losses(*(torch.zeros((1, 48, 48, 3), device=dev) for _ in range(3)))
    with pytest.raises(ValueError, match="1..32767"):
        runner.gan_losses(*(torch.zeros((0, 32, 32, 3), device=dev) for _ in range(3)))
    with pytest.raises(ValueError, match="contiguous"):
        runner.gan_losses(ok[0], torch.zeros((1, 32, 32, 6), device=dev)[..., ::2], ok[2])
    with pytest.raises(ValueError, match="mask_sv must be"):
        runner.gan_losses(ok[0], ok[1], ok[2][:, :16].contiguous())
    with pytest.raises(TypeError):
        runner.gan_losses(ok[0].double(), ok[1], ok[2])
    with pytest.raises(TypeError):
        runner.gan_losses(ok[0].cpu(), ok[1], ok[2])
    with pytest.raises(ValueError, match="blob"):
        runner.load_blob(b"\0" * 1024)
    with pytest.raises(ValueError, match="no weights"):
        Discriminators(0).gan_losses(*ok)
    lib = _lib.load()
    assert lib.bsr_disc_losses_scratch_bytes(1, 48) == 0 and lib.bsr_disc_losses_scratch_bytes(32768, 32) == 0 and lib.bsr_disc_losses_scratch_bytes(0, 32) == 0
    assert lib.bsr_disc_act_offset(1, 32, 1, 0) == 0 and lib.bsr_disc_act_offset(1, 32, 4, 0) == 2 ** 64 - 1 and lib.bsr_disc_act_offset(1, 32, 1, 6) == 2 ** 64 - 1
    assert lib.bsr_disc_act_offset(1, 32, 3, 5) < lib.bsr_disc_losses_scratch_bytes(1, 32)
    nbytes = lib.bsr_disc_blob_bytes()
    assert lib.bsr_disc_losses(0, None, nbytes, None, None, None, 1, 32, None, None, None, None, None) == 1
    assert b"bsr_disc_losses" in lib.bsr_last_error()
    blob = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    p = [t.data_ptr() for t in ok]
    sums, losses = torch.zeros((1, host.K), dtype=torch.float64, device=dev), torch.zeros(3, device=dev)
    scratch = torch.zeros(lib.bsr_disc_losses_scratch_bytes(1, 32) + 512, dtype=torch.uint8, device=dev)
    base = scratch.data_ptr() + (-scratch.data_ptr()) % 256
    for nb, b, s, sc in ((nbytes, 1, 48, base), (nbytes, 0, 32, base), (nbytes, 32768, 32, base), (nbytes, 1, 32, base + 8), (nbytes - 4, 1, 32, base)):
        assert lib.bsr_disc_losses(0, blob.data_ptr(), nb, *p, b, s, sums.data_ptr(), losses.data_ptr(), None, sc, None) == 1      # bad S, bad B twice, misaligned scratch, a blob of the wrong size
    torch.cuda.synchronize()
    assert not sums.any() and not losses.any() and not scratch.any()          # nothing was launched


def test_command_device_route_matches_the_host_route(tmp_path, capsys):
    folder = pairs_cases.write_pairs(tmp_path, ("a", "b"), batch=2)
    printed = []
    for extra in ([], ["--host"]):
        assert host.main([folder, "--batch", "2"] + extra) == 0
        last = capsys.readouterr().out.strip().split("\n")[-1]
        fields = dict(f.split(":") for f in last.split(", "))
        assert tuple(fields) == host.LOSS_NAMES
        printed.append(np.array([float(fields[k]) for k in host.LOSS_NAMES]))
    dev_route, host_route = printed
    print("discriminator command: device %s host %s" % (dev_route, host_route))
    assert np.isfinite(dev_route).all() and (dev_route[1:] > 0).all()
    # the two routes share the generator's outputs, so each term moves by at most three logit budgets on the scale of the host
    # route's own logits (loss_bound), which a third pass of the host route hands out; plus the rounding of the float32 losses
    stats = {}
    again = host.score_folder(folder, batch=2, host=True, quiet=True, stats=stats)
    assert np.allclose([again[k] for k in host.LOSS_NAMES], host_route, rtol=1e-8, atol=0) and stats["max_abs_logit"] > 0
    bound = 3 * 5 * STAGE_BUDGET * stats["max_abs_logit"] + 2.0 ** -23 * float(np.abs(host_route).max())
    print("discriminator command: largest host logit %.3g, allowed difference %.3g" % (stats["max_abs_logit"], bound))
    assert (np.abs(dev_route - host_route) <= bound).all()
