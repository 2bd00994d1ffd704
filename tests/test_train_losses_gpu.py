"""bsr_train_losses (csrc/train_losses_kernels.h) against the host statement blindshadowremoval_amd/train_losses.py: the three planes bit
for bit; the float64 sums within relative 1e-9 — an a-priori bound: a sum has at most 2^23 non-negative float64 additions, each within
2^-53 of its result, so any two orders agree to 2^23 2^-52 < 1e-9 relative; the three float32 losses equal or one ulp apart."""
import numpy as np
import pytest

from blindshadowremoval_amd import train_losses as host

import train_losses_cases as cases
import pairs_cases

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
f32 = np.float32


@pytest.fixture(scope="module")
def runner():
    from blindshadowremoval_amd import TrainLosses
    return TrainLosses(0)


def device_run(runner, *arrays, figs=True, raw=False):
    dev = torch.device("cuda", 0)
    res = runner.step_losses(*(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays), figs=figs)
    torch.cuda.synchronize()
    out = [r.cpu().numpy() for r in res]
    if raw:
        return out
    return dict(zip(("losses", "sums", "mask_edge", "bmaskgt", "dif_grad"), out))


def compare(got, want, label):
    for k in ("mask_edge", "bmaskgt", "dif_grad"):
        np.testing.assert_array_equal(got[k], want[k], err_msg="%s: %s" % (label, k))
    err = np.abs(got["sums"] - want["sums"])
    rel = float((err / np.maximum(np.abs(want["sums"]), 1e-300)).max()) if err.any() else 0.0
    print("train_losses %s: sums max relative |device - host| %.3g, losses device %s host %s" % (label, rel, got["losses"], want["losses"]))
    assert got["sums"].shape == want["sums"].shape and (err <= 1e-9 * np.abs(want["sums"])).all(), label
    assert cases.one_ulp_apart(got["losses"], want["losses"]), (label, got["losses"], want["losses"])


@pytest.fixture(scope="module")
def references():
    """The host statement's results, computed once per size: {(S, B): (arrays, result)}."""
    out = {}
    for S, B in ((32, 1), (32, 3), (64, 2), (256, 2)):
        arrays = host.example_inputs(S, B, seed=100 + S + B)
        out[(S, B)] = (arrays, host.step_losses(*arrays))
    return out


@pytest.mark.parametrize("S,B", [(32, 1), (32, 3), (64, 2), (256, 2)])
def test_device_against_host(runner, references, S, B):
    arrays, want = references[(S, B)]
    compare(device_run(runner, *arrays), want, "S=%d B=%d" % (S, B))


@pytest.mark.parametrize("check", cases.ALL, ids=lambda c: c.__name__)
def test_constructed_case_at_32(runner, check):
    check(lambda *arrays: device_run(runner, *arrays))


def test_repeated_calls_give_identical_bits_and_a_second_batch_size_is_correct(runner, references):
    arrays3, want3 = references[(32, 3)]
    first = device_run(runner, *arrays3, raw=True)
    second = device_run(runner, *arrays3, raw=True)                     # the same TrainLosses object: the same scratch
    for a, b in zip(first, second):
        assert a.tobytes() == b.tobytes()
    arrays1, want1 = references[(32, 1)]
    compare(device_run(runner, *arrays1), want1, "B=1 after B=3")       # stale slots and planes of items 1, 2 must not leak
    compare(device_run(runner, *arrays3), want3, "B=3 after B=1")
    arrays64, want64 = references[(64, 2)]
    compare(device_run(runner, *arrays64), want64, "S=64 after S=32")


def test_losses_do_not_depend_on_the_figures(runner, references):
    arrays, _ = references[(64, 2)]
    with_figs = device_run(runner, *arrays, figs=True, raw=True)
    without = device_run(runner, *arrays, figs=False, raw=True)
    assert len(without) == 2 and len(with_figs) == 5
    assert without[0].tobytes() == with_figs[0].tobytes() and without[1].tobytes() == with_figs[1].tobytes()


def test_argument_errors_raise_before_any_launch(runner):
    dev = torch.device("cuda", 0)
    ok = [torch.from_numpy(a).to(dev) for a in host.example_inputs(32, 1, 0)]
    with pytest.raises(ValueError, match="32, 64, 128 or 256"):
        runner.step_losses(*(torch.zeros((1, 48, 48, c), device=dev) for c in (3, 3, 3, 1, 3)))
    with pytest.raises(ValueError, match="contiguous"):
        runner.step_losses(ok[0], torch.zeros((1, 32, 32, 6), device=dev)[..., ::2], *ok[2:])
    with pytest.raises(ValueError, match="gs must be"):
        runner.step_losses(ok[0], ok[1], ok[2], ok[4], ok[4])
    with pytest.raises(TypeError):
        runner.step_losses(ok[0].double(), *ok[1:])
    with pytest.raises(TypeError):
        runner.step_losses(ok[0].cpu(), *ok[1:])
    with pytest.raises(TypeError):
        runner.step_losses(ok[0].cpu().numpy(), *ok[1:])
    from blindshadowremoval_amd import _lib
    lib = _lib.load()
    assert lib.bsr_train_losses_scratch_bytes(1, 48) == 0 and lib.bsr_train_losses_scratch_bytes(65536, 32) == 0 and lib.bsr_train_losses_scratch_bytes(0, 32) == 0
    assert lib.bsr_train_losses(0, None, None, None, None, None, 1, 32, None, None, None, None, None, None, None) == 1
    assert b"bsr_train_losses" in lib.bsr_last_error()
    p = [t.data_ptr() for t in ok]
    sums, losses = torch.zeros((1, host.K), dtype=torch.float64, device=dev), torch.zeros(3, device=dev)
    scratch = torch.zeros(lib.bsr_train_losses_scratch_bytes(1, 32) + 512, dtype=torch.uint8, device=dev)
    base = scratch.data_ptr() + (-scratch.data_ptr()) % 256
    for b, s, sc in ((1, 48, base), (0, 32, base), (65536, 32, base), (1, 32, base + 8)):          # bad S, bad B twice, misaligned scratch
        assert lib.bsr_train_losses(0, *p, b, s, sums.data_ptr(), losses.data_ptr(), None, None, None, sc, None) == 1
    torch.cuda.synchronize()
    assert not sums.any() and not losses.any()                          # nothing was launched


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
    print("train_losses command: device %s host %s" % (dev_route, host_route))
    assert np.isfinite(dev_route).all() and (dev_route > 0).all()
    assert (np.abs(dev_route - host_route) <= 2.0 ** -23 * np.abs(host_route)).all()          # float32 losses equal or one ulp apart
