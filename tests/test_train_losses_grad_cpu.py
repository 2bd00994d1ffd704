"""train_losses.step_losses_grad, the host statement of the reconstruction and gradient losses' backward, on the CPU: against torch
autograd in float64 on a restatement of the forward that shares no code with it (train_losses_grad_cases.torch_objective), the
float32-sign form against the float64 one, the three operators' adjoint identities, the 2 x 2 quarter-weight form of the resize S -> s,
the constructed cases, and the binding's checks and the entry point's argument checks ahead of any device work."""
import numpy as np
import pytest
import torch

from blindshadowremoval_amd import _lib
from blindshadowremoval_amd import train_losses as host
from blindshadowremoval_amd.build import build_library
from blindshadowremoval_amd.train_losses_gpu import G_TOTAL_WEIGHTS, TrainLosses
from blindshadowremoval_amd.ucb_post import resize_bilinear
from on_dev0 import BSR_ERR_ARG, DEV, P, d0

import train_losses_grad_cases as cases

f32 = np.float32
AUTOGRAD_BAR = 1e-12           # on the scale of the largest magnitude; discriminator.gen_grad met 8e-16 against autograd
ADJOINT_BAR = 1e-12
WEIGHTS = ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), tuple(float(w) for w in host.G_TOTAL_WEIGHTS))


@pytest.fixture(scope="module")
def seeded():
    """{(S, B): (seed, arrays)} with the first seed at which no difference a sign is taken from lies within 1e-9 of 0 without being 0."""
    out = {}
    for S, B in cases.CPU_SIZES:
        seed = cases.pick_seed(S, B)
        out[(S, B)] = (seed, host.example_inputs(S, B, seed))
    return out


def scaled(got, ref):
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / np.abs(ref).max())


@pytest.mark.parametrize("S,B", cases.CPU_SIZES)
def test_f64_statement_against_autograd(seeded, S, B):
    seed, arrays = seeded[(S, B)]
    print("train_losses grad S=%d B=%d seed %d: %d elements with con_rgb = gt exactly (kept: sign(0) = 0)" % (S, B, seed, int((arrays[4] == arrays[1]).sum())))
    for w in WEIGHTS:
        want_gs, want_con = cases.autograd_grads(arrays, w)
        got = host.step_losses_grad(*arrays, upstream=np.array(w, f32), f64=True)
        assert got["grad_gs"].dtype == got["grad_con"].dtype == np.float64
        for name, g, ref in (("grad_gs", got["grad_gs"], want_gs), ("grad_con", got["grad_con"], want_con)):
            if not np.abs(ref).max() > 0:
                assert not g.any(), (w, name)
                continue
            e = scaled(g, ref)
            print("train_losses grad S=%d B=%d seed %d weights %s %s: scaled error against autograd %.3g, largest %.3g" % (S, B, seed, w, name, e, np.abs(ref).max()))
            assert e <= AUTOGRAD_BAR, (w, name, e)


@pytest.mark.parametrize("S,B", cases.CPU_SIZES)
def test_f32_signs_against_f64(seeded, S, B):
    """The two forms are the same arithmetic on signs: where every sign a pixel's gradient is built from agrees they are equal up to the
    final rounding.  The pointwise terms show the signs themselves: an element differs exactly where one of its signs does."""
    seed, arrays = seeded[(S, B)]
    a, b = host.step_losses_grad(*arrays), host.step_losses_grad(*arrays, f64=True)
    assert a["losses"].tobytes() == b["losses"].tobytes() == host.step_losses(*arrays)["losses"].tobytes() and a["sums"].tobytes() == b["sums"].tobytes()
    worst = 0.0
    for name in ("grad_gs", "d_recon_c", "g0", "g1", "g2", "g3", "g4"):
        x, y = np.asarray(a[name], np.float64), b[name]
        differs = np.abs(x - y) > 1e-6 * np.abs(y).max()
        share = float(differs.mean())
        worst = max(worst, share)
        print("train_losses grad S=%d B=%d seed %d %s: share of elements a turned sign moves %.4g%%" % (S, B, seed, name, 100 * share))
        assert x.shape == y.shape and scaled(x[~differs], y[~differs]) <= 1e-6
    assert worst <= cases.SIGN_FLIP_CAP
    assert a["grad_con"].dtype == f32 and scaled(a["grad_con"], a["d_recon_c"].astype(np.float64) + a["d_grad"]) < 1e-6


@pytest.mark.parametrize("S", (32, 64))
def test_adjoint_identities(S):
    rng = np.random.default_rng(S)
    rel = lambda p, q: abs(p - q) / max(abs(p), abs(q))
    for l, scale in enumerate(host.SCALES):
        s = S // scale
        x_s, y_s, x_S, y_S = rng.normal(size=(s, s, 3)), rng.normal(size=(s, s, 3)), rng.normal(size=(S, S, 3)), rng.normal(size=(S, S, 3))
        up, down = host.resize_matrix(S, s), host.resize_matrix(s, S)
        if scale == 1:
            assert np.array_equal(up, np.eye(S)) and np.array_equal(down, np.eye(S))
        assert rel((host.apply_axes(up, x_s) * y_S).sum(), (x_s * host.apply_axes(up.T, y_S)).sum()) <= ADJOINT_BAR              # <U x, y> = <x, U^T y>
        assert rel((host.apply_axes(down, x_S) * y_s).sum(), (x_S * host.apply_axes(down.T, y_s)).sum()) <= ADJOINT_BAR          # R
        assert rel((host.apply_axes(down, x_S) * y_s).sum(), (x_S * host.resize_quarter_t(y_s, scale)).sum()) <= ADJOINT_BAR    # R^T as the quarter taps
        assert rel((host.diff5(x_s) * y_s).sum(), (x_s * host.diff5_t(y_s)).sum()) <= ADJOINT_BAR                               # the difference operator
        # the matrices are resize_bilinear's map: the float32 kernel on float32 data agrees to its own rounding
        x32 = x_S.astype(f32)
        assert np.abs(resize_bilinear(x32, s) - host.apply_axes(down, x32)).max() <= 1e-5
        assert np.abs(resize_bilinear(x_s.astype(f32), S) - host.apply_axes(up, x_s.astype(f32))).max() <= 1e-5


@pytest.mark.parametrize("S", (32, 64, 256))
def test_downsize_reads_two_by_two_quarters(S):
    """For the power-of-two scales, coarse pixel c of the resize S -> S / scale reads exactly rows and columns scale c + scale / 2 - 1 and
    scale c + scale / 2, weight 1/2 per axis: derived from resize_bilinear itself by feeding it unit impulses."""
    for scale in host.SCALES[1:]:
        s = S // scale
        lo, hi = host.resize_quarter_taps(scale)
        m = np.stack([resize_bilinear(np.tile(np.eye(S, dtype=f32)[k][:, None, None], (1, S, 1)), s)[:, 0, 0] for k in range(S)], axis=1)      # [s, S]: row weights
        want = np.zeros((s, S), f32)
        for c in range(s):
            want[c, scale * c + lo] = want[c, scale * c + hi] = 0.5
        assert np.array_equal(m, want), scale
        assert np.array_equal(host.resize_matrix(s, S), want.astype(np.float64))
        mx = np.stack([resize_bilinear(np.tile(np.eye(S, dtype=f32)[k][None, :, None], (S, 1, 1)), s)[0, :, 0] for k in range(S)], axis=1)      # column weights
        assert np.array_equal(mx, want), scale
        # so a fine pixel receives at most one contribution per level
        assert (np.count_nonzero(want, axis=0) <= 1).all()


@pytest.mark.parametrize("check", cases.CONSTRUCTED, ids=lambda c: c.__name__)
def test_constructed_case(check):
    check(cases.host_run)


def test_statement_argument_checks():
    a = host.example_inputs(32, 1)
    for bad in (np.ones(3), np.ones(2, f32), [1.0, 1.0, 1.0], 1.0):
        with pytest.raises(TypeError) as e:
            host.step_losses_grad(*a, upstream=bad)
        assert str(e.value) == host.UPSTREAM_TEXT
    with pytest.raises(ValueError, match="con_rgb must be"):
        host.step_losses_grad(*a[:4], a[4][:, :16])
    assert host.G_TOTAL_WEIGHTS == G_TOTAL_WEIGHTS == (200.0, 200.0, 2.0)
    r = host.step_losses_grad(*a)
    assert set(r) == {"losses", "sums", "grad_gs", "grad_con", "d_recon_c", "d_grad", "g0", "g1", "g2", "g3", "g4"}
    assert r["grad_gs"].shape == (1, 32, 32, 1) and r["grad_con"].shape == (1, 32, 32, 3) and [r["g%d" % l].shape for l in range(5)] == \
        [(1, 32 >> l, 32 >> l, 3) for l in range(5)]


# ---- the binding and the entry point, ahead of any device work
IMAGES = (("img", 3), ("gt", 3), ("mask_sv", 3), ("gs", 1), ("con_rgb", 3))
SIZE_TEXT = "train_losses takes 1..65535 items of side 32, 64, 128 or 256, got B=%d S=%d"
UPSTREAM_TEXT = "upstream must be a float32 tensor of three elements (the weights of recon_gs, recon_c and grad) on %s, or None" % (DEV,)


def _images(b=1, s=32):
    return [d0(b, s, s, c) for _, c in IMAGES]


def _needs_grad(*a):
    a = list(a)
    a[4] = a[4].detach().requires_grad_()                  # keeps the strides and the reported device
    return a


@pytest.mark.parametrize("call", [lambda r, *t: r.step_losses_grad(*t), lambda r, *t: r.step_losses_grad(*t, parts=True), lambda r, *t: r.loss(*t),
                                  lambda r, *t: r.loss(*_needs_grad(*t))], ids=["step_losses_grad", "parts", "loss", "loss_needs_grad"])
def test_binding_image_checks(call):
    runner = TrainLosses(0)

    def refused(error, args):
        with pytest.raises(error) as e:
            call(runner, *args)
        assert type(e.value) is error
        return str(e.value)

    good = _images()
    for k, (name, c) in enumerate(IMAGES):
        swapped = lambda t: good[:k] + [t] + good[k + 1:]
        for bad in (torch.zeros(1, 32, 32, c), d0(1, 32, 32, c, dtype=torch.float64), d0(1, 32, 32)):
            assert refused(TypeError, swapped(bad)) == "%s must be a float32 tensor [B,S,S,%d] on %s" % (name, c, DEV)
        assert refused(ValueError, swapped(d0(1, 32, 32, 2 * c)[..., ::2])) == "%s must be contiguous (NHWC, dense)" % name
        assert refused(ValueError, swapped(d0(1, 32, 32, c + 1))) == "%s must be [1,32,32,%d] like gt, got (1, 32, 32, %d)" % (name, c, c + 1)
    assert refused(ValueError, _images(s=48)) == SIZE_TEXT % (1, 48)
    assert refused(ValueError, _images(b=0)) == SIZE_TEXT % (0, 32)
    assert runner._scratch is None and not runner._weights


def test_binding_upstream_and_weights_checks():
    runner = TrainLosses(0)
    good = _images()
    for bad in (d0(3, dtype=torch.float64), d0(1), d0(2), d0(1, 3), torch.zeros(3), (200.0, 200.0, 2.0), 1.0):
        with pytest.raises(TypeError) as e:
            runner.step_losses_grad(*good, upstream=bad)
        assert str(e.value) == UPSTREAM_TEXT
    with pytest.raises(TypeError) as e:                    # the images come before upstream
        runner.step_losses_grad(*(good[:-1] + [torch.zeros(1, 32, 32, 3)]), upstream=1.0)
    assert str(e.value) == "con_rgb must be a float32 tensor [B,S,S,3] on %s" % (DEV,)
    with pytest.raises(ValueError) as e:
        runner.loss(*good, weights=(1.0, 2.0))
    assert str(e.value) == "weights must be three numbers: those of recon_gs, recon_c and grad"
    assert runner._scratch is None


@pytest.fixture(scope="module")
def lib():
    build_library()            # no-op when the in-tree .so is fresh
    return _lib.load()


def test_scratch_and_offset_queries(lib):
    q, fwd, off = lib.bsr_train_losses_grad_scratch_bytes, lib.bsr_train_losses_scratch_bytes, lib.bsr_train_losses_grad_offset
    for b, s in ((1, 32), (3, 32), (2, 64), (1, 256), (32, 256)):
        px = b * s * s
        maps = [b * (s >> l) ** 2 * 12 for l in range(5)]
        first = fwd(b, s) + 256 + 8 * px                    # the forward's bytes, the totals' block, mask_edge and the sign words
        assert [off(b, s, l) for l in range(5)] == [first + sum(maps[:l]) for l in range(5)]
        assert q(b, s) == (first + sum(maps) + 255) // 256 * 256 and q(b, s) % 256 == 0
    for b, s in ((0, 32), (1, 16), (1, 48), (1, 512), (65536, 32)):
        assert q(b, s) == 0 and off(b, s, 0) == 2 ** 64 - 1
    assert q(65535, 32) > 0 and off(1, 32, -1) == off(1, 32, 5) == 2 ** 64 - 1


def test_entry_point_argument_checks(lib):
    fn = "bsr_train_losses_grad"
    slots = "img gt mask_sv gs con_rgb upstream? B S sums losses3 grad_gs grad_con d_recon_c? d_grad? scratch".split()

    def refused(**over):
        args = [0]
        for slot in slots:
            value = {"B": 2, "S": 32}.get(slot, None if slot.endswith("?") else P)
            args.append(over.get(slot.rstrip("?"), value))
        return getattr(lib, fn)(*args, None), lib.bsr_last_error().decode()

    text = lambda what: (BSR_ERR_ARG, fn + ": " + what)
    for slot in (s for s in slots if not s.endswith("?") and s not in ("B", "S")):
        assert refused(**{slot: None}) == text("null argument"), slot
    for b, s in ((0, 32), (2, 16), (2, 48)):
        assert refused(B=b, S=s) == text("B must be positive and S one of 32, 64, 128, 256 (reference: 256)")
    assert refused(B=65536) == text("B must be 1..65535")
    assert refused(scratch=P + 8) == text("scratch must be 256-byte aligned")
    assert refused(sums=P + 4) == text("sums must be 8-byte aligned")
