"""The host statement of d per_loss / d con_rgb (blindshadowremoval_amd/perceptual.py: per_loss_grad) on its own.

Against torch autograd in float64 (perceptual_grad_cases.torch_grad, an independent form built from torch's own operators and their
registered gradients): within 4 x the difference tools/make_perceptual_grad_fixture.py measured over these very sizes and recorded in
tests/golden/perceptual_grad_*.npz, and never above 1e-9 of the largest gradient magnitude.

Against central finite differences of per_loss_f64 along random directions.  The loss is piecewise linear, so away from kinks the
difference quotient is exact and what is left is the rounding of the two float64 loss values: each is allowed 64 ulps (five means of
non-negative terms behind thirteen layers of 9 C_in-term sums; the measured figures, printed, are a few ulps), so
|fd - <grad, v>| <= 64 * 2^-53 * loss / step.  The inputs are uniform noise (perceptual.example_inputs has flat regions, whose pooling
windows tie: a kink the central difference averages over), and the step, 1e-7, and the seeds below were chosen on the CPU so that no
kink is crossed: at 1e-6 the same directions cross ReLU kinks and miss by 1e-2."""
import os

import numpy as np
import pytest

from blindshadowremoval_amd import pack, perceptual as host
from blindshadowremoval_amd.weights import VGG_LAYERS, init_vgg_weights, vgg_variable_shapes

import perceptual_cases as cases
import perceptual_grad_cases as gcases

f32 = np.float32
FD_STEP = 1e-7
FD_CASES = ((32, 2, 6, (100, 101)), (32, 1, 7, (100, 101)))          # S, B, the inputs' seed, the two directions' seeds


@pytest.fixture(scope="module")
def vgg_weights():
    return init_vgg_weights(21)


def host_run(weights, gt, con_rgb, upstream=None):
    return host.per_loss_grad(weights, gt, con_rgb, upstream=upstream)


@pytest.mark.parametrize("S,B", gcases.GRAD_SIZES)
def test_statement_matches_torch_autograd(golden_dir, vgg_weights, S, B):
    measured = float(np.load(os.path.join(golden_dir, "perceptual_grad_32.npz"))["measured_rel"])
    tol = 4 * measured
    assert 0 < tol <= 1e-9
    diff, want = gcases.autograd_difference(vgg_weights, *gcases.inputs(S, B))
    print("perceptual grad S=%d B=%d: statement against autograd %.3g of the largest magnitude %.3g (recorded %.3g)" % (S, B, diff, np.abs(want).max(), measured))
    assert want.shape == (B, S, S, 3) and np.abs(want).max() > 0
    assert diff <= tol


@pytest.mark.parametrize("S,B,seed,dirs", FD_CASES)
def test_statement_matches_central_differences(vgg_weights, S, B, seed, dirs):
    rng = np.random.default_rng(seed)
    gt, con = (rng.uniform(0, 1, (B, S, S, 3)).astype(f32) for _ in range(2))
    r = host.per_loss_grad(vgg_weights, gt, con)
    grad = gcases.statement_grad64(r)
    con64 = con.astype(np.float64)
    for d in dirs:
        v = np.random.default_rng(d).standard_normal(con.shape)
        up, down = (host.per_loss_f64(vgg_weights, gt, con64 + s * FD_STEP * v) for s in (1, -1))
        fd, an = (up - down) / (2 * FD_STEP), float((grad * v).sum())
        bound = 64 * 2.0 ** -53 * max(up, down) / FD_STEP
        print("perceptual grad S=%d B=%d direction %d: finite difference %.12g, <grad, v> %.12g, |difference| %.3g (bound %.3g)" % (S, B, d, fd, an, abs(fd - an), bound))
        assert abs(an) > 1e3 * bound and abs(fd - an) <= bound
    assert abs(host.per_loss_f64(vgg_weights, gt, con) - float(r["loss"][0])) <= 2.0 ** -22 * float(r["loss"][0])


@pytest.mark.parametrize("tap", range(9))
def test_one_tap_layers(tap):
    gcases.check_one_tap_layers(host_run, tap)


def test_tie_map_sends_the_gradient_to_the_first_maximum():
    gcases.check_tie_map(host_run)
    x = np.repeat(np.repeat(np.arange(1.0, 9.0).reshape(1, 2, 2, 2), 2, axis=1), 2, axis=2)          # [1,4,4,2]: four equal positive values per window
    g = np.arange(10.0, 18.0).reshape(1, 2, 2, 2)
    out = host.max_pool_grad(g, x)
    assert np.array_equal(out[:, 0::2, 0::2], g) and out.sum() == g.sum() and np.count_nonzero(out) == g.size
    x[0, 1, 1, 0] += 1                                                                               # now (1, 1) of the first window wins
    out = host.max_pool_grad(g, x)
    assert out[0, 1, 1, 0] == g[0, 0, 0, 0] and out[0, 0, 0, 0] == 0 and out[0, 0, 0, 1] == g[0, 0, 0, 1]
    np.testing.assert_array_equal(out, gcases.first_max_unpool(g, x))


def test_relu_mask_passes_nothing_at_zero():
    y = np.array([-0.0, 0.0, 1e-30, 2.0], f32)
    assert host.relu_mask(np.ones(4), y).tolist() == [0, 0, 1, 1]


def test_seeds_are_signs_times_the_tap_weights():
    B, S = 3, 32
    rng = np.random.default_rng(3)
    feats = [rng.standard_normal((2 * B, h, h, c)).astype(f32) for h, c in zip(host.tap_sides(S), host.TAP_CH)]
    feats[0][B:, 0, 0] = feats[0][:B, 0, 0]
    got = host.seeds(feats, B)
    for k, (s, f) in enumerate(zip(got, feats)):
        w = f32(1.0 / (B * f.shape[1] ** 2 * f.shape[3]))
        assert s.dtype == np.float32 and set(np.unique(s)) <= {-w, f32(0), w}
        np.testing.assert_array_equal(s > 0, f[B:] > f[:B])
    assert not got[0][:, 0, 0].any()


def test_equal_images_give_a_zero_gradient():
    gcases.check_equal_images(host_run)


def test_items_in_the_other_order_give_the_rows_in_the_other_order(vgg_weights):
    gcases.check_item_order(host_run, vgg_weights)


def test_upstream_is_one_float32_multiply(vgg_weights):
    gcases.check_upstream(host_run, vgg_weights)


def test_acts_replace_the_statements_own_forward(vgg_weights):
    gt, con = gcases.inputs(32, 1)
    own = host.per_loss_grad(vgg_weights, gt, con)
    again = host.per_loss_grad(vgg_weights, gt, con, acts=own["acts"])
    assert again["grad"].tobytes() == own["grad"].tobytes() and again["loss"].tobytes() == own["loss"].tobytes()
    flipped = dict(own["acts"])
    flipped["block1_conv1"] = np.zeros_like(own["acts"]["block1_conv1"])          # every mask of the first layer closed: nothing reaches the image
    assert not host.per_loss_grad(vgg_weights, gt, con, acts=flipped)["grad"].any()


def unpack_dgrad(blob):
    """numpy un-pack of pack.pack_vgg_dgrad, written from the layout's description: -> {layer: k' [3,3,C_out,N' padded]}."""
    layout, total = pack.vgg_dgrad_layout()
    arr = np.frombuffer(blob, f32)
    assert arr.size == total
    out = {}
    for name, off, shape in layout:
        nblk, nchunk, taps, cc, nb = shape
        a = arr[off:off + int(np.prod(shape))].reshape(shape)
        full = np.zeros((3, 3, nchunk * cc, nblk * nb), f32)
        for blk in range(nblk):
            for ch in range(nchunk):
                for t in range(taps):
                    full[t // 3, t % 3, ch * cc:(ch + 1) * cc, blk * nb:(blk + 1) * nb] = a[blk, ch, t]
        out[name[:-len("/dgrad")]] = full
    return out


def test_pack_vgg_dgrad_against_a_numpy_unpack(vgg_weights):
    layout, total = pack.vgg_dgrad_layout()
    blob = pack.pack_vgg_dgrad(vgg_weights)
    shapes = vgg_variable_shapes()
    assert [n for n, _, _ in layout] == [n + "/dgrad" for n in VGG_LAYERS]
    assert sum(int(np.prod(s)) for _, _, s in layout) == total and len(blob) == 4 * total
    assert [o for _, o, _ in layout] == list(np.cumsum([0] + [int(np.prod(s)) for _, _, s in layout[:-1]]))
    assert total == sum(9 * s[3] * max(64, s[2]) for n, s in shapes.items() if n.endswith("/kernel")) == 12_976_128
    got = unpack_dgrad(blob)
    for name in VGG_LAYERS:
        k = vgg_weights[name + "/kernel"]
        cin = k.shape[2]
        assert got[name].shape == (3, 3, k.shape[3], max(64, cin))
        for a in range(3):
            for b in range(3):
                np.testing.assert_array_equal(got[name][a, b, :, :cin], k[2 - a, 2 - b].T, err_msg=name)
        assert not got[name][..., cin:].any()
    assert got["block1_conv1"].shape[3] == 64 and np.abs(got["block1_conv1"][..., :3]).max() > 0
    # the packed layer, run as a forward cross-correlation, is the statement's data gradient
    rng = np.random.default_rng(5)
    g = rng.standard_normal((1, 6, 6, 64))
    from blindshadowremoval_amd.discriminator import conv2d_same
    np.testing.assert_allclose(conv2d_same(g, got["block1_conv1"][..., :3], np.zeros(3), 1), host.conv_dgrad(vgg_weights, "block1_conv1", g), rtol=0, atol=1e-12)
