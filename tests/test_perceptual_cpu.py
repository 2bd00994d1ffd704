"""The host statement blindshadowremoval_amd/perceptual.py on its own: the variable table, the `.npz` and blob round trips, the
preprocessing, the totals, and the constructed cases of tests/perceptual_cases.py (shared with the device suite)."""
import numpy as np
import pytest

from blindshadowremoval_amd import objective, pack
from blindshadowremoval_amd import perceptual as host
from blindshadowremoval_amd import weights as W

import perceptual_cases as cases

f32 = np.float32


@pytest.fixture(scope="module")
def vgg_weights():
    return W.init_vgg_weights(3)


def host_run(weights, gt, con_rgb):
    return host.per_loss(weights, gt, con_rgb)


def test_variable_table():
    shapes = W.vgg_variable_shapes()
    assert len(shapes) == 26 and len(W.VGG_LAYERS) == 13
    assert list(shapes)[:2] == ["block1_conv1/kernel", "block1_conv1/bias"] and list(shapes)[-2:] == ["block5_conv1/kernel", "block5_conv1/bias"]
    widths = [shapes[n + "/kernel"][3] for n in W.VGG_LAYERS]
    assert widths == [64, 64, 128, 128, 256, 256, 256, 256, 512, 512, 512, 512, 512]
    cin = 3
    for n in W.VGG_LAYERS:
        assert shapes[n + "/kernel"] == (3, 3, cin, shapes[n + "/bias"][0])
        cin = shapes[n + "/bias"][0]
    assert W.VGG_TAPS == ("block1_conv1", "block2_conv1", "block3_conv1", "block4_conv1", "block5_conv1")
    assert host.TAP_CH == (64, 128, 256, 512, 512) and host.tap_sides(32) == [32, 16, 8, 4, 2]
    assert sum(int(np.prod(s)) for s in shapes.values()) == 9 * 1_437_888 + 3_968         # kernel floats (sum of C_in * C_out = 1_437_888) + biases


def test_init_is_seeded_and_checked(vgg_weights):
    again = W.init_vgg_weights(3)
    assert all(vgg_weights[k].tobytes() == again[k].tobytes() and vgg_weights[k].dtype == f32 for k in vgg_weights)
    assert vgg_weights["block3_conv2/kernel"].tobytes() != W.init_vgg_weights(4)["block3_conv2/kernel"].tobytes()
    k = vgg_weights["block4_conv2/kernel"]
    assert abs(float(k.std()) / np.sqrt(2.0 / (9 * 512)) - 1) < 0.01          # He-normal
    bad = dict(vgg_weights)
    del bad["block2_conv1/bias"]
    with pytest.raises(ValueError, match="missing"):
        W.check_vgg_weights(bad)
    bad = dict(vgg_weights, **{"block2_conv1/bias": np.zeros(64, f32)})
    with pytest.raises(ValueError, match="shape"):
        W.check_vgg_weights(bad)


def test_npz_round_trip(tmp_path, vgg_weights):
    path = str(tmp_path / "vgg.npz")
    W.save_vgg_weights(path, vgg_weights)
    back = W.load_vgg_weights(path)
    assert list(back) == list(W.vgg_variable_shapes()) and all(back[k].tobytes() == vgg_weights[k].tobytes() for k in back)
    np.savez(str(tmp_path / "short.npz"), **{k: v for k, v in vgg_weights.items() if k != "block5_conv1/kernel"})
    with pytest.raises(ValueError, match="block5_conv1/kernel"):
        W.load_vgg_weights(str(tmp_path / "short.npz"))


def test_pack_round_trip_and_layout(vgg_weights):
    layout, total = pack.vgg_layout()
    assert len(layout) == 26 and all(off % 4 == 0 for _, off, _ in layout)
    assert layout[0] == ("block1_conv1/w", 0, (1, 1, 9, 8, 64)) and layout[2][2] == (1, 4, 9, 16, 64) and layout[-2][2] == (8, 32, 9, 16, 64)
    ends = [off + int(np.prod(shape)) for _, off, shape in layout]
    assert [off for _, off, _ in layout[1:]] == ends[:-1] and ends[-1] == total
    blob = pack.pack_vgg(vgg_weights)
    assert len(blob) == 4 * total == 51_791_360                                  # + 5 * 9 * 64 floats of padding in the first layer
    back = pack.unpack_vgg(blob)
    assert all(back[k].tobytes() == vgg_weights[k].tobytes() for k in vgg_weights)
    arr = np.frombuffer(blob, f32)
    # one word by hand: layer block3_conv2 (256 -> 256), tap (2, 1), input channel 37, output channel 200
    name, off, shape = next(e for e in layout if e[0] == "block3_conv2/w")
    idx = off + ((((200 // 64) * shape[1] + 37 // 16) * 9 + 2 * 3 + 1) * 16 + 37 % 16) * 64 + 200 % 64
    assert arr[idx] == vgg_weights["block3_conv2/kernel"][2, 1, 37, 200]
    first = arr[:9 * 8 * 64].reshape(9, 8, 64)
    assert not first[:, 3:].any() and np.array_equal(first[:, :3], vgg_weights["block1_conv1/kernel"].reshape(9, 3, 64))
    with pytest.raises(ValueError, match="blob"):
        pack.unpack_vgg(blob[:-4])


def test_preprocessing_is_caffe_mode_in_float32():
    gt, con = cases.inputs(32, 2, 5)
    x = host.preprocess(gt, con)
    assert x.dtype == f32 and x.shape == (4, 32, 32, 3)
    px = con[1, 7, 9]
    want = np.array([f32(px[2] * f32(255)) - f32(103.939), f32(px[1] * f32(255)) - f32(116.779), f32(px[0] * f32(255)) - f32(123.68)], f32)
    assert x[3, 7, 9].tobytes() == want.tobytes()
    assert host.preprocess(np.ones((1, 32, 32, 3), f32), np.zeros((1, 32, 32, 3), f32))[1, 0, 0].tolist() == [-f32(103.939), -f32(116.779), -f32(123.68)]


def test_forward_shapes_and_the_loss_formula(vgg_weights):
    gt, con = cases.inputs(32, 2, 6)
    r = host.per_loss(vgg_weights, gt, con)
    acts = r["acts"]
    assert list(acts) == ["input", "block1_conv1", "block1_conv2", "block1_pool", "block2_conv1", "block2_conv2", "block2_pool", "block3_conv1",
                          "block3_conv2", "block3_conv3", "block3_conv4", "block3_pool", "block4_conv1", "block4_conv2", "block4_conv3", "block4_conv4",
                          "block4_pool", "block5_conv1"]
    assert acts["block5_conv1"].shape == (4, 2, 2, 512) and acts["block3_pool"].shape == (4, 4, 4, 256) and acts["block1_conv2"].dtype == np.float64
    assert min(float(a.min()) for n, a in acts.items() if n != "input") == 0.0
    # one value by hand: block2_conv1 at (row 3, y 0, x 15, channel 5), a corner of the 16 x 16 map
    x, k = acts["block1_pool"][3], vgg_weights["block2_conv1/kernel"].astype(np.float64)
    v = sum(float(x[a - 1, 15 + b - 1] @ k[a, b, :, 5]) for a in (1, 2) for b in (0, 1)) + float(vgg_weights["block2_conv1/bias"][5])
    assert abs(acts["block2_conv1"][3, 0, 15, 5] - max(v, 0.0)) <= 1e-9 * max(abs(v), 1.0)
    # the loss from its definition: the means of |real - fake| over the float32 features
    m = [float(np.mean(np.abs(acts[n].astype(f32)[:2].astype(np.float64) - acts[n].astype(f32)[2:].astype(np.float64)))) for n in W.VGG_TAPS]
    assert r["sums"].shape == (2, 5) and r["loss"].dtype == f32 and r["loss"].shape == (1,)
    assert abs(float(r["loss"][0]) - sum(m)) <= 2.0 ** -23 * sum(m)
    assert host.PER_SUM_NAMES == ("l1_block1", "l1_block2", "l1_block3", "l1_block4", "l1_block5")


def test_totals_are_float32_in_the_reference_order():
    gs, c, grad, gen, per = f32(0.0123), f32(0.0345), f32(0.31), f32(-0.72), f32(39.5)
    recon = (gs + c) / f32(2)
    want = ((recon * f32(400) + gen) + per * f32(.005)) + grad * f32(2)
    got = objective.g_total_loss(gs, c, grad, gen, per)
    assert got.dtype == f32 and got.tobytes() == f32(want).tobytes()
    assert abs(float(got) - ((0.0123 + 0.0345) / 2 * 400 - 0.72 + 39.5 * .005 + 0.62)) < 1e-5
    d = objective.d_total_loss(f32(0.4), f32(0.7))
    assert d.dtype == f32 and d == f32(0.4) + f32(0.7)


def test_input_checks():
    z = np.zeros((1, 32, 32, 3), f32)
    with pytest.raises(ValueError, match="32, 64, 128 or 256"):
        host.check_inputs(np.zeros((1, 48, 48, 3), f32), np.zeros((1, 48, 48, 3), f32))
    with pytest.raises(ValueError, match="1..4096"):
        host.check_inputs(np.zeros((0, 32, 32, 3), f32), np.zeros((0, 32, 32, 3), f32))
    with pytest.raises(ValueError, match="con_rgb must be"):
        host.check_inputs(z, np.zeros((2, 32, 32, 3), f32))
    assert host.check_inputs(z, z) == (1, 32)


@pytest.mark.parametrize("tap", range(9))
def test_one_tap_layers_at_32(tap):
    cases.check_one_tap_layers(host_run, tap)


@pytest.mark.parametrize("check", cases.CONSTRUCTED, ids=lambda c: c.__name__)
def test_constructed_case_at_32(check):
    check(host_run)
