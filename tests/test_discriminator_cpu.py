"""The host statement of train_step's three discriminators and GAN losses (blindshadowremoval_amd/discriminator.py), its weights, bundle
reader and packer, without a GPU: the variable table against the reference's index files, the round trips, and the constructed cases
of discriminator_cases.py on the host statement."""
import json
import os

import numpy as np
import pytest

from blindshadowremoval_amd import discriminator as host
from blindshadowremoval_amd import pack, tf_bundle
from blindshadowremoval_amd.weights import (check_discriminator_weights, discriminator_variable_shapes, generator_variable_shapes,
                                            init_discriminator_weights)

import discriminator_cases as cases

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
f32 = np.float32


def host_run(weights, gt, con_rgb, mask_sv):
    return host.gan_losses(weights, gt, con_rgb, mask_sv)


def test_variable_shapes_equal_the_reference_index_files():
    with open(os.path.join(GOLDEN, "disc_ckpt_inventory.json")) as f:
        inv = json.load(f)
    spec = {k: list(v) for k, v in discriminator_variable_shapes().items()}
    assert sorted(inv) == ["gsc", "rgb", "tsm"] and len(spec) == 78
    for tag, rec in inv.items():
        assert rec["variables"] == spec, tag
        assert rec["n_params"] == sum(int(np.prod(s)) for s in spec.values())
    assert [tuple(spec["discriminator_2/conv_stack/%d/conv/kernel" % i]) for i in range(4)] == [(4, 4, 6, 32), (4, 4, 32, 32), (4, 4, 32, 64), (4, 4, 64, 64)]
    assert tuple(spec["discriminator_3/conv2/conv/kernel"]) == (4, 4, 64, 1)


def test_init_weights_follow_the_recipe_and_the_check_refuses_others():
    w = init_discriminator_weights(3)
    check_discriminator_weights(w)
    assert all(v.dtype == f32 for v in w.values())
    k = w["discriminator_1/conv_stack/3/conv/kernel"]
    assert abs(float(k.std()) / np.sqrt(1.6 / 1024) - 1) < 0.02
    assert w["discriminator_1/conv_stack/0/bnorm/gamma"].min() >= 0.8 and w["discriminator_2/conv_stack/1/bnorm/moving_variance"].max() <= 1.25
    assert not np.array_equal(w["discriminator_1/conv2/conv/kernel"], w["discriminator_2/conv2/conv/kernel"])
    assert np.array_equal(init_discriminator_weights(3)["discriminator_3/conv2/conv/kernel"], w["discriminator_3/conv2/conv/kernel"])
    bad = dict(w)
    del bad["discriminator_2/conv2/conv/bias"]
    with pytest.raises(ValueError, match="missing"):
        check_discriminator_weights(bad)
    bad = dict(w, **{"discriminator_1/conv_stack/0/conv/kernel": np.zeros((4, 4, 8, 32), f32)})
    with pytest.raises(ValueError, match="shape"):
        check_discriminator_weights(bad)
    assert len(generator_variable_shapes()) == 258                      # the generator's table is untouched


def test_bundle_round_trip_beside_a_generator(tmp_path):
    w = init_discriminator_weights(4)
    prefix = str(tmp_path / "ckpt-1")
    tf_bundle.write_bundle(prefix, w, key_prefix="")
    back = tf_bundle.load_discriminator_weights(prefix)
    assert sorted(back) == sorted(w) and all(np.array_equal(back[k], w[k]) for k in w)
    assert tf_bundle.discriminator_inventory(prefix + ".index") == {k: tuple(v.shape) for k, v in w.items()}
    assert tf_bundle.load_generator_weights(prefix) == {} and tf_bundle.latest_checkpoint(str(tmp_path)) == prefix
    # the default still writes generator/ keys, which the discriminator reader skips
    g = {"conv1/conv/bias": np.arange(32, dtype=f32)}
    tf_bundle.write_bundle(prefix, g)
    assert tf_bundle.load_discriminator_weights(prefix) == {} and np.array_equal(tf_bundle.load_generator_weights(prefix)["conv1/conv/bias"], g["conv1/conv/bias"])


def test_pack_round_trip_gives_the_folded_weights():
    w = init_discriminator_weights(5)
    blob = pack.pack_discriminators(w)
    layout, per = pack.disc_layout()
    assert len(blob) == 3 * per * 4 and all(off % 4 == 0 for _, off, _ in layout)
    back = pack.unpack_discriminators(blob)
    for k in (1, 2, 3):
        folded = pack.disc_folded(w, k)
        assert sorted(back[k - 1]) == sorted(folded) == ["conv0", "conv1", "conv2", "conv3", "head"]
        for name, (kern, bias) in folded.items():
            assert np.array_equal(back[k - 1][name][0], kern) and np.array_equal(back[k - 1][name][1], bias), name
        k0 = folded["conv0"][0]
        assert k0.shape == (16, 8, 32) and not k0[:, 6:].any() and k0[:, :6].all()
        # folded is what the statement computes: output pixel (1, 1) of the first layer on a 4 x 4 map, in float64
        st = "discriminator_%d/conv_stack/0/" % k
        x = np.random.default_rng(k).uniform(0, 1, (1, 4, 4, 6))
        want = host.layer(w, k, 0, x)[0, 1, 1]
        patch = np.zeros((16, 8))
        for a in range(4):
            for b in range(4):
                iy, ix = 2 + a - 1, 2 + b - 1
                if iy < 4 and ix < 4:
                    patch[a * 4 + b, :6] = x[0, iy, ix]
        y = np.einsum("tc,tcn->n", patch, k0.astype(np.float64)) + folded["conv0"][1]
        np.testing.assert_allclose(np.where(y >= 0, y, 0.3 * y), want, rtol=0, atol=2e-6)
        assert w[st + "conv/kernel"].shape == (4, 4, 6, 32)
    with pytest.raises(ValueError):
        pack.unpack_discriminators(blob[:-4])


def test_same_padding_and_map_sides():
    assert host.same_pad(8, 4, 2) == (1, 1) and host.same_pad(1, 4, 2) == (1, 2) and host.same_pad(2, 4, 2) == (1, 1)
    assert host.same_pad(1, 4, 1) == (1, 2) and host.same_pad(16, 4, 1) == (1, 2)
    assert host.map_sides(32, 3) == [8, 4, 2, 1, 1, 1] and host.map_sides(256, 1) == [256, 128, 64, 32, 16, 16]
    assert [host.final_side(S, k) for S in (32, 64, 128, 256) for k in (1, 2, 3)] == [2, 1, 1, 4, 2, 1, 8, 4, 2, 16, 8, 4]


def test_forward_returns_every_activation_and_the_resized_inputs_are_single_lerps():
    gt, con, mask = cases.inputs(32, 2, 3)
    acts = host.forward(init_discriminator_weights(2), gt, con, mask)
    assert sorted(acts) == sorted("d%d/%s" % (k, n) for k in (1, 2, 3) for n in ("in", "conv0", "conv1", "conv2", "conv3", "out"))
    x = acts["d1/in"]
    assert x.dtype == f32 and np.array_equal(x[:2, ..., :3], gt) and np.array_equal(x[2:, ..., :3], con) and np.array_equal(x[2:, ..., 3:], mask)
    half = f32(0.5)
    for k, lo in ((2, 0), (3, 1)):
        ds = host.DOWNSIZE[k - 1]
        tl, tr, bl, br = (x[:, lo + dy::ds, lo + dx::ds] for dy in (0, 1) for dx in (0, 1))
        top, bottom = tl + (tr - tl) * half, bl + (br - bl) * half
        assert np.array_equal(acts["d%d/in" % k], top + (bottom - top) * half)
    assert acts["d3/out"].shape == (4, 1, 1, 1) and acts["d1/conv2"].shape == (4, 4, 4, 64) and acts["d1/out"].dtype == np.float64


def test_losses_from_logits_by_hand():
    y1 = np.array([[[0.5, 2.0], [-1.5, 0.25]], [[-3.0, 0.0], [1.0, 4.0]]], f32)         # B = 1: a real and a fake 2 x 2 map
    y2 = np.array([[[0.75]], [[-0.5]]], f32)
    y3 = np.array([[[-2.0]], [[3.0]]], f32)
    r = host.losses_from_logits([y1, y2, y3])
    assert r["sums"].shape == (1, 9) and host.DISC_SUM_NAMES[:3] == ("hinge_real_1", "hinge_fake_1", "fake_1") and host.LOSS_NAMES == ("gen", "disc_real", "disc_fake")
    np.testing.assert_array_equal(r["sums"][0], [0.5 + 0 + 2.5 + 0.75, 0 + 1 + 2 + 5, 2.0, 0.25, 0.5, -0.5, 3.0, 4.0, 3.0])
    np.testing.assert_array_equal(r["losses"], np.array([(-0.5 + 0.5) - 3.0, (3.75 / 4 + 0.25) + 3.0, (8.0 / 4 + 0.5) + 4.0], f32))
    two = host.losses_from_logits([np.concatenate([y[:1], y[:1], y[1:], y[1:]]) for y in (y1, y2, y3)])          # B = 2, both items alike
    np.testing.assert_array_equal(two["losses"], r["losses"])
    np.testing.assert_array_equal(two["sums"], np.repeat(r["sums"], 2, axis=0))


def test_one_tap_layers_on_the_host_statement():
    cases.check_one_tap_layers(host_run)


@pytest.mark.parametrize("check", cases.CONSTRUCTED, ids=lambda c: c.__name__)
def test_constructed_case_on_the_host_statement(check):
    check(host_run)


def test_hinge_case_has_active_and_inactive_logits_on_every_term():
    assert cases.find_hinge_seed() == cases.HINGE_SEED
    args = cases.hinge_case()
    r = host.gan_losses(*args)
    assert cases.hinge_condition(r["logits"], 2)
    shares = []
    for y in r["logits"]:
        shares += [float((1 - y[:2] > 0).mean()), float((1 + y[2:] > 0).mean())]
    print("hinge case seed %d: active shares %s, losses %s" % (cases.HINGE_SEED, np.round(shares, 3), r["losses"]))
    assert all(0 < s < 1 for s in shares) and np.isfinite(r["losses"]).all()


def test_input_checks():
    gt, con, mask = cases.inputs(32, 1, 0)
    w = init_discriminator_weights(1)
    with pytest.raises(ValueError, match="32, 64, 128 or 256"):
        host.forward(w, np.zeros((1, 48, 48, 3), f32), np.zeros((1, 48, 48, 3), f32), np.zeros((1, 48, 48, 3), f32))
    with pytest.raises(ValueError, match="con_rgb must be"):
        host.forward(w, gt, con[:, :16], mask)
    with pytest.raises(ValueError, match="1..32767"):
        host.forward(w, gt[:0], con[:0], mask[:0])
