"""bsr_shadow_synth (csrc/shadow_synth_kernels.h) against the host statement blindshadowremoval_amd/shadow_synth.py: the Perlin map, its
threshold, the brightness mask, the composited mask and the status bit for bit; the three float outputs within the a-priori bound of
shadow_synth_cases.bound (0 for an item without subsurface scattering)."""
import numpy as np
import pytest

from blindshadowremoval_amd import shadow_synth as host

from shadow_synth_cases import all_branches, bound, corner_record, f32, inputs, largest_r, record

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def synth():
    from blindshadowremoval_amd import ShadowSynth
    return ShadowSynth(0)


def run(synth, arrays, draws, out=None):
    dev = torch.device("cuda", 0)
    t = [torch.from_numpy(a).to(dev) for a in arrays]
    B, S = arrays[1].shape[:2]
    aux = torch.zeros((B, 3, S, S), dtype=torch.float32, device=dev)
    res = synth.process_mask(*t, draws, out=out, aux=aux)
    torch.cuda.synchronize()
    return [r.cpu().numpy() for r in res], aux.cpu().numpy()


def check(synth, arrays, draws, label):
    """Device against host for a batch; prints the largest error per output, returns the device's results."""
    (img, mask_sv, mask_edge, status), aux = run(synth, arrays, draws)
    worst = [0.0, 0.0, 0.0]
    for i, d in enumerate(draws):
        ref = host.process_item(*(a[i] for a in arrays), d)
        assert status[i] == ref["status"], (label, i)
        np.testing.assert_array_equal(aux[i, 0], ref["perlin_map"], err_msg="%s item %d: Perlin map" % (label, i))
        np.testing.assert_array_equal((aux[i, 0] > f32(0.15)).astype(f32), ref["thre"])
        np.testing.assert_array_equal(aux[i, 1], ref["bright"], err_msg="%s item %d: brightness mask" % (label, i))
        if ref["status"] == 0:
            np.testing.assert_array_equal(aux[i, 2], ref["mask"][:, :, 0], err_msg="%s item %d: composited mask" % (label, i))
        b_mask, b_img = bound(d)
        for k, (got, want, b) in enumerate(((img[i], ref["img"], b_img), (mask_sv[i], ref["mask_sv"], b_mask), (mask_edge[i], ref["mask_edge"], b_mask))):
            err = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
            worst[k] = max(worst[k], err)
            assert np.isfinite(got).all() and err <= b, "%s item %d output %d: error %.3g over the bound %.3g" % (label, i, k, err, b)
    print("shadow_synth %s: max |device - host| img %.3g mask_sv %.3g mask_edge %.3g" % (label, *worst))
    return img, mask_sv, mask_edge, status


def test_sixteen_branch_combinations_in_one_batch(synth):
    rng = np.random.default_rng(11)
    draws = all_branches(rng, 64)
    arrays = inputs(64, 16, seed=1)
    # the wrapped terms of the disc blur are live: some Perlin item lights the last row and the last column
    thre = [host.process_item(*(a[i] for a in arrays), d)["thre"] for i, d in enumerate(draws)]
    assert any(t[-1, :].any() for t in thre) and any(t[:, -1].any() for t in thre)
    check(synth, arrays, draws, "16 branches S=64")


@pytest.mark.parametrize("disc", [1, 11])
def test_disc_radius_extremes_at_32(synth, disc):
    rng = np.random.default_rng(20 + disc)
    draws = [record(rng, 32, sv=False, ss=ss, disc_sz=np.int32(disc)) for ss in (True, False)]
    check(synth, inputs(32, 2, seed=2), draws, "disc %d S=32" % disc)


@pytest.mark.parametrize("blur", [1, 2])
def test_spatially_varying_blur_sizes(synth, blur):
    rng = np.random.default_rng(30 + blur)
    draws = [record(rng, S, sv=True, ss=False, blur_size=np.int32(blur)) for S in (32, 32)]
    check(synth, inputs(32, 2, seed=3), draws, "SV blur %d S=32" % blur)


@pytest.mark.parametrize("S", [32, 64])
def test_scale_one_and_the_largest_the_size_allows(synth, S):
    rng = np.random.default_rng(40 + S)
    big = largest_r(S)
    assert len(host.gaussian_taps(host.level_sigma(5, big))) == 2 * (S - 1) + 1          # the halo is larger than the image
    draws = [record(rng, S, perlin=p, r=r) for p in (True, False) for r in (f32(1.0), big)]
    check(synth, inputs(S, 4, seed=4), draws, "r in {1, %.4f} S=%d" % (big, S))


@pytest.mark.parametrize("S", [128, 256])
def test_full_range_scale_at_the_large_sizes(synth, S):
    rng = np.random.default_rng(50 + S)
    check(synth, inputs(S, 1, seed=5), [record(rng, S, r=np.nextafter(f32(15.0), f32(0)))], "r -> 15 S=%d" % S)


def test_an_item_equals_itself_run_alone(synth):
    rng = np.random.default_rng(60)
    draws = [record(rng, 64, *c) for c in ((True, True, True, True), (False, True, False, False), (True, False, True, False), (True, True, False, False),
                                           (False, False, True, True))]
    arrays = inputs(64, 5, seed=6)
    batch = check(synth, arrays, draws, "B=5 S=64")
    for k in range(5):
        alone, _ = run(synth, [np.ascontiguousarray(a[k:k + 1]) for a in arrays], draws[k:k + 1])
        for got, want in zip(alone, batch):
            np.testing.assert_array_equal(got[0], want[k])


def test_a_second_call_does_not_see_the_first_ones_extrema(synth):
    rng = np.random.default_rng(70)
    arrays = inputs(32, 3, seed=7)
    dense = [record(rng, 32, sv=sv) for sv in (True, False, True)]
    check(synth, arrays, dense, "dense S=32")
    empty = [record(rng, 32, sv=sv) for sv in (True, False, True)]
    for d in empty:
        for g in d.g_shadow + d.g_guide:
            g[:] = 0
    img, mask_sv, mask_edge, status = check(synth, arrays, empty, "empty S=32")
    assert (status == host.STATUS_EMPTY).all() and not mask_sv.any() and not mask_edge.any()
    np.testing.assert_array_equal(img, np.clip(arrays[1], 0, 1))
    check(synth, arrays, dense, "dense again S=32")


@pytest.mark.parametrize("S", [32, 64])
def test_lit_pixels_in_the_four_corners_only(synth, S):
    """Wrap and offset of the disc blur: a map lit only beside the corners, on all four borders, at the smallest and the largest disc, on
    the spatially varying route, and with the Gaussians behind it."""
    draws = [corner_record(S, sv=False, ss=False, disc_sz=np.int32(1)), corner_record(S, sv=False, ss=False, disc_sz=np.int32(11)),
             corner_record(S, sv=True, ss=False, blur_size=np.int32(2)), corner_record(S, sv=False, ss=True, disc_sz=np.int32(3))]
    arrays = inputs(S, 4, seed=10)
    arrays[3][:] = 1.0                      # the face region covers the corners
    thre = host.process_item(*(a[0] for a in arrays), draws[0])["thre"]
    ys, xs = np.nonzero(thre)
    assert len(ys) and (np.minimum(ys, S - 1 - ys) < 4).all() and (np.minimum(xs, S - 1 - xs) < 4).all()
    assert thre[0].any() and thre[-1].any() and thre[:, 0].any() and thre[:, -1].any()
    check(synth, arrays, draws, "corners S=%d" % S)


def test_a_constant_blend_guidance_selects_the_finest_level(synth):
    """Rule 3 on both sides: status 0 and the same planes where the reference would divide 0 by 0."""
    rng = np.random.default_rng(75)
    draws = [record(rng, 32, sv=True, ss=ss, blur_size=np.int32(b)) for ss, b in ((False, 1), (True, 2))]
    for d in draws:
        for g in d.g_guide:
            g[:] = 0
    img, mask_sv, mask_edge, status = check(synth, inputs(32, 2, seed=11), draws, "constant guidance S=32")
    assert (status == host.STATUS_OK).all() and mask_sv.any()


def test_command_line_entry_device_route_matches_the_host_route(tmp_path):
    from blindshadowremoval_amd.pngio import read_rgb_u8, write_png
    rng = np.random.default_rng(6)
    S = 32
    ang = np.linspace(0, 2 * np.pi, 40, endpoint=False)
    lm = np.concatenate([np.stack([16 + 12 * np.cos(ang), 16 + 12 * np.sin(ang)], 1), rng.uniform(8, 24, (28, 2))]).astype(np.float32)
    src = tmp_path / "src"
    for name in ("a", "b", "c"):
        write_png(str(src / name / (name + ".png")), rng.integers(30, 220, (S, S, 3), dtype=np.uint8))
        np.save(str(src / name / (name + ".npy")), lm)
    assert host.synthesise_folder(str(src), str(tmp_path / "host"), 3, host=True, batch=2) == ["a", "b", "c"]
    assert host.synthesise_folder(str(src), str(tmp_path / "dev"), 3, host=False, batch=2) == ["a", "b", "c"]
    for name in ("a", "b", "c"):
        for suffix in (".png", "-gt.png", "-mask.png"):
            h = read_rgb_u8(str(tmp_path / "host" / name / (name + suffix))).astype(np.int32)
            d = read_rgb_u8(str(tmp_path / "dev" / name / (name + suffix))).astype(np.int32)
            assert h.shape == d.shape == (S, S, 3) and np.abs(h - d).max() <= 1, (name, suffix)
        np.testing.assert_array_equal(np.load(str(tmp_path / "dev" / name / (name + ".npy"))), lm)
        assert read_rgb_u8(str(tmp_path / "dev" / name / (name + "-mask.png"))).any()


def test_out_is_written_in_place(synth):
    rng = np.random.default_rng(80)
    draws = [record(rng, 32), record(rng, 32, perlin=False)]
    arrays = inputs(32, 2, seed=8)
    want, _ = run(synth, arrays, draws)
    dev = torch.device("cuda", 0)
    out = tuple(torch.full((2, 32, 32, 3), 7.0, device=dev) for _ in range(3)) + (torch.full((2,), 9, dtype=torch.int32, device=dev),)
    got, _ = run(synth, arrays, draws, out=out)
    for o, g, w in zip(out, got, want):
        np.testing.assert_array_equal(o.cpu().numpy(), w)
        np.testing.assert_array_equal(g, w)


def test_argument_errors_raise_before_any_launch(synth):
    rng = np.random.default_rng(90)
    dev = torch.device("cuda", 0)
    ok = [torch.from_numpy(a).to(dev) for a in inputs(32, 1, seed=9)]
    bad_s = [torch.zeros((1, 48, 48, c), device=dev) for c in (1, 3, 3, 1)]
    with pytest.raises(ValueError, match="32, 64, 128 or 256"):
        synth.process_mask(*bad_s, [record(rng, 32)])
    strided = torch.zeros((1, 32, 32, 6), device=dev)[..., ::2]
    with pytest.raises(ValueError, match="contiguous"):
        synth.process_mask(ok[0], strided, ok[2], ok[3], [record(rng, 32)])
    with pytest.raises(ValueError, match="REFLECT"):
        synth.process_mask(*ok, [record(rng, 32, r=f32(6.0))])
    with pytest.raises(ValueError, match="records"):
        synth.process_mask(*ok, [])
    with pytest.raises(TypeError):
        synth.process_mask(ok[0].double(), *ok[1:], [record(rng, 32)])
    from blindshadowremoval_amd import _lib
    lib = _lib.load()
    assert lib.bsr_shadow_synth_scratch_bytes(1, 48) == 0 and lib.bsr_shadow_synth_scratch_bytes(65536, 32) == 0
    assert lib.bsr_shadow_synth(0, None, None, None, None, None, 0, 1, 32, None, None, None, None, None, None, None) == 1
    assert b"bsr_shadow_synth" in lib.bsr_last_error()
