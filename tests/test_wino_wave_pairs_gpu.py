"""-m gpu: the eight-wave form of the Winograd res*.conv2 kernel (csrc/wino_conv2.h: wino_conv2_pairs_kernel, two waves per SIMD, each
holding half of the transform positions) against the four- and two-wave forms, alone through bsr_debug_wino_conv and in a whole forward.

The eight-wave form issues the same matrix instructions in the same order into every accumulator and keeps the operand order of every
sum of the output transform, so it must give the BITS of the other forms (torch.equal), and with them their distance to the fp64 direct
convolution: 3 x 7.3e-7 of the largest output, the tolerance tests/test_wino_conv2_gpu.py derives.

What is new in it is the exchange of one value pair per (patch, output channel) between the two halves of a workgroup.  A random
kernel hides little of that (every tap feeds every transform position), so nine more cases use weights that are zero but for ONE 3x3
tap: the outputs are then O(1) copies of shifted inputs, and a dropped, stale or swapped exchanged value moves them by O(1)."""
import numpy as np
import pytest
import torch

from blindshadowremoval_amd import pack
from blindshadowremoval_amd.weights import init_weights
from wino_cases import hot_pixel_positions, random_case, random_weights

TOL = 3 * 7.3e-7


def _ref64(x: torch.Tensor, k9: np.ndarray, b: np.ndarray) -> torch.Tensor:
    """fp64 TF-SAME 3x3 convolution + bias + LeakyReLU(0.3), NHWC in and out (torch on the CPU)."""
    w = torch.from_numpy(k9.reshape(3, 3, 128, 128)).permute(3, 2, 0, 1).contiguous()            # [co, ci, a, b]
    y = torch.nn.functional.conv2d(x.double().permute(0, 3, 1, 2), w, torch.from_numpy(b), padding=1).permute(0, 2, 3, 1)
    return torch.where(y > 0, y, 0.3 * y)


class _Layer:
    """One layer's packed weights on the device; run(x, nw) = the kernel's output on the CPU (the output buffer starts as NaN)."""

    def __init__(self, k9: np.ndarray, b: np.ndarray):
        from blindshadowremoval_amd import _lib
        self._lib, self.lib = _lib, _lib.load()
        arr, bias = pack.pack_wino(k9, b)
        self.dw, self.db = torch.from_numpy(arr).cuda(), torch.from_numpy(bias).cuda()

    def run(self, x: torch.Tensor, nw: int) -> torch.Tensor:
        dx = x.cuda().contiguous()
        y = torch.full_like(dx, float("nan"))
        B, H, W, _ = x.shape
        self._lib.check(self.lib.bsr_debug_wino_conv(dx.data_ptr(), self.dw.data_ptr(), self.db.data_ptr(), y.data_ptr(), B, H, W, nw, None),
                        "bsr_debug_wino_conv")
        torch.cuda.synchronize()
        return y.cpu()


# 1x4x32: one tile, all four padded borders at once; 1x8x64: two tile rows by two tile columns, both seams; 3x36x64: not square, not a
# power of two
@pytest.mark.gpu
@pytest.mark.parametrize("B,H,W", [(1, 4, 32), (1, 8, 64), (3, 36, 64)])
def test_eight_waves_give_the_bits_of_four_and_two(B, H, W):
    x, k9, b = random_case(B, H, W, seed=B + H)
    x = torch.from_numpy(x)
    layer = _Layer(k9, b)
    got = layer.run(x, 8)
    assert torch.isfinite(got).all()
    ref = _ref64(x, k9, b)
    err = float((got.double() - ref).abs().max() / ref.abs().max())
    print("wino conv2 nw=8 B=%d %dx%d: rel err %.3e (tolerance %.3e)" % (B, H, W, err, TOL))
    assert err <= TOL
    assert torch.equal(got, layer.run(x, 4))
    assert torch.equal(got, layer.run(x, 2))


@pytest.mark.gpu
def test_a_single_hot_pixel_at_every_border_corner_and_seam():
    """One image per position of hot_pixel_positions(8, 64): zero but for one pixel (all 128 channels, random values)."""
    H, W = 8, 64
    k9, b = random_weights(3)
    layer = _Layer(k9, b)
    pos = hot_pixel_positions(H, W)
    for c in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
        assert c in pos
    rng = np.random.default_rng(17)
    for i0 in range(0, len(pos), 64):
        chunk = pos[i0:i0 + 64]
        x = torch.zeros(len(chunk), H, W, 128)
        for n, (yy, xx) in enumerate(chunk):
            x[n, yy, xx] = torch.from_numpy(rng.standard_normal(128).astype(np.float32)) * 4
        got, want = layer.run(x, 8), layer.run(x, 4)
        bad = [chunk[n] for n in range(len(chunk)) if not torch.equal(got[n], want[n])]
        assert not bad, bad[:8]
    print("wino conv2 nw=8 hot pixels %dx%d: %d positions bit-identical to nw=4" % (H, W, len(pos)))


@pytest.mark.gpu
@pytest.mark.parametrize("tap", range(9))
def test_one_tap_weights_expose_the_exchange(tap):
    """Weights that are zero but for tap (tap / 3, tap % 3): a random [128, 128] matrix at O(1 / sqrt(128)), so the outputs are O(1)."""
    rng = np.random.default_rng(40 + tap)
    k9 = np.zeros((9, 128, 128))
    k9[tap] = rng.standard_normal((128, 128)) / np.sqrt(128)
    b = 0.1 * rng.standard_normal(128)
    x = torch.from_numpy(random_case(1, 4, 32, seed=tap)[0])
    layer = _Layer(k9, b)
    got, want = layer.run(x, 8), layer.run(x, 4)
    assert float(want.abs().max()) > 1.0                                  # the O(1) scale the docstring claims
    assert torch.equal(got, want)


PROBES = ["y3x%d" % i for i in range(6)] + ["res%d" % i for i in range(6)] + ["bmask"]


@pytest.mark.gpu
def test_a_whole_forward_is_the_same_with_the_switch_on_and_off(monkeypatch):
    """B = 17 at 256x256 is the smallest batch whose conv2 grid (17 x 8 tiles, more than half of the compute units) takes the full-batch
    form: eight waves by default, four with BSR_WINO_PAIRS=0 (read at bsr_create).  Row 0 alone takes the two-wave form."""
    from blindshadowremoval_amd import Generator
    w = init_weights(1)
    g = torch.Generator().manual_seed(317)
    inp, uv = torch.rand(17, 256, 256, 3, generator=g).cuda(), torch.rand(17, 256, 256, 3, generator=g).cuda()
    pairs = Generator(dtype="f32").load_weights(w)
    monkeypatch.setenv("BSR_WINO_PAIRS", "0")
    four = Generator(dtype="f32").load_weights(w)
    monkeypatch.delenv("BSR_WINO_PAIRS")
    try:
        a = [t.clone() for t in pairs(inp, uv)]
        pa = {n: pairs.probe(n).clone() for n in PROBES}
        b = [t.clone() for t in four(inp, uv)]
        pb = {n: four.probe(n).clone() for n in PROBES}
        for x, y, name in zip(a, b, ("gs", "con_rgb", "mask22", "dif")):
            assert torch.isfinite(x).all(), name
            assert torch.equal(x, y), name
        for n in PROBES:
            assert torch.equal(pa[n], pb[n]), n
        alone = [t.clone() for t in pairs(inp[:1], uv[:1])]
        for x, y, name in zip(alone, a, ("gs", "con_rgb", "mask22", "dif")):
            assert torch.equal(x, y[:1]), name
        assert torch.equal(pairs.probe("bmask"), pa["bmask"][:1])
    finally:
        pairs.close()
        four.close()
