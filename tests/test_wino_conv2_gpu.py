"""-m gpu: the Winograd F(2x2, 3x3) kernel of the fp32 res*.conv2 alone (csrc/wino_conv2.h, through bsr_debug_wino_conv) against the
fp64 direct convolution on constructed inputs.

Tolerance: max|got - ref| / max|ref| <= 3 x 7.3e-7.  7.3e-7 is the error of the kernel's arithmetic emulated step by step in float32 on
the CPU (tools/wino_conv2_error.py: fp32 input transform, fp32 products accumulated in channel order, fp32 output transform, the filter
transform in fp64 rounded once) against the fp64 direct convolution, worst over the six res blocks' conv1 outputs of the
tests/golden/model_py_gsc_{64,256} inputs; tests/test_wino_pack_cpu.py checks that the constructed random case used here emulates to no
more than that.  The matrix cores fuse multiply and add where the emulation rounds twice, so the kernel is expected below the figure."""
import numpy as np
import pytest
import torch

from blindshadowremoval_amd import pack
from wino_cases import hot_pixel_positions, random_case, random_weights

TOL = 3 * 7.3e-7


def _ref64(x: torch.Tensor, k9: np.ndarray, b: np.ndarray) -> torch.Tensor:
    """fp64 TF-SAME 3x3 convolution + bias + LeakyReLU(0.3), NHWC in and out (torch on the CPU)."""
    w = torch.from_numpy(k9.reshape(3, 3, 128, 128)).permute(3, 2, 0, 1).contiguous()            # [co, ci, a, b]
    y = torch.nn.functional.conv2d(x.double().permute(0, 3, 1, 2), w, torch.from_numpy(b), padding=1).permute(0, 2, 3, 1)
    return torch.where(y > 0, y, 0.3 * y)


def _run(x: torch.Tensor, k9: np.ndarray, b: np.ndarray, nw: int = 0) -> torch.Tensor:
    from blindshadowremoval_amd import _lib
    lib = _lib.load()
    arr, bias = pack.pack_wino(k9, b)
    dx, dw, db = x.cuda().contiguous(), torch.from_numpy(arr).cuda(), torch.from_numpy(bias).cuda()
    y = torch.full_like(dx, float("nan"))
    B, H, W, _ = x.shape
    _lib.check(lib.bsr_debug_wino_conv(dx.data_ptr(), dw.data_ptr(), db.data_ptr(), y.data_ptr(), B, H, W, nw, None), "bsr_debug_wino_conv")
    torch.cuda.synchronize()
    return y.cpu()


def _rel(got, ref) -> float:
    return float((got.double() - ref).abs().max() / ref.abs().max())


# feature maps: 32x32 = a 256x256 image; 36x64 = a 288x512 one (not square, not a power of two, two tile columns)
@pytest.mark.gpu
@pytest.mark.parametrize("B,H,W", [(1, 32, 32), (2, 32, 32), (10, 32, 32), (16, 32, 32), (32, 32, 32), (2, 36, 64), (16, 36, 64)])
def test_random_inputs_track_the_fp64_direct_convolution(B, H, W):
    x, k9, b = random_case(B, H, W, seed=B + H)
    x = torch.from_numpy(x)
    ref = _ref64(x, k9, b)
    got = _run(x, k9, b)
    err = _rel(got, ref)
    print("wino conv2 B=%d %dx%d: rel err %.3e (tolerance %.3e)" % (B, H, W, err, TOL))
    assert torch.isfinite(got).all()
    assert err <= TOL
    # both workgroup shapes, and any batch an image is in, give the same bits
    assert torch.equal(_run(x, k9, b, 4), got) and torch.equal(_run(x, k9, b, 2), got)
    assert torch.equal(_run(x[-1:], k9, b), got[-1:])


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", [(32, 32), (36, 64)])
def test_a_single_hot_pixel_at_every_border_corner_and_seam(H, W):
    """One image per position: zero but for one pixel (all 128 channels, random values).  Its 3x3 footprint must come out as the direct
    convolution gives it — clipped by the SAME zero padding on all four sides, whole across the 4x32 tile seams — and everything else
    must be LeakyReLU(bias) exactly as the reference has it."""
    k9, b = random_weights(3)
    pos = hot_pixel_positions(H, W)
    for c in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
        assert c in pos
    rng = np.random.default_rng(17)
    worst = 0.0
    for i0 in range(0, len(pos), 32):
        chunk = pos[i0:i0 + 32]
        x = torch.zeros(len(chunk), H, W, 128)
        for n, (yy, xx) in enumerate(chunk):
            x[n, yy, xx] = torch.from_numpy(rng.standard_normal(128).astype(np.float32)) * 4
        ref = _ref64(x, k9, b)
        got = _run(x, k9, b)
        per_image = (got.double() - ref).abs().amax(dim=(1, 2, 3)) / ref.abs().amax(dim=(1, 2, 3))
        bad = [(chunk[n], float(e)) for n, e in enumerate(per_image) if not e <= TOL]
        assert not bad, bad[:8]
        worst = max(worst, float(per_image.max()))
    print("wino conv2 hot pixels %dx%d: %d positions, worst rel err %.3e (tolerance %.3e)" % (H, W, len(pos), worst, TOL))


@pytest.mark.gpu
def test_bad_shapes_are_refused():
    from blindshadowremoval_amd import _lib
    lib = _lib.load()
    x = torch.zeros(1, 32, 32, 128).cuda()
    w = torch.zeros(8 * 16 * 128 * 16).cuda()
    for (H, W, nw) in ((30, 32, 0), (32, 48, 0), (32, 32, 3)):
        assert lib.bsr_debug_wino_conv(x.data_ptr(), w.data_ptr(), w.data_ptr(), x.data_ptr(), 1, H, W, nw, None) != 0
