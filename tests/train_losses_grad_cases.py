"""What the CPU and the GPU tests of the reconstruction and gradient losses' backward share (train_losses.step_losses_grad,
bsr_train_losses_grad): the sizes, a float64 torch restatement of the forward for autograd that shares no code with the statement
(F.interpolate for both resizes, a max-pool for the two dilations), the seed rule, and the constructed cases with closed forms.  A
constructed case takes `run(img, gt, mask_sv, gs, con_rgb, upstream=None)` -> dict(grad_gs, grad_con, d_recon_c, d_grad float32,
g0..g4), so the host statement and the device chain run the same cases."""
import numpy as np

from blindshadowremoval_amd import train_losses as host

f32 = np.float32
CPU_SIZES = ((32, 3), (64, 2))                          # (S, B)
GPU_SIZES = ((32, 1), (32, 3), (64, 2), (256, 1))      # S = 32: level 4 is 2 x 2, every coarse pixel an edge pixel of U_4; B = 3: item order
NEAR_ZERO = 1e-9
SIGN_FLIP_CAP = 1e-3                                    # the share of signs that float32 rounding may turn, a condition on the inputs
E2E_MEASURED = 8.3e-8          # the largest scaled error of grad_con measured on GPU_SIZES: S = 32, B = 3 (tools/train_losses_bench.py --grad --parity)
E2E_BOUND = min(4 * E2E_MEASURED, 1e-4)


# ---- the float64 restatement for autograd
def torch_objective(img, gt, mask_sv, gs, con_rgb, weights):
    """numpy float32 inputs -> (objective, gs, con_rgb as float64 leaves, the differences every sign is taken from): the three losses
    weighted by `weights` in float64 torch."""
    import torch
    import torch.nn.functional as F
    nchw = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, f32))).permute(0, 3, 1, 2).double()
    gt_t, mask_t = nchw(gt), nchw(mask_sv)
    gs_t, con_t = nchw(gs).requires_grad_(), nchw(con_rgb).requires_grad_()
    B, _, S, _ = gt_t.shape
    m32 = torch.from_numpy(np.ascontiguousarray(np.asarray(mask_sv, f32))).permute(0, 3, 1, 2)
    bi = (m32 > f32(.01)).double()
    mean_c = ((m32[:, 0] + m32[:, 1]) + m32[:, 2]) / f32(3.0)
    edge0 = (mean_c > f32(.01)).double() - (m32.min(dim=1).values > f32(.3)).double()
    e = (F.max_pool2d(edge0[:, None], 9, 1, 4) > 0).double()                              # two 5 x 5 dilations clipped to the image
    n, d_bi, d_edge = float(B * S * S), bi.sum() + 1e-6, e.sum() + 1e-6
    mix = lambda x, w: (x[:, 0:1] * float(w[0]) + x[:, 1:2] * float(w[1])) + x[:, 2:3] * float(w[2])
    diffs = [gs_t - mix(gt_t, host.GRAY_W), con_t - gt_t] + [mix(con_t, w) - mix(gt_t, w) for w in host.YUV_W]

    def l1(d, channels):                     # l1_loss with no mask, under mask_bi, under mask_edge
        a = d.abs()
        return a.sum() / (n * channels), (a * bi).sum() / d_bi / channels, (a * e).sum() / d_edge / channels
    g0, g1, g2 = l1(diffs[0], 1)
    recon_gs = (g0 + g1 * 30 + g2 * 10) / 41
    c0, c1, c2 = l1(diffs[1], 3)
    yuv = [l1(d, 1) for d in diffs[2:]]
    y0, y1, y2 = (sum(t[i] for t in yuv) / 2 for i in range(3))
    recon_c = (c0 + c1 * 30 + c2 * 10 + y0 + y1 * 30 + y2 * 10) / 82

    def img_grad(x, scale):
        r = x if scale == 1 else F.interpolate(x, size=(S // scale, S // scale), mode="bilinear", align_corners=False, antialias=False)
        dy = F.pad(r[:, :, 1:] - r[:, :, :-1], (0, 0, 0, 1))
        dx = F.pad(r[:, :, :, 1:] - r[:, :, :, :-1], (0, 1, 0, 0))
        g = (dy + dx) * 5
        return g if scale == 1 else F.interpolate(g, size=(S, S), mode="bilinear", align_corners=False, antialias=False)
    dif = 0
    for scale in host.SCALES:
        d = img_grad(con_t, scale) - img_grad(gt_t, scale)
        diffs.append(d)
        a = d.abs()
        dif = dif + (a + 30 * a * bi + 10 * a * e) / 41
    grad = dif.sum() / d_edge
    return (weights[0] * recon_gs + weights[1] * recon_c) + weights[2] * grad, gs_t, con_t, diffs


def autograd_grads(arrays, weights):
    """-> float64 numpy (grad_gs [B,S,S,1], grad_con [B,S,S,3]) of torch_objective."""
    obj, gs_t, con_t, _ = torch_objective(*arrays, weights)
    obj.backward()
    return gs_t.grad.permute(0, 2, 3, 1).numpy().copy(), con_t.grad.permute(0, 2, 3, 1).numpy().copy()


def seed_is_clean(arrays) -> bool:
    """No difference that a sign is taken from lies within NEAR_ZERO of 0 without being exactly 0."""
    import torch
    with torch.no_grad():
        diffs = torch_objective(*arrays, (1.0, 1.0, 1.0))[3]
    return not any(bool(((d.abs() < NEAR_ZERO) & (d != 0)).any()) for d in diffs)


def pick_seed(S: int, B: int, start: int = 0) -> int:
    seed = start
    while not seed_is_clean(host.example_inputs(S, B, seed)):
        seed += 1
    return seed


# ---- the constructed cases
def host_run(img, gt, mask_sv, gs, con_rgb, upstream=None):
    return host.step_losses_grad(img, gt, mask_sv, gs, con_rgb, upstream)


def _flat(S=32, B=1, seed=5):
    """Smooth gt and img, an empty mask, gs = gray(gt) and con_rgb = gt exactly."""
    img, gt, mask_sv, _, _ = host.example_inputs(S, B, seed)
    return [img, gt, np.zeros_like(mask_sv), host.gray(gt)[..., None].astype(f32), gt.copy()]


def case_equal_inputs_give_exact_zeros(run):
    """con_rgb = gt and gs = gray(gt): every difference is exactly 0 at every level, sign(0) = 0, every gradient is exactly +0."""
    a = _flat(32, 2)
    a[2] = host.example_inputs(32, 2, 5)[2]                      # with a mask: the weights are not what makes it 0
    r = run(*a)
    for k in ("grad_gs", "grad_con", "d_recon_c", "d_grad"):
        assert r[k].dtype == f32 and r[k].tobytes() == np.zeros_like(r[k]).tobytes(), k
    for l in range(5):
        assert not np.asarray(r["g%d" % l]).any(), l


def case_constant_gs_offset_empty_mask(run):
    """gs - gray(gt) > 0 everywhere, no mask: grad_gs = u / (41 n) everywhere (n a power of two: the closed form is exact)."""
    a = _flat(32, 2)
    a[3] = (a[3] + f32(0.25)).astype(f32)
    n = 2 * 32 * 32
    for u in (1.0, 4.0):
        r = run(*a, upstream=np.array([u, 1, 1], f32))
        assert r["grad_gs"].tobytes() == np.full((2, 32, 32, 1), u / (41.0 * n), np.float64).astype(f32).tobytes()
        assert not r["grad_con"].any()
    r = run(*a, upstream=np.array([-1, 1, 1], f32))
    assert r["grad_gs"].tobytes() == np.full((2, 32, 32, 1), -1.0 / (41.0 * n), np.float64).astype(f32).tobytes()
    a[3] = (a[3] - f32(0.5)).astype(f32)                         # now below: the sign turns
    r = run(*a)
    assert r["grad_gs"].tobytes() == np.full((2, 32, 32, 1), -1.0 / (41.0 * n), np.float64).astype(f32).tobytes()


def case_mask_channels_weight_the_terms(run):
    """Blocks with one, two and three lit channels of mask_bi.  gs above gray(gt) and channel 0 of con_rgb above gt's everywhere: the
    one-channel terms (gs, Y, U, V) weigh a pixel by nb, the number of lit channels, L1 weighs channel c by bi_c."""
    a = _flat(32, 1)
    m = a[2]
    m[0, 4:8, 4:8, 0] = 0.5
    m[0, 12:16, 4:8, :2] = 0.5
    m[0, 20:24, 4:8, :] = 0.5
    a[3] = (a[3] + f32(0.25)).astype(f32)
    a[4][..., 0] = (a[4][..., 0] + f32(0.125)).astype(f32)
    r = run(*a)
    e = host.find_edge(m)[0].astype(np.float64)
    bi = (m[0] > f32(.01)).astype(np.float64)
    nb = bi.sum(-1)
    assert set(nb[4:8, 4:8].ravel()) == {1.0} and set(nb[12:16, 4:8].ravel()) == {2.0} and set(nb[20:24, 4:8].ravel()) == {3.0}
    n, d_bi, d_edge = 32.0 * 32.0, bi.sum() + 1e-6, e.sum() + 1e-6
    w1 = 1 / n + 30 * nb / d_bi + 10 * e / d_edge
    np.testing.assert_allclose(r["grad_gs"][0, ..., 0], w1 / 41, rtol=1e-6, atol=0)
    s_yuv = np.array([1.0, -1.0, 1.0])                           # the signs of YUV_W[k][0]: channel 0 rose
    for c in range(3):
        a_c = 1 / (3 * n) + 30 * bi[..., c] / (3 * d_bi) + 10 * e / (3 * d_edge)
        yuv_c = sum(s_yuv[k] * float(host.YUV_W[k][c]) for k in range(3))
        want = ((1.0 if c == 0 else 0.0) * a_c + yuv_c * w1 / 2) / 82
        np.testing.assert_allclose(r["d_recon_c"][0, ..., c], want, rtol=1e-6, atol=0)
    # one lit channel against three, away from the edge band's changes: the ratio of the mask_bi parts is 3
    p1, p3 = r["grad_gs"][0, 5, 5, 0] * 41.0 - (1 / n + 10 * e[5, 5] / d_edge), r["grad_gs"][0, 21, 5, 0] * 41.0 - (1 / n + 10 * e[21, 5] / d_edge)
    assert abs(p3 / p1 - 3.0) < 1e-4


def level0_pattern(S, y, x):
    """Where the level-0 part of d_grad lands when con_rgb rises at (y, x) alone, in units of w = weight / d_edge per position: the
    transpose of (dy + dx) * 5 applied to the signs of the three differences that move, written out from the definition."""
    sign = np.zeros((S, S))
    sign[y, x] = -1.0 if (y + 1 < S or x + 1 < S) else 0.0        # g[y, x] loses 5 per neighbour it still has
    if y >= 1:
        sign[y - 1, x] = 1.0
    if x >= 1:
        sign[y, x - 1] = 1.0
    return sign


def case_single_pixel_level0_neighbours(run):
    """con_rgb = gt except channel 1 of one pixel, in the interior, on the last row, on the last column and in the corner.  Levels 1..4
    are silenced by taking their own stated part away: d_grad - sum over l >= 1 of R_l^T rbar_l of the run's own maps g1..g4.  What
    is left is level 0: the transpose of the difference operator applied to three signs, each times its pixel's weight / d_edge."""
    S = 32
    for y, x in ((13, 9), (S - 1, 9), (13, S - 1), (S - 1, S - 1)):
        a = _flat(S, 1)
        a[2][0, 2, 2, :] = 0.2                                    # one lit pixel far away: d_edge is the 7 x 7 band it leaves clipped, not 1e-6
        a[4][0, y, x, 1] = a[4][0, y, x, 1] + f32(0.25)
        r = run(*a)
        e = host.find_edge(a[2])[0].astype(np.float64)
        bi = (a[2][0] > f32(.01)).astype(np.float64)
        d_edge = e.sum() + 1e-6
        d0 = np.zeros((S, S, 3))
        d0[..., 1] = level0_pattern(S, y, x) * ((1 + 30 * bi[..., 1] + 10 * e) / 41) / d_edge
        np.testing.assert_allclose(np.asarray(r["g0"], np.float64)[0], d0, rtol=1e-6, atol=0)
        want = host.diff5_t(d0)
        maps = [np.zeros_like(np.asarray(r["g0"], np.float64))] + [np.asarray(r["g%d" % l], np.float64) for l in range(1, 5)]
        level0 = np.asarray(r["d_grad"], np.float64)[0] - host.d_grad_from_maps(maps)[0]
        scale = np.abs(want).max()
        assert scale > 0 and np.abs(level0 - want).max() <= 1e-5 * scale, (y, x)
        if (y, x) == (13, 9):                                     # the interior, position by position in units of w
            w = 1 / 41 / d_edge
            got = {k: level0[y + k[0], x + k[1], 1] / w for k in ((0, 0), (1, 0), (0, 1), (-1, 0), (0, -1), (-1, 1), (1, -1), (1, 1), (-1, -1))}
            for k, v in {(0, 0): 20, (1, 0): -5, (0, 1): -5, (-1, 0): -10, (0, -1): -10, (-1, 1): 5, (1, -1): 5, (1, 1): 0, (-1, -1): 0}.items():
                assert abs(got[k] - v) < 1e-3, (k, got[k])
        assert not level0[..., 0].any() and not level0[..., 2].any()


def case_upstream_zeros_give_zeros(run):
    a = host.example_inputs(32, 2, 3)
    r = run(*a, upstream=np.zeros(3, f32))
    for k in ("grad_gs", "grad_con", "d_recon_c", "d_grad"):
        assert not r[k].any(), k


def case_each_weight_alone_matches_the_parts(run):
    a = host.example_inputs(32, 2, 3)
    full = run(*a, upstream=np.array([3, 0.5, 7], f32))
    only_gs = run(*a, upstream=np.array([3, 0, 0], f32))
    only_c = run(*a, upstream=np.array([0, 0.5, 0], f32))
    only_g = run(*a, upstream=np.array([0, 0, 7], f32))
    assert only_gs["grad_gs"].tobytes() == full["grad_gs"].tobytes() and not only_gs["grad_con"].any()
    assert only_c["grad_con"].tobytes() == full["d_recon_c"].tobytes() == only_c["d_recon_c"].tobytes() and not only_c["grad_gs"].any()
    assert only_g["grad_con"].tobytes() == full["d_grad"].tobytes() == only_g["d_grad"].tobytes() and not only_g["grad_gs"].any()
    assert np.abs(full["d_grad"]).max() > 0 and np.abs(full["d_recon_c"]).max() > 0


CONSTRUCTED = (case_equal_inputs_give_exact_zeros, case_constant_gs_offset_empty_mask, case_mask_channels_weight_the_terms,
               case_single_pixel_level0_neighbours, case_upstream_zeros_give_zeros, case_each_weight_alone_matches_the_parts)
