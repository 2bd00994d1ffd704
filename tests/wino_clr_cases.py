"""Shared by tests/test_wino_clr_cpu.py and tests/test_wino_clr_gpu.py: constructed weights and inputs of the colour tail, its float64
statement (the oracle's colour_tail arithmetic on folded weights: clr_conv1 3x3 SAME over cat[gs, f] + LeakyReLU(0.3), clr_conv2 1x1 +
LeakyReLU(0.3), clr_conv3 1x1, dif = gray(con_rgb) - gray(inputs)), and a float32 emulation of csrc/wino_clr.h's arithmetic."""
import numpy as np

from blindshadowremoval_amd import pack

# the emulation's max|emulated - fp64| / max|fp64| of clr_conv1 (before the activation) as printed by tests/test_wino_clr_cpu.py on random
# inputs at 16x64, gs in [0, 1], f at scales 1 and 8: 3.0e-7 .. 4.1e-7 over the seeds there; the direct fp32 chain gives 8.7e-7 .. 9.7e-7
EMULATED_ERROR = 4.1e-7

GRAY = np.array([0.2989, 0.5870, 0.1140])


def random_weights(seed: int):
    """Folded weights as the blob holds them (float32 values): k1 [9 taps, 65 = gs | f, 16], b1 [16], k2 [16, 16], b2 [16], k3 [16, 3], b3 [3]."""
    g = np.random.default_rng(seed)
    f32 = lambda a: a.astype(np.float32)
    return {"k1": f32(g.normal(0, (9 * 65) ** -0.5, (9, 65, 16))), "b1": f32(g.normal(0, 0.1, 16)),
            "k2": f32(g.normal(0, 0.25, (16, 16))), "b2": f32(g.normal(0, 0.1, 16)),
            "k3": f32(g.normal(0, 0.25, (16, 3))), "b3": f32(g.normal(0, 0.1, 3))}


def images(w):
    """The blob's images of these weights: 'clr_conv1' [2][9][16][36], 'clr_conv1.gs' [16][16], bias [16], 'tail.w' [337]."""
    direct, bias = pack.pack_taps(w["k1"][:, 1:, :], w["b1"], 32, 64, 16)
    w_gs = np.zeros((16, 16), np.float32)
    w_gs[:, :9] = w["k1"][:, 0, :].T
    tail = np.concatenate([w["k2"].reshape(-1), w["b2"], w["k3"].reshape(-1), w["b3"]]).astype(np.float32)
    return np.ascontiguousarray(direct), w_gs, bias, tail


def random_inputs(B: int, H: int, W: int, seed: int, f_scale: float = 1.0):
    g = np.random.default_rng(seed)
    gs = g.random((B, H, W, 1)).astype(np.float32)
    f = (g.normal(0, f_scale, (B, H, W, 64))).astype(np.float32)
    inputs = g.random((B, H, W, 3)).astype(np.float32)
    return gs, f, inputs


def conv1_64(gs, f, w):
    """clr_conv1 before its activation, float64: [B,H,W,16]."""
    x = np.concatenate([gs, f], axis=3).astype(np.float64)
    B, H, W, _ = x.shape
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))
    y = np.zeros((B, H, W, 16))
    k1 = w["k1"].astype(np.float64)
    for a in range(3):
        for b in range(3):
            y += xp[:, a:a + H, b:b + W, :] @ k1[3 * a + b]
    return y + w["b1"].astype(np.float64)


def tail64(gs, f, inputs, w):
    """-> (con_rgb [B,H,W,3], dif [B,H,W,1]) in float64."""
    leaky = lambda v: np.maximum(v, 0.3 * v)
    y1 = leaky(conv1_64(gs, f, w))
    y2 = leaky(y1 @ w["k2"].astype(np.float64) + w["b2"].astype(np.float64))
    con = y2 @ w["k3"].astype(np.float64) + w["b3"].astype(np.float64)
    dif = (con @ GRAY - inputs.astype(np.float64) @ GRAY)[..., None]
    return con, dif


WINO_BT = np.array([[1.0, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], np.float32)
WINO_AT = np.array([[1.0, 1, 1, 0], [0, 1, -1, -1]], np.float32)


def conv1_wino32(gs, f, w):
    """clr_conv1 before its activation the way csrc/wino_clr.h computes it, every operation in float32: U = pack's transform (float64,
    rounded once), V = B^T d B per 2x2 output patch, the 64 f channels then the gs channel accumulated one by one at each of the 16
    positions, Y = A^T M A, + bias."""
    k1 = w["k1"]
    u = pack.wino_filter_transform(np.concatenate([k1[:, 1:, :], k1[:, :1, :]], axis=1))      # [16, 65 = f | gs, 16] float32
    x = np.concatenate([f, gs], axis=3).astype(np.float32)
    B, H, W, K = x.shape
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))
    # d[b, py, px, a, c, k]: the 4x4 window of patch (py, px)
    d = np.stack([np.stack([xp[:, a:a + H:2, c:c + W:2, :] for c in range(4)], axis=3) for a in range(4)], axis=3)
    t = np.zeros_like(d)
    for i in range(4):      # rows: adds and subtractions only, float32 throughout
        t[:, :, :, i] = sum(WINO_BT[i, a] * d[:, :, :, a] for a in range(4) if WINO_BT[i, a] != 0)
    v = np.zeros_like(d)
    for j in range(4):
        v[:, :, :, :, j] = sum(WINO_BT[j, c] * t[:, :, :, :, c] for c in range(4) if WINO_BT[j, c] != 0)
    m = np.zeros(d.shape[:5] + (16,), np.float32)
    for k in range(K):
        m += v[..., k:k + 1] * u.reshape(4, 4, K, 16)[None, None, None, :, :, k, :]
    t2 = np.stack([(m[:, :, :, 0] + m[:, :, :, 1]) + m[:, :, :, 2], (m[:, :, :, 1] - m[:, :, :, 2]) - m[:, :, :, 3]], axis=3)      # [b, py, px, 2, 4, n]
    y = np.stack([(t2[:, :, :, :, 0] + t2[:, :, :, :, 1]) + t2[:, :, :, :, 2], (t2[:, :, :, :, 1] - t2[:, :, :, :, 2]) - t2[:, :, :, :, 3]], axis=4)
    assert y.dtype == np.float32 and v.dtype == np.float32
    out = y.transpose(0, 1, 3, 2, 4, 5).reshape(B, H, W, 16)      # [b, py, dy, px, dx, n]
    return out + w["b1"]


def conv1_direct32(gs, f, w):
    """The direct fp32 chain: taps and channels accumulated one by one in float32."""
    x = np.concatenate([f, gs], axis=3).astype(np.float32)
    k1 = np.concatenate([w["k1"][:, 1:, :], w["k1"][:, :1, :]], axis=1)
    B, H, W, K = x.shape
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))
    y = np.zeros((B, H, W, 16), np.float32)
    for k in range(K):
        for tap in range(9):
            y += xp[:, tap // 3:tap // 3 + H, tap % 3:tap % 3 + W, k:k + 1] * k1[tap, k]
    return y + w["b1"]
