"""CPU emulation of the Winograd F(2x2, 3x3) form of res*.conv2 (csrc/wino_conv2.h) against the fp64 direct convolution.

Emulates the kernel's arithmetic step by step in float32 — input transform V = B^T d B, products and accumulation over the 128 input
channels in channel order per transform position (bias as the start value of position (1, 1)), output transform A^T m A, LeakyReLU —
with the filter transform U = G g G^T of the float32 weights done in float64 and rounded once (pack.wino_filter_transform).  The same is done for the direct
form (float32 products, accumulation over taps x channels) so that the two can be set side by side.

Inputs: every res block's conv1 output on the tests/golden/model_py_gsc_{64,256}.npz inputs (fp64 oracle, rounded to float32 as the
GPU's t1 is).  Reported per block: max|t2 - t2_ref| / max|t2_ref|, and the same after the fp64 conv3 + skip (the y3x probe the
stage-parity test `res_head` holds to 1e-5).

    python tools/wino_conv2_error.py
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from blindshadowremoval_amd.pack import fold_bn, wino_filter_transform   # noqa: E402


def direct64(t1: np.ndarray, k9: np.ndarray, bias: np.ndarray) -> np.ndarray:
    """fp64 TF-SAME 3x3 stride-1 convolution + bias + LeakyReLU(0.3).  t1 [B,H,W,K], k9 [9,K,N]."""
    B, H, W, K = t1.shape
    x = np.zeros((B, H + 2, W + 2, K), np.float64)
    x[:, 1:-1, 1:-1] = t1
    acc = np.zeros((B, H, W, k9.shape[2]), np.float64) + bias.astype(np.float64)
    for a in range(3):
        for b in range(3):
            acc += x[:, a:a + H, b:b + W] @ k9[a * 3 + b].astype(np.float64)
    return np.where(acc > 0, acc, 0.3 * acc)


def direct32(t1: np.ndarray, k9: np.ndarray, bias: np.ndarray) -> np.ndarray:
    """The direct kernel's arithmetic: float32 weights, float32 products, float32 accumulation over (tap, channel) from the bias."""
    B, H, W, K = t1.shape
    x = np.zeros((B, H + 2, W + 2, K), np.float32)
    x[:, 1:-1, 1:-1] = t1
    w = k9.astype(np.float32)
    acc = np.zeros((B, H, W, k9.shape[2]), np.float32) + bias.astype(np.float32)
    for a in range(3):
        for b in range(3):
            xs = x[:, a:a + H, b:b + W]
            for k in range(K):
                acc = acc + xs[..., k:k + 1] * w[a * 3 + b, k]
    return np.where(acc > 0, acc, np.float32(0.3) * acc)


def wino32(t1: np.ndarray, k9: np.ndarray, bias: np.ndarray) -> np.ndarray:
    """The Winograd kernel's arithmetic in float32 (see the module docstring)."""
    B, H, W, K = t1.shape
    N = k9.shape[2]
    U = wino_filter_transform(k9.astype(np.float32))                # [16, K, N] float32, from the float32 weights as bsr_create does
    x = np.zeros((B, H + 2, W + 2, K), np.float32)
    x[:, 1:-1, 1:-1] = t1
    # d[a][b]: [B, H/2, W/2, K] — input pixel (2 py - 1 + a, 2 px - 1 + b) of patch (py, px)
    d = [[x[:, a:a + H:2, b:b + W:2] for b in range(4)] for a in range(4)]
    wr = [[d[0][b] - d[2][b] for b in range(4)], [d[1][b] + d[2][b] for b in range(4)],
          [d[2][b] - d[1][b] for b in range(4)], [d[1][b] - d[3][b] for b in range(4)]]
    V = [[wr[a][0] - wr[a][2], wr[a][1] + wr[a][2], wr[a][2] - wr[a][1], wr[a][1] - wr[a][3]] for a in range(4)]
    m = []
    for p in range(16):
        v = V[p // 4][p % 4]
        acc = np.zeros((B, H // 2, W // 2, N), np.float32)
        if p == 5:
            acc = acc + bias.astype(np.float32)
        for k in range(K):
            acc = acc + v[..., k:k + 1] * U[p, k]
        m.append(acc)
    out = np.zeros((B, H, W, N), np.float32)
    t = [[(m[0 + nu] + m[4 + nu]) + m[8 + nu] for nu in range(4)], [(m[4 + nu] - m[8 + nu]) - m[12 + nu] for nu in range(4)]]
    for i in range(2):
        out[:, i::2, 0::2] = (t[i][0] + t[i][1]) + t[i][2]
        out[:, i::2, 1::2] = (t[i][1] - t[i][2]) - t[i][3]
    return np.where(out > 0, out, np.float32(0.3) * out)


def rel(got, ref) -> float:
    return float(np.abs(got.astype(np.float64) - ref).max() / np.abs(ref).max())


def main() -> None:
    import torch
    from blindshadowremoval_amd.weights import init_weights
    from oracle.gsc_oracle import GeneratorOracle, conv2d_same, batchnorm_infer, leaky_relu
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from stage_parity import BLOCK_IN, y3x_ref

    worst = {"wino": (0.0, 0.0), "direct": (0.0, 0.0)}
    for name in ("model_py_gsc_64", "model_py_gsc_256"):
        z = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
        w = init_weights(int(z["weights_seed"]))
        o = GeneratorOracle(w, dtype=torch.float64)
        pr = {}
        o.forward(z["inputs"], z["uv"], probes=pr)
        for i in range(6):
            st = "res_stack/%d/" % i
            xin = pr[BLOCK_IN[i]]
            bn = lambda y, s: batchnorm_infer(y, *[o.w[st + s + "/" + p] for p in ("gamma", "beta", "moving_mean", "moving_variance")])
            t1 = leaky_relu(bn(conv2d_same(xin, o.w[st + "conv1/kernel"], o.w[st + "conv1/bias"], 1), "bnorm1"))
            t1 = t1.numpy().astype(np.float32)
            kk = w[st + "conv2/kernel"]
            k9, b = fold_bn(kk.reshape(9, 128, 128), w[st + "conv2/bias"], {p: w[st + "bnorm2/" + p] for p in ("gamma", "beta", "moving_mean", "moving_variance")})
            ref = direct64(t1, k9, b)

            def y3x(t2):
                y3 = bn(conv2d_same(torch.from_numpy(np.asarray(t2, np.float64)), o.w[st + "conv3/kernel"], o.w[st + "conv3/bias"], 1), "bnorm3")
                return y3x_ref(y3, xin).numpy()
            yref = y3x(ref)
            for form, fn in (("wino", wino32), ("direct", direct32)):
                t2 = fn(t1, k9, b)
                e2, e3 = rel(t2, ref), rel(y3x(t2), yref)
                worst[form] = (max(worst[form][0], e2), max(worst[form][1], e3))
                print("%-18s res%d %-6s t2 %.3e   y3x (conv2's share) %.3e" % (name, i, form, e2, e3))
    for form, (e2, e3) in worst.items():
        print("worst %-6s t2 %.3e  y3x %.3e" % (form, e2, e3))


if __name__ == "__main__":
    main()
