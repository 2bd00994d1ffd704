"""CPU emulation of the 25-product form of the transposed 3x3 layers up2 / up3 / clr_up3 (csrc/wino_convt.h) against the fp64 phase
definition of the layer.

Emulates the kernel's arithmetic step by step in float32 — input transform V = B^T d B, products and accumulation over the input
channels in channel order per position, output transform in the kernel's operand order, bias, LeakyReLU — with the filter transform
U = G g G^T of the float32 weights done in float64 and rounded once (pack.wino_convt_filter_transform).  The same is done for the direct
form (float32 products, accumulation over taps x channels from the bias) so that the two can be set side by side.

Inputs: the three layers' real inputs on the tests/golden/model_py_gsc_{64,256}.npz inputs (fp64 oracle, teacher-forced, rounded to
float32 as the GPU's activations are).  Reported per layer: max|out - ref| / max|ref|.  Gate: the worst emulated error of the new form
is at most half of the stages' fp32 budget (F32_CEILING = 1e-5 in tests/test_stage_parity_gpu.py).

    python tools/wino_convt_error.py            # writes what profiles/wino_convt_error.txt holds
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from blindshadowremoval_amd.pack import wino_convt_filter_transform   # noqa: E402

F32_CEILING = 1e-5      # tests/test_stage_parity_gpu.py


def _act(y, act, dtype):
    return np.where(y > 0, y, dtype(0.3) * y) if act else y


def convt_direct64(x: np.ndarray, k9: np.ndarray, bias: np.ndarray, act: bool = True) -> np.ndarray:
    """The repo's phase definition of ConvT(3x3, stride 2, SAME) (csrc/igemm_conv.h) in float64: tap (a, b) of the kernel feeds output
    phase (a == 1, b == 1) from input pixel (i - (a == 2), j - (b == 2)), zero outside.  x [B,H,W,K], k9 [9 = 3a + b, K, N] -> [B,2H,2W,N]."""
    B, H, W, K = x.shape
    xp = np.zeros((B, H + 1, W + 1, K), np.float64)
    xp[:, 1:, 1:] = x
    out = np.zeros((B, 2 * H, 2 * W, k9.shape[2]), np.float64) + bias.astype(np.float64)
    for a in range(3):
        for b in range(3):
            sy, sx = (0 if a == 2 else 1), (0 if b == 2 else 1)
            out[:, (1 if a == 1 else 0)::2, (1 if b == 1 else 0)::2] += xp[:, sy:sy + H, sx:sx + W] @ k9[3 * a + b].astype(np.float64)
    return _act(out, act, np.float64)


def convt_direct32(x: np.ndarray, k9: np.ndarray, bias: np.ndarray, act: bool = True) -> np.ndarray:
    """The direct kernel's arithmetic: float32 weights and products, float32 accumulation over (channel chunk, tap, channel) from the bias."""
    B, H, W, K = x.shape
    xp = np.zeros((B, H + 1, W + 1, K), np.float32)
    xp[:, 1:, 1:] = x
    w = k9.astype(np.float32)
    out = np.zeros((B, 2 * H, 2 * W, k9.shape[2]), np.float32) + bias.astype(np.float32)
    for k0 in range(0, K, 32):
        for a in range(3):
            for b in range(3):
                sy, sx = (0 if a == 2 else 1), (0 if b == 2 else 1)
                xs = xp[:, sy:sy + H, sx:sx + W]
                acc = out[:, (1 if a == 1 else 0)::2, (1 if b == 1 else 0)::2]
                for k in range(k0, min(k0 + 32, K)):
                    acc = acc + xs[..., k:k + 1] * w[3 * a + b, k]
                out[:, (1 if a == 1 else 0)::2, (1 if b == 1 else 0)::2] = acc
    return _act(out, act, np.float32)


def convt_wino32(x: np.ndarray, k9: np.ndarray, bias: np.ndarray, act: bool = True) -> np.ndarray:
    """The 25-product kernel's arithmetic in float32 (see the module docstring).  H and W even."""
    B, H, W, K = x.shape
    N = k9.shape[2]
    U = wino_convt_filter_transform(k9.astype(np.float32))          # [25, K, N] float32, from the float32 weights as bsr_create does
    xp = np.zeros((B, H + 1, W + 1, K), np.float32)
    xp[:, 1:, 1:] = x
    # d[a][b]: [B, H/2, W/2, K] — input pixel (2 py - 1 + a, 2 px - 1 + b) of patch (py, px)
    d = [[xp[:, a:a + H:2, b:b + W:2] for b in range(3)] for a in range(3)]
    c = [[d[1][b] for b in range(3)], [d[2][b] for b in range(3)], [d[0][b] - d[1][b] for b in range(3)], [d[1][b] - d[2][b] for b in range(3)]]
    V = [[c[k][1], c[k][2], c[k][0] - c[k][1], c[k][1] - c[k][2]] for k in range(4)]
    dmap = (0, 1, 2, 0, 3)
    m = {}
    for r in range(5):
        for s in range(5):
            v = V[dmap[r]][dmap[s]]
            acc = np.zeros((B, H // 2, W // 2, N), np.float32)
            for k in range(K):
                acc = acc + v[..., k:k + 1] * U[5 * r + s, k]
            m[r, s] = acc
    out = np.zeros((B, 2 * H, 2 * W, N), np.float32)
    p0 = {s: m[2, s] + m[3, s] for s in range(5)}
    p2 = {s: m[3, s] - m[4, s] for s in range(5)}
    for a, row in ((0, p0), (1, {s: m[0, s] for s in range(5)}), (2, p2), (3, {s: m[1, s] for s in range(5)})):
        out[:, a::4, 0::4] = row[2] + row[3]
        out[:, a::4, 1::4] = row[0]
        out[:, a::4, 2::4] = row[3] - row[4]
        out[:, a::4, 3::4] = row[1]
    out = out + bias.astype(np.float32)
    return _act(out, act, np.float32)


def rel(got, ref) -> float:
    return float(np.abs(got.astype(np.float64) - ref).max() / np.abs(ref).max())


def main() -> int:
    import torch
    from blindshadowremoval_amd import pack
    from blindshadowremoval_amd.weights import init_weights
    from oracle.gsc_oracle import GeneratorOracle

    worst = {"wino": 0.0, "direct": 0.0}
    for name in ("model_py_gsc_64", "model_py_gsc_256"):
        z = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
        w = init_weights(int(z["weights_seed"]))
        o = GeneratorOracle(w, dtype=torch.float64)
        pr = {}
        o.forward(z["inputs"], z["uv"], probes=pr)
        lm = pack.layer_matrices(w)
        ins = {"up2": torch.cat([pr["up1"], pr["x3"]], dim=3), "up3": torch.cat([pr["up2"], pr["x2"]], dim=3), "clr_up3": pr["f2"]}
        outs = {"up2": pr["up2"], "up3": pr["y"], "clr_up3": pr["f"]}
        for layer in ("up2", "up3", "clr_up3"):
            x = ins[layer].numpy().astype(np.float32)
            k9, b = lm[layer]
            k9, b = k9.astype(np.float32), b.astype(np.float32)      # the blob's float32 weights
            ref = convt_direct64(x, k9, b)
            oracle = outs[layer].numpy()
            print("%-18s %-8s in %s  phase definition against the oracle's layer: %.3e" % (name, layer, "x".join(map(str, x.shape)), rel(ref, oracle)))
            for form, fn in (("wino", convt_wino32), ("direct", convt_direct32)):
                e = rel(fn(x, k9, b), ref)
                worst[form] = max(worst[form], e)
                print("%-18s %-8s %-6s max|out - ref| / max|ref| %.3e" % (name, layer, form, e))
    for form, e in worst.items():
        print("worst %-6s %.3e" % (form, e))
    ok = worst["wino"] <= 0.5 * F32_CEILING
    print("gate (worst wino <= %.1e = half the stages' fp32 budget): %s" % (0.5 * F32_CEILING, "PASS" if ok else "FAIL"))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
