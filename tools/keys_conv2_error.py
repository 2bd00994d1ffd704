"""CPU emulation of the two fp32 forms of the NonLocalBlock's logits (csrc/bsr_api.hip: keys_compose, env BSR_KEYS_CONV2) against fp64.

  projected   theta = t2 Wq + bq and phi = t2 Wk + bk, each a float32 GEMM rounded on its own; logits theta . phi   (BSR_KEYS_CONV2=0)
  composed    q' = t2 (Wq Wk^T) + bq Wk^T, ONE float32 GEMM with the composed weights (float64, rounded once, as bsr_create does); logits
              q' . t2 — conv2's output itself is the key tensor                                                     (the default)

Both continue the same way in float32 — the query scaled by log2 e, logits accumulated over the 128 channels in channel order, base-2
softmax over the keys, P . g accumulated over the keys in key order, divided by the row sum — and are compared with the fp64
softmax(theta phi^T) g of the same float32 weights.  This is the arithmetic of the kernels, not their blocking (the online softmax
rescales per key tile; its error is of the same order).

Inputs: every res block's conv2 output t2 on the tests/golden/model_py_gsc_{64,256}.npz inputs (fp64 oracle, rounded to float32 as the
GPU's t2 is).  Reported per block: max|att - att_ref| / max|att_ref| for both forms, and the largest |logit|.

    python tools/keys_conv2_error.py
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from blindshadowremoval_amd.pack import compose_keys   # noqa: E402

LOG2E = np.float32(1.4426950408889634)


def gemm32(x: np.ndarray, w: np.ndarray, b: np.ndarray) -> np.ndarray:
    """float32 x [T, K] . w [K, N] + b: float32 products, float32 accumulation over k in order, starting from the bias."""
    x, w = x.astype(np.float32), w.astype(np.float32)
    acc = np.zeros((x.shape[0], w.shape[1]), np.float32) + b.astype(np.float32)
    for k in range(x.shape[1]):
        acc = acc + x[:, k:k + 1] * w[k]
    return acc


def attention32(q: np.ndarray, keys: np.ndarray, g: np.ndarray) -> np.ndarray:
    """float32 softmax_j(q_i . keys_j) g_j for one image: q, keys, g [T, 128] float32."""
    qs = q * LOG2E
    s = np.zeros((q.shape[0], keys.shape[0]), np.float32)
    for c in range(q.shape[1]):
        s = s + qs[:, c:c + 1] * keys[:, c][None, :]
    p = np.exp2(s - s.max(axis=1, keepdims=True)).astype(np.float32)
    o = np.zeros((q.shape[0], g.shape[1]), np.float32)
    l = np.zeros((q.shape[0], 1), np.float32)
    for j in range(keys.shape[0]):
        o = o + p[:, j:j + 1] * g[j]
        l = l + p[:, j:j + 1]
    return o / l


def attention64(theta: np.ndarray, phi: np.ndarray, g: np.ndarray) -> np.ndarray:
    s = theta @ phi.T
    p = np.exp(s - s.max(axis=1, keepdims=True))
    return (p / p.sum(axis=1, keepdims=True)) @ g


def both_forms(t2: np.ndarray, kc: np.ndarray, bc: np.ndarray):
    """t2 [T, 128] float32 (one image); kc [128, 672], bc [672] = the c3q layer's [y3 288 | theta | phi | g] matrices (rounded to
    float32 here, as the blob holds them).  Returns (att projected, att composed, att fp64, max |logit|)."""
    kc, bc = kc.astype(np.float32), bc.astype(np.float32)
    wq, wk, wg = kc[:, 288:416], kc[:, 416:544], kc[:, 544:672]
    bq, bk, bg = bc[288:416], bc[416:544], bc[544:672]
    t64 = t2.astype(np.float64)
    theta64, phi64, g64 = (t64 @ w.astype(np.float64) + b for w, b in ((wq, bq), (wk, bk), (wg, bg)))
    ref = attention64(theta64, phi64, g64)
    g32 = gemm32(t2, wg, bg)
    old = attention32(gemm32(t2, wq, bq), gemm32(t2, wk, bk), g32)
    a, ab = compose_keys(wq, bq, wk)
    new = attention32(gemm32(t2, a.astype(np.float32), ab.astype(np.float32)), t2.astype(np.float32), g32)
    return old, new, ref, float(np.abs(theta64 @ phi64.T).max())


def rel(got, ref) -> float:
    return float(np.abs(got.astype(np.float64) - ref).max() / np.abs(ref).max())


def main() -> None:
    import torch
    from blindshadowremoval_amd.pack import fold_bn, layer_matrices
    from blindshadowremoval_amd.weights import init_weights
    from oracle.gsc_oracle import GeneratorOracle, conv2d_same, batchnorm_infer, leaky_relu
    from wino_conv2_error import direct64
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from stage_parity import BLOCK_IN

    worst = {"projected": 0.0, "composed": 0.0}
    for name in ("model_py_gsc_64", "model_py_gsc_256"):
        z = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
        w = init_weights(int(z["weights_seed"]))
        mats = layer_matrices(w)
        o = GeneratorOracle(w, dtype=torch.float64)
        pr = {}
        o.forward(z["inputs"], z["uv"], probes=pr)
        for i in range(6):
            st = "res_stack/%d/" % i
            xin = pr[BLOCK_IN[i]]
            bn = lambda y, s: batchnorm_infer(y, *[o.w[st + s + "/" + p] for p in ("gamma", "beta", "moving_mean", "moving_variance")])
            t1 = leaky_relu(bn(conv2d_same(xin, o.w[st + "conv1/kernel"], o.w[st + "conv1/bias"], 1), "bnorm1")).numpy()
            k9, b = fold_bn(w[st + "conv2/kernel"].reshape(9, 128, 128), w[st + "conv2/bias"],
                            {p: w[st + "bnorm2/" + p] for p in ("gamma", "beta", "moving_mean", "moving_variance")})
            t2 = direct64(t1, k9, b).astype(np.float32)
            kc, bc = mats["res%d.c3q" % i]
            for img in range(t2.shape[0]):
                old, new, ref, logit = both_forms(t2[img].reshape(-1, 128), kc[0], bc)
                eo, en = rel(old, ref), rel(new, ref)
                worst["projected"], worst["composed"] = max(worst["projected"], eo), max(worst["composed"], en)
                print("%-18s image %d res%d  att: projected %.3e  composed %.3e   max|logit| %.1f" % (name, img, i, eo, en, logit))
    for form, e in worst.items():
        print("worst %-9s att %.3e" % (form, e))
    print("composed / projected %.2f" % (worst["composed"] / worst["projected"]))


if __name__ == "__main__":
    main()
