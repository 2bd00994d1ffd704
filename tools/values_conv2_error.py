"""CPU emulation of the three fp32 forms of the NonLocalBlock, from conv2's output t2 to the block output and to `att` as bsr_probe
returns it, against fp64 (csrc/bsr_api.hip: keys_compose / values_compose, env BSR_KEYS_CONV2 / BSR_VALUES_CONV2).

  projected    theta, phi, g = t2 W + b, three float32 GEMMs; att = softmax(theta phi^T) g; out = lrelu(y3x + att Ww + bw)
                                                                                                  (BSR_KEYS_CONV2=0)
  keys         q' = t2 (Wq Wk^T) + bq Wk^T, keys = t2; att = softmax(q' t2^T) g; out as above       (BSR_VALUES_CONV2=0)
  keys+values  values = t2 too: O = softmax(q' t2^T) t2; out = lrelu(y3x + O (Wg Ww) + (bg Ww + bw)) with the composed weights (float64,
               rounded once, as bsr_create does); att, which only the probe needs, = O Wg + bg as one float32 GEMM      (the default)

Every GEMM is float32 products accumulated in float32 over k in order from the bias, the attention as tools/keys_conv2_error.py states
it, y3x = t2 W3 + b3 + pad(x) with the block input x.  The reference is the same block in fp64 on the same float32 weights and t2.

Inputs: those of tools/keys_conv2_error.py — every res block's t2 on the tests/golden/model_py_gsc_{64,256}.npz inputs.  Reported per
block and form: max|att - ref| / max|ref|, max|out - ref| / max|ref|, and the default form against the projected one.

The gate the values form ships under (RULE below) is checked at the end; the exit status is 1 if it fails.

    python tools/values_conv2_error.py > profiles/values_conv2_error.txt
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from blindshadowremoval_amd.pack import compose_keys, compose_values   # noqa: E402
from keys_conv2_error import attention32, attention64, gemm32, rel      # noqa: E402

LRELU_ALPHA = 0.2
FORMS = ("projected", "keys", "keys+values")

# The budgets are the measured columns of res_att / res_block for f32 in tests/test_stage_parity_gpu.py (TOL[..]["f32"][1]); today's GPU
# figures use GPU_SHARE of both.  The emulation runs on other inputs than the GPU tests, so its absolute figures do not compare with the
# budgets; what carries over is the ratio of a form to the projected form in the SAME emulation.  Condition 1: scaled by that ratio,
# today's share must stay inside the budget — new <= projected / GPU_SHARE, for att and for the block output.  Condition 2: the default
# against the fully projected form stays inside FORM_TOL of tests/test_keys_conv2_gpu.py (3 x KEYS_EMULATED_ERR), relative to the largest
# magnitude, on the block output (the probes that test compares).
BUDGET = {"att": 2.0e-6, "out": 6.6e-7}
GPU_SHARE = 0.65
FORM_TOL = 3 * 2.6e-6


def lrelu(x):
    return np.where(x >= 0, x, x * x.dtype.type(LRELU_ALPHA))


def pad288(x: np.ndarray) -> np.ndarray:
    out = np.zeros((x.shape[0], 288), x.dtype)
    out[:, :x.shape[1]] = x
    return out


def three_forms(t2: np.ndarray, x: np.ndarray, kc: np.ndarray, bc: np.ndarray, kw: np.ndarray, bw: np.ndarray, defect: str = ""):
    """t2 [T, 128] float32, x [T, C <= 288] the block input (one image); kc [128, 672], bc [672] the c3q layer's [y3 288 | theta | phi | g]
    matrices and kw [128, N <= 288], bw [N] the `w` layer's (BN folded), rounded to float32 here as the blob holds them.
    ``defect`` plants a wrong composition into the keys+values form: "bias" drops bg Ww from the composed bias, "transpose" composes
    Wg^T in place of Wg.  Returns ({form: (att, out)}, (att fp64, out fp64)), out over 288 channels."""
    kc, bc = kc.astype(np.float32), bc.astype(np.float32)
    ww, wb = pad288(kw.astype(np.float32)), pad288(bw.astype(np.float32)[None])[0]
    w3, b3 = kc[:, :288], bc[:288]
    wq, wk, wg = kc[:, 288:416], kc[:, 416:544], kc[:, 544:672]
    bq, bk, bg = bc[288:416], bc[416:544], bc[544:672]
    t2 = t2.astype(np.float32)
    x32 = pad288(x.astype(np.float32))
    f64 = lambda a: a.astype(np.float64)

    t64 = f64(t2)
    att_ref = attention64(t64 @ f64(wq) + bq, t64 @ f64(wk) + bk, t64 @ f64(wg) + bg)
    out_ref = lrelu(t64 @ f64(w3) + b3 + f64(x32) + att_ref @ f64(ww) + wb)

    y3x = gemm32(t2, w3, b3) + x32                                  # the c3q epilogue: bias-started accumulation, then the residual
    tail = lambda a, w, b: lrelu(gemm32(a, w, b) + y3x)             # the `w` GEMM's: + y3x, LeakyReLU
    g32 = gemm32(t2, wg, bg)
    res = {}
    att = attention32(gemm32(t2, wq, bq), gemm32(t2, wk, bk), g32)
    res["projected"] = (att, tail(att, ww, wb))
    a, ab = compose_keys(wq, bq, wk)
    qc = gemm32(t2, a.astype(np.float32), ab.astype(np.float32))
    att = attention32(qc, t2, g32)
    res["keys"] = (att, tail(att, ww, wb))
    o = attention32(qc, t2, t2)
    w2, b2 = compose_values(wg.T if defect == "transpose" else wg, bg, ww, wb)
    if defect == "bias":
        b2 = f64(wb)
    res["keys+values"] = (gemm32(o, wg, bg), tail(o, w2.astype(np.float32), b2.astype(np.float32)))
    return res, (att_ref, out_ref)


def gate(worst: dict, form_diff: float):
    """(condition 1 holds, condition 2 holds, lines): worst[form] = (att error, out error) of the emulation."""
    lines, ok1 = [], True
    for j, what in enumerate(("att", "out")):
        ratio = worst["keys+values"][j] / worst["projected"][j]
        scaled = ratio * GPU_SHARE * BUDGET[what]
        hold = scaled <= BUDGET[what]
        ok1 = ok1 and hold
        lines.append("condition 1 %-3s keys+values / projected %.2f -> %.0f %% of the %.1e budget (today %.0f %%): %s"
                     % (what, ratio, 100 * ratio * GPU_SHARE, BUDGET[what], 100 * GPU_SHARE, "holds" if hold else "FAILS"))
    ok2 = form_diff <= FORM_TOL
    lines.append("condition 2 out keys+values against projected %.3e of max|out|, FORM_TOL %.2e: %s" % (form_diff, FORM_TOL, "holds" if ok2 else "FAILS"))
    return ok1, ok2, lines


def main() -> int:
    import torch
    from blindshadowremoval_amd.pack import fold_bn, layer_matrices
    from blindshadowremoval_amd.weights import init_weights
    from oracle.gsc_oracle import GeneratorOracle, conv2d_same, batchnorm_infer, leaky_relu
    from wino_conv2_error import direct64
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from stage_parity import BLOCK_IN

    worst = {f: [0.0, 0.0] for f in FORMS}
    form_diff = 0.0
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
            kw, bw = mats["res%d.w" % i]
            x = xin.numpy().astype(np.float32)
            for img in range(t2.shape[0]):
                res, (att_ref, out_ref) = three_forms(t2[img].reshape(-1, 128), x[img].reshape(-1, x.shape[-1]), kc[0], bc, kw[0], bw)
                cols = []
                for f in FORMS:
                    ea, eo = rel(res[f][0], att_ref), rel(res[f][1], out_ref)
                    worst[f][0], worst[f][1] = max(worst[f][0], ea), max(worst[f][1], eo)
                    cols.append("%s att %.3e out %.3e" % (f, ea, eo))
                d = rel(res["keys+values"][1], res["projected"][1].astype(np.float64))
                form_diff = max(form_diff, d)
                print("%-18s image %d res%d  %s   default vs projected out %.3e" % (name, img, i, "  ".join(cols), d))
    for f in FORMS:
        print("worst %-11s att %.3e  out %.3e" % (f, worst[f][0], worst[f][1]))
    print("worst keys+values against projected, out %.3e" % form_diff)
    ok1, ok2, lines = gate(worst, form_diff)
    print("\n".join(lines))
    return 0 if ok1 and ok2 else 1


if __name__ == "__main__":
    sys.exit(main())
