"""The three attention kernels' arithmetic restated in float32 numpy, on the constructed cases of tests/attention_cases.py.

    python tools/attention_error.py            # writes profiles/attention_edges_emulation.txt
    python tools/attention_error.py --quick    # T <= 384 only, to the terminal
    python tools/attention_error.py --merge LOG
                                               # LOG = the output of `pytest -m gpu -s tests/test_attention_edges_gpu.py` on the device:
                                               # its measured lines beside the emulated column -> profiles/attention_edges_gpu.txt

What each emulation keeps of its kernel (all: base-2 logits from theta x log2 e; 32-key tiles; P = exp2(S - m) with the LAZY running
maximum, raised — and O, l rescaled — only when some query of a wave's 32 sees a tile maximum more than 8 above it, one decision per wave;
a lane half's own partial row sum over its 16 keys of a tile, keys (i & 3) + 8 (i >> 2) + 4 h, the two halves added at the end;
out = O x (1 / l)):

f32   csrc/attention.h: S by v_mfma_f32_32x32x2f32 steps, channels (8 g + j, 8 g + 4 + j) per step, emulated as acc + a0 b0 + a1 b1 with
      every product and sum rounded; P.V by the same instruction, keys (k, k + 4) per step in register order; the even and the odd tiles
      as two streams with their own (m, l, O), m from -inf; the merge O0 s0 + O1 s1, l0 s0 + l1 s1 with s = exp2(m_stream - max).
h16   csrc/attention_h16.h: operands hi = fp16(x), lo = fp16(x - hi) (mfma_common.h split2); S per 16-channel K step as
      lo.hi + hi.lo + hi.hi, each a v_mfma_f32_32x32x16_f16 emulated as a float32 dot product of 16 exact products added to the
      accumulator; m taken from tile 0, moved between iterations by the next tile's maximum; l as one chain per lane half; P split into
      hi / lo fp16; P.V per 16 keys as g_lo.P_hi + g_hi.P_lo + g_hi.P_hi — `pv1`: g_hi.P_hi alone.
d256  csrc/attention256.h: the f32 arithmetic at 256 channels with ONE key stream and no merge.

For the 128-channel kernels the emulation also returns, per query, the number of rescales its wave took (the first tile's, from -inf,
not counted) and the largest P it formed.

Planted defects (`defect=`), for tests/test_attention_cases_cpu.py to show that the budgets can tell a broken kernel:
    drop_last_tile   the last key tile is never multiplied
    merge_unscaled   (f32) the merge adds stream 1 with factor 1
    rescale_o_only   a rescale scales O but not l
    hi_only          (h16) hi.hi products only, in S and in P.V
    swap_g_rows      keys 1 and 2 of every tile swap their g rows
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
LOG2E = f32(1.4426950408889634)
THRESH = f32(8.0)
KT = 32
# register i of lane half h holds key (i & 3) + 8 (i >> 2) + 4 h of the tile
HALF_KEYS = [np.array([(i & 3) + 8 * (i >> 2) + 4 * h for i in range(16)]) for h in (0, 1)]
DEFECTS = ("drop_last_tile", "merge_unscaled", "rescale_o_only", "hi_only", "swap_g_rows")


def _exp2(x):
    with np.errstate(under="ignore"):
        return np.exp2(x.astype(f32)).astype(f32)


def _wave_any(flag: np.ndarray) -> np.ndarray:
    """flag [T] per query -> the wave-uniform decision, per query (a wave = 32 consecutive queries)."""
    return np.repeat(flag.reshape(-1, 32).any(axis=1), 32)


def _swap_rows(g: np.ndarray) -> np.ndarray:
    g = g.copy()
    g[1::KT], g[2::KT] = g[2::KT].copy(), g[1::KT].copy()
    return g


class _Stream:
    """(m, l per lane half, O) of one key stream over all T queries at once, and the lazy-rescale bookkeeping."""

    def __init__(self, T: int, D: int, m0=None):
        self.m = np.full(T, -np.inf, f32) if m0 is None else m0.astype(f32)
        self.l = np.zeros((2, T), f32)
        self.o = np.zeros((T, D), f32)
        self.rescales = np.zeros(T, np.int64)
        self.pmax = np.zeros(T, f32)
        self.first = m0 is None

    def maybe_rescale(self, mx: np.ndarray, defect=None) -> None:
        with np.errstate(invalid="ignore"):
            go = _wave_any(mx > self.m + THRESH)
        if not go.any():
            return
        m_new = np.maximum(self.m, mx)
        with np.errstate(invalid="ignore"):
            scale = _exp2(np.where(np.isneginf(self.m), -np.inf, self.m - m_new))
        scale = np.where(go, scale, f32(1)).astype(f32)
        if defect != "rescale_o_only":
            self.l *= scale[None, :]
        self.o *= scale[:, None]
        self.m = np.where(go, m_new, self.m).astype(f32)
        if not self.first:
            self.rescales += go
        self.first = False


def _s_f32(theta2: np.ndarray, phi: np.ndarray) -> np.ndarray:
    """S[q, key] by 32x32x2 steps: per step channels (8 g + j, 8 g + 4 + j), products and sums rounded to float32 one by one."""
    T, D = theta2.shape
    s = np.zeros((T, phi.shape[0]), f32)
    blk = 256
    for q0 in range(0, T, blk):
        acc = np.zeros((min(blk, T - q0), phi.shape[0]), f32)
        tq = theta2[q0:q0 + blk]
        for g in range(D // 8):
            for j in range(4):
                for c in (8 * g + j, 8 * g + 4 + j):
                    acc += tq[:, c:c + 1] * phi[None, :, c]
        s[q0:q0 + blk] = acc
    return s


def _pv_f32(o: np.ndarray, p: np.ndarray, g_tile: np.ndarray) -> None:
    """O += P . g of one tile by 32x32x2 steps: keys (k, k + 4) per step, k in register order."""
    for i in range(16):
        k0 = (i & 3) + 8 * (i >> 2)
        for k in (k0, k0 + 4):
            o += p[:, k:k + 1] * g_tile[None, k, :]


def _emulate_f32_like(qkv: np.ndarray, D: int, streams: int, defect=None):
    T = qkv.shape[0]
    theta2 = (qkv[:, :D].astype(f32) * LOG2E).astype(f32)
    phi, g = qkv[:, D:2 * D].astype(f32), qkv[:, 2 * D:].astype(f32)
    if defect == "swap_g_rows":
        g = _swap_rows(g)
    s_all = _s_f32(theta2, phi)
    nt = T // KT
    st = [_Stream(T, D) for _ in range(streams)]
    for t in range(nt):
        if defect == "drop_last_tile" and t == nt - 1:
            continue
        x = st[t % streams]
        s = s_all[:, t * KT:(t + 1) * KT]
        x.maybe_rescale(s.max(axis=1), defect)
        p = _exp2(s - x.m[:, None])
        x.pmax = np.maximum(x.pmax, p.max(axis=1))
        for h in (0, 1):
            ph = p[:, HALF_KEYS[h]]
            if D == 128:                                  # packed pairs: the even and the odd registers as two chains
                a, b = np.zeros(T, f32), np.zeros(T, f32)
                for i in range(0, 16, 2):
                    a += ph[:, i]
                    b += ph[:, i + 1]
                x.l[h] += a + b
            else:
                a = np.zeros(T, f32)
                for i in range(16):
                    a += ph[:, i]
                x.l[h] += a
        _pv_f32(x.o, p, g[t * KT:(t + 1) * KT])
    info = {}
    if streams == 2:
        a, b = st
        m = np.maximum(a.m, b.m)
        with np.errstate(invalid="ignore"):
            s0, s1 = _exp2(a.m - m), _exp2(b.m - m)
        if defect == "merge_unscaled":
            s1 = np.ones_like(s1)
        l = a.l * s0[None, :] + b.l * s1[None, :]
        o = a.o * s0[:, None] + b.o * s1[:, None]
        info = {"s0": s0, "s1": s1, "rescales": a.rescales + b.rescales, "rescales_stream": (a.rescales, b.rescales),
                "pmax": np.maximum(a.pmax, b.pmax)}
    else:
        l, o = st[0].l, st[0].o
        info = {"rescales": st[0].rescales, "pmax": st[0].pmax}
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = (f32(1) / (l[0] + l[1])).astype(f32)
        out = (o * inv[:, None]).astype(f32)
    return out, info


def emulate_f32(qkv: np.ndarray, defect=None):
    """One image [T, 384] -> (out [T, 128] float32, info)."""
    return _emulate_f32_like(qkv, 128, 2, defect)


def emulate_d256(qkv: np.ndarray, defect=None):
    """One image [T, 768] -> (out [T, 256] float32, info)."""
    return _emulate_f32_like(qkv, 256, 1, defect)


def split2(x: np.ndarray):
    """mfma_common.h split2: hi = fp16(x), lo = fp16(x - hi), both returned as float32 (exact)."""
    with np.errstate(over="ignore", under="ignore"):
        hi = x.astype(np.float16).astype(f32)
        lo = (x - hi).astype(f32).astype(np.float16).astype(f32)
    return hi, lo


def emulate_h16(qkv: np.ndarray, pv1: bool = False, defect=None):
    """One image [T, 384] -> (out [T, 128] float32, info): csrc/attention_h16.h, `pv1` its hi-planes-only P.V form."""
    D = 128
    T = qkv.shape[0]
    th, tl = split2((qkv[:, :D].astype(f32) * LOG2E).astype(f32))
    kh, kl = split2(qkv[:, D:2 * D].astype(f32))
    g = qkv[:, 2 * D:].astype(f32)
    if defect == "swap_g_rows":
        g = _swap_rows(g)
    gh, gl = split2(g)
    hi_only = defect == "hi_only"
    s_all = np.zeros((T, T), f32)
    for ks in range(D // 16):
        c = slice(16 * ks, 16 * ks + 16)
        if not hi_only:
            s_all += th[:, c] @ kl[:, c].T
            s_all += tl[:, c] @ kh[:, c].T
        s_all += th[:, c] @ kh[:, c].T
    nt = T // KT
    x = _Stream(T, D, m0=s_all[:, :KT].max(axis=1))
    x.first = False
    for t in range(nt):
        if defect == "drop_last_tile" and t == nt - 1:
            break
        p = _exp2(s_all[:, t * KT:(t + 1) * KT] - x.m[:, None])
        x.pmax = np.maximum(x.pmax, p.max(axis=1))
        for h in (0, 1):
            ph = p[:, HALF_KEYS[h]]
            for i in range(16):
                x.l[h] += ph[:, i]
        p_hi, p_lo = split2(p)
        gt_h, gt_l = gh[t * KT:(t + 1) * KT], gl[t * KT:(t + 1) * KT]
        for t2 in (0, 1):
            k = slice(16 * t2, 16 * t2 + 16)
            if not (pv1 or hi_only):
                x.o += p_hi[:, k] @ gt_l[k]
                x.o += p_lo[:, k] @ gt_h[k]
            x.o += p_hi[:, k] @ gt_h[k]
        if t + 1 < nt:
            x.maybe_rescale(s_all[:, (t + 1) * KT:(t + 2) * KT].max(axis=1), defect)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = (f32(1) / (x.l[0] + x.l[1])).astype(f32)
        out = (x.o * inv[:, None]).astype(f32)
    return out, {"rescales": x.rescales, "pmax": x.pmax}


KERNELS = {
    "f32": (128, lambda q, d=None: emulate_f32(q, d)),
    "h16": (128, lambda q, d=None: emulate_h16(q, False, d)),
    "h16_pv1": (128, lambda q, d=None: emulate_h16(q, True, d)),
    "d256": (256, lambda q, d=None: emulate_d256(q, d)),
}


def emulate_batch(kernel: str, qkv, defect=None):
    """qkv [B, T, 3 D] (torch or numpy) -> (out [B, T, D] float32 numpy, [info per image])."""
    qkv = np.asarray(qkv, dtype=f32)
    outs, infos = [], []
    for b in range(qkv.shape[0]):
        o, i = KERNELS[kernel][1](qkv[b], defect)
        outs.append(o)
        infos.append(i)
    return np.stack(outs), infos


def emulated_error(kernel: str, case: str, B: int, T: int, defect=None):
    """(err, image, query) of the emulation on a constructed case, by the metric of tests/attention_cases.py."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import attention_cases as ac
    qkv, ref, scale = ac.reference(case, B, T, KERNELS[kernel][0])
    out, _ = emulate_batch(kernel, qkv.numpy(), defect)
    return ac.case_error(out, ref, scale)


def merge(measured_path: str) -> None:
    """profiles/attention_edges_gpu.txt: every line the GPU tests printed, with the emulated error of the same (kernel, case, T)."""
    import re
    emu = {}
    with open(os.path.join(ROOT, "profiles", "attention_edges_emulation.txt")) as f:
        for line in f:
            m = re.match(r"(\S+)\s+(\S+)\s+T\s+(\d+)\s+B\s+(\d+)\s+err (\S+)", line)
            if m:
                emu[(m.group(1), m.group(2), int(m.group(3)))] = (int(m.group(4)), float(m.group(5)))
    out = ["# measured on an MI355X by tests/test_attention_edges_gpu.py; emulated: tools/attention_error.py at the B in brackets;",
           "# budget = 3 x the emulated maximum over T (tests/attention_cases.py EMULATED), one_hot on the fp32 kernels 1e-6",
           "%-8s %-17s %5s %2s  %-9s  %-15s  %-9s  %s" % ("kernel", "case", "T", "B", "measured", "emulated", "budget", "findings")]
    with open(measured_path) as f:
        for line in f:
            m = re.search(r"(f32|h16_pv1|h16|d256)\s+(\S+)\s+T\s+(\d+)\s+B\s+(\d+)\s+err (\S+)\s+budget (\S+)\s+at \((.*?)\)(.*)", line)
            if not m:
                continue
            k, c, T, B, err, bud, at, rest = m.groups()
            e = emu.get((k, c, int(T)))
            etxt = "%.3e [B %d]" % (e[1], e[0]) if e else "-"
            out.append("%-8s %-17s %5s %2s  %-9s  %-15s  %-9s  worst at (%s)%s" % (k, c, T, B, err, etxt, bud, at, rest.rstrip()))
    with open(os.path.join(ROOT, "profiles", "attention_edges_gpu.txt"), "w") as f:
        f.write("\n".join(out) + "\n")
    print("wrote %d rows" % (len(out) - 3))


def main() -> None:
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import attention_cases as ac
    if "--merge" in sys.argv:
        return merge(sys.argv[sys.argv.index("--merge") + 1])
    quick = "--quick" in sys.argv
    rows, worst = [], {}
    for kernel, (D, _) in KERNELS.items():
        ts = ac.T_256 if D == 256 else ac.T_128
        B = ac.B_256 if D == 256 else ac.B_128
        plan = [(case, B, T) for case in ac.CASES for T in ts if not (quick and T > 384)]
        if D == 128 and not quick:
            plan += [(case, 1, ac.T_128_BIG) for case in ac.BIG_CASES]
        for case, b, T in plan:
            err, img, q = emulated_error(kernel, case, b, T)
            worst[(kernel, case)] = max(worst.get((kernel, case), 0.0), err)
            rows.append("%-8s %-17s T %5d  B %d  err %.3e  at (image %d, query %d)" % (kernel, case, T, b, err, img, q))
            print(rows[-1], flush=True)
    lines = ["# emulated err per (kernel, case, T): tools/attention_error.py, metric of tests/attention_cases.py", *rows, "",
             "# maximum over T per (kernel, case): tests/attention_cases.py EMULATED (budget = 3 x)"]
    for kernel in KERNELS:
        lines.append("%s: {%s}" % (kernel, ", ".join('"%s": %.2e' % (c, worst[(kernel, c)]) for c in ac.CASES)))
    text = "\n".join(lines) + "\n"
    print("\n".join(lines[len(rows) + 2:]))
    if not quick:
        with open(os.path.join(ROOT, "profiles", "attention_edges_emulation.txt"), "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
