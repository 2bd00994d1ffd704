"""Offline weight preparation for libbsr_hip: BatchNorm folding + MFMA-friendly packing.

Input: the reference's generator variables by their checkpoint names (HWIO ``Conv2D`` kernels,
``[kh,kw,Cout,Cin]`` ``Conv2DTranspose`` kernels, BatchNormalization gamma/beta/moving stats —
/root/reference/model.py:115-177, 81-113, 6-61; names per blindshadowremoval_amd/weights.py).

Output: one blob (bytes) that ``bsr_create`` uploads as is.  Per MFMA conv layer the weights become
``[chunk][tap][n_pad][CC+4]`` float32 — the exact LDS image the kernel stages per (chunk, tap) step,
including the 4-float bank pad — and a ``[n_pad]`` bias.  Every BatchNormalization on the path
follows a conv and runs with ``training=False`` (/root/reference/train_test_GSC.py:404,856), so it
folds exactly:  s = gamma * rsqrt(var + 1e-3);  W' = W * s;  b' = (b - mean) * s + beta.
"""
from __future__ import annotations

import struct
from typing import Dict, List, Tuple

import numpy as np

from .weights import BN_EPS, N_RES, check_weights, detect_variant

BLOB_MAGIC = 0x57525342   # "BSRW"
BLOB_VERSION = 1
_ENTRY = struct.Struct("<40sQQ4i")
_HEADER = struct.Struct("<4I")

TRANSPOSED = ("up1", "up2", "up3", "clr_up1", "clr_up2", "clr_up3")

DTYPES = {"f32": 0, "f16": 1, "f32x3": 2}     # BSR_DTYPE_* of include/bsr_hip.h
# layers the 16-bit modes run on igemm_h16_kernel (csrc/igemm_h16.h): every 3x3 / stride-2 3x3 / transposed 3x3 igemm layer
H16_LAYERS = ("down1", "down2", "down3", "up1", "up2", "up3", "clr_up1", "clr_up2", "clr_up3") + tuple("res%d.conv2" % i for i in range(6))
# f16 mode: the stride-1 3x3 and the transposed 3x3 layers run on conv3_f16_kernel (csrc/conv3_f16.h) from their `w3` images
W3_LAYERS = ("up1", "up2", "up3", "clr_up1", "clr_up2", "clr_up3") + tuple("res%d.conv2" % i for i in range(6))
# 1x1 layers (igemm_h16_kernel<1,1> / gemm_nloop_kernel<.., H = 2>): split-precision (hi + lo planes) in BOTH 16-bit modes
X3_LAYERS = tuple("res%d.%s" % (i, n) for i in range(6) for n in ("conv1", "c3q", "w")) + ("heads", "clr_conv1", "conv1")      # + conv_n16_kernel / stem7_kernel<.., H = 2>


def geometry(variant: str = "gsc", dtype: str = "f32") -> Dict[str, Tuple[int, int, int]]:
    """name -> (CC, k_pad, n_pad): must match the launch table in csrc/bsr_api.hip.  The TSM variant
    (/root/reference/model_with_TSM.py) only widens the K of the layers fed by the ShareLayer concats: 291 -> 312, 877 -> 888
    (320 / 896 in the 16-bit modes).
    The 16-bit modes use 32-channel K chunks, so the 257 / 261-wide trunk tensors get stride 288 instead of 264 (kGSC16)."""
    if variant == "rgb":
        return geometry_rgb(dtype)
    tsm = variant == "tsm"
    h16 = dtype != "f32"
    if tsm:
        k_a, k_r, k_h = (320, 320, 896) if h16 else (312, 312, 888)
    else:
        k_a, k_r, k_h = (128, 288, 288) if h16 else (120, 264, 264)
    cu = 32 if h16 else 24
    g: Dict[str, Tuple[int, int, int]] = {
        "conv1": (32, 32, 32) if h16 else (24, 24, 32), "down1": (16, 32, 64), "down2": (16, 64, 64), "down3": (16, 64, 96),
        "up1": (cu, k_r, 96), "up2": (32, 160, 64), "up3": (32, 128, 64), "heads": (32, 64, 16),
        "clr_up1": (cu, k_h, 128), "clr_up2": (32, 128, 96), "clr_up3": (32, 96, 64), "clr_conv1": (32, 64, 16),
    }
    for i in range(N_RES):
        g["res%d.conv1" % i] = (cu, k_a if i == 0 else (k_r if i < N_RES // 2 else k_h), 128)
        g["res%d.conv2" % i] = (32, 128, 128)
        g["res%d.c3q" % i] = (32, 128, 768)       # [y3: 257 real of 288 | theta|phi|g: 384 | 3 zero tiles of slack]
        g["res%d.w" % i] = (32, 128, 384)         # 257 real of 288 + 3 zero tiles of slack (gemm_nloop group reads)
    return g


def geometry_rgb(dtype: str = "f32") -> Dict[str, Tuple[int, int, int]]:
    """The RGB baseline (/root/reference/model_RGB.py; fp32 only): name -> (CC, k_pad, n_pad), matching bsr_forward_rgb in csrc/bsr_api.hip.
    The 513-wide block outputs and y3x live at stride 544 (17 tiles of 32); xa = cat[x, uv] (99) at stride 128.
    c3q: N = [y3 513 of 544 | theta|phi|g 768] + 2 zero tiles of slack (gemm_nloop group reads, NI = 3); w: 513 of 544 + 3 zero tiles.
    rgb_head: conv2 as a 7x1 conv, taps = ky, K = 128 channels, N = (kx, co) = 21 of 32."""
    if dtype != "f32":
        raise ValueError("the RGB baseline is provided in f32 only (dtype 'f32x3' / 'f16' are not)")
    g: Dict[str, Tuple[int, int, int]] = {
        "conv1": (24, 24, 32), "down1": (16, 32, 64), "down2": (16, 64, 64), "down3": (16, 64, 96),
        "up1": (32, 544, 192), "up2": (32, 256, 128), "up3": (32, 192, 128), "rgb_head": (32, 128, 32),
    }
    for i in range(N_RES // 2):
        g["res%d.conv1" % i] = (32, 128 if i == 0 else 544, 256)
        g["res%d.conv2" % i] = (32, 256, 256)
        g["res%d.c3q" % i] = (32, 256, 544 + 768 + 64)
        g["res%d.w" % i] = (32, 256, 544 + 96)
    return g


GEOMETRY = geometry("gsc")


def fold_bn(kernel_tkn: np.ndarray, bias: np.ndarray, bn: Dict[str, np.ndarray] | None):
    """kernel_tkn: [taps, K, N] float64.  Returns folded (kernel, bias) in float64."""
    k = kernel_tkn.astype(np.float64)
    b = bias.astype(np.float64)
    if bn is None:
        return k, b
    s = bn["gamma"].astype(np.float64) / np.sqrt(bn["moving_variance"].astype(np.float64) + BN_EPS)
    return k * s[None, None, :], (b - bn["moving_mean"].astype(np.float64)) * s + bn["beta"].astype(np.float64)


def _bn(w: Dict[str, np.ndarray], stem: str) -> Dict[str, np.ndarray]:
    return {p: w[stem + "/" + p] for p in ("gamma", "beta", "moving_mean", "moving_variance")}


def pack_taps(kernel_tkn: np.ndarray, bias: np.ndarray, cc: int, k_pad: int, n_pad: int):
    """[taps, K, N] -> ([k_pad/cc, taps, n_pad, cc+4] float32, [n_pad] float32), zero padded."""
    taps, k, n = kernel_tkn.shape
    assert k <= k_pad and n <= n_pad and k_pad % cc == 0
    full = np.zeros((taps, k_pad, n_pad), np.float64)
    full[:, :k, :n] = kernel_tkn
    arr = np.zeros((k_pad // cc, taps, n_pad, cc + 4), np.float32)
    arr[..., :cc] = full.reshape(taps, k_pad // cc, cc, n_pad).transpose(1, 0, 3, 2)
    b = np.zeros(n_pad, np.float32)
    b[:n] = bias
    return arr, b


def pack_taps_h16(kernel_tkn: np.ndarray, bias: np.ndarray, cc: int, k_pad: int, n_pad: int, nsplit: int, swizzle: bool = False):
    """[taps, K, N] -> the fp16 LDS image of csrc/igemm_h16.h as float32 words: [k_pad/cc, taps, n_pad, (nsplit*cc + 8) / 2].
    Row of output channel n: cc halves hi = fp16(w) | (nsplit == 2) cc halves lo = fp16(w - hi) | 8 halves of zero pad, where
    w is the fp32 value the fp32 path uses (so hi + lo reproduces it to ~2^-22)."""
    taps, k, n = kernel_tkn.shape
    assert k <= k_pad and n <= n_pad and k_pad % cc == 0 and cc % 16 == 0 and nsplit in (1, 2)
    full = np.zeros((taps, k_pad, n_pad), np.float64)
    full[:, :k, :n] = kernel_tkn.astype(np.float32)
    rows = full.reshape(taps, k_pad // cc, cc, n_pad).transpose(1, 0, 3, 2)          # [chunk, tap, n, cc]
    hi = rows.astype(np.float16)
    if not np.all(np.isfinite(hi)):
        raise ValueError("a folded weight exceeds the fp16 range (65504): this layer cannot run in the 16-bit modes")
    planes = [hi]
    if nsplit == 2:
        planes.append((rows - hi.astype(np.float64)).astype(np.float16))
    if swizzle:
        # unpadded 128-byte rows for the LDS-DMA-fed f32x3 layers (H16Cfg::SWZ in csrc/igemm_h16.h): the eight 16-byte slots
        # [hi k0-7, hi k8-15, hi k16-23, hi k24-31, lo ...] of row n are stored at slot ^ ((n >> 1) & 7)
        assert nsplit == 2 and cc == 32
        lin = np.concatenate(planes, axis=3).reshape(rows.shape[:3] + (8, 8))          # [chunk, tap, n, slot, 8 halves]
        img = np.empty_like(lin)
        for row in range(n_pad):
            sw = (row >> 1) & 7
            for slot in range(8):
                img[:, :, row, slot ^ sw] = lin[:, :, row, slot]
        img = np.ascontiguousarray(img.reshape(rows.shape[:3] + (64,)))
    else:
        planes.append(np.zeros(rows.shape[:3] + (8,), np.float16))
        img = np.ascontiguousarray(np.concatenate(planes, axis=3))                    # [chunk, tap, n, nsplit*cc + 8] halves
    arr = img.view(np.float32)                                                         # two halves per 32-bit word, little endian
    b = np.zeros(n_pad, np.float32)
    b[:n] = bias
    return arr, b


def pack_w3(kernel_tkn: np.ndarray, bias: np.ndarray, k_pad: int):
    """A 3x3 / transposed 3x3 layer ([9, K, N] folded) as the weight stream of csrc/conv3_f16.h (f16 mode): per 64-channel output block and
    32-channel K chunk one 36-KB run of nine tap images [64 rows n][32 halves k] — three 12-KB trios, each moved by LDS-DMA as it lies.
    Rows are unpadded (64 bytes); the 16-byte unit u = k / 8 of row n sits at position u ^ ((n >> 2) & 3), which makes a ds_read_b128 over
    16 different rows conflict-free.  Returns ([nblk * nchunk, 9, 64, 16] float32 words, [nblk * 64] bias)."""
    taps, k, n = kernel_tkn.shape
    assert taps == 9 and k <= k_pad and k_pad % 32 == 0
    nblk, nchunk = (n + 63) // 64, k_pad // 32
    full = np.zeros((9, k_pad, nblk * 64), np.float64)
    full[:, :k, :n] = kernel_tkn.astype(np.float32)
    hi = full.astype(np.float16)
    if not np.all(np.isfinite(hi)):
        raise ValueError("a folded weight exceeds the fp16 range (65504): this layer cannot run in the 16-bit modes")
    rows = hi.reshape(9, nchunk, 4, 8, nblk, 64).transpose(4, 1, 0, 5, 2, 3)          # [blk, chunk, tap, row, unit, 8 halves]
    img = np.empty_like(rows)
    for row in range(64):
        sw = (row >> 2) & 3
        for u in range(4):
            img[:, :, :, row, u ^ sw] = rows[:, :, :, row, u]
    arr = np.ascontiguousarray(img.reshape(nblk * nchunk, 9, 64, 32)).view(np.float32)     # [.., 16] words
    b = np.zeros(nblk * 64, np.float32)
    b[:n] = bias
    return arr, b


def pack_w4(kernel_tkn: np.ndarray, bias: np.ndarray):
    """The NonLocalBlock's `w` conv ([1, 128, N <= 288] folded) as the LDS image of the attention kernel's fused tail
    (csrc/attention_h16.h): 9 tiles of 32 output channels, row n = 512 bytes = 16 chunks of 8 halves hi | 16 chunks lo.  Chunk
    c = 4 dt + 2 p + h holds k = 32 dt + 16 p + 4 h + (j & 3) + 8 (j >> 2), j = 0..7 — the order in which registers 8p .. 8p + 7 of the
    O^T accumulator tile dt present the attention output as the A operand — and sits at chunk position c ^ (n & 15) (conflict-free
    ds_read_b128 over 16 different rows; the image goes to LDS by DMA as it lies).  Returns ([9, 1, 32, 128] float32 words, [288] bias)."""
    taps, k, n = kernel_tkn.shape
    assert taps == 1 and k == 128 and n <= 288
    full = np.zeros((128, 288), np.float64)
    full[:, :n] = kernel_tkn[0].astype(np.float32)
    hi = full.astype(np.float16)
    if not np.all(np.isfinite(hi)):
        raise ValueError("a folded weight exceeds the fp16 range (65504): this layer cannot run in the 16-bit modes")
    lo = (full - hi.astype(np.float64)).astype(np.float16)
    korder = np.array([[32 * dt + 16 * p + 4 * h + (j & 3) + 8 * (j >> 2) for j in range(8)]
                       for dt in range(4) for p in range(2) for h in range(2)])                      # [16 chunks, 8]
    img = np.zeros((288, 32, 8), np.float16)
    for row in range(288):
        sw = row & 15
        for c in range(16):
            img[row, c ^ sw] = hi[korder[c], row]
            img[row, 16 + (c ^ sw)] = lo[korder[c], row]
    arr = np.ascontiguousarray(img.reshape(9, 1, 32, 256)).view(np.float32)                          # [9, 1, 32, 128] words
    b = np.zeros(288, np.float32)
    b[:n] = bias
    return arr, b


# Winograd F(2x2, 3x3) filter transform matrix (Lavin & Gray 2016): U = G g G^T
WINO_G = np.array([[1.0, 0.0, 0.0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0.0, 0.0, 1.0]])
WINO_CC = 16          # channels per K chunk of csrc/wino_conv2.h


def wino_filter_transform(kernel_tkn: np.ndarray, dtype=np.float32) -> np.ndarray:
    """A folded 3x3 kernel [9 = (a, b), K, N] -> its 16 transform-position matrices U[4 xi + nu] = sum_ab G[xi, a] g[a, b] G[nu, b],
    [16, K, N], computed in float64 and rounded ONCE to ``dtype`` (float32 for the kernel)."""
    taps, k, n = kernel_tkn.shape
    assert taps == 9
    g = kernel_tkn.astype(np.float64).reshape(3, 3, k, n)
    return np.einsum("xa,abkn,yb->xykn", WINO_G, g, WINO_G).reshape(16, k, n).astype(dtype)


def pack_wino(kernel_tkn: np.ndarray, bias: np.ndarray):
    """res*.conv2 ([9, 128, 128] folded) as the weight stream of csrc/wino_conv2.h: [K chunk][transform position][cout][WINO_CC
    channels] float32, unpadded (the kernel adds the LDS bank pad when it stages a step).  Returns ([8, 16, 128, 16], [128] bias).

    The blob's layout is pinned (one image per layer), so the stream is not a blob entry: bsr_create derives it, once per handle, from
    the float32 weights of the layer's direct image with this very arithmetic (bsr_api.hip: wino_filter_transform, float64, rounded
    once).  This function is its statement — it transforms the float32-rounded folded weights, as the library does — and what the
    kernel's test hook is fed; tests/test_wino_pack_cpu.py holds the library's transform to it."""
    taps, k, n = kernel_tkn.shape
    assert k % WINO_CC == 0
    u = wino_filter_transform(kernel_tkn.astype(np.float32))                                    # [16, K, N]
    arr = np.ascontiguousarray(u.reshape(16, k // WINO_CC, WINO_CC, n).transpose(1, 0, 3, 2))    # [chunk, pos, n, cc]
    return arr, bias.astype(np.float32)


# The transposed 3x3 layers (stride 2) in 25 products per 2x2 input patch instead of 36 (csrc/wino_convt.h).  Per axis
# out(2i) = w0 x(i) + w2 x(i-1), out(2i+1) = w1 x(i); for the patch i = 2p:  t = Bt [x(i-1), x(i), x(i+1)],  u = G [w0, w1, w2],
# m = t . u,  [out(2i) .. out(2i+3)] = At m.
WINO_CONVT_BT = np.array([[0.0, 1, 0], [0, 0, 1], [1, -1, 0], [0, 1, 0], [0, 1, -1]])
WINO_CONVT_G = np.array([[0.0, 1, 0], [0, 1, 0], [0, 0, 1], [1, 0, 1], [1, 0, 0]])
WINO_CONVT_AT = np.array([[0.0, 0, 1, 1, 0], [1, 0, 0, 0, 0], [0, 0, 0, 1, -1], [0, 1, 0, 0, 0]])


def wino_convt_filter_transform(kernel_tkn: np.ndarray, dtype=np.float32) -> np.ndarray:
    """A folded transposed 3x3 kernel [9 = (a, b), K, N] -> its 25 position matrices U[5 r + s] = sum_ab G[r, a] g[a, b] G[s, b],
    [25, K, N], computed in float64 and rounded ONCE to ``dtype`` (float32 for the kernel)."""
    taps, k, n = kernel_tkn.shape
    assert taps == 9
    g = kernel_tkn.astype(np.float64).reshape(3, 3, k, n)
    return np.einsum("xa,abkn,yb->xykn", WINO_CONVT_G, g, WINO_CONVT_G).reshape(25, k, n).astype(dtype)


def pack_wino_convt(kernel_tkn: np.ndarray, bias: np.ndarray):
    """up2 / up3 / clr_up3 ([9, K, 64] folded, K a multiple of 16) as the weight stream of csrc/wino_convt.h, in the order a wave reads its
    B fragments: [K / 16 chunks][25 positions 5 r + s][2 cout halves][2 K groups g][64 lanes 32 h + n][4 j] float32, where the element is
    U[5 r + s, channel 16 chunk + 8 g + 4 h + j, cout 32 half + n].  Returns ([K / 16, 25, 2, 2, 64, 4], [64] bias).

    Like pack_wino's, the stream is not a blob entry: bsr_create derives it, once per fp32 GSC handle, from the float32 weights of the
    layer's direct image with this very arithmetic (bsr_api.hip: wino_convt_filter_transform).  This function is its statement;
    tests/test_wino_convt_pack_cpu.py holds the library's transform to it."""
    taps, k, n = kernel_tkn.shape
    assert k % WINO_CC == 0 and n == 64
    u = wino_convt_filter_transform(kernel_tkn.astype(np.float32))                    # [25, K, N]
    u = u.reshape(25, k // WINO_CC, 2, 2, 4, 2, 32)                                   # [pos, chunk, g, h, j, half, n]
    arr = np.ascontiguousarray(u.transpose(1, 0, 5, 2, 3, 6, 4)).reshape(k // WINO_CC, 25, 2, 2, 64, 4)
    return arr, bias.astype(np.float32)


def pack_wino_clr(kernel_tkn: np.ndarray, gs_tn: np.ndarray) -> np.ndarray:
    """clr_conv1 (folded; kernel_tkn [9, 64, 16] = the f channels, gs_tn [9, 16] = the gs channel) as the weight image of csrc/wino_clr.h:
    [16 positions 4 xi + nu][4 K groups g][64 lanes 16 q + r][4 j] = U[position, channel 16 g + 4 q + j, cout r] in A-fragment order, then
    [16 positions][16 cout] of the gs channel; 16640 float32, flat.

    Like pack_wino's, the image is not a blob entry: bsr_create derives it, once per fp32 handle, from the float32 weights of the blob's
    direct images ('clr_conv1', 'clr_conv1.gs') with this very arithmetic (bsr_api.hip: wino_clr_filter_transform, float64, rounded once).
    This function is its statement; tests/test_wino_clr_cpu.py holds the library's transform to it."""
    taps, k, n = kernel_tkn.shape
    assert (taps, k, n) == (9, 64, 16) and gs_tn.shape == (9, 16)
    u = wino_filter_transform(kernel_tkn.astype(np.float32))                                         # [16, 64, 16]
    u = u.reshape(16, 4, 4, 4, 16).transpose(0, 1, 2, 4, 3)                                          # [pos, g, q, j, r] -> [pos, g, q, r, j]
    ugs = wino_filter_transform(gs_tn.astype(np.float32).reshape(9, 1, 16))                          # [16, 1, 16]
    return np.concatenate([np.ascontiguousarray(u).reshape(-1), ugs.reshape(-1)])


KEYS_N = 288 + 256        # [y3 288 | q' 128 | g 128]
KEYS_N_PAD = KEYS_N + 64  # + two zero tiles of slack (gemm_nloop group reads, NI = 3)


def compose_keys(wq: np.ndarray, bq: np.ndarray, wk: np.ndarray):
    """theta composed onto phi's weights.  With theta = t Wq + bq and phi = t Wk + bk the NonLocalBlock's logits are
    theta_i . phi_j = (theta_i Wk^T) . t_j + theta_i . bk, and the softmax over j removes the second term exactly: with
    q'_i = t_i (Wq Wk^T) + bq Wk^T,  softmax_j(theta_i . phi_j) = softmax_j(q'_i . t_j) — the keys are t itself.
    wq, wk [K, D], bq [D] -> (Wq Wk^T [K, K], bq Wk^T [K]) in float64."""
    wq, wk, bq = wq.astype(np.float64), wk.astype(np.float64), bq.astype(np.float64)
    return wq @ wk.T, bq @ wk.T


def compose_keys_c3q(c3q_w: np.ndarray, c3q_b: np.ndarray):
    """A res<i>.c3q blob entry ([4, 1, 768, 36] image, [768] bias: N = [y3 288 | theta | phi | g | slack]) -> the image of the fp32
    forward that takes conv2's output as the attention keys: ([4, 1, KEYS_N_PAD, 36], [KEYS_N_PAD]), N = [y3 288 | q' 128 | g 128 | 0].

    The blob's layout is pinned, so this image is not a blob entry: bsr_create derives it, once per handle, from the float32 values of
    the blob's image with this very arithmetic (bsr_api.hip: keys_compose — float64 sums, rounded once).  This function is its
    statement; tests/test_keys_conv2_cpu.py holds the library to it."""
    assert c3q_w.shape == (4, 1, 768, 36) and c3q_b.shape == (768,)
    kn = c3q_w[:, 0, :, :32].transpose(0, 2, 1).reshape(128, 768)          # [K, N] float32
    a, ab = compose_keys(kn[:, 288:416], c3q_b[288:416], kn[:, 416:544])
    out = np.zeros((4, 1, KEYS_N_PAD, 36), np.float32)
    out[:, :, :288] = c3q_w[:, :, :288]
    out[:, 0, 288:416, :32] = a.astype(np.float32).reshape(4, 32, 128).transpose(0, 2, 1)
    out[:, :, 416:544] = c3q_w[:, :, 544:672]
    b = np.zeros(KEYS_N_PAD, np.float32)
    b[:288], b[288:416], b[416:544] = c3q_b[:288], ab.astype(np.float32), c3q_b[544:672]
    return out, b


VALUES_N = 288 + 128         # [y3 288 | q' 128]
VALUES_N_PAD = VALUES_N + 64  # + two zero tiles of slack (gemm_nloop group reads, NI = 3)
W_N_PAD = 384                 # res<i>.w: 257 real of 288 + 3 zero tiles of slack (geometry())


def compose_values(wg: np.ndarray, bg: np.ndarray, ww: np.ndarray, bw: np.ndarray):
    """g composed onto the `w` conv.  With g = t Wg + bg and no non-linearity between g and w (model.py:53-56), and softmax rows that
    sum to 1,  softmax(f) g Ww + bw = (softmax(f) t) (Wg Ww) + (bg Ww + bw): the values of the attention are t itself.
    wg [K, D], bg [D], ww [D, N], bw [N] -> (Wg Ww [K, N], bw + bg Ww [N]) in float64, summed over the g channel in channel order
    (float32 inputs have exact float64 products, so the library's loop in the same order gives the same bits)."""
    wg, bg, ww, bw = (a.astype(np.float64) for a in (wg, bg, ww, bw))
    w2, b2 = np.zeros((wg.shape[0], ww.shape[1])), bw.copy()
    for c in range(wg.shape[1]):
        w2 += wg[:, c:c + 1] * ww[c][None, :]
        b2 += bg[c] * ww[c]
    return w2, b2


def compose_values_w(c3q_w: np.ndarray, c3q_b: np.ndarray, w_w: np.ndarray, w_b: np.ndarray):
    """A res<i>.c3q blob entry ([4, 1, 768, 36], [768]: N = [y3 288 | theta | phi | g | slack]) and the block's res<i>.w entry
    ([4, 1, 384, 36], [384]) -> the `w` image of the fp32 forward that takes conv2's output as the attention VALUES as well:
    ([4, 1, 384, 36], [384]) in the layout of res<i>.w, rounded once to float32.

    Like compose_keys_c3q this is the statement of what bsr_create derives per handle (bsr_api.hip: values_compose);
    tests/test_values_conv2_cpu.py holds the library to it bit for bit."""
    assert c3q_w.shape == (4, 1, 768, 36) and c3q_b.shape == (768,) and w_w.shape == (4, 1, W_N_PAD, 36) and w_b.shape == (W_N_PAD,)
    wg = c3q_w[:, 0, 544:672, :32].transpose(0, 2, 1).reshape(128, 128)        # [K, D] float32
    ww = w_w[:, 0, :, :32].transpose(0, 2, 1).reshape(128, W_N_PAD)            # [D, N]
    w2, b2 = compose_values(wg, c3q_b[544:672], ww, w_b)
    out = np.zeros((4, 1, W_N_PAD, 36), np.float32)
    out[:, 0, :, :32] = w2.astype(np.float32).reshape(4, 32, W_N_PAD).transpose(0, 2, 1)
    return out, b2.astype(np.float32)


def layer_matrices(w: Dict[str, np.ndarray]) -> "Dict[str, Tuple[np.ndarray, np.ndarray]]":
    """Folded [taps, K, N] kernels + biases (float64) of every MFMA layer, in kernel K/N order."""
    out: Dict[str, Tuple[np.ndarray, np.ndarray]] = {}

    def hwio(stem):            # Conv2D kernel [kh,kw,ci,co] -> [kh*kw, ci, co]
        k = w[stem + "/kernel"]
        return k.reshape(k.shape[0] * k.shape[1], k.shape[2], k.shape[3])

    # stem 7x7x3: taps = ky, K = kx*3 + c   (im2row7_kernel layout)
    k = w["conv1/conv/kernel"]                                    # [7,7,3,32]
    out["conv1"] = fold_bn(k.reshape(7, 21, 32), w["conv1/conv/bias"], _bn(w, "conv1/bnorm"))
    for nm in ("down1", "down2", "down3"):
        out[nm] = fold_bn(hwio(nm + "/conv"), w[nm + "/conv/bias"], _bn(w, nm + "/bnorm"))
    for nm in TRANSPOSED:                                         # [3,3,co,ci] -> [9, ci, co]
        k = w[nm + "/conv/kernel"]
        out[nm] = fold_bn(k.reshape(9, k.shape[2], k.shape[3]).transpose(0, 2, 1), w[nm + "/conv/bias"], _bn(w, nm + "/bnorm"))
    # heads: taps = ky, K = c, N = kx*2 + head (head 0 = conv2/mask, 1 = conv3/con); bias applied in heads_post
    k2, k3 = w["conv2/conv/kernel"][..., 0], w["conv3/conv/kernel"][..., 0]      # [7,7,64]
    hk = np.stack([k2, k3], axis=-1)                              # [ky,kx,c,head]
    out["heads"] = (hk.transpose(0, 2, 1, 3).reshape(7, 64, 14).astype(np.float64), np.zeros(14))
    # clr_conv1: reference input cat[gs, f] (model.py:267): the 64 f channels go through the K = 64 MFMA loop,
    # the gs channel (reference channel 0) is a separate 9-tap K group ("clr_conv1.gs", see clr_gs_weights)
    k, b = fold_bn(hwio("clr_conv1/conv"), w["clr_conv1/conv/bias"], _bn(w, "clr_conv1/bnorm"))   # [9,65,16]
    out["clr_conv1"] = (k[:, 1:, :], b)
    for i in range(N_RES):
        st = "res_stack/%d/" % i
        out["res%d.conv1" % i] = fold_bn(hwio(st + "conv1"), w[st + "conv1/bias"], _bn(w, st + "bnorm1"))
        out["res%d.conv2" % i] = fold_bn(hwio(st + "conv2"), w[st + "conv2/bias"], _bn(w, st + "bnorm2"))
        # conv3 + bnorm3 -> y3 (257), then theta | phi | g = 1x1 convs of y3 with NO nonlinearity in between
        # (model.py:101-102, 33-46): composed offline into one K = 128 GEMM, N = [y3 (257, padded to 288) | q k v (3 x 128)].
        # theta | phi | g keep the query / key / value order of the attention kernel.
        k3, b3 = fold_bn(hwio(st + "conv3"), w[st + "conv3/bias"], _bn(w, st + "bnorm3"))            # [1,128,257], [257]
        qkv = np.concatenate([hwio(st + "non_local/" + n) for n in ("theta", "phi", "g")], axis=2).astype(np.float64)   # [1,257,384]
        qb = np.concatenate([w[st + "non_local/%s/bias" % n] for n in ("theta", "phi", "g")]).astype(np.float64)
        kc = np.zeros((1, 128, 672))
        bc = np.zeros(672)
        kc[0, :, :257] = k3[0]
        bc[:257] = b3
        kc[0, :, 288:] = k3[0] @ qkv[0]
        bc[288:] = b3 @ qkv[0] + qb
        out["res%d.c3q" % i] = (kc, bc)
        out["res%d.w" % i] = fold_bn(hwio(st + "non_local/w"), w[st + "non_local/w/bias"], _bn(w, st + "non_local/bnorm"))
    return out


def layer_matrices_rgb(w: Dict[str, np.ndarray]) -> "Dict[str, Tuple[np.ndarray, np.ndarray]]":
    """layer_matrices() of the RGB baseline (/root/reference/model_RGB.py:198-266): folded [taps, K, N] kernels + biases (float64)."""
    out: Dict[str, Tuple[np.ndarray, np.ndarray]] = {}

    def hwio(stem):
        k = w[stem + "/kernel"]
        return k.reshape(k.shape[0] * k.shape[1], k.shape[2], k.shape[3])

    k = w["conv1/conv/kernel"]
    out["conv1"] = fold_bn(k.reshape(7, 21, 32), w["conv1/conv/bias"], _bn(w, "conv1/bnorm"))
    for nm in ("down1", "down2", "down3"):
        out[nm] = fold_bn(hwio(nm + "/conv"), w[nm + "/conv/bias"], _bn(w, nm + "/bnorm"))
    for nm in ("up1", "up2", "up3"):
        k = w[nm + "/conv/kernel"]
        out[nm] = fold_bn(k.reshape(9, k.shape[2], k.shape[3]).transpose(0, 2, 1), w[nm + "/conv/bias"], _bn(w, nm + "/bnorm"))
    # conv2 'tconv3' (7x7, 128 -> 3, no BN): taps = ky, K = c, N = kx * 3 + co; its bias is added after the horizontal sum (rgb_head.h)
    k2 = w["conv2/conv/kernel"].astype(np.float64)                             # [ky, kx, c, co]
    out["rgb_head"] = (k2.transpose(0, 2, 1, 3).reshape(7, 128, 21), np.zeros(21))
    for i in range(N_RES // 2):
        st = "res_stack/%d/" % i
        out["res%d.conv1" % i] = fold_bn(hwio(st + "conv1"), w[st + "conv1/bias"], _bn(w, st + "bnorm1"))
        out["res%d.conv2" % i] = fold_bn(hwio(st + "conv2"), w[st + "conv2/bias"], _bn(w, st + "bnorm2"))
        # conv3 + bnorm3 -> y3 (513), then theta | phi | g with no nonlinearity in between: one K = 256 GEMM, N = [y3 (513 of 544) | q k v]
        k3, b3 = fold_bn(hwio(st + "conv3"), w[st + "conv3/bias"], _bn(w, st + "bnorm3"))            # [1,256,513], [513]
        qkv = np.concatenate([hwio(st + "non_local/" + n) for n in ("theta", "phi", "g")], axis=2).astype(np.float64)   # [1,513,768]
        qb = np.concatenate([w[st + "non_local/%s/bias" % n] for n in ("theta", "phi", "g")]).astype(np.float64)
        kc = np.zeros((1, 256, 544 + 768))
        bc = np.zeros(544 + 768)
        kc[0, :, :513] = k3[0]
        bc[:513] = b3
        kc[0, :, 544:] = k3[0] @ qkv[0]
        bc[544:] = b3 @ qkv[0] + qb
        out["res%d.c3q" % i] = (kc, bc)
        out["res%d.w" % i] = fold_bn(hwio(st + "non_local/w"), w[st + "non_local/w/bias"], _bn(w, st + "non_local/bnorm"))
    return out


def rgb_tail_weights(w: Dict[str, np.ndarray]) -> np.ndarray:
    """conv3 'tconv4' (7x7, 3 -> 3, no BN) as HWIO [7][7][3][3] then its bias [3], for rgb_conv7_kernel (csrc/rgb_head.h)."""
    return np.concatenate([w["conv3/conv/kernel"].reshape(-1), w["conv3/conv/bias"]]).astype(np.float32)


def clr_gs_weights(w: Dict[str, np.ndarray]) -> np.ndarray:
    """[16 n][16 k] float32: BN-folded clr_conv1 weights of the gs input channel, k = 3x3 tap index (k >= 9 zero)."""
    k, _ = fold_bn(w["clr_conv1/conv/kernel"].reshape(9, 65, 16), w["clr_conv1/conv/bias"], _bn(w, "clr_conv1/bnorm"))
    out = np.zeros((16, 16), np.float32)
    out[:, :9] = k[:, 0, :].T
    return out


def tail_weights(w: Dict[str, np.ndarray]) -> np.ndarray:
    """clr_conv2 (folded, k-major [16][16]) | bias[16] | clr_conv3 [16][3] | bias[3] for the fused tail of conv_n16_kernel (csrc/conv_n16.h)."""
    k2, b2 = fold_bn(w["clr_conv2/conv/kernel"].reshape(1, 16, 16), w["clr_conv2/conv/bias"], _bn(w, "clr_conv2/bnorm"))
    k3 = w["clr_conv3/conv/kernel"].reshape(16, 3).astype(np.float64)
    return np.concatenate([k2.reshape(-1), b2, k3.reshape(-1), w["clr_conv3/conv/bias"].astype(np.float64)]).astype(np.float32)


def pack_generator(weights: Dict[str, np.ndarray], dtype: str = "f32") -> bytes:
    """reference-named variables -> blob for ``bsr_create(..., dtype)`` (the blob header records the dtype it was packed for)."""
    if dtype not in DTYPES:
        raise ValueError("dtype must be one of %s" % sorted(DTYPES))
    variant = detect_variant(weights)
    check_weights(weights, variant)
    if variant == "rgb":
        return _pack_rgb(weights, dtype)
    geo = geometry(variant, dtype)
    entries: List[Tuple[str, np.ndarray, Tuple[int, int, int, int]]] = []
    for name, (k, b) in layer_matrices(weights).items():
        cc, k_pad, n_pad = geo[name]
        if dtype != "f32" and name in H16_LAYERS:
            arr, bias = pack_taps_h16(k, b, cc, k_pad, n_pad, 2 if dtype == "f32x3" else 1, swizzle=(dtype == "f32x3" and cc == 32))
        elif dtype != "f32" and name in X3_LAYERS:
            arr, bias = pack_taps_h16(k, b, cc, k_pad, n_pad, 2)
        else:
            arr, bias = pack_taps(k, b, cc, k_pad, n_pad)
        entries.append((name + ".w", arr, tuple(arr.shape)))
        entries.append((name + ".b", bias, (n_pad, 0, 0, 0)))
        if dtype == "f16" and name in W3_LAYERS:
            arr3, bias3 = pack_w3(k, b, k_pad)
            entries.append((name + ".w3.w", arr3, tuple(arr3.shape)))
            entries.append((name + ".w3.b", bias3, (bias3.shape[0], 0, 0, 0)))
        if dtype != "f32" and name.startswith("res") and name.endswith(".w"):
            arr4, bias4 = pack_w4(k, b)
            entries.append((name + "4.w", arr4, tuple(arr4.shape)))
            entries.append((name + "4.b", bias4, (288, 0, 0, 0)))
    entries.append(("heads.bias", np.array([weights["conv2/conv/bias"][0], weights["conv3/conv/bias"][0]], np.float32), (2, 0, 0, 0)))
    entries.append(("clr_conv1.gs", clr_gs_weights(weights), (16, 16, 0, 0)))
    entries.append(("tail.w", tail_weights(weights), (323, 0, 0, 0)))
    return _write_blob(entries, dtype)


def _pack_rgb(weights: Dict[str, np.ndarray], dtype: str) -> bytes:
    geo = geometry_rgb(dtype)
    entries: List[Tuple[str, np.ndarray, Tuple[int, int, int, int]]] = []
    for name, (k, b) in layer_matrices_rgb(weights).items():
        cc, k_pad, n_pad = geo[name]
        arr, bias = pack_taps(k, b, cc, k_pad, n_pad)
        entries.append((name + ".w", arr, tuple(arr.shape)))
        entries.append((name + ".b", bias, (n_pad, 0, 0, 0)))
    entries.append(("rgb.head_bias", weights["conv2/conv/bias"].astype(np.float32), (3, 0, 0, 0)))
    entries.append(("rgb.tail", rgb_tail_weights(weights), (444, 0, 0, 0)))
    return _write_blob(entries, dtype)


def _write_blob(entries, dtype: str) -> bytes:
    off = _HEADER.size + _ENTRY.size * len(entries)
    off = (off + 255) & ~255
    table = bytearray()
    chunks = []
    for name, arr, dims in entries:
        raw = np.ascontiguousarray(arr, dtype="<f4").tobytes()
        table += _ENTRY.pack(name.encode(), off, arr.size, *dims)
        chunks.append((off, raw))
        off = (off + len(raw) + 255) & ~255
    blob = bytearray(off)
    blob[:_HEADER.size] = _HEADER.pack(BLOB_MAGIC, BLOB_VERSION, len(entries), DTYPES[dtype])
    blob[_HEADER.size:_HEADER.size + len(table)] = table
    for o, raw in chunks:
        blob[o:o + len(raw)] = raw
    return bytes(blob)


# ---- the three patch discriminators (csrc/disc_kernels.h): a blob of its own, no header, float32 ----
DISC_CC = 8                  # channels per K chunk of disc_conv_kernel; the first layer's 6 input channels are padded to 8
DISC_TAPS = 16


def disc_layout():
    """([(name, offset in floats, shape)] of ONE discriminator, floats per discriminator).  A stride-2 layer `conv<i>` is stored as the
    kernel stages it, a chunk of 8 input channels at a time: w [C_in / 8][16 taps (a * 4 + b)][8][N], then bias [N], BatchNormalization
    folded; the head as w [16 taps][64], then [bias, 0, 0, 0].  Every offset is a multiple of 4 floats.  The blob is the three
    discriminators' records in order."""
    from .weights import DISC_CH, DISC_IN_CH
    out, off, cin = [], 0, -(-DISC_IN_CH // DISC_CC) * DISC_CC
    for i, n in enumerate(DISC_CH):
        out.append(("conv%d/w" % i, off, (cin // DISC_CC, DISC_TAPS, DISC_CC, n)))
        off += DISC_TAPS * cin * n
        out.append(("conv%d/b" % i, off, (n,)))
        off += n
        cin = n
    out.append(("head/w", off, (DISC_TAPS, cin)))
    off += DISC_TAPS * cin
    out.append(("head/b", off, (4,)))
    return out, off + 4


def disc_folded(weights: Dict[str, np.ndarray], k: int):
    """{`conv<i>`: (kernel [16, C_in padded to 8, N], bias [N]), `head`: (kernel [16, 64, 1], bias [1])} of discriminator k, float32,
    BatchNormalization folded with fold_bn."""
    from .weights import DISC_CH
    out = {}
    for i in range(len(DISC_CH)):
        st = "discriminator_%d/conv_stack/%d" % (k, i)
        kern = np.asarray(weights[st + "/conv/kernel"])
        kt, b = fold_bn(kern.reshape(DISC_TAPS, kern.shape[2], kern.shape[3]), np.asarray(weights[st + "/conv/bias"]), _bn(weights, st + "/bnorm"))
        cin = -(-kt.shape[1] // DISC_CC) * DISC_CC
        full = np.zeros((DISC_TAPS, cin, kt.shape[2]), np.float32)
        full[:, :kt.shape[1]] = kt
        out["conv%d" % i] = (full, b.astype(np.float32))
    st = "discriminator_%d/conv2/conv/" % k
    kern = np.asarray(weights[st + "kernel"])
    out["head"] = (kern.reshape(DISC_TAPS, kern.shape[2], 1).astype(np.float32), np.asarray(weights[st + "bias"]).astype(np.float32))
    return out


def pack_discriminators(weights: Dict[str, np.ndarray]) -> bytes:
    """The three discriminators' variables (weights.discriminator_variable_shapes) -> the blob bsr_disc_losses takes (disc_layout)."""
    from .weights import check_discriminator_weights
    check_discriminator_weights(weights)
    layout, per = disc_layout()
    blob = np.zeros((3, per), np.float32)
    for k in (1, 2, 3):
        folded = disc_folded(weights, k)
        for name, off, shape in layout:
            kern, bias = folded[name.split("/")[0]]
            if name == "head/w":
                a = kern[:, :, 0]
            elif name == "head/b":
                a = np.array([bias[0], 0, 0, 0], np.float32)
            elif name.endswith("/w"):
                a = kern.reshape(DISC_TAPS, shape[0], DISC_CC, shape[3]).transpose(1, 0, 2, 3)
            else:
                a = bias
            assert a.shape == tuple(shape)
            blob[k - 1, off:off + a.size] = a.reshape(-1)
    return blob.tobytes()


def unpack_discriminators(blob: bytes):
    """The inverse of pack_discriminators: [disc_folded(w, 1), disc_folded(w, 2), disc_folded(w, 3)]."""
    layout, per = disc_layout()
    arr = np.frombuffer(blob, np.float32)
    if arr.size != 3 * per:
        raise ValueError("a discriminator blob holds %d bytes, got %d" % (3 * per * 4, len(blob)))
    out = []
    for k in range(3):
        rec = {name: arr[k * per + off:k * per + off + int(np.prod(shape))].reshape(shape) for name, off, shape in layout}
        d = {}
        for name in rec:
            stem = name.split("/")[0]
            if stem == "head" or stem in d:
                continue
            w = rec[stem + "/w"]
            d[stem] = (w.transpose(1, 0, 2, 3).reshape(DISC_TAPS, w.shape[0] * DISC_CC, w.shape[3]).copy(), rec[stem + "/b"].copy())
        d["head"] = (rec["head/w"][:, :, None].copy(), rec["head/b"][:1].copy())
        out.append(d)
    return out


DISC_GRAD_IN_C = 3           # the image channels of a discriminator's input: the only ones whose gradient is wanted


def disc_dgrad_layout():
    """([(name, offset in floats, shape)] of ONE discriminator, floats per discriminator) of the gradient layers' blob
    (csrc/disc_grad_kernels.h).  The input gradient of `conv<i>`, i = 1, 2, 3, runs from its C' = C_out to its N' = C_in channels and is
    stored as disc_dgrad_kernel stages it, a chunk of 8 output channels at a time: [C_out / 8][16 taps (a * 4 + b)][8][C_in], the folded
    kernel of disc_folded with the channel roles swapped (k'[t, o, c] = k[t, c, o]); the taps keep their places, the kernel picks the
    four of each sub-pixel phase.  `conv0`, whose gradient is wanted on the 3 image channels only, as [16 taps][3][32].  No bias.  The
    blob is the three discriminators' records in order."""
    from .weights import DISC_CH
    out, off, cin = [("conv0/dgrad", 0, (DISC_TAPS, DISC_GRAD_IN_C, DISC_CH[0]))], DISC_TAPS * DISC_GRAD_IN_C * DISC_CH[0], DISC_CH[0]
    for i, n in list(enumerate(DISC_CH))[1:]:
        out.append(("conv%d/dgrad" % i, off, (n // DISC_CC, DISC_TAPS, DISC_CC, cin)))
        off += DISC_TAPS * cin * n
        cin = n
    return out, off


def pack_discriminators_dgrad(weights: Dict[str, np.ndarray]) -> bytes:
    """The three discriminators' variables -> the blob bsr_disc_gen_grad takes beside pack_discriminators' (disc_dgrad_layout)."""
    from .weights import check_discriminator_weights
    check_discriminator_weights(weights)
    layout, per = disc_dgrad_layout()
    blob = np.zeros((3, per), np.float32)
    for k in (1, 2, 3):
        folded = disc_folded(weights, k)
        for name, off, shape in layout:
            swapped = folded[name.split("/")[0]][0].transpose(0, 2, 1)             # [16][N][C_in padded]
            if name == "conv0/dgrad":
                a = swapped[:, :, :DISC_GRAD_IN_C].transpose(0, 2, 1)
            else:
                a = swapped.reshape(DISC_TAPS, shape[0], DISC_CC, shape[3]).transpose(1, 0, 2, 3)
            assert a.shape == tuple(shape)
            blob[k - 1, off:off + a.size] = a.reshape(-1)
    return blob.tobytes()


def unpack_discriminators_dgrad(blob: bytes):
    """The inverse of pack_discriminators_dgrad: per discriminator {`conv<i>`: the folded kernel [16, C_in, N] of disc_folded}, conv0's
    cut to its 3 image channels."""
    layout, per = disc_dgrad_layout()
    arr = np.frombuffer(blob, np.float32)
    if arr.size != 3 * per:
        raise ValueError("a discriminator gradient blob holds %d bytes, got %d" % (3 * per * 4, len(blob)))
    out = []
    for k in range(3):
        d = {}
        for name, off, shape in layout:
            a = arr[k * per + off:k * per + off + int(np.prod(shape))].reshape(shape)
            if name == "conv0/dgrad":
                d["conv0"] = a.copy()
            else:
                d[name.split("/")[0]] = a.transpose(1, 0, 2, 3).reshape(DISC_TAPS, shape[0] * DISC_CC, shape[3]).transpose(0, 2, 1).copy()
        out.append(d)
    return out


DISC_WGRAD_VECS = ("bias", "inv", "moving_mean", "rstd")


def disc_wgrad_layout():
    """([(name, offset in floats, shape)] of ONE discriminator, floats per discriminator) of the weight-gradient chain's blob
    (csrc/disc_wgrad_kernels.h): per stride-2 layer `conv<i>` the UNFOLDED kernel [16 taps (a * 4 + b)][C_in padded to 8][N] (d gamma
    is formed from it), then four vectors [4][N]: the convolution's bias, inv = gamma / sqrt(moving_variance + eps), moving_mean and
    rstd = 1 / sqrt(moving_variance + eps), inv and rstd formed in float64 and rounded once.  The head needs nothing here.  The blob is
    the three discriminators' records in order."""
    from .weights import DISC_CH, DISC_IN_CH
    out, off, cin = [], 0, -(-DISC_IN_CH // DISC_CC) * DISC_CC
    for i, n in enumerate(DISC_CH):
        out.append(("conv%d/kernel" % i, off, (DISC_TAPS, cin, n)))
        off += DISC_TAPS * cin * n
        out.append(("conv%d/vecs" % i, off, (len(DISC_WGRAD_VECS), n)))
        off += len(DISC_WGRAD_VECS) * n
        cin = n
    return out, off


def disc_wgrad_record(weights: Dict[str, np.ndarray], k: int):
    """{`conv<i>/kernel`: [16, C_in padded to 8, N], `conv<i>/vecs`: [4, N] (DISC_WGRAD_VECS)} of discriminator k, float32."""
    from .weights import BN_EPS, DISC_CH
    out = {}
    for i in range(len(DISC_CH)):
        st = "discriminator_%d/conv_stack/%d" % (k, i)
        kern = np.asarray(weights[st + "/conv/kernel"], np.float32)
        cin = -(-kern.shape[2] // DISC_CC) * DISC_CC
        full = np.zeros((DISC_TAPS, cin, kern.shape[3]), np.float32)
        full[:, :kern.shape[2]] = kern.reshape(DISC_TAPS, kern.shape[2], kern.shape[3])
        rstd = 1.0 / np.sqrt(np.asarray(weights[st + "/bnorm/moving_variance"], np.float64) + BN_EPS)
        inv = np.asarray(weights[st + "/bnorm/gamma"], np.float64) * rstd
        out["conv%d/kernel" % i] = full
        out["conv%d/vecs" % i] = np.stack([np.asarray(weights[st + "/conv/bias"], np.float64), inv,
                                          np.asarray(weights[st + "/bnorm/moving_mean"], np.float64), rstd]).astype(np.float32)
    return out


def pack_discriminators_wgrad(weights: Dict[str, np.ndarray]) -> bytes:
    """The three discriminators' variables -> the blob bsr_disc_wgrad takes beside the other two (disc_wgrad_layout)."""
    from .weights import check_discriminator_weights
    check_discriminator_weights(weights)
    layout, per = disc_wgrad_layout()
    blob = np.zeros((3, per), np.float32)
    for k in (1, 2, 3):
        rec = disc_wgrad_record(weights, k)
        for name, off, shape in layout:
            assert rec[name].shape == tuple(shape)
            blob[k - 1, off:off + rec[name].size] = rec[name].reshape(-1)
    return blob.tobytes()


def unpack_discriminators_wgrad(blob: bytes):
    """The inverse of pack_discriminators_wgrad: [disc_wgrad_record(w, 1), disc_wgrad_record(w, 2), disc_wgrad_record(w, 3)]."""
    layout, per = disc_wgrad_layout()
    arr = np.frombuffer(blob, np.float32)
    if arr.size != 3 * per:
        raise ValueError("a discriminator weight-gradient blob holds %d bytes, got %d" % (3 * per * 4, len(blob)))
    return [{name: arr[k * per + off:k * per + off + int(np.prod(shape))].reshape(shape).copy() for name, off, shape in layout} for k in range(3)]


# ---- the generator's colour tail backward (csrc/clr_tail_grad_kernels.h): a blob of its own, no header, float32 ----
CLR_TAIL_VECS = ("bias", "inv", "moving_mean", "rstd")


def clr_tail_grad_layout():
    """([(name, offset in floats, shape)], floats) of the colour tail's gradient blob:
      fwd/w, fwd/bias, fwd/gs  the forward images conv_n16_kernel<3,3,GS> recomputes a1 from: pack_taps of the BN-folded clr_conv1
                               kernel's 64 f channels, its folded bias, clr_gs_weights
      tail/k2f, tail/b2f       clr_conv2 BN-folded, [16 k][16 n] and [16]: z2 = a1 k2f + b2f, and (gz2 inv2) K2^T = gz2 k2f^T
      tail/k3                  clr_conv3's kernel [16 k][4], column 3 zero
      dgrad/w, dgrad/gs        the BN-folded clr_conv1 kernel FLIPPED for the data gradient: [9 taps (ta, tb)][64 c][16 o] =
                               k1f[2 - ta, 2 - tb, 1 + c, o] and [9][16 o] = k1f[2 - ta, 2 - tb, 0, o] (gz1 inv1 through K1 = gz1
                               through k1f)
      k1, k2                   the UNFOLDED kernels [9][65][16] and [16][16] (d gamma is formed from them)
      vecs1, vecs2             [4][16] per layer: the convolution's bias, inv, moving_mean, rstd (CLR_TAIL_VECS)
    inv, rstd and every folded product are formed in float64 and rounded once."""
    out, off = [], 0
    for name, shape in (("fwd/w", (2, 9, 16, 36)), ("fwd/bias", (16,)), ("fwd/gs", (16, 16)), ("tail/k2f", (16, 16)), ("tail/b2f", (16,)),
                        ("tail/k3", (16, 4)), ("dgrad/w", (9, 64, 16)), ("dgrad/gs", (9, 16)), ("k1", (9, 65, 16)), ("k2", (16, 16)),
                        ("vecs1", (4, 16)), ("vecs2", (4, 16))):
        out.append((name, off, shape))
        off += int(np.prod(shape))
    return out, off


def clr_tail_grad_record(weights: Dict[str, np.ndarray]) -> Dict[str, np.ndarray]:
    """name -> float32 array of clr_tail_grad_layout's shapes."""
    from .weights import BN_EPS
    k1 = np.asarray(weights["clr_conv1/conv/kernel"], np.float64).reshape(9, 65, 16)
    k2 = np.asarray(weights["clr_conv2/conv/kernel"], np.float64).reshape(1, 16, 16)
    k1f, b1f = fold_bn(k1, weights["clr_conv1/conv/bias"], _bn(weights, "clr_conv1/bnorm"))
    k2f, b2f = fold_bn(k2, weights["clr_conv2/conv/bias"], _bn(weights, "clr_conv2/bnorm"))
    rec = {}
    rec["fwd/w"], rec["fwd/bias"] = pack_taps(k1f[:, 1:, :], b1f, 32, 64, 16)
    rec["fwd/gs"] = clr_gs_weights(weights)
    rec["tail/k2f"], rec["tail/b2f"] = k2f[0], b2f
    k3 = np.zeros((16, 4), np.float64)
    k3[:, :3] = np.asarray(weights["clr_conv3/conv/kernel"], np.float64).reshape(16, 3)
    rec["tail/k3"] = k3
    flipped = k1f.reshape(3, 3, 65, 16)[::-1, ::-1].reshape(9, 65, 16)
    rec["dgrad/w"], rec["dgrad/gs"] = flipped[:, 1:, :], flipped[:, 0, :]
    rec["k1"], rec["k2"] = k1, k2[0]
    for i, stem in ((1, "clr_conv1"), (2, "clr_conv2")):
        rstd = 1.0 / np.sqrt(np.asarray(weights[stem + "/bnorm/moving_variance"], np.float64) + BN_EPS)
        rec["vecs%d" % i] = np.stack([np.asarray(weights[stem + "/conv/bias"], np.float64), np.asarray(weights[stem + "/bnorm/gamma"], np.float64) * rstd,
                                      np.asarray(weights[stem + "/bnorm/moving_mean"], np.float64), rstd])
    return {name: np.ascontiguousarray(a, np.float32) for name, a in rec.items()}


def pack_clr_tail_grad(weights: Dict[str, np.ndarray]) -> bytes:
    """The generator's variables (the colour tail's 16 are read) -> the blob bsr_clr_tail_grad takes (clr_tail_grad_layout)."""
    layout, total = clr_tail_grad_layout()
    rec = clr_tail_grad_record(weights)
    blob = np.zeros(total, np.float32)
    for name, off, shape in layout:
        assert rec[name].shape == tuple(shape), name
        blob[off:off + rec[name].size] = rec[name].reshape(-1)
    return blob.tobytes()


def unpack_clr_tail_grad(blob: bytes) -> Dict[str, np.ndarray]:
    """The inverse of pack_clr_tail_grad: clr_tail_grad_record's dict."""
    layout, total = clr_tail_grad_layout()
    arr = np.frombuffer(blob, np.float32)
    if arr.size != total:
        raise ValueError("a colour tail gradient blob holds %d bytes, got %d" % (total * 4, len(blob)))
    return {name: arr[off:off + int(np.prod(shape))].reshape(shape).copy() for name, off, shape in layout}


# ---- the generator's colour decoder backward (csrc/clr_up_grad_kernels.h): a blob of its own, no header, float32 ----
CLR_DECODER_SHAPES = ((128, 261, 288), (96, 128, 128), (64, 96, 96))          # (O, C, C padded) of clr_up1, clr_up2, clr_up3
CLR_DECODER_TSM_TEXT = "the colour decoder's device chain takes the GSC width only: clr_up1's kernel must be [3,3,128,261], got %s (TSM's 877 is covered by generator_grad.decoder_grad)"


def clr_decoder_grad_layout():
    """([(name, offset in floats, shape)], floats) of the colour decoder's gradient blob, per layer i = 1, 2, 3:
      k<i>       the UNFOLDED kernel [9 taps (a * 3 + b)][O][C], the variable's own order (d gamma is formed from it)
      kf<i>      the data gradient's kernel inv[o] K [9][O][C padded]: clr_up1's 261 columns padded with zeros to 288
      vecs<i>    [4][O]: the convolution's bias, inv, moving_mean, rstd (CLR_TAIL_VECS)
    inv, rstd and the folded kernel are formed in float64 and rounded once."""
    out, off = [], 0
    for i, (o, c, cp) in enumerate(CLR_DECODER_SHAPES, 1):
        for name, shape in (("k%d" % i, (9, o, c)), ("kf%d" % i, (9, o, cp)), ("vecs%d" % i, (4, o))):
            out.append((name, off, shape))
            off += int(np.prod(shape))
    return out, off


def clr_decoder_grad_record(weights: Dict[str, np.ndarray]) -> Dict[str, np.ndarray]:
    """name -> float32 array of clr_decoder_grad_layout's shapes.  ValueError for any width but the GSC one."""
    from .weights import BN_EPS
    rec = {}
    for i, (o, c, cp) in enumerate(CLR_DECODER_SHAPES, 1):
        stem = "clr_up%d" % i
        k = np.asarray(weights[stem + "/conv/kernel"], np.float64)
        if k.shape != (3, 3, o, c):
            raise ValueError(CLR_DECODER_TSM_TEXT % (k.shape,) if i == 1 else "%s/conv/kernel must be [3,3,%d,%d], got %s" % (stem, o, c, k.shape))
        k = k.reshape(9, o, c)
        rstd = 1.0 / np.sqrt(np.asarray(weights[stem + "/bnorm/moving_variance"], np.float64) + BN_EPS)
        inv = np.asarray(weights[stem + "/bnorm/gamma"], np.float64) * rstd
        kf = np.zeros((9, o, cp), np.float64)
        kf[:, :, :c] = k * inv[None, :, None]
        rec["k%d" % i], rec["kf%d" % i] = k, kf
        rec["vecs%d" % i] = np.stack([np.asarray(weights[stem + "/conv/bias"], np.float64), inv, np.asarray(weights[stem + "/bnorm/moving_mean"], np.float64), rstd])
    return {name: np.ascontiguousarray(a, np.float32) for name, a in rec.items()}


def pack_clr_decoder_grad(weights: Dict[str, np.ndarray]) -> bytes:
    """The generator's variables (the colour decoder's 18 are read) -> the blob bsr_clr_decoder_grad takes (clr_decoder_grad_layout)."""
    layout, total = clr_decoder_grad_layout()
    rec = clr_decoder_grad_record(weights)
    blob = np.zeros(total, np.float32)
    for name, off, shape in layout:
        assert rec[name].shape == tuple(shape), name
        blob[off:off + rec[name].size] = rec[name].reshape(-1)
    return blob.tobytes()


def unpack_clr_decoder_grad(blob: bytes) -> Dict[str, np.ndarray]:
    """The inverse of pack_clr_decoder_grad: clr_decoder_grad_record's dict."""
    layout, total = clr_decoder_grad_layout()
    arr = np.frombuffer(blob, np.float32)
    if arr.size != total:
        raise ValueError("a colour decoder gradient blob holds %d bytes, got %d" % (total * 4, len(blob)))
    return {name: arr[off:off + int(np.prod(shape))].reshape(shape).copy() for name, off, shape in layout}


# ---- the generator's grey decoder backward (csrc/grey_up_grad_kernels.h): the colour decoder's blob at the grey widths ----
GREY_DECODER_SHAPES = ((96, 257, 288), (64, 160, 160), (64, 128, 128))          # (O, C, C padded) of up1, up2 (on cat[up1, x3]), up3 (on cat[up2, x2])
GREY_DECODER_WIDTH_TEXT = ("the grey decoder's device chain takes the GSC widths only: %s/conv/kernel must be [3,3,%d,%d], got %s (TSM's 291-wide up1 and the "
                           "RGB baseline's 513-wide one are covered by generator_grad.grey_decoder_grad's arithmetic, not by this blob)")


def grey_decoder_grad_layout():
    """([(name, offset in floats, shape)], floats) of the grey decoder's gradient blob, per layer i = 1, 2, 3, as clr_decoder_grad_layout:
      k<i>       the UNFOLDED kernel [9 taps (a * 3 + b)][O][C], the variable's own order, C in the cat order
      kf<i>      the data gradient's kernel inv[o] K [9][O][C padded]: up1's 257 columns padded with zeros to 288
      vecs<i>    [4][O]: the convolution's bias, inv, moving_mean, rstd
    inv, rstd and the folded kernel are formed in float64 and rounded once."""
    out, off = [], 0
    for i, (o, c, cp) in enumerate(GREY_DECODER_SHAPES, 1):
        for name, shape in (("k%d" % i, (9, o, c)), ("kf%d" % i, (9, o, cp)), ("vecs%d" % i, (4, o))):
            out.append((name, off, shape))
            off += int(np.prod(shape))
    return out, off


def grey_decoder_grad_record(weights: Dict[str, np.ndarray]) -> Dict[str, np.ndarray]:
    """name -> float32 array of grey_decoder_grad_layout's shapes.  ValueError for any width but the GSC one (TSM, RGB)."""
    from .weights import BN_EPS
    rec = {}
    for i, (o, c, cp) in enumerate(GREY_DECODER_SHAPES, 1):
        stem = "up%d" % i
        k = np.asarray(weights[stem + "/conv/kernel"], np.float64)
        if k.shape != (3, 3, o, c):
            raise ValueError(GREY_DECODER_WIDTH_TEXT % (stem, o, c, k.shape))
        k = k.reshape(9, o, c)
        rstd = 1.0 / np.sqrt(np.asarray(weights[stem + "/bnorm/moving_variance"], np.float64) + BN_EPS)
        inv = np.asarray(weights[stem + "/bnorm/gamma"], np.float64) * rstd
        kf = np.zeros((9, o, cp), np.float64)
        kf[:, :, :c] = k * inv[None, :, None]
        rec["k%d" % i], rec["kf%d" % i] = k, kf
        rec["vecs%d" % i] = np.stack([np.asarray(weights[stem + "/conv/bias"], np.float64), inv, np.asarray(weights[stem + "/bnorm/moving_mean"], np.float64), rstd])
    return {name: np.ascontiguousarray(a, np.float32) for name, a in rec.items()}


def pack_grey_decoder_grad(weights: Dict[str, np.ndarray]) -> bytes:
    """The generator's variables (the grey decoder's 18 are read) -> the blob bsr_grey_decoder_grad takes (grey_decoder_grad_layout)."""
    layout, total = grey_decoder_grad_layout()
    rec = grey_decoder_grad_record(weights)
    blob = np.zeros(total, np.float32)
    for name, off, shape in layout:
        assert rec[name].shape == tuple(shape), name
        blob[off:off + rec[name].size] = rec[name].reshape(-1)
    return blob.tobytes()


def unpack_grey_decoder_grad(blob: bytes) -> Dict[str, np.ndarray]:
    """The inverse of pack_grey_decoder_grad: grey_decoder_grad_record's dict."""
    layout, total = grey_decoder_grad_layout()
    arr = np.frombuffer(blob, np.float32)
    if arr.size != total:
        raise ValueError("a grey decoder gradient blob holds %d bytes, got %d" % (total * 4, len(blob)))
    return {name: arr[off:off + int(np.prod(shape))].reshape(shape).copy() for name, off, shape in layout}


# ---- the generator's non-local block backward (csrc/nonlocal_grad_kernels.h): a blob of its own, no header, float32 ----
NONLOCAL_TSM_TEXT = "the non-local block's device chain takes the GSC width only (TSM's 877 is covered by generator_grad.nonlocal_grad)"
NONLOCAL_CP = 272            # 257 channels padded to the GEMMs' 16-channel steps


def nonlocal_grad_layout():
    """([(name, offset in floats, shape)], floats) of the non-local block's gradient blob:
      wqkv   [272][384]  the FORWARD image [Wt | Wp | Wg], rows = y3's channels (257..271 zero)
      bqkv   [384]       [bt | bp | bg]
      wwf    [272][128]  the TRANSPOSED, BN-folded image of w for the data gradient: wwf[n][k] = inv[n] Ww[k][n] (rows 257..271 zero)
      wqkvT  [384][384]  the TRANSPOSED image of [Wt | Wp | Wg] for the data gradient: wqkvT[j][c] = wqkv[c][j] (columns 257.. zero)
      ww     [128][257]  w's kernel in the variable's own order (d gamma is formed from it)
      vecs   [4][257]    w's bias, inv, moving_mean, rstd (CLR_TAIL_VECS)
    inv, rstd and the folded image are formed in float64 and rounded once."""
    out, off = [], 0
    for name, shape in (("wqkv", (NONLOCAL_CP, 384)), ("bqkv", (384,)), ("wwf", (NONLOCAL_CP, 128)), ("wqkvT", (384, 384)), ("ww", (128, 257)),
                        ("vecs", (4, 257))):
        out.append((name, off, shape))
        off += int(np.prod(shape))
    return out, off


def nonlocal_grad_record(weights: Dict[str, np.ndarray], block: int = 5) -> Dict[str, np.ndarray]:
    """name -> float32 array of nonlocal_grad_layout's shapes.  ValueError for shapes other than the GSC generator's."""
    from .weights import BN_EPS
    st = "res_stack/%d/non_local/" % block
    k = {}
    for name in ("theta", "phi", "g"):
        k[name] = np.asarray(weights[st + name + "/kernel"], np.float64)
        if k[name].shape != (1, 1, 257, 128):
            raise ValueError("%s%s/kernel must be [1,1,257,128], got %s" % (st, name, k[name].shape))
    ww = np.asarray(weights[st + "w/kernel"], np.float64)
    if ww.shape != (1, 1, 128, 257):
        raise ValueError("%sw/kernel must be [1,1,128,257], got %s" % (st, ww.shape))
    ww = ww[0, 0]
    rstd = 1.0 / np.sqrt(np.asarray(weights[st + "bnorm/moving_variance"], np.float64) + BN_EPS)
    inv = np.asarray(weights[st + "bnorm/gamma"], np.float64) * rstd
    wqkv = np.zeros((NONLOCAL_CP, 384), np.float64)
    wqkv[:257] = np.concatenate([k[n][0, 0] for n in ("theta", "phi", "g")], axis=1)
    wwf = np.zeros((NONLOCAL_CP, 128), np.float64)
    wwf[:257] = (ww * inv[None, :]).T
    wqkvT = np.zeros((384, 384), np.float64)
    wqkvT[:, :NONLOCAL_CP] = wqkv.T
    rec = {"wqkv": wqkv, "bqkv": np.concatenate([np.asarray(weights[st + n + "/bias"], np.float64) for n in ("theta", "phi", "g")]), "wwf": wwf,
           "wqkvT": wqkvT, "ww": ww,
           "vecs": np.stack([np.asarray(weights[st + "w/bias"], np.float64), inv, np.asarray(weights[st + "bnorm/moving_mean"], np.float64), rstd])}
    return {name: np.ascontiguousarray(a, np.float32) for name, a in rec.items()}


def pack_nonlocal_grad(weights: Dict[str, np.ndarray], block: int = 5) -> bytes:
    """The generator's variables (res_stack/<block>/non_local's 12 are read) -> the blob bsr_nonlocal_grad takes (nonlocal_grad_layout).
    ValueError for TSM weights: the chain's skip is 261 wide."""
    if tuple(np.shape(weights["res_stack/%d/conv1/kernel" % block])) != (1, 1, BOTTLENECK_WIDTH, 128):
        raise ValueError(NONLOCAL_TSM_TEXT)
    return _join_record(nonlocal_grad_layout(), nonlocal_grad_record(weights, block))


def unpack_nonlocal_grad(blob: bytes) -> Dict[str, np.ndarray]:
    """The inverse of pack_nonlocal_grad: nonlocal_grad_record's dict."""
    layout, total = nonlocal_grad_layout()
    arr = np.frombuffer(blob, np.float32)
    if arr.size != total:
        raise ValueError("a non-local gradient blob holds %d bytes, got %d" % (total * 4, len(blob)))
    return {name: arr[off:off + int(np.prod(shape))].reshape(shape).copy() for name, off, shape in layout}


# ---- the generator's bottleneck backward (csrc/bottleneck_grad_kernels.h): a blob of its own, no header, float32 ----
BOTTLENECK_TSM_TEXT = "the bottleneck's device chain takes the GSC width only (TSM's 877 is covered by generator_grad.bottleneck_grad)"
BOTTLENECK_BLOCK_TEXT = "block must be 3, 4 or 5 (the colour branch's blocks share their shapes), got %r"
BLOCK_WIDTHS = {0: 99, 1: 257, 2: 257, 3: 261, 4: 261, 5: 261}      # conv1's input width per block of res_stack: the one table
BOTTLENECK_WIDTH, LOWER_TRUNK_WIDTHS = BLOCK_WIDTHS[5], {b: BLOCK_WIDTHS[b] for b in (0, 1, 2)}     # blocks 3..5; the blocks below the hole
LOWER_TRUNK_TEXT = ("the lower trunk's device chain takes the GSC widths only: res_stack/%d/conv1/kernel must be [1,1,%d,128], got %s (TSM's blocks "
                    "0..2 are 291 wide, the RGB baseline's 513)")


def _pad_to(n: int, step: int) -> int:
    return (n + step - 1) // step * step


def bottleneck_grad_layout(width: int = BOTTLENECK_WIDTH):
    """([(name, offset in floats, shape)], floats) of the bottleneck's gradient blob, d = 128, taps in row-major order t = 3 a + b, for a
    block whose input is `width` channels wide (261; 257 and 99 for the blocks below the hole), xp = width rounded up to 16, w1t's
    columns = width rounded up to 128:
      w1f   [xp][128]      the BN-folded FORWARD image of conv1: w1f[c][k] = W1[c][k] inv1[k] (rows width.. zero; [272][128] at 261)
      b1f   [128]          (b1 - mean1) inv1 + beta1
      w2f   [9][128][128]  the folded forward image of conv2: w2f[t][c][o] = K2[a][b][c][o] inv2[o]
      b2f   [128]          (b2 - mean2) inv2 + beta2
      w3t   [272][128]     conv3 for the data gradient: w3t[n][k] = inv3[n] W3[k][n] (rows 257..271 zero)
      w2t   [9][128][128]  conv2 for the data gradient, taps turned by 180 degrees, channel roles swapped:
                           w2t[t][o][c] = inv2[o] K2[2 - a][2 - b][c][o]
      w1t   [128][..]      conv1 for the data gradient: w1t[k][c] = inv1[k] W1[c][k] (columns width.. zero; [128][384] at 261)
      k1    [width][128], k2 [9][128][128], k3 [128][257]   the three kernels in the variables' own order (d gamma is formed from them)
      vecs1 [4][128], vecs2 [4][128], vecs3 [4][257]      per layer: bias, inv, moving_mean, rstd
    inv, rstd and every folded image are formed in float64 and rounded once."""
    out, off = [], 0
    for name, shape in (("w1f", (_pad_to(width, 16), 128)), ("b1f", (128,)), ("w2f", (9, 128, 128)), ("b2f", (128,)), ("w3t", (NONLOCAL_CP, 128)),
                        ("w2t", (9, 128, 128)), ("w1t", (128, _pad_to(width, 128))), ("k1", (width, 128)), ("k2", (9, 128, 128)), ("k3", (128, 257)),
                        ("vecs1", (4, 128)), ("vecs2", (4, 128)), ("vecs3", (4, 257))):
        out.append((name, off, shape))
        off += int(np.prod(shape))
    return out, off


def bottleneck_grad_record(weights: Dict[str, np.ndarray], block: int = 5, width: int = BOTTLENECK_WIDTH) -> Dict[str, np.ndarray]:
    """name -> float32 array of bottleneck_grad_layout's shapes.  ValueError for shapes other than the GSC generator's, and for a block
    outside 3..5 (lower_trunk_bottleneck_record is the blocks below the hole's)."""
    if block not in (3, 4, 5):
        raise ValueError(BOTTLENECK_BLOCK_TEXT % (block,))
    return _bottleneck_record(weights, block, width)


def _bottleneck_record(weights: Dict[str, np.ndarray], block: int, width: int) -> Dict[str, np.ndarray]:
    from .weights import BN_EPS
    st = "res_stack/%d/" % block
    k = {}
    for j, shape in ((1, (1, 1, width, 128)), (2, (3, 3, 128, 128)), (3, (1, 1, 128, 257))):
        k[j] = np.asarray(weights[st + "conv%d/kernel" % j], np.float64)
        if k[j].shape != shape:
            raise ValueError("%sconv%d/kernel must be %s, got %s" % (st, j, list(shape), k[j].shape))
    vec = {}
    for j in (1, 2, 3):
        bias = np.asarray(weights[st + "conv%d/bias" % j], np.float64)
        gamma, beta, mean, var = (np.asarray(weights[st + "bnorm%d/%s" % (j, p)], np.float64)
                                  for p in ("gamma", "beta", "moving_mean", "moving_variance"))
        rstd = 1.0 / np.sqrt(var + BN_EPS)
        vec[j] = (bias, gamma * rstd, mean, rstd, beta)
    inv1, inv2, inv3 = vec[1][1], vec[2][1], vec[3][1]
    w1, w2, w3 = k[1][0, 0], k[2].reshape(9, 128, 128), k[3][0, 0]
    w1f = np.zeros((_pad_to(width, 16), 128), np.float64)
    w1f[:width] = w1 * inv1[None, :]
    w3t = np.zeros((NONLOCAL_CP, 128), np.float64)
    w3t[:257] = (w3 * inv3[None, :]).T
    w1t = np.zeros((128, _pad_to(width, 128)), np.float64)
    w1t[:, :width] = (w1 * inv1[None, :]).T
    w2f = w2 * inv2[None, None, :]
    rec = {"w1f": w1f, "b1f": (vec[1][0] - vec[1][2]) * inv1 + vec[1][4], "w2f": w2f, "b2f": (vec[2][0] - vec[2][2]) * inv2 + vec[2][4],
           "w3t": w3t, "w2t": np.transpose(w2f[::-1], (0, 2, 1)), "w1t": w1t, "k1": w1, "k2": w2, "k3": w3}
    for j in (1, 2, 3):
        rec["vecs%d" % j] = np.stack(vec[j][:4])
    return {name: np.ascontiguousarray(a, np.float32) for name, a in rec.items()}


def pack_bottleneck_grad(weights: Dict[str, np.ndarray], block: int = 5) -> bytes:
    """The generator's variables (res_stack/<block>'s 18 outside non_local are read; block 3, 4 or 5) -> the blob bsr_bottleneck_grad
    takes (bottleneck_grad_layout).  ValueError for TSM weights: the chain's input is 261 wide."""
    if block not in (3, 4, 5):
        raise ValueError(BOTTLENECK_BLOCK_TEXT % (block,))
    if tuple(np.shape(weights["res_stack/%d/conv1/kernel" % block])) != (1, 1, BOTTLENECK_WIDTH, 128):
        raise ValueError(BOTTLENECK_TSM_TEXT)
    return _join_record(bottleneck_grad_layout(), bottleneck_grad_record(weights, block))


def _join_record(layout_total, rec: Dict[str, np.ndarray]) -> bytes:
    layout, total = layout_total
    blob = np.zeros(total, np.float32)
    for name, off, shape in layout:
        assert rec[name].shape == tuple(shape), name
        blob[off:off + rec[name].size] = rec[name].reshape(-1)
    return blob.tobytes()


def unpack_bottleneck_grad(blob: bytes, width: int = BOTTLENECK_WIDTH) -> Dict[str, np.ndarray]:
    """The inverse of pack_bottleneck_grad (and, at a block's `width`, of one bottleneck part of pack_lower_trunk_grad):
    bottleneck_grad_record's dict."""
    layout, total = bottleneck_grad_layout(width)
    arr = np.frombuffer(blob, np.float32)
    if arr.size != total:
        raise ValueError("a bottleneck gradient blob holds %d bytes, got %d" % (total * 4, len(blob)))
    return {name: arr[off:off + int(np.prod(shape))].reshape(shape).copy() for name, off, shape in layout}


# ---- a chain of blocks' backward (csrc/block_chain_grad.h): per block as launched the non-local blob, then the bottleneck's at its width ----
def block_chain_width(weights: Dict[str, np.ndarray], block: int) -> int:
    """BLOCK_WIDTHS[block] if conv1's kernel has it; else ValueError: NONLOCAL_TSM_TEXT for blocks 3..5, LOWER_TRUNK_TEXT below."""
    width = BLOCK_WIDTHS[block]
    shape = tuple(np.shape(weights["res_stack/%d/conv1/kernel" % block]))
    if shape != (1, 1, width, 128):
        raise ValueError(NONLOCAL_TSM_TEXT if block >= 3 else LOWER_TRUNK_TEXT % (block, width, shape))
    return width


def block_chain_parts(blocks):
    """[(kind, block, floats)] of pack_block_chain's parts: ("nl", b), ("bn", b) per block.  Every part is a multiple of four floats."""
    return [(kind, b, nonlocal_grad_layout()[1] if kind == "nl" else bottleneck_grad_layout(BLOCK_WIDTHS[b])[1]) for b in blocks for kind in ("nl", "bn")]


def pack_block_chain(weights: Dict[str, np.ndarray], blocks) -> bytes:
    """The generator's variables (those of `blocks` are read) -> block_chain_parts' blobs end to end.  A block's width check comes first."""
    parts = []
    for b in blocks:
        width = block_chain_width(weights, b)
        parts.append(_join_record(nonlocal_grad_layout(), nonlocal_grad_record(weights, b)))
        parts.append(_join_record(bottleneck_grad_layout(width), _bottleneck_record(weights, b, width)))
    return b"".join(parts)


def unpack_block_chain(blob: bytes, blocks, what: str) -> Dict[str, np.ndarray]:
    """The inverse of pack_block_chain: "nl<b>.<name>" -> nonlocal_grad_record's arrays, "bn<b>.<name>" -> bottleneck_grad_record's."""
    parts = block_chain_parts(blocks)
    total = sum(n for _, _, n in parts)
    if len(blob) != 4 * total:
        raise ValueError("a %s gradient blob holds %d bytes, got %d" % (what, total * 4, len(blob)))
    out, at = {}, 0
    for kind, b, n in parts:
        part = blob[4 * at:4 * (at + n)]
        rec = unpack_nonlocal_grad(part) if kind == "nl" else unpack_bottleneck_grad(part, BLOCK_WIDTHS[b])
        out.update(("%s%d.%s" % (kind, b, name), a) for name, a in rec.items())
        at += n
    return out


def pack_colour_trunk_grad(weights: Dict[str, np.ndarray]) -> bytes:
    """The generator's variables (res_stack/4's and res_stack/3's are read) -> the blob bsr_colour_trunk_grad takes: pack_nonlocal_grad and
    pack_bottleneck_grad of block 4, then of block 3, in the order of the chain's launches.  ValueError (NONLOCAL_TSM_TEXT) for TSM weights."""
    return pack_block_chain(weights, (4, 3))


def lower_trunk_bottleneck_record(weights: Dict[str, np.ndarray], block: int) -> Dict[str, np.ndarray]:
    """bottleneck_grad_record for block 0, 1 or 2 at its own input width.  ValueError (LOWER_TRUNK_TEXT) for TSM and RGB weights."""
    return _bottleneck_record(weights, block, block_chain_width(weights, block))


def lower_trunk_grad_parts():
    """block_chain_parts of pack_lower_trunk_grad's six: ("nl", 2), ("bn", 2), ("nl", 1), ("bn", 1), ("nl", 0), ("bn", 0)."""
    return block_chain_parts((2, 1, 0))


def pack_lower_trunk_grad(weights: Dict[str, np.ndarray]) -> bytes:
    """The generator's variables (res_stack/0's, /1's and /2's are read) -> the blob bsr_lower_trunk_grad takes: per block 2, 1, 0 the
    non-local blob (nonlocal_grad_layout: it does not carry the input's width) and the bottleneck blob at the block's width (257, 257, 99).
    ValueError (LOWER_TRUNK_TEXT) for TSM and RGB weights, whose blocks 0..2 are 291 and 513 wide."""
    return pack_block_chain(weights, (2, 1, 0))


def unpack_lower_trunk_grad(blob: bytes) -> Dict[str, np.ndarray]:
    """The inverse of pack_lower_trunk_grad: unpack_block_chain's dict for b = 0, 1, 2."""
    return unpack_block_chain(blob, (2, 1, 0), "lower trunk")


# ---- the generator's grey heads' backward (csrc/heads_grad_kernels.h): a blob of its own, no header, float32 ----
HEADS_RGB_TEXT = "the heads' device chain takes the GSC / TSM heads (7x7, 64 -> 1 twice); model_RGB.py's are 128 -> 3 and chained"
HEADS_K, HEADS_KP = 98, 100


def heads_grad_layout():
    """([(name, offset in floats, shape)], floats) of the heads' gradient blob: one image,
      kt    [100][64]   the data-gradient image of both heads: kt[2 (7 a + b) + j][c] = K_j[a][b][c][0], j = 0 conv2 (the mask head),
                        j = 1 conv3 (the con head); rows 98, 99 zero.
    The taps are NOT turned: the kernel's operand reads g2 at the pixel p - (a - 3, b - 3), which is the turning.  98 is padded to 100, the
    next multiple of the MFMA's k = 4 (25 k-steps); the kernel feeds zeros against the two pad rows as well."""
    return [("kt", 0, (HEADS_KP, 64))], HEADS_KP * 64


def heads_grad_record(weights: Dict[str, np.ndarray]) -> Dict[str, np.ndarray]:
    """name -> float32 array of heads_grad_layout's shapes.  ValueError for the RGB baseline's weights."""
    k2, k3 = (np.asarray(weights[n + "/conv/kernel"], np.float32) if n + "/conv/kernel" in weights else None for n in ("conv2", "conv3"))
    if k2 is None or k3 is None or k2.shape != (7, 7, 64, 1) or k3.shape != (7, 7, 64, 1):
        raise ValueError(HEADS_RGB_TEXT)
    kt = np.zeros((HEADS_KP, 64), np.float32)
    kt[0:HEADS_K:2] = k2[..., 0].reshape(49, 64)
    kt[1:HEADS_K:2] = k3[..., 0].reshape(49, 64)
    return {"kt": kt}


def pack_heads_grad(weights: Dict[str, np.ndarray]) -> bytes:
    """The generator's variables (conv2's and conv3's kernels are read; GSC or TSM) -> the blob bsr_heads_grad takes (heads_grad_layout).
    ValueError for RGB weights."""
    return heads_grad_record(weights)["kt"].tobytes()


def unpack_heads_grad(blob: bytes) -> Dict[str, np.ndarray]:
    """The inverse of pack_heads_grad: dict(`kt` [100,64], and the two kernels it holds, `conv2/conv/kernel`, `conv3/conv/kernel`
    [7,7,64,1])."""
    _, total = heads_grad_layout()
    arr = np.frombuffer(blob, np.float32)
    if arr.size != total:
        raise ValueError("a heads gradient blob holds %d bytes, got %d" % (total * 4, len(blob)))
    kt = arr.reshape(HEADS_KP, 64).copy()
    return {"kt": kt, "conv2/conv/kernel": kt[0:HEADS_K:2].reshape(7, 7, 64, 1).copy(), "conv3/conv/kernel": kt[1:HEADS_K:2].reshape(7, 7, 64, 1).copy()}


# ---- VGG19 up to block5_conv1 (csrc/vgg_kernels.h): a blob of its own, no header, float32 ----
VGG_NB = 64                  # output channels per workgroup of vgg_conv_kernel
VGG_IN_C = 8                 # the first layer's 3 input channels (BGR) are padded to 8


def vgg_chunk(layer: int) -> int:
    """Input channels per K chunk of vgg_conv_kernel: 8 for the first layer, 16 after it."""
    return 8 if layer == 0 else 16


def vgg_layout():
    """([(name, offset in floats, shape)], floats in all).  Layer `block<b>_conv<i>` is stored as the kernel stages it, a block of 64
    output channels and a chunk of CC input channels at a time: w [N / 64][C_in / CC][9 taps (a * 3 + b)][CC][64], then bias [N]; CC =
    vgg_chunk(layer), the first layer's C_in padded with zeros to 8.  Every offset is a multiple of 4 floats."""
    from .weights import VGG_LAYERS, vgg_variable_shapes
    shapes = vgg_variable_shapes()
    out, off = [], 0
    for i, st in enumerate(VGG_LAYERS):
        _, _, cin, n = shapes[st + "/kernel"]
        cin = VGG_IN_C if i == 0 else cin
        cc = vgg_chunk(i)
        out.append((st + "/w", off, (n // VGG_NB, cin // cc, 9, cc, VGG_NB)))
        off += 9 * cin * n
        out.append((st + "/b", off, (n,)))
        off += n
    return out, off


def vgg_dgrad_layout():
    """([(name, offset in floats, shape)], floats in all) of the gradient layers' blob (csrc/vgg_grad_kernels.h).  The data gradient of
    layer `block<b>_conv<i>` is a 3 x 3 SAME convolution from its C' = C_out to its N' = C_in channels, stored like vgg_layout's w in
    chunks of 16: [N' / 64][C' / 16][9 taps (a * 3 + b)][16][64]; the first layer's N' = 3 is padded with zeros to one 64-block.  No
    bias."""
    from .weights import VGG_LAYERS, vgg_variable_shapes
    shapes = vgg_variable_shapes()
    out, off = [], 0
    for st in VGG_LAYERS:
        _, _, cin, n = shapes[st + "/kernel"]
        npad = -(-cin // VGG_NB) * VGG_NB
        out.append((st + "/dgrad", off, (npad // VGG_NB, n // 16, 9, 16, VGG_NB)))
        off += 9 * n * npad
    return out, off


def pack_vgg_dgrad(weights: Dict[str, np.ndarray]) -> bytes:
    """The VGG19 kernels -> the blob bsr_vgg_per_loss_grad takes beside pack_vgg's (vgg_dgrad_layout): per layer
    k'[a, b, o, c] = k[2 - a, 2 - b, c, o], the taps turned by 180 degrees and the channel roles swapped."""
    from .weights import check_vgg_weights
    check_vgg_weights(weights)
    layout, total = vgg_dgrad_layout()
    blob = np.zeros(total, np.float32)
    for name, off, shape in layout:
        kern = np.asarray(weights[name[:-len("/dgrad")] + "/kernel"], np.float32)
        nblk, nchunk, _, cc, _ = shape
        full = np.zeros((9, kern.shape[3], nblk * VGG_NB), np.float32)
        full[:, :, :kern.shape[2]] = kern[::-1, ::-1].transpose(0, 1, 3, 2).reshape(9, kern.shape[3], kern.shape[2])
        a = full.reshape(9, nchunk, cc, nblk, VGG_NB).transpose(3, 1, 0, 2, 4)
        assert a.shape == tuple(shape)
        blob[off:off + a.size] = a.reshape(-1)
    return blob.tobytes()


def pack_vgg(weights: Dict[str, np.ndarray]) -> bytes:
    """The 26 VGG19 variables (weights.vgg_variable_shapes) -> the blob bsr_vgg_per_loss takes (vgg_layout)."""
    from .weights import check_vgg_weights
    check_vgg_weights(weights)
    layout, total = vgg_layout()
    blob = np.zeros(total, np.float32)
    for name, off, shape in layout:
        st = name[:-2]
        if name.endswith("/b"):
            a = np.asarray(weights[st + "/bias"], np.float32)
        else:
            kern = np.asarray(weights[st + "/kernel"], np.float32)
            nblk, nchunk, _, cc, _ = shape
            full = np.zeros((9, nchunk * cc, kern.shape[3]), np.float32)
            full[:, :kern.shape[2]] = kern.reshape(9, kern.shape[2], kern.shape[3])
            a = full.reshape(9, nchunk, cc, nblk, VGG_NB).transpose(3, 1, 0, 2, 4)
        assert a.shape == tuple(shape)
        blob[off:off + a.size] = a.reshape(-1)
    return blob.tobytes()


def unpack_vgg(blob: bytes) -> Dict[str, np.ndarray]:
    """The inverse of pack_vgg: the 26 variables (the first layer's kernel cut back to its 3 input channels)."""
    from .weights import vgg_variable_shapes
    layout, total = vgg_layout()
    arr = np.frombuffer(blob, np.float32)
    if arr.size != total:
        raise ValueError("a VGG19 blob holds %d bytes, got %d" % (total * 4, len(blob)))
    shapes = vgg_variable_shapes()
    out = {}
    for name, off, shape in layout:
        a = arr[off:off + int(np.prod(shape))].reshape(shape)
        st = name[:-2]
        if name.endswith("/b"):
            out[st + "/bias"] = a.copy()
        else:
            nblk, nchunk, _, cc, _ = shape
            k = a.transpose(2, 1, 3, 0, 4).reshape(3, 3, nchunk * cc, nblk * VGG_NB)
            out[st + "/kernel"] = k[:, :, :shapes[st + "/kernel"][2]].copy()
    return out
