"""The reference's training-shadow synthesis as a host statement: `process_mask` (train_test_GSC.py:81-105) and the utils.py functions
it calls (utils.py:435-900), restated in numpy with the reference's float32 dtype flow and operation order.  It plays the role for
csrc/shadow_synth_kernels.h (bsr_shadow_synth, shadow_synth_gpu.ShadowSynth) that ucb_post.py and wild_paste.py play for theirs.

RANDOMNESS IS AN ARGUMENT.  The reference draws from tf.random inside these functions; here every draw is a field of a `ShadowDraws`
record per item, whether the chosen branch uses it or not.  `draw(rng, S)` fills one from a numpy Generator with the reference's ranges
and types: the DISTRIBUTIONS are the reference's, TensorFlow's random STREAM is not reproduced (no seed gives the reference's images).
Perlin gradients are stored as float32 (cos, sin) pairs per lattice point, computed once on the host.

THE ARITHMETIC (float32 throughout unless said; every product and sum rounded on its own).
  perlin(S, n, grads)       sample positions tf.linspace(0, n, S) stated as i * (n / (S - 1)); t = v - floor(v) (floormod 1);
                            fade = (6 t5 - 15 t4) + 10 t3 with t2 = t t, t3 = t2 t, t4 = t3 t, t5 = t4 t; the meshgrid / transpose of
                            utils.py:809-812 leaves channel 0 = the row's t, channel 1 = the column's t; the four gradient planes are
                            NEAREST resizes (half-pixel centres: floor((i + 0.5) n / S)) of grads[:-1,:-1], [1:,:-1], [:-1,1:], [1:,1:]
                            ([row][column]); dot products c t_row + s t_col; three lerps a (1 - f) + b f, rows first; times sqrt 2.
  perlin_collection         noise = ((0 + 1 P0) + p P1) + (p p) P2 + ...; resolution doubles per octave.
  create_disc_filter(r)     the (2r+1)^2 taps with x^2 + y^2 <= r^2, each 1 / count.
  apply_disc_filter         the reference computes abs(ifft2(fft2(pad(img)) fft2(pad(disc)))) cropped at offset r - 1: a circular
                            convolution of period S + r.  The crop offset is one less than the disc's centre, so the taps land on
                            source pixels (y - 1 + dy, x - 1 + dx); and one wrapped term reaches the first row and the first column
                            (source row / column S - 1).  Stated twice: `apply_disc_filter_fft` is the literal form in float64,
                            `apply_disc_filter` the direct sum over the taps with the same wrap and offset, float64 accumulation,
                            rounded to float32 once.  The kernel implements the direct form.
  apply_spatially_varying_blur   discs of r = b, 2b, 4b; guidance = 1-octave Perlin, minus its min, over its max, / float32(1/3),
                            clipped to [0, 3]; lerp(p1, p2, clip(g - 1)) then lerp(p0, ., clip(g)), lerp(a, b, x) = a + x (b - a).
  gaussian_filter(img, s)   r = ceil(2 s); taps exp(-0.5 (n / s)^2) / sum, n = -r..r (sum taken left to right); REFLECT padding; an x
                            pass then a y pass, each sum taken tap by tap from n = -r upward.
  wavelength_filter         six levels, s = float32(ss_weights[l][0]) * r; red (blur w_r) gain_l, green blur w_g, blue blur w_b, summed
                            level by level; apply_ss_shadow_map = min(1, . / 0.6).
  get_brightness_mask       2-octave Perlin / float32(1 / (min_val + 1e-6)) + min_val, min(., 1).
  process_mask              _mask = mask if u_mask > 0.4 else face * render_perlin_mask; mask_ss = apply_ss_shadow_map(1 - _mask) if
                            u_ss > 0.25 else 1 - _mask on three channels; mask_sv = 1 - mask_ss; intensity with min_val 0.3 if
                            u_bright > 0.5 else 0.5; img = clip(gt mask_ss + (img_dark mask_sv) intensity, 0, 1);
                            mask_edge = |mask_sv - _mask|.

THREE RULES OF OUR OWN.
  1. Where the blurred mask's maximum is not above 0 (a thresholded Perlin map without a lit pixel; a NaN is not counted) the
     reference divides 0 by 0.  Such an item returns status 1 with img = clip(gt, 0, 1), mask_sv = 0 and mask_edge = 0.
  2. gaussian_filter needs ceil(2 * 2.722 * r) <= S - 1, TensorFlow's REFLECT pad limit.  A larger r for the given S raises ValueError
     (`check_scale`), here and in the device binding.  At S = 256 the reference's full range r < 15 fits.

  3. Where the blend guidance of the spatially varying blur is constant (its maximum minus its minimum is not above 0: all its
     gradients zero) the reference divides 0 by 0.  The guidance then counts as 0 everywhere: the finest level, r = blur_size, is used.

WHAT IS NOT PINNED.  TensorFlow's own arithmetic (its exp, its reduction orders inside depthwise_conv2d and reduce_sum, complex64 FFTs)
is not reproduced bit for bit; tests/golden/shadow_synth_*.npz, holds the reference's functions executed over a numpy
stand-in (tools/make_shadow_synth_fixture.py), and tests/test_shadow_synth_fixture.py holds this statement to it.

`python -m blindshadowremoval_amd.shadow_synth SRC DST --seed N [--host] [--batch 16]` turns folders of clean 256 x 256 crops (as
wild_crop writes them: <name>/<name>.png + <name>.npy) into shadowed inputs with known ground truth, readable by Dataset(config, 'test').
"""
from __future__ import annotations

import dataclasses
import os
import sys
from typing import List, Optional, Sequence, Tuple

import numpy as np

f32 = np.float32
SIZES = (32, 64, 128, 256)
MAX_SS_SIGMA, MAX_BLUR_SIGMA, SV_SIGMA = 15, 12, 0.5                 # utils.py:16-18
SS_WEIGHTS = np.array([[0.042, 0.22, 0.437, 0.635], [0.220, 0.101, 0.355, 0.365], [0.433, 0.119, 0.208, 0], [0.753, 0.114, 0, 0],
                       [1.412, 0.364, 0, 0], [2.722, 0.080, 0, 0]])  # utils.py:695-700
SHADOW_CELLS, GUIDE_CELLS, BRIGHT_CELLS = (4, 8, 16, 32), (2,), (2, 4)      # lattice sides are cells + 1: 5 9 17 33 | 3 | 3 5
STATUS_OK, STATUS_EMPTY, STATUS_BAD_DRAWS = 0, 1, 2
STATUS_TEXT = {STATUS_EMPTY: "the blurred mask has no pixel above 0", STATUS_BAD_DRAWS: "a draws record holds an integer out of range"}

# the packed record (32-bit words), as csrc/shadow_synth_kernels.h states it
DRAW_WORDS = 4096
DRAW_U, DRAW_DISC, DRAW_BLUR, DRAW_PERS, DRAW_R, DRAW_GAIN, DRAW_RAD = 0, 4, 5, 6, 9, 10, 16
DRAW_GRAD_SHADOW, DRAW_GRAD_GUIDE, DRAW_GRAD_BRIGHT, DRAW_TAPS, MAX_TAPS = 32, 3000, 3018, 3088, 165


@dataclasses.dataclass
class ShadowDraws:
    """Every draw the reference makes for one item of process_mask."""
    u_mask: float            # process_mask: > 0.4 keeps the given mask, else the Perlin mask
    u_ss: float              # > 0.25: subsurface scattering
    u_bright: float          # > 0.5: min_val 0.3, else 0.5
    u_sv: float              # render_shadow_from_mask: > 0.5 spatially varying blur, else one disc
    disc_sz: int             # 1..11
    blur_size: int           # 1..2
    p_shadow: float          # persistences: [0.05, 0.85), [0.05, 0.25), [0.05, 0.25)
    p_guide: float
    p_bright: float
    r: float                 # SS scale, [1, 15)
    gains: np.ndarray        # float32 [6], [1.1, 1.5)
    g_shadow: List[np.ndarray]      # float32 [n+1, n+1, 2] (cos, sin) for n = 4, 8, 16, 32
    g_guide: List[np.ndarray]       # n = 2
    g_bright: List[np.ndarray]      # n = 2, 4


def _grads(rng: np.random.Generator, n: int) -> np.ndarray:
    a = f32(2.0 * np.pi) * rng.random((n + 1, n + 1), dtype=f32)
    return np.stack([np.cos(a), np.sin(a)], axis=2).astype(f32)


def draw(rng: np.random.Generator, S: int = 256) -> ShadowDraws:
    """One record with the reference's ranges and types (uniform float32 in [lo, hi), int32 in [lo, hi)).  The distributions match the
    reference; TensorFlow's stream does not.  r is drawn from [1, 15), cut to what rule 2 admits where S < 256."""
    def u(lo=0.0, hi=1.0):
        return f32(f32(lo) + rng.random(dtype=f32) * f32(hi - lo))
    r = u(1.0, min(float(MAX_SS_SIGMA), max_scale(S)))
    while int(np.ceil(f32(2.0) * level_sigma(5, r))) > S - 1 or not r < f32(MAX_SS_SIGMA):      # float32 rounding at the upper end
        r = np.nextafter(r, f32(0))
    return ShadowDraws(u_mask=u(), u_ss=u(), u_bright=u(), u_sv=u(), disc_sz=np.int32(rng.integers(1, MAX_BLUR_SIGMA)),
                       blur_size=np.int32(rng.integers(1, 3)), p_shadow=u(0.05, 0.85), p_guide=u(0.05, 0.25), p_bright=u(0.05, 0.25), r=r,
                       gains=np.array([u(1.1, 1.5) for _ in range(6)], f32), g_shadow=[_grads(rng, n) for n in SHADOW_CELLS],
                       g_guide=[_grads(rng, n) for n in GUIDE_CELLS], g_bright=[_grads(rng, n) for n in BRIGHT_CELLS])


# ---- Perlin
def _axis(S: int, n: int):
    step = f32(n) / f32(S - 1)
    v = (np.arange(S, dtype=f32) * step).astype(f32)
    t = (v - np.floor(v)).astype(f32)
    t2 = t * t; t3 = t2 * t; t4 = t3 * t; t5 = t4 * t
    fade = (f32(6.0) * t5 - f32(15.0) * t4) + f32(10.0) * t3
    cell = np.minimum(np.floor((np.arange(S, dtype=f32) + f32(0.5)) * (f32(n) / f32(S))).astype(np.int64), n - 1)
    return t, fade.astype(f32), cell


def perlin(S: int, n: int, grads: np.ndarray) -> np.ndarray:
    grads = np.asarray(grads, f32)
    if grads.shape != (n + 1, n + 1, 2):
        raise ValueError("perlin: a lattice of %d cells needs gradients [%d,%d,2], got %s" % (n, n + 1, n + 1, grads.shape))
    t, fade, cell = _axis(S, n)
    ty, tx, fy, fx = t[:, None], t[None, :], fade[:, None], fade[None, :]
    g00, g10 = grads[cell][:, cell], grads[cell + 1][:, cell]
    g01, g11 = grads[cell][:, cell + 1], grads[cell + 1][:, cell + 1]
    one = f32(1.0)
    d1 = g00[..., 0] * ty + g00[..., 1] * tx
    d2 = g10[..., 0] * (ty - one) + g10[..., 1] * tx
    d3 = g01[..., 0] * ty + g01[..., 1] * (tx - one)
    d4 = g11[..., 0] * (ty - one) + g11[..., 1] * (tx - one)
    i1 = d1 * (one - fy) + d2 * fy
    i2 = d3 * (one - fy) + d4 * fy
    i3 = i1 * (one - fx) + i2 * fx
    out = np.sqrt(f32(2.0)) * i3
    assert out.dtype == f32
    return out


def perlin_collection(S: int, n0: int, octaves: int, persistence, grads: Sequence[np.ndarray]) -> np.ndarray:
    noise, amp, n = np.zeros((S, S), f32), f32(1.0), n0
    for o in range(octaves):
        noise = noise + amp * perlin(S, n, grads[o])
        amp = f32(amp * f32(persistence))
        n *= 2
    return noise


# ---- disc blur
def create_disc_filter(r: int) -> np.ndarray:
    x, y = np.meshgrid(np.arange(-r, r + 1), np.arange(-r, r + 1))
    m = (x * x + y * y <= r * r).astype(f32)
    return (m / m.sum(dtype=f32)).astype(f32)


def apply_disc_filter_fft(img: np.ndarray, r: int) -> np.ndarray:
    """The reference's form, literally, in float64: [S,S] -> float64 [S,S]."""
    img = np.asarray(img, np.float64)
    S, r = img.shape[0], int(r)
    disc = create_disc_filter(r).astype(np.float64)
    pad = np.pad(img, ((0, r), (0, r)))
    dpad = np.pad(disc, ((0, pad.shape[0] - disc.shape[0]), (0, pad.shape[1] - disc.shape[1])))
    out = np.abs(np.fft.ifft2(np.fft.fft2(pad) * np.fft.fft2(dpad)))
    return out[r - 1:r - 1 + S, r - 1:r - 1 + S]


def apply_disc_filter_direct(img: np.ndarray, r: int) -> np.ndarray:
    """The same as a direct sum over the disc's taps with the period-(S + r) wrap and the r - 1 offset: float64 [S,S]."""
    img = np.asarray(img, np.float64)
    S, r = img.shape[0], int(r)
    P = S + r
    disc = create_disc_filter(r).astype(np.float64)
    pad = np.zeros((P, P))
    pad[:S, :S] = img
    acc = np.zeros((S, S))
    i = np.arange(S) + r - 1
    for dy in range(2 * r + 1):
        rows = (i - dy) % P
        for dx in range(2 * r + 1):
            if disc[dy, dx] != 0:
                acc += disc[dy, dx] * pad[np.ix_(rows, (i - dx) % P)]
    return acc


def apply_disc_filter(img: np.ndarray, r: int) -> np.ndarray:
    return apply_disc_filter_direct(img, r).astype(f32)


def blend_guidance(S: int, d: ShadowDraws) -> np.ndarray:
    g = perlin_collection(S, 2, 1, d.p_guide, d.g_guide)
    g = g - g.min()
    span = g.max()
    if not span > 0:                       # rule 3: a constant guidance (the reference divides 0 by 0) selects the finest level everywhere
        return np.zeros((S, S), f32)
    g = g / span
    return np.clip(g / f32(1.0 / 3), f32(0.0), f32(3.0)).astype(f32)


def apply_spatially_varying_blur(img: np.ndarray, blur_size: int, d: ShadowDraws) -> np.ndarray:
    S = img.shape[0]
    p = [apply_disc_filter(img, (2 ** i) * int(blur_size)) for i in range(3)]
    gb = blend_guidance(S, d)
    zero, one = f32(0.0), f32(1.0)
    with np.errstate(invalid="ignore"):
        r1 = p[1] + np.clip(gb - one, zero, one) * (p[2] - p[1])
        return (p[0] + np.clip(gb - zero, zero, one) * (r1 - p[0])).astype(f32)


# ---- Gaussians
def gaussian_taps(sigma) -> np.ndarray:
    sigma = f32(sigma)
    r = int(np.ceil(f32(2.0) * sigma))
    n = np.arange(-r, r + 1, dtype=f32)
    q = n / sigma
    c = np.exp(f32(-0.5) * (q * q)).astype(f32)
    return (c / np.cumsum(c, dtype=f32)[-1]).astype(f32)


def _reflect(i: np.ndarray, S: int) -> np.ndarray:
    i = np.where(i < 0, -i, i)
    return np.where(i >= S, 2 * (S - 1) - i, i)


def gaussian_filter(img: np.ndarray, sigma) -> np.ndarray:
    """[S,S] float32, REFLECT padding, x pass then y pass; ValueError where TensorFlow's pad would refuse (radius > S - 1)."""
    img = np.asarray(img, f32)
    S = img.shape[0]
    taps = gaussian_taps(sigma)
    r = (len(taps) - 1) // 2
    if r > S - 1:
        raise ValueError("gaussian_filter: radius %d exceeds the REFLECT pad limit S - 1 = %d" % (r, S - 1))
    idx = np.arange(S)
    out = img
    for axis in (1, 0):
        acc = np.zeros((S, S), f32)
        for k in range(2 * r + 1):
            acc = acc + taps[k] * np.take(out, _reflect(idx - r + k, S), axis=axis)
        out = acc
    return out


def level_sigma(lv: int, r) -> np.float32:
    return f32(f32(SS_WEIGHTS[lv, 0]) * f32(r))


def max_scale(S: int) -> float:
    """The supremum of the r that rule 2 admits at S (an r strictly below it always fits)."""
    return (S - 1) / (2.0 * 2.722)


def check_scale(r, S: int) -> None:
    rad = int(np.ceil(f32(2.0) * level_sigma(5, r)))
    if rad > S - 1:
        raise ValueError("shadow_synth: r = %g needs a Gaussian radius of %d, over the REFLECT pad limit S - 1 = %d" % (float(r), rad, S - 1))


def wavelength_filter(img: np.ndarray, r, gains) -> np.ndarray:
    acc = None
    for lv in range(6):
        blur = gaussian_filter(img, level_sigma(lv, r))
        lvl = np.stack([(blur * f32(SS_WEIGHTS[lv, 1])) * f32(gains[lv]), blur * f32(SS_WEIGHTS[lv, 2]), blur * f32(SS_WEIGHTS[lv, 3])], axis=2)
        acc = (np.zeros_like(lvl) + lvl) if acc is None else acc + lvl
    return acc


def apply_ss_shadow_map(img: np.ndarray, r, gains) -> np.ndarray:
    return np.minimum(f32(1.0), wavelength_filter(img, r, gains) / f32(0.6)).astype(f32)


def get_brightness_mask(S: int, min_val: float, d: ShadowDraws) -> np.ndarray:
    m = perlin_collection(S, 2, 2, d.p_bright, d.g_bright)
    return np.minimum(m / f32(1.0 / (min_val + 1e-6)) + f32(min_val), f32(1.0)).astype(f32)


def render_shadow_from_mask(mask: np.ndarray, d: ShadowDraws) -> Tuple[Optional[np.ndarray], int]:
    """[S,S] -> (the blurred mask over its max, 0) or (None, 1) under rule 1."""
    blurred = apply_spatially_varying_blur(mask, d.blur_size, d) if f32(d.u_sv) > f32(SV_SIGMA) else apply_disc_filter(mask, d.disc_sz)
    mx = np.fmax.reduce(blurred.reshape(-1))
    if not mx > 0:
        return None, STATUS_EMPTY
    return (blurred / mx).astype(f32), STATUS_OK


def render_perlin_mask(S: int, d: ShadowDraws):
    """-> (shadow mask or None, status, the Perlin map, its threshold)."""
    pmap = perlin_collection(S, 4, 4, d.p_shadow, d.g_shadow)
    thre = (pmap > f32(0.15)).astype(f32)
    m, st = render_shadow_from_mask(thre, d)
    return m, st, pmap, thre


def process_item(mask, gt, img_dark, face, d: ShadowDraws) -> dict:
    """One item: mask, face [S,S,1], gt, img_dark [S,S,3] -> dict(img, mask_sv, mask_edge [S,S,3], status, perlin_map, thre, bright, mask)."""
    mask, gt, img_dark, face = (np.asarray(a, f32) for a in (mask, gt, img_dark, face))
    S = gt.shape[0]
    if S not in SIZES or gt.shape != (S, S, 3) or img_dark.shape != (S, S, 3) or mask.shape != (S, S, 1) or face.shape != (S, S, 1):
        raise ValueError("process_mask takes mask, face [S,S,1] and gt, img_dark [S,S,3] with S in %s, got %s %s %s %s"
                         % (SIZES, mask.shape, gt.shape, img_dark.shape, face.shape))
    check_scale(d.r, S)
    one = f32(1.0)
    bright = get_brightness_mask(S, 0.3 if f32(d.u_bright) > f32(0.5) else 0.5, d)
    res = {"status": STATUS_OK, "perlin_map": np.zeros((S, S), f32), "thre": np.zeros((S, S), f32), "bright": bright}
    if f32(d.u_mask) > f32(0.4):
        m = mask
    else:
        pm, st, res["perlin_map"], res["thre"] = render_perlin_mask(S, d)
        if st != STATUS_OK:
            res.update(status=st, img=np.clip(gt, 0, 1), mask_sv=np.zeros((S, S, 3), f32), mask_edge=np.zeros((S, S, 3), f32),
                       mask=np.zeros((S, S, 1), f32))
            return res
        m = face * pm[:, :, None]
    if f32(d.u_ss) > f32(0.25):
        mask_ss = apply_ss_shadow_map((one - m)[:, :, 0], d.r, d.gains)
    else:
        mask_ss = np.repeat(one - m, 3, axis=2)
    mask_sv = one - mask_ss
    img = gt * mask_ss + (img_dark * mask_sv) * bright[:, :, None]
    res.update(img=np.clip(img, f32(0), one), mask_sv=mask_sv, mask_edge=np.abs(mask_sv - m), mask=m)
    assert res["img"].dtype == f32 and mask_sv.dtype == f32
    return res


def process_mask(mask, gt, img_dark, face, draws: Sequence[ShadowDraws]):
    """Batches [B,S,S,C] + B records -> (img, mask_sv, mask_edge [B,S,S,3] float32, status [B] int32)."""
    if not (len(mask) == len(gt) == len(img_dark) == len(face) == len(draws)):
        raise ValueError("process_mask: the four batches and the draws differ in length")
    items = [process_item(mask[i], gt[i], img_dark[i], face[i], draws[i]) for i in range(len(draws))]
    return (np.stack([it["img"] for it in items]), np.stack([it["mask_sv"] for it in items]), np.stack([it["mask_edge"] for it in items]),
            np.array([it["status"] for it in items], np.int32))


def pack_draws(draws: Sequence[ShadowDraws], S: int) -> np.ndarray:
    """The records bsr_shadow_synth reads: uint32 [B, DRAW_WORDS].  The Gaussian taps are computed here (the device calls no exp)."""
    out = np.zeros((len(draws), DRAW_WORDS), np.uint32)
    fl = out.view(f32)
    it = out.view(np.int32)
    for b, d in enumerate(draws):
        check_scale(d.r, S)
        if not (1 <= int(d.disc_sz) < MAX_BLUR_SIGMA and 1 <= int(d.blur_size) <= 2):
            raise ValueError("shadow_synth: disc_sz is 1..11 and blur_size 1..2, got %d and %d" % (d.disc_sz, d.blur_size))
        fl[b, DRAW_U:DRAW_U + 4] = [d.u_mask, d.u_ss, d.u_bright, d.u_sv]
        it[b, DRAW_DISC], it[b, DRAW_BLUR] = int(d.disc_sz), int(d.blur_size)
        fl[b, DRAW_PERS:DRAW_PERS + 3] = [d.p_shadow, d.p_guide, d.p_bright]
        fl[b, DRAW_R] = d.r
        fl[b, DRAW_GAIN:DRAW_GAIN + 6] = np.asarray(d.gains, f32)
        for off, cells, gs in ((DRAW_GRAD_SHADOW, SHADOW_CELLS, d.g_shadow), (DRAW_GRAD_GUIDE, GUIDE_CELLS, d.g_guide), (DRAW_GRAD_BRIGHT, BRIGHT_CELLS, d.g_bright)):
            for n, g in zip(cells, gs):
                g = np.asarray(g, f32)
                if g.shape != (n + 1, n + 1, 2):
                    raise ValueError("shadow_synth: a lattice of %d cells needs gradients [%d,%d,2], got %s" % (n, n + 1, n + 1, g.shape))
                fl[b, off:off + g.size] = g.reshape(-1)
                off += g.size
        for lv in range(6):
            taps = gaussian_taps(level_sigma(lv, d.r))
            it[b, DRAW_RAD + lv] = (len(taps) - 1) // 2
            fl[b, DRAW_TAPS + lv * MAX_TAPS:DRAW_TAPS + lv * MAX_TAPS + len(taps)] = taps
    return out


def unpack_draws(words: np.ndarray) -> ShadowDraws:
    """The inverse of pack_draws for one record of DRAW_WORDS words (the radii and taps follow from r and are not read)."""
    words = np.ascontiguousarray(words, np.uint32).reshape(DRAW_WORDS)
    fl, it = words.view(f32), words.view(np.int32)

    def lattices(off, cells):
        out = []
        for n in cells:
            size = (n + 1) * (n + 1) * 2
            out.append(fl[off:off + size].reshape(n + 1, n + 1, 2).copy())
            off += size
        return out
    return ShadowDraws(u_mask=fl[DRAW_U], u_ss=fl[DRAW_U + 1], u_bright=fl[DRAW_U + 2], u_sv=fl[DRAW_U + 3], disc_sz=np.int32(it[DRAW_DISC]),
                       blur_size=np.int32(it[DRAW_BLUR]), p_shadow=fl[DRAW_PERS], p_guide=fl[DRAW_PERS + 1], p_bright=fl[DRAW_PERS + 2], r=fl[DRAW_R],
                       gains=fl[DRAW_GAIN:DRAW_GAIN + 6].copy(), g_shadow=lattices(DRAW_GRAD_SHADOW, SHADOW_CELLS),
                       g_guide=lattices(DRAW_GRAD_GUIDE, GUIDE_CELLS), g_bright=lattices(DRAW_GRAD_BRIGHT, BRIGHT_CELLS))


def example_inputs(S: int, B: int, seed: int = 0):
    """mask, gt, img_dark, face for B items of side S from a seed: values in [0, 1], a disc-shaped face region, a given mask under it.
    What the tests, the fixture tool and the bench tool feed process_mask with."""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.linspace(-1, 1, S), np.linspace(-1, 1, S), indexing="ij")
    face = np.clip(1.5 - 1.6 * np.sqrt(yy * yy + xx * xx), 0, 1).astype(f32)[None, :, :, None].repeat(B, 0)
    mask = rng.random((B, S, S, 1), dtype=f32) * face
    return mask, rng.random((B, S, S, 3), dtype=f32), rng.random((B, S, S, 3), dtype=f32), np.ascontiguousarray(face)


# ---- face_darken (utils.py:1029-1047), with explicit gains; it stays on the host
def _getbias(x, bias):
    return x / ((1.0 / bias - 2.0) * (1.0 - x) + 1.0 + 1e-6)


def apply_tone_curve_rgb(image: np.ndarray, gain) -> np.ndarray:
    image = np.asarray(image)
    image_max = np.max(image)
    image = (image / (image_max + 1e-6)).astype(f32)
    ch = []
    for c in range(3):
        v = image[..., c]
        m = (v > 0.499).astype(f32)
        ch.append(_getbias(v * 2.0, gain[c]) / 2.0 * (1.0 - m) + (_getbias(v * 2.0 - 1.0, 1.0 - gain[c]) / 2.0 + 0.5) * m)
    return np.stack(ch, axis=2) * image_max


def colour_matrix(image: np.ndarray, target: np.ndarray) -> np.ndarray:
    """get_ctm_ls: the 3 x 3 matrix minimising |C image - target|."""
    return np.linalg.lstsq(image.reshape(-1, 3), target.reshape(-1, 3), rcond=None)[0].T


def apply_ctm(image: np.ndarray, ctm: np.ndarray) -> np.ndarray:
    return np.tensordot(image.reshape(-1, 3), ctm, axes=[[-1], [-1]]).reshape(image.shape)


def face_darken(img: np.ndarray, gain_aug, gain_tone):
    """float image [S,S,3] + the two tone-curve gains (the reference draws each as 0.5 + U(-0.3, 0.3)^3) -> (img_aug, img_tone, the
    second colour matrix)."""
    img = np.asarray(img).astype(f32)
    img_aug = apply_ctm(img, colour_matrix(img, apply_tone_curve_rgb(img, gain_aug)))
    cm = colour_matrix(img, apply_tone_curve_rgb(img, gain_tone))
    return img_aug, apply_ctm(img, cm), cm


TONE_SIGMA = 0.3


# ---- the command-line entry
def synthesise_folder(src: str, dst: str, seed: int, host: bool = False, batch: int = 16, device: int = 0) -> List[str]:
    """Every `<src>/<name>/<name>.png` (a 256 x 256 crop) with its `<name>.npy` (68 landmarks in the crop's pixels) -> `<dst>/<name>/` with the
    shadowed crop under the input's name, the landmarks, `<name>-gt.png` and `<name>-mask.png`; -> the names written.  The Perlin
    branch is forced (the reference's silhouette PNGs are not shipped); an item whose status is not 0 is skipped and reported."""
    from .dataset import generate_face_region
    from .pngio import read_rgb_u8, write_png
    rng = np.random.default_rng(seed)
    names = sorted(n for n in os.listdir(src) if os.path.isfile(os.path.join(src, n, n + ".png")) and os.path.isfile(os.path.join(src, n, n + ".npy")))
    done: List[str] = []
    runner = None
    for lo in range(0, len(names), max(1, batch)):
        group = names[lo:lo + max(1, batch)]
        gts, darks, faces, lms, draws = [], [], [], [], []
        for n in group:
            crop = read_rgb_u8(os.path.join(src, n, n + ".png"))
            S = crop.shape[0]
            if crop.shape != (S, S, 3) or S not in SIZES:
                raise ValueError("shadow_synth: %s is %s, not a square crop of side %s" % (n, crop.shape, SIZES))
            lm = np.load(os.path.join(src, n, n + ".npy"))
            gt = crop.astype(f32) / f32(255)
            g1 = 0.5 + rng.uniform(-TONE_SIGMA, TONE_SIGMA, 3)
            g2 = 0.5 + rng.uniform(-TONE_SIGMA, TONE_SIGMA, 3)
            img_aug, img_dark, _ = face_darken(gt, g1, g2)
            d = draw(rng, S)
            d.u_mask = f32(0.0)                                       # the Perlin branch
            gts.append(img_aug.astype(f32)); darks.append(img_dark.astype(f32)); faces.append(generate_face_region(np.asarray(lm, np.float64) / S, S)); lms.append(lm); draws.append(d)
        gt_b, dark_b, face_b = np.stack(gts), np.stack(darks), np.stack(faces)
        mask_b = np.zeros_like(face_b)
        if host:
            img, mask_sv, _, status = process_mask(mask_b, gt_b, dark_b, face_b, draws)
        else:
            import torch
            from .shadow_synth_gpu import ShadowSynth
            runner = runner or ShadowSynth(device)
            dev = torch.device("cuda", device)
            res = runner.process_mask(*(torch.from_numpy(a).to(dev) for a in (mask_b, gt_b, dark_b, face_b)), draws)
            img, mask_sv, _, status = (t.cpu().numpy() for t in res)
        for i, n in enumerate(group):
            if status[i] != STATUS_OK:
                sys.stderr.write("shadow_synth: %s skipped: %s\n" % (n, STATUS_TEXT.get(int(status[i]), "status %d" % status[i])))
                continue
            to_u8 = lambda a: np.rint(np.clip(a, 0, 1) * f32(255)).astype(np.uint8)
            write_png(os.path.join(dst, n, n + ".png"), to_u8(img[i]))
            write_png(os.path.join(dst, n, n + "-gt.png"), to_u8(gt_b[i]))
            write_png(os.path.join(dst, n, n + "-mask.png"), to_u8(mask_sv[i]))
            np.save(os.path.join(dst, n, n + ".npy"), lms[i])
            done.append(n)
    return done


def main(argv=None) -> int:
    import argparse
    ap = argparse.ArgumentParser(prog="python -m blindshadowremoval_amd.shadow_synth", description="Synthesise training shadows on clean crops.")
    ap.add_argument("src")
    ap.add_argument("dst")
    ap.add_argument("--seed", type=int, required=True)
    ap.add_argument("--host", action="store_true", help="use the host statement instead of the device chain")
    ap.add_argument("--batch", type=int, default=16)
    a = ap.parse_args(argv)
    for name in synthesise_folder(a.src, a.dst, a.seed, host=a.host, batch=a.batch):
        print(os.path.join(a.dst, name))
    return 0


if __name__ == "__main__":
    sys.exit(main())
