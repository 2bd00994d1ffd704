"""Cropping in-the-wild photographs to the network's input — the reference's "Preprocessing New Images" procedure
(/root/reference/dataprocess.py:25-77) restated in numpy: no OpenCV, no file I/O in the core.

    python -m blindshadowremoval_amd.wild_crop 'sample_uncropped_images/*.png' sample_uncropped_images_cropped

`crop_face(img, lm)` takes an uncropped RGB photograph and its 68 landmarks (the `.npy` the landmark detector of
bmvc2022-dataprocess.py writes beside the `.png`) and returns what the script writes for it: the 256 x 256 face, the landmarks in
the crop's coordinates, the box.  `preprocess_folder` is the script itself: one `<dst>/<name>/<name>.png` + `.npy` per photograph
that passes its size rule, the folder layout `Dataset(config, 'test')` reads.

WHAT IS PINNED TO WHAT.  The wiring — box, skip rule, padding, landmark shift and scale — is pinned to the reference's own text
(tools/make_wild_crop_fixture.py executes dataprocess.py over stand-ins; tests/golden/wild_crop.npz).  The two `cv2.resize` calls
and `cv2.imwrite`'s conversion are OUR restatement of OpenCV's arithmetic, written down below and pinned to itself (host statement
against device kernel, csrc/wild_crop_kernels.h, byte for byte), not to OpenCV: the same standing as the rest of the loaders.

dtype flow (numpy 1.x scalar rules, the reference's environment, as dataset.face_crop_and_resize): the landmarks are float32; the box
centre is float32 arithmetic; the half-length becomes float64 by its `* 1.45`.

cv2.resize(face, (S, S)), INTER_LINEAR (modules/imgproc/src/resize.cpp).  Per axis of n source pixels, for output index o:

    scale = 1 / (S / n)                          (double)
    f  = float32((o + 0.5) * scale - 0.5)        (double arithmetic, then one rounding to float32)
    s  = floor(f);  f = f - s                    (float32)
    x axis:  s < 0      -> f = 0, s = 0;   s >= n - 1 -> f = 0, s = n - 1;   taps s and min(s + 1, n - 1)
    y axis:  taps clip(s, 0, n - 1) and clip(s + 1, 0, n - 1), f unchanged
    weights  w0 = float32(1) - f,  w1 = f        (float32)

  8-bit image (`resize_u8`, the in-bounds branch: the crop stays uint8):
    a0, a1, b0, b1 = rint(w * 2048) as integers (11 fractional bits; rint = round half to even, cvRound)
    D[y][o]  = S[y][x0] * a0 + S[y][x1] * a1                                  (int, horizontal pass)
    out[o']  = uint8((((b0 * (D[y0] >> 4)) >> 16) + ((b1 * (D[y1] >> 4)) >> 16) + 2) >> 2)      (vertical pass: the low byte)
  This differs from the float64 bilinear value rounded half-even by at most one grey level (tests/test_wild_crop.py).

  float64 image (`resize_f64`, the padded branch: the reference pastes the photograph into np.zeros(...), a float64 canvas):
    D[y][o]  = S[y][x0] * double(w0) + S[y][x1] * double(w1)                  (double, no fused multiply-add)
    out      = D[y0] * double(v0) + D[y1] * double(v1)
  and cv2.imwrite converts the float64 image to bytes by cvRound (half to even) with saturation (`to_u8`).

(OpenCV switches INTER_LINEAR to INTER_AREA when both scales are exactly 2; for these two arithmetics the 2 x 2 mean it then takes is
the same number — the weights are all one half — so no case is made of it.)
"""
from __future__ import annotations

import glob
import os
import sys
from typing import List, Optional, Tuple

import numpy as np

OUT_SIZE = 256            # dataprocess.py:72
MIN_LENGTH = 250          # dataprocess.py:66: `if length > 250`


def _axis(n: int, size: int, is_x: bool):
    """(tap 0, tap 1, f float32) of OpenCV's INTER_LINEAR along an axis of n source pixels resized to `size` (module docstring)."""
    scale = 1.0 / (float(size) / float(n))
    f = ((np.arange(size, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f)
    f = (f - s).astype(np.float32)
    s = s.astype(np.int64)
    if is_x:
        lo, hi = s < 0, s >= n - 1
        f = np.where(lo | hi, np.float32(0), f).astype(np.float32)
        s = np.where(lo, 0, np.where(hi, n - 1, s))
        return s, np.minimum(s + 1, n - 1), f
    return np.clip(s, 0, n - 1), np.clip(s + 1, 0, n - 1), f


def resize_u8(img: np.ndarray, size: int = OUT_SIZE) -> np.ndarray:
    """cv2.resize(img, (size, size)) of a uint8 [h,w,C] image: OpenCV's 8-bit INTER_LINEAR in fixed point (module docstring)."""
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[0] < 1 or img.shape[1] < 1:
        raise ValueError("resize_u8 takes a non-empty uint8 [h,w,C] image, got %s %s" % (img.dtype, img.shape))
    y0, y1, fy = _axis(img.shape[0], size, False)
    x0, x1, fx = _axis(img.shape[1], size, True)
    k = np.float32(2048)
    a0, a1 = np.rint((np.float32(1) - fx) * k).astype(np.int32), np.rint(fx * k).astype(np.int32)
    b0, b1 = np.rint((np.float32(1) - fy) * k).astype(np.int32), np.rint(fy * k).astype(np.int32)
    rows = img.astype(np.int32)
    d = rows[:, x0] * a0[None, :, None] + rows[:, x1] * a1[None, :, None]
    out = (((b0[:, None, None] * (d[y0] >> 4)) >> 16) + ((b1[:, None, None] * (d[y1] >> 4)) >> 16) + 2) >> 2
    return (out & 255).astype(np.uint8)


def resize_f64(img: np.ndarray, size: int = OUT_SIZE) -> np.ndarray:
    """cv2.resize(img, (size, size)) of a float64 [h,w,C] image: the floating INTER_LINEAR with float32 coefficients (module docstring)."""
    img = np.asarray(img)
    if img.dtype != np.float64 or img.ndim != 3 or img.shape[0] < 1 or img.shape[1] < 1:
        raise ValueError("resize_f64 takes a non-empty float64 [h,w,C] image, got %s %s" % (img.dtype, img.shape))
    y0, y1, fy = _axis(img.shape[0], size, False)
    x0, x1, fx = _axis(img.shape[1], size, True)
    a0, a1 = (np.float32(1) - fx).astype(np.float64)[None, :, None], fx.astype(np.float64)[None, :, None]
    b0, b1 = (np.float32(1) - fy).astype(np.float64)[:, None, None], fy.astype(np.float64)[:, None, None]
    d = img[:, x0] * a0 + img[:, x1] * a1
    return d[y0] * b0 + d[y1] * b1


def to_u8(a: np.ndarray) -> np.ndarray:
    """What cv2.imwrite stores of a float64 image: cvRound (half to even), saturated to a byte."""
    return np.clip(np.rint(np.asarray(a, np.float64)), 0, 255).astype(np.uint8)


def box_length(lm: np.ndarray) -> float:
    """dataprocess.py:38: the half-length of the box, the number the skip rule (:66) looks at."""
    lm = np.asarray(lm, np.float32)
    two = np.float32(2)
    return float(max((lm[:, 0].max() - lm[:, 0].min()) / two, (lm[:, 1].max() - lm[:, 1].min()) / two)) * 1.45


def crop_geometry(lm0: np.ndarray, h: int, w: int):
    """Everything dataprocess.py derives from the landmarks and the photograph's size alone (:37-62, :75), or None where it writes
    nothing (:66): -> (box in canvas coordinates [x0, y0, x1, y1], preset_x, preset_y, lm256 float32 [68,2]).  Both presets 0: the box
    lies in the photograph; otherwise in the zero canvas of (h + 2 preset_y + 2) x (w + 2 preset_x + 2) pixels that holds the
    photograph at (preset_y, preset_x)."""
    pred = np.array(lm0, np.float32)
    two = np.float32(2)
    center = [(pred[:, 0].min() + pred[:, 0].max()) / two, (pred[:, 1].min() + pred[:, 1].max()) / two]
    length = box_length(pred)
    box = [int(center[0]) - int(length),
           int(center[1]) - int(length * 1.2),
           int(center[0]) + int(length),
           int(center[1]) + int(length) + int(length) - int(length * 1.2)]
    pred[:, 0] = pred[:, 0] - np.float32(box[0])
    pred[:, 1] = pred[:, 1] - np.float32(box[1])
    preset_x = preset_y = 0
    if box[0] < 0 or box[2] > w:
        preset_x = max(-box[0], box[2] - w)
    if box[1] < 0 or box[3] > h:
        preset_y = max(-box[1], box[3] - h)
    if preset_x > 0 or preset_y > 0:
        box = [box[0] + preset_x, box[1] + preset_y, box[2] + preset_x, box[3] + preset_y]
    if not length > MIN_LENGTH:
        return None
    side = box[3] - box[1]                                 # face.shape[0]: the box lies inside what it is cut from
    lm256 = pred / np.float32(side) * np.float32(OUT_SIZE)
    return box, int(preset_x), int(preset_y), lm256.astype(np.float32)


def crop_face(img: np.ndarray, lm: np.ndarray, size: int = OUT_SIZE) -> Optional[Tuple[np.ndarray, np.ndarray, List[int]]]:
    """dataprocess.py:25-77 for one photograph: uint8 [h,w,3] + landmarks [68,2] -> (face uint8 [256,256,3], lm256 float32 [68,2], box)
    or None where the script skips the photograph (`length > 250` fails).  `box` is the script's final one — shifted by the presets
    when the photograph had to be padded.  `size` other than 256 only changes the resize target (tests)."""
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
        raise ValueError("crop_face takes a uint8 [h,w,3] photograph, got %s %s" % (img.dtype, img.shape))
    h, w = img.shape[:2]
    geo = crop_geometry(lm, h, w)
    if geo is None:
        return None
    box, preset_x, preset_y, lm256 = geo
    return crop_pixels(img, box, preset_x, preset_y, size), lm256, box


def crop_pixels(img: np.ndarray, box, preset_x: int, preset_y: int, size: int = OUT_SIZE) -> np.ndarray:
    """The pixel half of crop_face for a given box (canvas coordinates) and presets: the statement the device kernel is held to."""
    h, w = img.shape[:2]
    if preset_x > 0 or preset_y > 0:
        large = np.zeros((h + preset_y + preset_y + 2, w + preset_x + preset_x + 2, img.shape[2]))
        large[preset_y:preset_y + h, preset_x:preset_x + w, :] = img
        return to_u8(resize_f64(large[box[1]:box[3], box[0]:box[2], :], size))
    return resize_u8(img[box[1]:box[3], box[0]:box[2], :], size)


def unfilter_tall_host(raw: np.ndarray, h: int, w: int, c: int) -> np.ndarray:
    """Filtered PNG scanlines of any height -> uint8 [h,w,c] on the host: pngio.unfilter_host has no row limit (the 256 rows are the
    device kernel's), so it is the reference of bsr_png_unfilter_tall as it is."""
    from .pngio import unfilter_host
    return unfilter_host(raw, h, w, c)


def preprocess_folder(src_glob: str, dst_dir: str) -> List[str]:
    """dataprocess.py as a function: every `<name>.png` of `src_glob` with its `<name>.npy` beside it becomes `<dst_dir>/<name>/<name>.png`
    and `.npy` unless the script skips it; -> the names written.  The PNG is lossless, so Dataset(config, 'test') reads `crop_face`'s bytes."""
    from .pngio import read_rgb_u8, write_png
    done = []
    for path in sorted(glob.glob(src_glob)):
        name = os.path.basename(path).split(".")[0]
        lm_path = os.path.join(os.path.dirname(path), name + ".npy")
        if not path.endswith(".png") or not os.path.isfile(lm_path):
            continue
        res = crop_face(read_rgb_u8(path), np.load(lm_path))
        if res is None:
            continue
        face, lm256, _ = res
        write_png(os.path.join(dst_dir, name, name + ".png"), face)
        np.save(os.path.join(dst_dir, name, name + ".npy"), lm256)
        done.append(name)
    return done


def main(argv=None) -> int:
    argv = sys.argv[1:] if argv is None else list(argv)
    if len(argv) != 2:
        sys.stderr.write("usage: python -m blindshadowremoval_amd.wild_crop SRC_GLOB DST_DIR\n")
        return 2
    for name in preprocess_folder(argv[0], argv[1]):
        print(os.path.join(argv[1], name))
    return 0


if __name__ == "__main__":
    sys.exit(main())
