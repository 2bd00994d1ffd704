"""Writing the de-shadowed face back into the uncropped photograph — the inverse of wild_crop.py's crop, for the in-the-wild route.

`paste_face(photo, box, preset_x, preset_y, im, con, face, mode)` takes the photograph the crop was cut from, the crop's geometry
(`wild_crop.crop_geometry`: the box in canvas coordinates and the presets) and three S x S planes of one item of the forward — `im`
(the network's input, channels 0:3 of the row), `con` (`con_rgb`) and `face` (the blurred face hull, channel 15 of the row) — and
returns the photograph with the network's change resized to the box and written into it.

WHAT IS PINNED TO WHAT.  The reference has no such step for in-the-wild photographs (its `test_step` resizes the prediction to the
crop box and composites it under a mask for UCB only), so nothing here is pinned to the reference: this module is the statement,
and the device kernel (csrc/wild_paste_kernels.h, bsr_paste_faces) is held to it byte for byte.  The bilinear taps are
`wild_crop._axis` as it stands — OpenCV's INTER_LINEAR coefficients, the x rule with its edge clamps and the y rule.

Geometry.  The photograph lies at (preset_y, preset_x) of the canvas; photograph pixel (y, x) is canvas pixel (y + preset_y,
x + preset_x).  The box [x0, y0, x1, y1] has nx = x1 - x0 columns and ny = y1 - y0 rows (crop_geometry's boxes are square).  A pixel
whose canvas position is outside the box is returned unchanged.  Only pixels of the photograph are produced: where the box leaves
the photograph (a preset > 0) the part outside it is simply not computed, the zero canvas is never materialised.

Pixels inside the box, output index (oy, ox) = (y + preset_y - y0, x + preset_x - x0).  Everything is float32, every product and sum
rounded on its own (no fused multiply-add):

    xa, xb, fx = _axis(S, nx, True)[ox]          ya, yb, fy = _axis(S, ny, False)[oy]
    a0 = 1 - fx,  a1 = fx,  b0 = 1 - fy,  b1 = fy
    interp(P) = (P[ya][xa] * a0 + P[ya][xb] * a1) * b0 + (P[yb][xa] * a0 + P[yb][xb] * a1) * b1      (horizontal pass, then vertical)
    con is clipped to [0, 1] first (train_test_GSC.py:873)

  mode "residual" (default): only the network's low-frequency change travels, the photograph keeps its detail
    P_c = (con_c - im_c) * face                  (formed per tap)
    out_c = sat_u8(rint(float32(photo_c) + interp(P_c) * 255))
  mode "replace":
    a = interp(face),  r_c = interp(con_c)
    out_c = sat_u8(rint((r_c * a + (float32(photo_c) / 255) * (1 - a)) * 255))

rint is round half to even; sat_u8 clamps to [0, 255].
"""
from __future__ import annotations

import numpy as np

from .wild_crop import _axis

MODES = ("residual", "replace")          # bsr_paste_faces' mode argument is the index


def _interp(plane: np.ndarray, xa, xb, a0, a1, ya, yb, b0, b1) -> np.ndarray:
    """float32 [S,S,C] -> [len(ya), len(xa), C]: the horizontal pass, then the vertical pass (module docstring)."""
    d = plane[:, xa] * a0[None, :, None] + plane[:, xb] * a1[None, :, None]
    return d[ya] * b0[:, None, None] + d[yb] * b1[:, None, None]


def paste_region(box, preset_x: int, preset_y: int, h: int, w: int):
    """box ∩ photograph in the photograph's coordinates: (x_lo, y_lo, x_hi, y_hi), empty when hi <= lo."""
    return (max(int(box[0]) - preset_x, 0), max(int(box[1]) - preset_y, 0), min(int(box[2]) - preset_x, w), min(int(box[3]) - preset_y, h))


def paste_face(photo: np.ndarray, box, preset_x: int, preset_y: int, im: np.ndarray, con: np.ndarray, face: np.ndarray,
               mode: str = "residual") -> np.ndarray:
    """uint8 [h,w,3] photograph + the crop's geometry + float32 im [S,S,3], con [S,S,3], face [S,S,1] -> uint8 [h,w,3] (module docstring)."""
    photo = np.asarray(photo)
    if photo.dtype != np.uint8 or photo.ndim != 3 or photo.shape[2] != 3:
        raise ValueError("paste_face takes a uint8 [h,w,3] photograph, got %s %s" % (photo.dtype, photo.shape))
    if mode not in MODES:
        raise ValueError("paste_face: mode is one of %s, got %r" % (MODES, mode))
    im, con, face = np.asarray(im, np.float32), np.asarray(con, np.float32), np.asarray(face, np.float32)
    S = im.shape[0]
    if im.shape != (S, S, 3) or con.shape != (S, S, 3) or face.shape != (S, S, 1):
        raise ValueError("paste_face takes im [S,S,3], con [S,S,3] and face [S,S,1], got %s %s %s" % (im.shape, con.shape, face.shape))
    preset_x, preset_y = int(preset_x), int(preset_y)
    nx, ny = int(box[2]) - int(box[0]), int(box[3]) - int(box[1])
    if nx < 2 or ny < 2 or preset_x < 0 or preset_y < 0:
        raise ValueError("paste_face: the box needs a side of at least 2 pixels and presets >= 0, got box %s presets %d %d" % (list(box), preset_x, preset_y))
    h, w = photo.shape[:2]
    out = photo.copy()
    x_lo, y_lo, x_hi, y_hi = paste_region(box, preset_x, preset_y, h, w)
    if x_hi <= x_lo or y_hi <= y_lo:
        return out
    one = np.float32(1)
    xa, xb, fx = _axis(S, nx, True)
    ya, yb, fy = _axis(S, ny, False)
    ox = np.arange(x_lo, x_hi) + preset_x - int(box[0])
    oy = np.arange(y_lo, y_hi) + preset_y - int(box[1])
    taps = (xa[ox], xb[ox], (one - fx[ox]).astype(np.float32), fx[ox], ya[oy], yb[oy], (one - fy[oy]).astype(np.float32), fy[oy])
    con = np.clip(con, np.float32(0), one)
    old = photo[y_lo:y_hi, x_lo:x_hi].astype(np.float32)
    k = np.float32(255)
    if mode == "residual":
        v = old + _interp((con - im) * face, *taps) * k
    else:
        a = _interp(face, *taps)
        v = (_interp(con, *taps) * a + (old / k) * (one - a)) * k
    assert v.dtype == np.float32
    out[y_lo:y_hi, x_lo:x_hi] = np.clip(np.rint(v), 0, 255).astype(np.uint8)
    return out
