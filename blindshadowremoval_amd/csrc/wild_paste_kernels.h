// In-the-wild photographs on the device, the way back: the network's change resized to the crop box and written into the photograph
// the crop was cut from.  The reference has no such step for in-the-wild photographs (train_test_GSC.py's test_step does the like for
// UCB only); the statement this kernel is held to, byte for byte, is blindshadowremoval_amd/wild_paste.py (paste_face).
//
//   paste_faces_kernel: one thread per pixel of box ∩ photograph, 16 x 16 blocks, item and tile taken from the grid; a block past its
//     item's last tile leaves at once.  The thread computes its own bilinear coefficients (crop_coef, wild_crop_kernels.h: S source
//     pixels resized to the box's side), reads its four taps of im | con_rgb | face through pointers and pixel strides (a channel slice
//     of the packed NHWC row is fine), and rewrites its photograph pixel IN PLACE in the blob.  Pixels outside the box already hold the
//     photograph: nothing is launched for them.  float32 throughout, contraction into FMA off.  No atomics, no shared memory: a thread
//     reads and writes only its own pixel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wild_crop_kernels.h"

#pragma clang fp contract(off)

namespace bsr {

struct PasteItem {
  int64_t photo_off;          // RGB8 photograph [h][w][3] in the blob, rewritten in place
  int32_t h, w;
  int32_t box[4];             // x0, y0, x1, y1 in CANVAS pixels, as CropItem
  int32_t preset_x, preset_y; // where the photograph lies in the canvas
  int32_t row, pad_;          // the item's row of im / con / face
};
static_assert(sizeof(PasteItem) == 48, "PasteItem is 48 bytes (prep.py PASTE_DTYPE)");

constexpr int kPasteResidual = 0, kPasteReplace = 1;

struct PastePlanes {
  const float* im;            // [n][S][S] pixels of 3 floats, im_ps floats apart
  const float* con;
  const float* face;          // one float per pixel
  int im_ps, con_ps, face_ps;
};

// box ∩ photograph in the photograph's coordinates
__host__ __device__ __forceinline__ void paste_region(const PasteItem& it, int& x_lo, int& y_lo, int& x_hi, int& y_hi) {
  x_lo = it.box[0] - it.preset_x > 0 ? it.box[0] - it.preset_x : 0;
  y_lo = it.box[1] - it.preset_y > 0 ? it.box[1] - it.preset_y : 0;
  x_hi = it.box[2] - it.preset_x < it.w ? it.box[2] - it.preset_x : it.w;
  y_hi = it.box[3] - it.preset_y < it.h ? it.box[3] - it.preset_y : it.h;
}

__host__ __device__ __forceinline__ unsigned paste_tiles(const PasteItem& it) {
  int x_lo, y_lo, x_hi, y_hi;
  paste_region(it, x_lo, y_lo, x_hi, y_hi);
  if (x_hi <= x_lo || y_hi <= y_lo) return 0u;
  return (unsigned)((x_hi - x_lo + 15) / 16) * (unsigned)((y_hi - y_lo + 15) / 16);
}

__device__ __forceinline__ unsigned char paste_sat_u8(float v) {
  v = __builtin_rintf(v);                                       // round half to even
  return (unsigned char)(v < 0.f ? 0.f : (v > 255.f ? 255.f : v));
}

// grid (max over items of paste_tiles, n); block 256 = 16 x 16 photograph pixels
__global__ __launch_bounds__(256) void paste_faces_kernel(unsigned char* __restrict__ blob, const PasteItem* __restrict__ items, int S, PastePlanes pl, int mode) {
  const PasteItem it = items[blockIdx.y];
  int x_lo, y_lo, x_hi, y_hi;
  paste_region(it, x_lo, y_lo, x_hi, y_hi);
  if (x_hi <= x_lo || y_hi <= y_lo) return;
  const unsigned tpr = (unsigned)((x_hi - x_lo + 15) / 16);
  if (blockIdx.x >= tpr * (unsigned)((y_hi - y_lo + 15) / 16)) return;
  const int px = x_lo + (int)(blockIdx.x % tpr) * 16 + (int)(threadIdx.x & 15), py = y_lo + (int)(blockIdx.x / tpr) * 16 + (int)(threadIdx.x >> 4);
  if (px >= x_hi || py >= y_hi) return;
  int xa, xb, ya, yb;
  float fx, fy;
  crop_coef(px + it.preset_x - it.box[0], S, it.box[2] - it.box[0], true, xa, xb, fx);
  crop_coef(py + it.preset_y - it.box[1], S, it.box[3] - it.box[1], false, ya, yb, fy);
  const float a0 = 1.f - fx, a1 = fx, b0 = 1.f - fy, b1 = fy;
  const size_t base = (size_t)it.row * S * S;
  const size_t t00 = base + (size_t)ya * S + xa, t01 = base + (size_t)ya * S + xb, t10 = base + (size_t)yb * S + xa, t11 = base + (size_t)yb * S + xb;
  unsigned char* p = blob + it.photo_off + ((size_t)py * it.w + px) * 3;
  auto clip01 = [](float v) -> float { return v < 0.f ? 0.f : (v > 1.f ? 1.f : v); };
  auto interp = [&](float v00, float v01, float v10, float v11) -> float {
    const float d0 = v00 * a0 + v01 * a1;
    const float d1 = v10 * a0 + v11 * a1;
    return d0 * b0 + d1 * b1;
  };
  const float f00 = pl.face[t00 * pl.face_ps], f01 = pl.face[t01 * pl.face_ps], f10 = pl.face[t10 * pl.face_ps], f11 = pl.face[t11 * pl.face_ps];
  if (mode == kPasteResidual) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float v00 = (clip01(pl.con[t00 * pl.con_ps + c]) - pl.im[t00 * pl.im_ps + c]) * f00;
      const float v01 = (clip01(pl.con[t01 * pl.con_ps + c]) - pl.im[t01 * pl.im_ps + c]) * f01;
      const float v10 = (clip01(pl.con[t10 * pl.con_ps + c]) - pl.im[t10 * pl.im_ps + c]) * f10;
      const float v11 = (clip01(pl.con[t11 * pl.con_ps + c]) - pl.im[t11 * pl.im_ps + c]) * f11;
      const float val = interp(v00, v01, v10, v11);
      p[c] = paste_sat_u8((float)p[c] + val * 255.f);
    }
  } else {
    const float a = interp(f00, f01, f10, f11);
    const float na = 1.f - a;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float r = interp(clip01(pl.con[t00 * pl.con_ps + c]), clip01(pl.con[t01 * pl.con_ps + c]), clip01(pl.con[t10 * pl.con_ps + c]),
                             clip01(pl.con[t11 * pl.con_ps + c]));
      const float old = (float)p[c] / 255.f;
      p[c] = paste_sat_u8((r * a + old * na) * 255.f);
    }
  }
}

}  // namespace bsr
