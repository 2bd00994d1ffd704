// In-the-wild photographs on the device: what the reference's `dataprocess.py` ("Preprocessing New Images", /root/reference/dataprocess.py:25-77)
// does to an uncropped photograph between cv2.imread and cv2.imwrite, behind the copy to the device.
//
//   png_unfilter_tall_kernel: PNG scanline reconstruction (RFC 2083 section 6) of files of ANY height.  prep_kernels.h's
//     png_unfilter_kernel owns one row per thread and stops at 256 rows; this one walks the image in BANDS of 256 rows with the same
//     anti-diagonal scheme, one workgroup per image.  Inside a band the pixel above comes through LDS from the thread above; for the
//     band's first row it comes from the last row of the band before, which the workgroup has just written to the output area and
//     thread 0 reads back four pixels at a time, requested sixteen steps ahead like the filtered bytes.  `rows_needed` (0 = all) stops
//     the walk after that row: nothing below the crop box is ever read.
//   crop_faces_kernel: the face box cut out of the photograph and cv2.resize'd to S x S, one thread per output pixel, 16 x 16 blocks,
//     coefficients computed in the thread.  preset_x == preset_y == 0: the crop is 8-bit and the resize OpenCV's 8-bit INTER_LINEAR
//     (11-bit coefficients, integer horizontal pass, fixed-point vertical pass with its rounding shift).  Otherwise the reference pastes
//     the photograph into a float64 zero canvas (never materialised here: a tap outside the photograph is 0.0) and the resize is the
//     floating INTER_LINEAR on doubles with float32 coefficients; the byte is round-half-even with saturation (cv2.imwrite of a float64
//     image).  The arithmetic is blindshadowremoval_amd/wild_crop.py's (resize_u8 / resize_f64), statement for statement, contraction
//     into FMA off: every byte equals the host statement's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "prep_kernels.h"

#pragma clang fp contract(off)

namespace bsr {

struct UnfilterTallItem {
  int64_t raw_off, out_off;   // as UnfilterItem: h x (1 + w c) filtered scanlines -> RGB8 [h][w][3] (grey8 [h][w] with grey_out)
  int32_t h, w, c, grey_out;
  int32_t rows_needed, pad_;  // rows_needed: 0 = all h rows, else the walk stops after that many
};
static_assert(sizeof(UnfilterTallItem) == 40, "UnfilterTallItem is 40 bytes (prep.py UNFILTER_TALL_DTYPE)");

struct CropItem {
  int64_t src_off, out_off;   // RGB8 photograph [h][w][3] -> RGB8 crop [S][S][3]
  int32_t h, w;
  int32_t box[4];             // x0, y0, x1, y1 in CANVAS pixels (the photograph's own when both presets are 0)
  int32_t preset_x, preset_y; // where the photograph lies in the (h + 2 preset_y + 2) x (w + 2 preset_x + 2) zero canvas
};
static_assert(sizeof(CropItem) == 48, "CropItem is 48 bytes (prep.py CROP_DTYPE)");

// One image of any height, band by band.  The band's body is png_unfilter_image's (prep_kernels.h) with the row index offset by the band
// and one more source for "above": see the file comment.
template <int C, bool GREY = false>
__device__ __forceinline__ void png_unfilter_tall_image(unsigned char* __restrict__ blob, const UnfilterTallItem& it, unsigned (*s_px)[256]) {
  constexpr int NCH = C == 1 ? 1 : 3;
  constexpr int OB = GREY ? 1 : 3;                              // output bytes per pixel
  const int tid = threadIdx.x, w = it.w;
  const int hh = (it.rows_needed > 0 && it.rows_needed < it.h) ? it.rows_needed : it.h;
  const size_t rb = 1 + (size_t)w * C;
  struct Group { unsigned d[C]; };
  struct UpGroup { unsigned d[OB]; };
#pragma unroll 1
  for (int row0 = 0; row0 < hh; row0 += kUnfilterMaxRows) {
    const int hb = min(hh - row0, kUnfilterMaxRows);
    const bool row = tid < hb;
    const bool seam = row0 > 0;                                 // (uniform) the band has a reconstructed row above it
    const size_t r = (size_t)row0 + (size_t)(row ? tid : 0);
    const unsigned char* rp = blob + it.raw_off + r * rb;
    unsigned char* op = blob + it.out_off + r * (size_t)w * OB;
    const unsigned char* upp = blob + it.out_off + (size_t)(seam ? row0 - 1 : 0) * (size_t)w * OB;      // the output row above the band
    const int ft = row ? rp[0] : 0;
    rp += 1;
    auto fetch = [&](int x0) -> Group {                         // pixels x0 .. x0 + 3 (a group without a pixel of the row: any readable address)
      const unsigned char* q = rp + ((x0 <= -4 || x0 >= w) ? 0 : x0 * C);
      Group g;
      __builtin_memcpy(g.d, q, 4 * C);
      return g;
    };
    auto fetch_up = [&](int x0) -> UpGroup {                    // thread 0: output pixels x0 .. x0 + 3 of the row above the band (everyone else: its first bytes)
      const unsigned char* q = upp + ((tid != 0 || x0 < 0 || x0 >= w) ? 0 : x0 * OB);
      UpGroup g;
      __builtin_memcpy(g.d, q, 4 * OB);
      return g;
    };
    int left[3] = {0, 0, 0}, upl[3] = {0, 0, 0};
    const int m1 = -(int)(ft == 1), m2 = -(int)(ft == 2), m3 = -(int)(ft == 3), m4 = -(int)(ft == 4);
    const bool from_out = seam && tid == 0;
    const bool has_up = seam || tid > 0;
    Group win[4];
    UpGroup upwin[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      win[i] = fetch(4 * i - tid);
#pragma unroll
      for (int j = 0; j < OB; ++j) upwin[i].d[j] = 0u;
      if (seam) upwin[i] = fetch_up(4 * i - tid);
    }
    const int steps = (w + hb - 1 + 15) & ~15;
    for (int t = 0; t < steps; t += 16) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int x0 = t + 4 * i - tid;
        const Group g = win[i];
        const UpGroup ug = upwin[i];
        unsigned od[3] = {0u, 0u, 0u};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int x = x0 + k;
          const bool act = row && x >= 0 && x < w;
          unsigned above = s_px[(k + 1) & 1][tid > 0 ? tid - 1 : 0];      // thread tid - 1 wrote its pixel x one step ago
          {
            unsigned upv;                                         // pixel k of the group read back from the output row above the band
            if constexpr (GREY) {
              upv = (ug.d[0] >> (8 * k)) & 255u;
            } else {
              const int sh = 8 * ((3 * k) & 3), dw = (3 * k) >> 2;
              upv = ug.d[dw] >> sh;
              if (sh > 8) upv |= ug.d[dw + 1] << (32 - sh);
              upv &= 0xFFFFFFu;
            }
            above = from_out ? upv : above;
          }
          int up[3];
          up[0] = has_up ? (int)(above & 255u) : 0; up[1] = has_up ? (int)((above >> 8) & 255u) : 0; up[2] = has_up ? (int)((above >> 16) & 255u) : 0;
          int o[3];
#pragma unroll
          for (int ch = 0; ch < 3; ++ch) {
            if (ch < NCH) {
              const int bi = k * C + ch;                          // byte of the group
              const int a = left[ch], b = up[ch], c0 = upl[ch];
              const int pa = abs(b - c0), pb = abs(a - c0), pc = abs(a + b - 2 * c0);
              const int paeth = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c0);
              const int pred = (a & m1) | (b & m2) | (((a + b) >> 1) & m3) | (paeth & m4);
              o[ch] = (int)(((g.d[bi >> 2] >> (8 * (bi & 3))) & 255u) + (unsigned)pred) & 255;
              left[ch] = act ? o[ch] : left[ch];
              upl[ch] = act ? b : upl[ch];
            }
          }
          if (NCH == 1) { o[1] = o[0]; o[2] = o[0]; }
          const unsigned px = (unsigned)o[0] | ((unsigned)o[1] << 8) | ((unsigned)o[2] << 16);
          if (act) s_px[k & 1][tid] = px;
          if constexpr (GREY) {
            od[0] |= (px & 255u) << (8 * k);
          } else {
            const int sh = 8 * ((3 * k) & 3), dw = (3 * k) >> 2;
            od[dw] |= px << sh;
            if (sh > 8) od[dw + 1] |= px >> (32 - sh);
          }
          asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        }
        if (row && x0 >= 0 && x0 + 3 < w) {
          __builtin_memcpy(op + OB * (size_t)x0, od, 4 * OB);
        } else if (row && x0 > -4 && x0 < w) {
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if (x0 + k >= 0 && x0 + k < w)
#pragma unroll
              for (int ch = 0; ch < OB; ++ch) op[OB * (x0 + k) + ch] = (unsigned char)(od[(OB * k + ch) >> 2] >> (8 * ((OB * k + ch) & 3)));
        }
        win[i] = fetch(x0 + 16);
        if (seam) upwin[i] = fetch_up(x0 + 16);
      }
    }
    // the band's rows are in memory before the next band's thread 0 reads its last one back (one workgroup: a workgroup-scope fence)
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void png_unfilter_tall_kernel(unsigned char* __restrict__ blob, const UnfilterTallItem* __restrict__ items) {
  __shared__ unsigned s_px[2][256];
  const UnfilterTallItem it = items[blockIdx.x];
  if (it.c == 3) png_unfilter_tall_image<3>(blob, it, s_px);
  else if (it.c == 4) png_unfilter_tall_image<4>(blob, it, s_px);
  else if (it.grey_out) png_unfilter_tall_image<1, true>(blob, it, s_px);
  else png_unfilter_tall_image<1>(blob, it, s_px);
}

// OpenCV's coefficient of output index o along an axis of n source pixels resized to S (resize.cpp: fx = (float)((dx + 0.5) * scale - 0.5),
// sx = cvFloor(fx), fx -= sx).  The x axis zeroes the weight where it clamps the index; the y axis clips the two ROW indices and keeps
// the weight.
__device__ __forceinline__ void crop_coef(int o, int n, int S, bool is_x, int& i0, int& i1, float& f) {
  const double inv = (double)S / (double)n;
  const double scale = 1.0 / inv;
  float fx = (float)(((double)o + 0.5) * scale - 0.5);
  int s = (int)__builtin_floorf(fx);
  fx = fx - (float)s;
  if (is_x) {
    if (s < 0) { fx = 0.f; s = 0; }
    if (s >= n - 1) { fx = 0.f; s = n - 1; }
    i0 = s;
    i1 = s + 1 < n - 1 ? s + 1 : n - 1;
  } else {
    i0 = s < 0 ? 0 : (s > n - 1 ? n - 1 : s);
    i1 = s + 1 < 0 ? 0 : (s + 1 > n - 1 ? n - 1 : s + 1);
  }
  f = fx;
}

// grid (S / 16 * S / 16, n); block 256 = 16 x 16 output pixels
__global__ __launch_bounds__(256) void crop_faces_kernel(unsigned char* __restrict__ blob, const CropItem* __restrict__ items, int S) {
  const CropItem it = items[blockIdx.y];
  const int bpr = S / 16;
  const int oy = (int)(blockIdx.x / bpr) * 16 + (int)(threadIdx.x >> 4), ox = (int)(blockIdx.x % bpr) * 16 + (int)(threadIdx.x & 15);
  const int nx = it.box[2] - it.box[0], ny = it.box[3] - it.box[1];
  int x0, x1, y0, y1;
  float fx, fy;
  crop_coef(ox, nx, S, true, x0, x1, fx);
  crop_coef(oy, ny, S, false, y0, y1, fy);
  const unsigned char* src = blob + it.src_off;
  unsigned char* dst = blob + it.out_off + ((size_t)oy * S + ox) * 3;
  if (it.preset_x == 0 && it.preset_y == 0) {
    // 8-bit INTER_LINEAR: coefficients as shorts with 11 fractional bits, D = S0 a0 + S1 a1 along x, then
    // ((b0 (D0 >> 4)) >> 16) + ((b1 (D1 >> 4)) >> 16) + 2) >> 2 along y, stored as the low byte
    const int a0 = (int)__builtin_rintf((1.f - fx) * 2048.f), a1 = (int)__builtin_rintf(fx * 2048.f);
    const int b0 = (int)__builtin_rintf((1.f - fy) * 2048.f), b1 = (int)__builtin_rintf(fy * 2048.f);
    const unsigned char* r0 = src + ((size_t)(it.box[1] + y0) * it.w + it.box[0]) * 3;
    const unsigned char* r1 = src + ((size_t)(it.box[1] + y1) * it.w + it.box[0]) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int d0 = (int)r0[3 * x0 + c] * a0 + (int)r0[3 * x1 + c] * a1;
      const int d1 = (int)r1[3 * x0 + c] * a0 + (int)r1[3 * x1 + c] * a1;
      dst[c] = (unsigned char)((((b0 * (d0 >> 4)) >> 16) + ((b1 * (d1 >> 4)) >> 16) + 2) >> 2);
    }
  } else {
    // float64 canvas: photograph at (preset_y, preset_x), zero elsewhere; float32 coefficients widened to double, x first, then y
    const double a0 = (double)(1.f - fx), a1 = (double)fx, b0 = (double)(1.f - fy), b1 = (double)fy;
    auto tap = [&](int cy, int cx, int c) -> double {
      const int iy = it.box[1] + cy - it.preset_y, ix = it.box[0] + cx - it.preset_x;
      if (iy < 0 || iy >= it.h || ix < 0 || ix >= it.w) return 0.0;
      return (double)src[((size_t)iy * it.w + ix) * 3 + c];
    };
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double d0 = tap(y0, x0, c) * a0 + tap(y0, x1, c) * a1;
      const double d1 = tap(y1, x0, c) * a0 + tap(y1, x1, c) * a1;
      const double v = __builtin_rint(d0 * b0 + d1 * b1);      // round half to even
      dst[c] = (unsigned char)(v < 0.0 ? 0.0 : (v > 255.0 ? 255.0 : v));
    }
  }
}

}  // namespace bsr
