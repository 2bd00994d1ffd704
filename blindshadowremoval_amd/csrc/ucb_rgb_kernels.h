// UCB post-processing of the RGB baseline's FSRNet.test_step (/root/reference/train_RGB_test.py:403-505) ON THE DEVICE.
//
// Everything after the generator call, for a batch of B items: row 0's ground truth, prediction and input are resized to the crop-box
// size (tf.image.resize, bilinear, half-pixel) and zero-padded back to S; the with-hair face mask is resized and rounded (the six other
// masks the reference resizes are never read again: they are not inputs here); the prediction is composited over the input inside the
// mask and clipped (:468,475 — the prediction itself is not clipped first); SSIM / PSNR against the ground truth (:481-482); the three
// figures [input, composite, ground truth] (:502) as one uint8 strip.  blindshadowremoval_amd/ucb_post_rgb.py is the host statement:
// every figure is bit-identical to it (same float32 operations in the same order, fp contraction off, as ucb_resize_kernel).
//
// Two kernels per batch:
//   ucb_rgb_pixel_kernel  grid (S*S/256, B), one thread per output pixel: 10 resized planes (gt 3, pred 3, input 3, mask 1), pad,
//                         composite, clip; writes the SSIM operands (gt_sc, out) to the scratch, the strip [B][S][3S][3] directly and
//                         the float figures when asked;
//   ucb_rgb_ssim_kernel   tf.image.ssim's 11x11 window + the squared error of PSNR per 16x16 tile (ucb_ssim_tile, shared with the GSC
//                         chain), then ucb_ssim_finish_kernel folds the tiles in a fixed order.
// No atomics; every scratch word a later kernel reads is written by an earlier kernel of the same call.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ucb_kernels.h"

namespace bsr {

constexpr int kUcbRgbFigs = 3;

struct UcbRgbScratch {                   // per item, inside the caller's scratch block
  double* ssim_part;                     // [2][nblk] SSIM map / squared-error sums per tile
  float* gt;                             // [N][3] gt_sc
  float* out;                            // [N][3] composite
};

__host__ __device__ inline size_t ucb_rgb_item_scratch_bytes(int S) {
  const size_t N = (size_t)S * S;
  const size_t nblk = (size_t)((S + kSsimTile - 1) / kSsimTile) * ((S + kSsimTile - 1) / kSsimTile);
  const size_t b = 2 * nblk * 8 + N * 3 * 4 * 2;
  return (b + 255) & ~size_t(255);
}

__host__ __device__ inline UcbRgbScratch ucb_rgb_scratch(void* base, int item, int S) {
  const size_t N = (size_t)S * S;
  const size_t nblk = (size_t)((S + kSsimTile - 1) / kSsimTile) * ((S + kSsimTile - 1) / kSsimTile);
  unsigned char* p = static_cast<unsigned char*>(base) + (size_t)item * ucb_rgb_item_scratch_bytes(S);
  UcbRgbScratch s;
  s.ssim_part = reinterpret_cast<double*>(p); p += 2 * nblk * 8;
  s.gt = reinterpret_cast<float*>(p); p += N * 3 * 4;
  s.out = reinterpret_cast<float*>(p);
  return s;
}

// rows9: [B][S][S][9] float32 = input 3 | ground truth 3 | con 3 of row 0 of each item; masks: [B][S][S] uint8 grey levels of the
// with-hair face mask (cv2.imread(...) / 255.0, one of the three equal channels); boxes: [B][4] float32.
// strips: [B][S][3 S][3] uint8; figs: optional [B][3][S][S][3] float32; status: [B] (UCB_BAD_BOX: empty box or larger than S).
__global__ __launch_bounds__(256) void ucb_rgb_pixel_kernel(const float* __restrict__ rows9, const unsigned char* __restrict__ masks,
                                                            const float* __restrict__ boxes, int S, void* scratch,
                                                            unsigned char* __restrict__ strips, float* __restrict__ figs, int* __restrict__ status) {
#pragma clang fp contract(off)
  const int item = blockIdx.y;
  const int p = blockIdx.x * 256 + threadIdx.x;
  const int N = S * S;
  if (p >= N) return;
  const int oy = p / S, ox = p % S;
  const int size = ucb_box_size(boxes + 4 * item);
  const bool bad = size <= 0 || size > S;
  if (p == 0) status[item] = bad ? UCB_BAD_BOX : UCB_OK;
  float f[kUcbRgbFigs][3];                                    // tmp | out | gt_sc
  if (bad || oy >= size || ox >= size) {                      // the zero pad of :447-465 (a bad box: a black strip, NaN losses)
#pragma unroll
    for (int k = 0; k < kUcbRgbFigs; ++k) f[k][0] = f[k][1] = f[k][2] = 0.f;
  } else {
    // TensorFlow's half-pixel bilinear weights and lerp order, exactly as ucb_resize_kernel
    const float scale = (float)S / (float)size;
    const float sy = ((float)oy + 0.5f) * scale - 0.5f, sx = ((float)ox + 0.5f) * scale - 0.5f;
    const float fy = floorf(sy), fx = floorf(sx);
    const int y0 = max((int)fy, 0), y1 = min((int)ceilf(sy), S - 1);
    const int x0 = max((int)fx, 0), x1 = min((int)ceilf(sx), S - 1);
    const float yl = sy - fy, xl = sx - fx;
    const float* r = rows9 + (size_t)item * N * 9;
    const float* tl = r + ((size_t)y0 * S + x0) * 9; const float* tr = r + ((size_t)y0 * S + x1) * 9;
    const float* bl = r + ((size_t)y1 * S + x0) * 9; const float* br = r + ((size_t)y1 * S + x1) * 9;
    auto lerp = [&](float a, float b, float c, float d) {
      const float top = a + (b - a) * xl;
      const float bottom = c + (d - c) * xl;
      return top + (bottom - top) * yl;
    };
    const unsigned char* mk = masks + (size_t)item * N;
    auto g = [&](int y, int x) { return (float)((double)mk[y * S + x] / 255.0); };          // np.asarray(.., float64) / 255.0, then float32
    const float m = rintf(lerp(g(y0, x0), g(y0, x1), g(y1, x0), g(y1, x1)));              // tf.round: half to even
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float tmp = lerp(tl[c], tr[c], bl[c], br[c]);
      const float pred = lerp(tl[6 + c], tr[6 + c], bl[6 + c], br[6 + c]);
      f[0][c] = tmp;
      f[1][c] = fminf(fmaxf(pred * m + tmp * (1.f - m), 0.f), 1.f);
      f[2][c] = lerp(tl[3 + c], tr[3 + c], bl[3 + c], br[3 + c]);
    }
  }
  const UcbRgbScratch sc = ucb_rgb_scratch(scratch, item, S);
#pragma unroll
  for (int c = 0; c < 3; ++c) { sc.gt[(size_t)p * 3 + c] = f[2][c]; sc.out[(size_t)p * 3 + c] = f[1][c]; }
  unsigned char* strip = strips + (size_t)item * N * kUcbRgbFigs * 3;
#pragma unroll
  for (int k = 0; k < kUcbRgbFigs; ++k) {
    unsigned char* dst = strip + ((size_t)oy * (kUcbRgbFigs * S) + (size_t)k * S + ox) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) dst[c] = (unsigned char)rintf(fminf(fmaxf(f[k][c], 0.f), 1.f) * 255.f);
    if (figs != nullptr) {
      float* fd = figs + (((size_t)item * kUcbRgbFigs + k) * N + p) * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) fd[c] = f[k][c];
    }
  }
}

struct UcbRgbSsimOperands {              // ucb_ssim_tile's operands: gt_sc and the composite, [N][3] each
  const float* gt;
  const float* out;
  __device__ float x(size_t q, int c) const { return gt[q * 3 + c]; }
  __device__ float y(size_t q, int c) const { return out[q * 3 + c]; }
};

__global__ __launch_bounds__(256) void ucb_rgb_ssim_kernel(int S, void* scratch) {
  const UcbRgbScratch sc = ucb_rgb_scratch(scratch, blockIdx.y, S);
  ucb_ssim_tile(UcbRgbSsimOperands{sc.gt, sc.out}, S, sc.ssim_part);
}

__global__ __launch_bounds__(64) void ucb_rgb_ssim_finish_kernel(int S, void* scratch, const int* __restrict__ status, float* __restrict__ losses) {   // grid (B), one wave
  const int item = blockIdx.x;
  ucb_ssim_finish(ucb_rgb_scratch(scratch, item, S).ssim_part, S, status[item] == UCB_OK, losses + 2 * item);
}

inline hipError_t launch_ucb_post_rgb(const float* rows9, const unsigned char* masks, const float* boxes, int B, int S, float* losses,
                                      unsigned char* strips, float* figs, int* status, void* scratch, hipStream_t stream) {
  const int N = S * S;
  hipLaunchKernelGGL(ucb_rgb_pixel_kernel, dim3((unsigned)((N + 255) / 256), (unsigned)B), dim3(256), 0, stream, rows9, masks, boxes, S, scratch,
                     strips, figs, status);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const int tiles = (S + kSsimTile - 1) / kSsimTile;
  hipLaunchKernelGGL(ucb_rgb_ssim_kernel, dim3((unsigned)(tiles * tiles), (unsigned)B), dim3(256), 0, stream, S, scratch);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(ucb_rgb_ssim_finish_kernel, dim3((unsigned)B), dim3(64), 0, stream, S, scratch, status, losses);
  return hipGetLastError();
}

}  // namespace bsr
