// The reconstruction and gradient losses of the reference's train_step ON THE DEVICE: recon_gs, recon_c and grad
// (train_test_GSC.py:107-115, 253-258, 287-301, 307-328, 357; utils.py:22-52, 116-125).  blindshadowremoval_amd/train_losses.py is the
// host statement and writes the arithmetic out; the pixel arithmetic here is float32 in its operation order with contraction off, so
// the three planes (mask_edge, bmaskgt, dif_grad / 1.2) are bit-identical to it.  Every reduction is a float64 sum in a FIXED order:
// there is no floating-point atomic anywhere, nothing depends on scheduling, and every word of scratch that a launch reads was written
// by an earlier launch of the same call.
//
// One chain of three launches on the caller's stream, no host synchronisation, no parallel branches:
//   losses_coarse_kernel   grid (ceil(P / 256), B), P = S^2 (1 + 1/4 + 1/16 + 1/64 + 1/256): the ten coarse planes (dy + dx) * 5 of gt
//                          and con_rgb resized to S / scale, scale = 1, 2, 4, 8, 16, six floats per coarse pixel (gt's three channels,
//                          then con_rgb's).  A thread samples its pixel, the one below and the one to the right.
//   losses_pixel_kernel    grid ((S / 16)^2, B), a 16 x 16 tile per workgroup.  edge0 of the tile and a halo of 4 goes to LDS (positions
//                          outside the image hold 0: they do not take part in the reference's dilations); two 5 x 5 maxima are one
//                          9 x 9 window, taken as a row pass and a column pass.  A thread then forms every term of its pixel — the
//                          coarse planes sampled bilinearly back to S — writes the requested figures, and the K = 18 sums are folded
//                          in float64 per wave by cross-lane moves and per workgroup through LDS, waves in index order.  The
//                          workgroup writes its K-vector into its own slot.
//   losses_finish_kernel   one workgroup: adds each item's slots in index order into sums[item][K], then the items in order, and
//                          forms the three losses in float64, rounded once to float32.
#pragma once
#include "post_common.h"

namespace bsr {

constexpr int kLossK = 18;                     // train_losses.SUM_NAMES, in its order
enum { LS_GS = 0, LS_C = 3, LS_Y = 6, LS_U = 9, LS_V = 12, LS_NBI = 15, LS_NEDGE = 16, LS_DG = 17 };      // a triple is: unmasked, mask_bi, mask_edge
constexpr int kLossTile = 16, kLossHalo = 4, kLossIn = kLossTile + 2 * kLossHalo, kLossLevels = 5;

__host__ __device__ inline int loss_tiles(int S) { return (S / kLossTile) * (S / kLossTile); }
__host__ __device__ inline int loss_level_side(int S, int l) { return S >> l; }                                  // scale 2^l
__host__ __device__ inline int loss_level_offset(int S, int l) { int o = 0; for (int i = 0; i < l; ++i) o += (S >> i) * (S >> i); return o; }      // in coarse pixels
__host__ __device__ inline int loss_coarse_pixels(int S) { return loss_level_offset(S, kLossLevels); }

struct LossScratch {                     // per item, in layout order
  float* coarse;                         // [P][6]
  double* slots;                         // [tiles][K]
  __host__ __device__ static LossScratch carve(ScratchCarver& c, int S) {
    LossScratch s;
    s.coarse = c.take<float>((size_t)loss_coarse_pixels(S) * 6);
    c.align(8);
    s.slots = c.take<double>((size_t)loss_tiles(S) * kLossK);
    return s;
  }
};
__host__ __device__ inline size_t loss_item_scratch_bytes(int S) { return item_scratch_bytes<LossScratch>(S); }

__device__ inline float loss_weighted(const float* x, float w0, float w1, float w2) {
#pragma clang fp contract(off)
  return (x[0] * w0 + x[1] * w1) + x[2] * w2;
}
__device__ inline float loss_gray(const float* x) { return loss_weighted(x, 0.2989f, 0.587f, 0.114f); }

// channel c of image `x` ([S][S][3] of one item) resized to s x s, at (cy, cx)
__device__ inline float loss_resized(const float* __restrict__ x, int S, int s, int cy, int cx, int c) {
  if (s == S) return x[((size_t)cy * S + cx) * 3 + c];
  const BilinearTap t(cy, cx, s, S);
  return t.lerp(x[((size_t)t.y0 * S + t.x0) * 3 + c], x[((size_t)t.y0 * S + t.x1) * 3 + c], x[((size_t)t.y1 * S + t.x0) * 3 + c],
                x[((size_t)t.y1 * S + t.x1) * 3 + c]);
}

__global__ __launch_bounds__(256) void losses_coarse_kernel(const float* __restrict__ gt, const float* __restrict__ con, int S, void* scratch) {
#pragma clang fp contract(off)
  const int item = blockIdx.y;
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= loss_coarse_pixels(S)) return;
  int l = 0;
  while (l + 1 < kLossLevels && p >= loss_level_offset(S, l + 1)) ++l;
  const int s = loss_level_side(S, l), q = p - loss_level_offset(S, l);
  const int cy = q / s, cx = q % s;
  const LossScratch sc = item_scratch<LossScratch>(scratch, item, S);
  const size_t base = (size_t)item * S * S * 3;
  float* out = sc.coarse + (size_t)p * 6;
  for (int h = 0; h < 2; ++h) {
    const float* x = (h == 0 ? gt : con) + base;
    for (int c = 0; c < 3; ++c) {
      const float v = loss_resized(x, S, s, cy, cx, c);
      const float dy = cy + 1 < s ? loss_resized(x, S, s, cy + 1, cx, c) - v : 0.f;
      const float dx = cx + 1 < s ? loss_resized(x, S, s, cy, cx + 1, c) - v : 0.f;
      out[h * 3 + c] = (dy + dx) * 5.0f;
    }
  }
}

__global__ __launch_bounds__(256) void losses_pixel_kernel(const float* __restrict__ img, const float* __restrict__ gt, const float* __restrict__ mask_sv,
                                                           const float* __restrict__ gs, const float* __restrict__ con, int S, void* scratch,
                                                           float* __restrict__ mask_edge, float* __restrict__ bmaskgt, float* __restrict__ dif_grad) {
#pragma clang fp contract(off)
  __shared__ int s_e0[kLossIn][kLossIn + 1];
  __shared__ int s_row[kLossIn][kLossTile + 1];
  __shared__ double s_red[4][kLossK];
  const int item = blockIdx.y, tid = threadIdx.x;
  const int tiles_x = S / kLossTile;
  const int ty0 = (blockIdx.x / tiles_x) * kLossTile, tx0 = (blockIdx.x % tiles_x) * kLossTile;
  const size_t N = (size_t)S * S, base = (size_t)item * N;
  const LossScratch sc = item_scratch<LossScratch>(scratch, item, S);
  for (int i = tid; i < kLossIn * kLossIn; i += 256) {
    const int yy = i / kLossIn, xx = i % kLossIn;
    const int y = ty0 - kLossHalo + yy, x = tx0 - kLossHalo + xx;
    int e = 0;
    if (y >= 0 && y < S && x >= 0 && x < S) {
      const float* m = mask_sv + (base + (size_t)y * S + x) * 3;
      const float mean_c = ((m[0] + m[1]) + m[2]) / 3.0f;
      e = (mean_c > 0.01f ? 1 : 0) - (m[0] > 0.3f && m[1] > 0.3f && m[2] > 0.3f ? 1 : 0);          // min_c > .3: every channel is
    }
    s_e0[yy][xx] = e;
  }
  __syncthreads();
  for (int i = tid; i < kLossIn * kLossTile; i += 256) {          // the row pass: 9 columns
    const int yy = i / kLossTile, xx = i % kLossTile;
    int e = s_e0[yy][xx];
#pragma unroll
    for (int k = 1; k <= 2 * kLossHalo; ++k) e = max(e, s_e0[yy][xx + k]);
    s_row[yy][xx] = e;
  }
  __syncthreads();
  const int ly = tid / kLossTile, lx = tid % kLossTile;
  const int y = ty0 + ly, x = tx0 + lx;
  int e9 = s_row[ly][lx];
#pragma unroll
  for (int k = 1; k <= 2 * kLossHalo; ++k) e9 = max(e9, s_row[ly + k][lx]);
  const bool edge = e9 > 0;
  const size_t p1 = (size_t)y * S + x, q = (base + p1) * 3;
  float g3[3], c3[3];
  bool bi[3];
  int nb = 0;
  for (int c = 0; c < 3; ++c) { g3[c] = gt[q + c]; c3[c] = con[q + c]; bi[c] = mask_sv[q + c] > 0.01f; nb += bi[c] ? 1 : 0; }
  const float gray_gt = loss_gray(g3);
  const bool bm = (gray_gt - loss_gray(img + q)) > 0.04f;
  if (mask_edge != nullptr) mask_edge[base + p1] = edge ? 1.0f : 0.f;
  if (bmaskgt != nullptr) bmaskgt[base + p1] = bm ? 1.0f : 0.f;
  double acc[kLossK];
  // a one-channel |x - y| under the three-channel mask_bi counts once per lit channel; under the one-channel mask_edge once
  auto triple = [&](int k0, float a) { acc[k0] = (double)a; acc[k0 + 1] = (double)a * (double)nb; acc[k0 + 2] = edge ? (double)a : 0.0; };
  triple(LS_GS, fabsf(gs[base + p1] - gray_gt));
  triple(LS_Y, fabsf(loss_weighted(c3, .299f, .587f, .114f) - loss_weighted(g3, .299f, .587f, .114f)));
  triple(LS_U, fabsf(loss_weighted(c3, -.168736f, -.331264f, .5f) - loss_weighted(g3, -.168736f, -.331264f, .5f)));
  triple(LS_V, fabsf(loss_weighted(c3, .5f, -.418688f, -.081312f) - loss_weighted(g3, .5f, -.418688f, -.081312f)));
  double ca = 0.0, cb = 0.0;
  for (int c = 0; c < 3; ++c) { const float a = fabsf(c3[c] - g3[c]); ca += (double)a; if (bi[c]) cb += (double)a; }
  acc[LS_C] = ca; acc[LS_C + 1] = cb; acc[LS_C + 2] = edge ? ca : 0.0;
  acc[LS_NBI] = (double)nb;
  acc[LS_NEDGE] = edge ? 1.0 : 0.0;
  // the five gradient planes back at S: level 0 is read as it stands, the others are bilinear samples of the coarse planes
  float total[3] = {0.f, 0.f, 0.f};
  for (int l = 0; l < kLossLevels; ++l) {
    const int s = loss_level_side(S, l);
    const float* pl = sc.coarse + (size_t)loss_level_offset(S, l) * 6;
    float v[6];
    if (l == 0) {
      for (int j = 0; j < 6; ++j) v[j] = pl[p1 * 6 + j];
    } else {
      const BilinearTap t(y, x, S, s);
      const float* a = pl + ((size_t)t.y0 * s + t.x0) * 6;
      const float* b = pl + ((size_t)t.y0 * s + t.x1) * 6;
      const float* c = pl + ((size_t)t.y1 * s + t.x0) * 6;
      const float* d = pl + ((size_t)t.y1 * s + t.x1) * 6;
      for (int j = 0; j < 6; ++j) v[j] = t.lerp(a[j], b[j], c[j], d[j]);
    }
    for (int c = 0; c < 3; ++c) {
      const float a = fabsf(v[3 + c] - v[c]);
      const float d = ((a + (30.0f * a) * (bi[c] ? 1.0f : 0.f)) + (10.0f * a) * (edge ? 1.0f : 0.f)) / 41.0f;
      total[c] = l == 0 ? d : total[c] + d;
    }
  }
  if (dif_grad != nullptr)
    for (int c = 0; c < 3; ++c) dif_grad[q + c] = total[c] / 1.2f;
  acc[LS_DG] = ((double)total[0] + (double)total[1]) + (double)total[2];
  // the wave's 64 pixels by a butterfly of cross-lane moves, then the four waves in index order
  const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int k = 0; k < kLossK; ++k) {
    double v = acc[k];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if (lane == 0) s_red[wave][k] = v;
  }
  __syncthreads();
  if (tid < kLossK) sc.slots[(size_t)blockIdx.x * kLossK + tid] = ((s_red[0][tid] + s_red[1][tid]) + s_red[2][tid]) + s_red[3][tid];
}

// t[K] (the batch totals) -> recon_gs, recon_c, grad in float64, in train_losses.losses_from_sums' order
__device__ inline void loss_formulas(const double* t, double n, float* losses3) {
#pragma clang fp contract(off)
  const double d_bi = t[LS_NBI] + 1e-6, d_edge = t[LS_NEDGE] + 1e-6;
  const double recon_gs = ((t[LS_GS] / n + (t[LS_GS + 1] / d_bi) * 30.0) + (t[LS_GS + 2] / d_edge) * 10.0) / 41.0;
  const double l1 = t[LS_C] / (n * 3.0), l1_bi = t[LS_C + 1] / d_bi / 3.0, l1_edge = t[LS_C + 2] / d_edge / 3.0;
  const double yuv_all = ((t[LS_Y] / n + t[LS_U] / n) + t[LS_V] / n) / 2.0;
  const double yuv_bi = ((t[LS_Y + 1] / d_bi + t[LS_U + 1] / d_bi) + t[LS_V + 1] / d_bi) / 2.0;
  const double yuv_edge = ((t[LS_Y + 2] / d_edge + t[LS_U + 2] / d_edge) + t[LS_V + 2] / d_edge) / 2.0;
  const double recon_c = (((((l1 + l1_bi * 30.0) + l1_edge * 10.0) + yuv_all) + yuv_bi * 30.0) + yuv_edge * 10.0) / 82.0;
  losses3[0] = (float)recon_gs;
  losses3[1] = (float)recon_c;
  losses3[2] = (float)(t[LS_DG] / d_edge);
}

__global__ __launch_bounds__(256) void losses_finish_kernel(int B, int S, void* scratch, double* sums, float* losses3) {      // grid (1)
#pragma clang fp contract(off)
  __shared__ double s_tot[kLossK];
  const int tid = threadIdx.x, tiles = loss_tiles(S);
  for (int i = tid; i < B * kLossK; i += 256) {
    const int item = i / kLossK, k = i % kLossK;
    const double* slots = item_scratch<LossScratch>(scratch, item, S).slots;
    double a = 0.0;
    for (int t = 0; t < tiles; ++t) a += slots[(size_t)t * kLossK + k];
    sums[i] = a;
  }
  __syncthreads();                                   // sums[] was written by this workgroup: visible to it after the barrier
  if (tid < kLossK) {
    double a = 0.0;
    for (int item = 0; item < B; ++item) a += sums[(size_t)item * kLossK + tid];
    s_tot[tid] = a;
  }
  __syncthreads();
  if (tid == 0) loss_formulas(s_tot, (double)B * (double)S * (double)S, losses3);
}

inline hipError_t launch_train_losses(const float* img, const float* gt, const float* mask_sv, const float* gs, const float* con, int B, int S, double* sums,
                                      float* losses3, float* mask_edge, float* bmaskgt, float* dif_grad, void* scratch, hipStream_t stream) {
  hipLaunchKernelGGL(losses_coarse_kernel, dim3((unsigned)((loss_coarse_pixels(S) + 255) / 256), (unsigned)B), dim3(256), 0, stream, gt, con, S, scratch);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(losses_pixel_kernel, dim3((unsigned)loss_tiles(S), (unsigned)B), dim3(256), 0, stream, img, gt, mask_sv, gs, con, S, scratch, mask_edge,
                     bmaskgt, dif_grad);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(losses_finish_kernel, dim3(1), dim3(256), 0, stream, B, S, scratch, sums, losses3);
  return hipGetLastError();
}

}  // namespace bsr
