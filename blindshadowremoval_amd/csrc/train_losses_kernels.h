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

// the six coarse planes of level l (gt's three channels, then con_rgb's) back at S, at fine pixel (y, x): level 0 is read as it stands,
// the others are bilinear samples of the coarse planes
__device__ inline void loss_level_samples(const float* __restrict__ coarse, int S, int l, int y, int x, float* v) {
  const int s = loss_level_side(S, l);
  const float* pl = coarse + (size_t)loss_level_offset(S, l) * 6;
  if (l == 0) {
    for (int j = 0; j < 6; ++j) v[j] = pl[((size_t)y * S + x) * 6 + j];
  } else {
    const BilinearTap t(y, x, S, s);
    const float* a = pl + ((size_t)t.y0 * s + t.x0) * 6;
    const float* b = pl + ((size_t)t.y0 * s + t.x1) * 6;
    const float* c = pl + ((size_t)t.y1 * s + t.x0) * 6;
    const float* d = pl + ((size_t)t.y1 * s + t.x1) * 6;
    for (int j = 0; j < 6; ++j) v[j] = t.lerp(a[j], b[j], c[j], d[j]);
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
    float v[6];
    loss_level_samples(sc.coarse, S, l, y, x, v);
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

__global__ __launch_bounds__(256) void losses_finish_kernel(int B, int S, void* scratch, double* sums, float* losses3, double* totals) {      // grid (1)
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
  if (totals != nullptr && tid < kLossK) totals[tid] = s_tot[tid];          // the backward reads n_bi and n_edge here
}

inline hipError_t launch_train_losses(const float* img, const float* gt, const float* mask_sv, const float* gs, const float* con, int B, int S, double* sums,
                                      float* losses3, float* mask_edge, float* bmaskgt, float* dif_grad, void* scratch, hipStream_t stream,
                                      double* totals = nullptr) {
  hipLaunchKernelGGL(losses_coarse_kernel, dim3((unsigned)((loss_coarse_pixels(S) + 255) / 256), (unsigned)B), dim3(256), 0, stream, gt, con, S, scratch);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(losses_pixel_kernel, dim3((unsigned)loss_tiles(S), (unsigned)B), dim3(256), 0, stream, img, gt, mask_sv, gs, con, S, scratch, mask_edge,
                     bmaskgt, dif_grad);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(losses_finish_kernel, dim3(1), dim3(256), 0, stream, B, S, scratch, sums, losses3, totals);
  return hipGetLastError();
}

// ---- THE BACKWARD: d (u_gs recon_gs + u_c recon_c + u_g grad) / d (gs, con_rgb), train_losses.step_losses_grad.  The forward's three
// launches run first, with mask_edge and the batch totals left in the gradient part of the scratch; then three more on the same stream:
//   losses_sign_kernel     grid (S^2 / 256, B), a thread per pixel: the forward's float32 samples of the ten planes once more (the same
//                          device function, so the same bits) and the sign of each of the 15 differences.  Level 0 needs no resize:
//                          g_0 = D_0 is written as it stands.  The 12 signs of levels 1..4, the pixel's three mask_bi bits and its
//                          mask_edge bit go into ONE 32-bit word (two bits per sign): D_l is never stored.
//   losses_upT_kernel      grid (S/2 + S/4 + S/8 + S/16, B), a workgroup per coarse row of a level: U_l^T as a separable GATHER.  The row
//                          pass sums, for every fine row the coarse row receives from and every coarse column, the fine pixels of that
//                          column's footprint (2 scale of them, 1.5 scale at a clamped edge; the weights tabulated once per workgroup
//                          from BilinearTap) in index order into LDS; the column pass
//                          sums the rows in index order.  float64 throughout, the map g_l is stored as float32.
//   losses_grad_kernel     grid (S^2 / 256, B), a thread per pixel: grad_gs and d_recon_c in float64 in the statement's order (bit-identical
//                          to it); the transpose of (dy + dx) * 5 read off g_l at the one coarse pixel per level whose 2 x 2 quarter
//                          taps hold this pixel (R_l^T as a gather); grad_con = d_recon_c + d_grad added in float64, rounded once.
// No atomics, every sum in a fixed order, every scratch word read was written earlier in the same call.
struct LossGradScratch {                 // per batch, behind the forward's B items
  double* totals;                        // [K]: the batch totals the forward's finish kernel formed
  float* mask_edge;                      // [B][S][S]
  uint32_t* words;                       // [B][S][S]: bits 0..23 the signs of levels 1..4 (0: zero, 1: plus, 2: minus), 24..26 mask_bi, 27 mask_edge
  float* g[kLossLevels];                 // [B][s][s][3]
  __host__ __device__ static LossGradScratch carve(ScratchCarver& c, int B, int S) {
    LossGradScratch s;
    s.totals = c.take<double>(32);                     // K of them, the block padded to 256 bytes
    s.mask_edge = c.take<float>((size_t)B * S * S);
    s.words = c.take<uint32_t>((size_t)B * S * S);
    for (int l = 0; l < kLossLevels; ++l) s.g[l] = c.take<float>((size_t)B * loss_level_side(S, l) * loss_level_side(S, l) * 3);
    return s;
  }
};
__host__ __device__ inline LossGradScratch loss_grad_scratch(void* base, int B, int S) {
  ScratchCarver c{static_cast<unsigned char*>(base) + (size_t)B * loss_item_scratch_bytes(S)};
  return LossGradScratch::carve(c, B, S);
}
__host__ __device__ inline size_t loss_grad_scratch_bytes(int B, int S) {
  ScratchCarver c{nullptr};
  LossGradScratch::carve(c, B, S);
  return (size_t)B * loss_item_scratch_bytes(S) + c.end();
}
__host__ __device__ inline size_t loss_grad_map_offset(int B, int S, int l) {
  return (size_t)reinterpret_cast<uintptr_t>(loss_grad_scratch(nullptr, B, S).g[l]);          // carved from a null base: the pointer is the offset
}
__host__ __device__ inline int loss_up_rows(int S) { return (S >> 1) + (S >> 2) + (S >> 3) + (S >> 4); }

__device__ inline int loss_sign(float d) { return (d > 0.f ? 1 : 0) - (d < 0.f ? 1 : 0); }
// ((1 + 30 bi_c) + 10 e) / 41: a difference's weight in dif_grad
__device__ inline double loss_grad_weight(int bi, int e) {
#pragma clang fp contract(off)
  return ((1.0 + 30.0 * (double)bi) + 10.0 * (double)e) / 41.0;
}
// what coarse index `coarse` receives from fine index `fine` along one axis of the resize s -> S
__device__ inline double loss_up_weight(int fine, int coarse, int S, int s) {
  const BilinearTap t(fine, fine, S, s);
  return (t.y0 == coarse ? 1.0 - (double)t.yl : 0.0) + (t.y1 == coarse ? (double)t.yl : 0.0);
}
// the fine indices [lo, hi) whose taps can hold coarse index c
__device__ inline void loss_up_range(int c, int scale, int S, int& lo, int& hi) {
  lo = max(scale * c - scale / 2, 0);
  hi = min(scale * c + 3 * scale / 2, S);
}

__global__ __launch_bounds__(256) void losses_sign_kernel(const float* __restrict__ mask_sv, int B, int S, void* scratch) {
#pragma clang fp contract(off)
  const int item = blockIdx.y, p1 = blockIdx.x * 256 + threadIdx.x;
  const int y = p1 / S, x = p1 % S;
  const size_t px = (size_t)item * S * S + p1;
  const LossScratch sc = item_scratch<LossScratch>(scratch, item, S);
  const LossGradScratch gsc = loss_grad_scratch(scratch, B, S);
  const double d_edge = gsc.totals[LS_NEDGE] + 1e-6;
  const int e = gsc.mask_edge[px] != 0.f ? 1 : 0;
  int bi[3];
  uint32_t word = (uint32_t)e << 27;
  for (int c = 0; c < 3; ++c) { bi[c] = mask_sv[px * 3 + c] > 0.01f ? 1 : 0; word |= (uint32_t)bi[c] << (24 + c); }
  for (int l = 0; l < kLossLevels; ++l) {
    float v[6];
    loss_level_samples(sc.coarse, S, l, y, x, v);
    for (int c = 0; c < 3; ++c) {
      const int sg = loss_sign(v[3 + c] - v[c]);
      if (l == 0) gsc.g[0][px * 3 + c] = (float)(((double)sg * loss_grad_weight(bi[c], e)) / d_edge);
      else word |= (uint32_t)(sg > 0 ? 1 : (sg < 0 ? 2 : 0)) << (2 * ((l - 1) * 3 + c));
    }
  }
  gsc.words[px] = word;
}

__global__ __launch_bounds__(256) void losses_upT_kernel(int B, int S, void* scratch) {
#pragma clang fp contract(off)
  __shared__ double s_t[6 * 256];              // [rows <= 2 scale][s][3]: 6 S doubles at most
  __shared__ double s_w[4];                    // weight / d_edge by (bi, e)
  __shared__ double s_wx[2 * 256];             // [s][2 scale]: what coarse column cx receives from fine column scale cx - scale / 2 + j
  const int item = blockIdx.y, tid = threadIdx.x;
  int l = 1, cy = blockIdx.x;
  while (cy >= (S >> l)) { cy -= S >> l; ++l; }
  const int s = S >> l, scale = 1 << l;
  const LossGradScratch gsc = loss_grad_scratch(scratch, B, S);
  if (tid < 4) s_w[tid] = loss_grad_weight(tid >> 1, tid & 1) / (gsc.totals[LS_NEDGE] + 1e-6);
  for (int i = tid; i < 2 * S; i += 256) {
    const int cx = i / (2 * scale), x = scale * cx - scale / 2 + i % (2 * scale);
    s_wx[i] = x >= 0 && x < S ? loss_up_weight(x, cx, S, s) : 0.0;
  }
  __syncthreads();
  int ylo, yhi;
  loss_up_range(cy, scale, S, ylo, yhi);
  const int rows = yhi - ylo;
  const uint32_t* words = gsc.words + (size_t)item * S * S;
  for (int i = tid; i < rows * s; i += 256) {              // the row pass: a thread per (fine row, coarse column), its three channels
    const int cx = i % s, y = ylo + i / s;
    const int shift = 6 * (l - 1);
    int xlo, xhi;
    loss_up_range(cx, scale, S, xlo, xhi);
    const double* wx = s_wx + (scale * cx + scale / 2);          // cx's row of the table, indexed by the fine column: 2 scale cx - (scale cx - scale / 2)
    double acc[3] = {0.0, 0.0, 0.0};
    for (int x = xlo; x < xhi; ++x) {
      const uint32_t w = words[(size_t)y * S + x];
      const uint32_t e = (w >> 27) & 1u;
      const double wgt = wx[x];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const uint32_t code = (w >> (shift + 2 * c)) & 3u;
        const double d = s_w[(((w >> (24 + c)) & 1u) << 1) | e];
        acc[c] += wgt * (code == 1u ? d : (code == 2u ? -d : 0.0));
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) s_t[(size_t)i * 3 + c] = acc[c];
  }
  __syncthreads();
  for (int i = tid; i < s * 3; i += 256) {                 // the column pass
    const int c = i % 3, cx = i / 3;
    double acc = 0.0;
    for (int r = 0; r < rows; ++r) acc += loss_up_weight(ylo + r, cy, S, s) * s_t[((size_t)r * s + cx) * 3 + c];
    gsc.g[l][(((size_t)item * s + cy) * s + cx) * 3 + c] = (float)acc;
  }
}

// rbar[i, j] of channel c of one item's map g [s][s][3]: the transpose of (dy + dx) * 5 with its zero last row and last column
__device__ inline double loss_diff_t(const float* __restrict__ g, int s, int i, int j, int c) {
#pragma clang fp contract(off)
  const double own = (double)g[((size_t)i * s + j) * 3 + c];
  const double up = i >= 1 ? (double)g[((size_t)(i - 1) * s + j) * 3 + c] : 0.0;
  const double left = j >= 1 ? (double)g[((size_t)i * s + j - 1) * 3 + c] : 0.0;
  return 5.0 * (((up - (i + 1 < s ? own : 0.0)) + left) - (j + 1 < s ? own : 0.0));
}

__global__ __launch_bounds__(256) void losses_grad_kernel(const float* __restrict__ gt, const float* __restrict__ mask_sv, const float* __restrict__ gs,
                                                          const float* __restrict__ con, const float* __restrict__ upstream, int B, int S, void* scratch,
                                                          float* __restrict__ grad_gs, float* __restrict__ grad_con, float* __restrict__ d_recon_c,
                                                          float* __restrict__ d_grad) {
#pragma clang fp contract(off)
  const int item = blockIdx.y, p1 = blockIdx.x * 256 + threadIdx.x;
  const int y = p1 / S, x = p1 % S;
  const size_t px = (size_t)item * S * S + p1, q = px * 3;
  const LossGradScratch gsc = loss_grad_scratch(scratch, B, S);
  const double u_gs = upstream != nullptr ? (double)upstream[0] : 1.0, u_c = upstream != nullptr ? (double)upstream[1] : 1.0,
               u_g = upstream != nullptr ? (double)upstream[2] : 1.0;
  const double n = (double)B * (double)S * (double)S, d_bi = gsc.totals[LS_NBI] + 1e-6, d_edge = gsc.totals[LS_NEDGE] + 1e-6;
  const double e = gsc.mask_edge[px] != 0.f ? 1.0 : 0.0;
  float g3[3], c3[3];
  double bi[3], nb = 0.0;
  for (int c = 0; c < 3; ++c) { g3[c] = gt[q + c]; c3[c] = con[q + c]; bi[c] = mask_sv[q + c] > 0.01f ? 1.0 : 0.0; }
  nb = (bi[0] + bi[1]) + bi[2];
  const double w1 = (1.0 / n + (30.0 * nb) / d_bi) + (10.0 * e) / d_edge;
  grad_gs[px] = (float)(((u_gs * (double)loss_sign(gs[px] - loss_gray(g3))) * w1) / 41.0);
  const float yuv_w[3][3] = {{.299f, .587f, .114f}, {-.168736f, -.331264f, .5f}, {.5f, -.418688f, -.081312f}};
  double sk[3];
  for (int k = 0; k < 3; ++k)
    sk[k] = (double)loss_sign(loss_weighted(c3, yuv_w[k][0], yuv_w[k][1], yuv_w[k][2]) - loss_weighted(g3, yuv_w[k][0], yuv_w[k][1], yuv_w[k][2]));
  for (int c = 0; c < 3; ++c) {
    const double a_c = (1.0 / (3.0 * n) + (30.0 * bi[c]) / (3.0 * d_bi)) + (10.0 * e) / (3.0 * d_edge);
    const double yuv_c = (sk[0] * (double)yuv_w[0][c] + sk[1] * (double)yuv_w[1][c]) + sk[2] * (double)yuv_w[2][c];
    const double rc = (u_c * ((double)loss_sign(c3[c] - g3[c]) * a_c + (yuv_c * w1) / 2.0)) / 82.0;
    double acc = loss_diff_t(gsc.g[0] + (size_t)item * S * S * 3, S, y, x, c);
    for (int l = 1; l < kLossLevels; ++l) {
      const int scale = 1 << l, s = S >> l, ry = y & (scale - 1), rx = x & (scale - 1);
      const bool hit = (ry == scale / 2 - 1 || ry == scale / 2) && (rx == scale / 2 - 1 || rx == scale / 2);
      acc = acc + (hit ? 0.25 * loss_diff_t(gsc.g[l] + (size_t)item * s * s * 3, s, y >> l, x >> l, c) : 0.0);
    }
    const double dg = u_g * acc;
    grad_con[q + c] = (float)(rc + dg);
    if (d_recon_c != nullptr) d_recon_c[q + c] = (float)rc;
    if (d_grad != nullptr) d_grad[q + c] = (float)dg;
  }
}

inline hipError_t launch_train_losses_grad(const float* img, const float* gt, const float* mask_sv, const float* gs, const float* con, const float* upstream,
                                           int B, int S, double* sums, float* losses3, float* grad_gs, float* grad_con, float* d_recon_c, float* d_grad,
                                           void* scratch, hipStream_t stream) {
  const LossGradScratch gsc = loss_grad_scratch(scratch, B, S);
  hipError_t e = launch_train_losses(img, gt, mask_sv, gs, con, B, S, sums, losses3, gsc.mask_edge, nullptr, nullptr, scratch, stream, gsc.totals);
  if (e != hipSuccess) return e;
  const dim3 pixels((unsigned)(S * S / 256), (unsigned)B);
  hipLaunchKernelGGL(losses_sign_kernel, pixels, dim3(256), 0, stream, mask_sv, B, S, scratch);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(losses_upT_kernel, dim3((unsigned)loss_up_rows(S), (unsigned)B), dim3(256), 0, stream, B, S, scratch);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(losses_grad_kernel, pixels, dim3(256), 0, stream, gt, mask_sv, gs, con, upstream, B, S, scratch, grad_gs, grad_con, d_recon_c, d_grad);
  return hipGetLastError();
}

}  // namespace bsr
