// The three multi-scale patch discriminators of the reference's train_step and its three GAN losses ON THE DEVICE: gen, disc_real and
// disc_fake (train_test_GSC.py:264-268, 302, 334-336; model.py:115-147, 292-312; utils.py:100-102), training=False.
// blindshadowremoval_amd/discriminator.py is the host statement and writes the arithmetic out; pack.pack_discriminators writes the
// weight blob (BatchNormalization folded, the first layer's 6 input channels padded to 8).
//
// One chain of seven launches on the caller's stream, no host synchronisation, no parallel branch, no floating-point atomic; every
// word of scratch that a launch reads was written by an earlier launch of the same call.
//   disc_input_kernel    a thread per pixel of the three inputs [2B][s][s][8], s = S, S / 2, S / 4: rows [0, B) from gt, rows [B, 2B) from
//                        con_rgb, mask_sv under both; channels 6, 7 are written as 0.  The 1/2 and 1/4 inputs are tf.image.resize's
//                        bilinear taps (one lerp of 0.5 per axis) with contraction off: bit-identical to the host statement.
//   disc_conv_kernel     x 4, one launch per layer for all three discriminators: the workgroup index maps to (discriminator, row,
//                        tile) and selects the weight set.  4 x 4, stride 2, SAME padding (1 before on every size that occurs) as an
//                        implicit GEMM on v_mfma_f32_32x32x2_f32: a workgroup of four waves owns an 8 x 16 tile of output pixels and all N
//                        output channels, a wave 2 x 16 pixels (M = 32) and N / 32 accumulator tiles.  K = 16 C_in runs in chunks of 8
//                        input channels: the 18 x 34 input patch of the chunk (halo included; padding and pixels outside the map are
//                        stored as 0) and the chunk's [16][8][N] weights go to LDS, and each tap reads the patch at a shifted address.
//                        Epilogue: bias (bias_tile) + LeakyReLU(0.3).  Output pixels outside the map are computed and not stored, so
//                        maps smaller than a tile, down to 1 x 1 -> 1 x 1, take the same path.  LDS: 22 KB + 32 KB.
//   disc_head_kernel     a workgroup per (discriminator, row): the 4 x 4 stride-1 one-channel conv (pad 1 before, 2 after) as a dot product
//                        per output pixel, a wave per pixel and a lane per input channel; writes the logits, forms the hinge terms
//                        in float32 (1 - y and 1 + y rounded once) and folds them and the fake logits in float64: wave butterfly, then
//                        the waves in index order, into the row's own words of sums[B][9].
//   disc_finish_kernel   one wave: adds the items in order and forms the three losses in float64, rounded once to float32.
#pragma once
#include "mfma_common.h"
#include "post_common.h"

namespace bsr {

constexpr int kDiscLayers = 4, kDiscCC = 8, kDiscTaps = 16, kDiscInC = 8, kDiscSums = 9;
constexpr int kDiscTH = 8, kDiscTW = 16, kDiscPH = 2 * kDiscTH + 2, kDiscPW = 2 * kDiscTW + 2, kDiscLd = kDiscCC + 1;
constexpr int kDiscMaxB = 32767;

__host__ __device__ inline int disc_ch(int i) { return i < 2 ? 32 : 64; }                      // output channels of conv_stack[i]
__host__ __device__ inline int disc_cin(int i) { return i == 0 ? kDiscInC : disc_ch(i - 1); }
// float offset of layer i's weights (i = 4: the head) inside one discriminator's record: pack.disc_layout
__host__ __device__ inline size_t disc_w_off(int i) {
  size_t o = 0;
  for (int j = 0; j < i; ++j) o += (size_t)kDiscTaps * disc_cin(j) * disc_ch(j) + disc_ch(j);
  return o;
}
__host__ __device__ inline size_t disc_record_floats() { return disc_w_off(kDiscLayers) + (size_t)kDiscTaps * disc_ch(kDiscLayers - 1) + 4; }
// side of map l of discriminator k (0-based): l = 0 its input, 1..4 the stride-2 outputs, 5 the head's output
__host__ __device__ inline int disc_side(int S, int k, int l) {
  int s = S >> k;
  for (int i = 0; i < l && i < kDiscLayers; ++i) s = (s + 1) / 2;
  return s;
}
__host__ __device__ inline int disc_map_ch(int l) { return l == 0 ? kDiscInC : l <= kDiscLayers ? disc_ch(l - 1) : 1; }
__host__ __device__ inline size_t disc_map_bytes(int B, int S, int k, int l) {
  const size_t s = (size_t)disc_side(S, k, l);
  return ((size_t)2 * B * s * s * disc_map_ch(l) * sizeof(float) + 255) & ~size_t(255);
}
// byte offset of map l of discriminator k inside the scratch; (3, 0) is the total
__host__ __device__ inline size_t disc_map_offset(int B, int S, int k, int l) {
  size_t o = 0;
  for (int kk = 0; kk < 3; ++kk)
    for (int ll = 0; ll <= kDiscLayers + 1; ++ll) {
      if (kk == k && ll == l) return o;
      o += disc_map_bytes(B, S, kk, ll);
    }
  return o;
}
__host__ __device__ inline float* disc_map(void* scratch, int B, int S, int k, int l) {
  return reinterpret_cast<float*>(static_cast<unsigned char*>(scratch) + disc_map_offset(B, S, k, l));
}

__global__ __launch_bounds__(256) void disc_input_kernel(const float* __restrict__ gt, const float* __restrict__ con, const float* __restrict__ mask_sv, int B,
                                                         int S, float* __restrict__ in0, float* __restrict__ in1, float* __restrict__ in2) {
#pragma clang fp contract(off)
  const size_t n0 = (size_t)2 * B * S * S, n1 = n0 / 4, n2 = n0 / 16;
  size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= n0 + n1 + n2) return;
  int k = 0;
  float* dst = in0;
  if (p >= n0 + n1) { k = 2; p -= n0 + n1; dst = in2; }
  else if (p >= n0) { k = 1; p -= n0; dst = in1; }
  const int s = S >> k;
  const int x = (int)(p % s), y = (int)((p / s) % s), row = (int)(p / ((size_t)s * s));
  const size_t item = (size_t)(row < B ? row : row - B) * S * S * 3;
  const float* im = (row < B ? gt : con) + item;
  const float* mk = mask_sv + item;
  float v[8];
  if (k == 0) {
    const size_t q = ((size_t)y * S + x) * 3;
    for (int c = 0; c < 3; ++c) { v[c] = im[q + c]; v[3 + c] = mk[q + c]; }
  } else {
    const BilinearTap t(y, x, s, S);
    const size_t a = ((size_t)t.y0 * S + t.x0) * 3, b = ((size_t)t.y0 * S + t.x1) * 3, c_ = ((size_t)t.y1 * S + t.x0) * 3, d = ((size_t)t.y1 * S + t.x1) * 3;
    for (int c = 0; c < 3; ++c) {
      v[c] = t.lerp(im[a + c], im[b + c], im[c_ + c], im[d + c]);
      v[3 + c] = t.lerp(mk[a + c], mk[b + c], mk[c_ + c], mk[d + c]);
    }
  }
  v[6] = v[7] = 0.f;
  f32x4* o = reinterpret_cast<f32x4*>(dst + p * kDiscInC);
  o[0] = f32x4{v[0], v[1], v[2], v[3]};
  o[1] = f32x4{v[4], v[5], v[6], v[7]};
}

struct DiscConvSet {
  const float* in;        // [2B][H][H][CIN]
  float* out;             // [2B][Ho][Ho][N]
  const float* w;         // [CIN / 8][16][8][N]
  const float* bias;      // [N]
  int H, Ho, tiles_x, tiles;          // tiles per row = tiles_x * tiles_y
  unsigned first_block;               // the set's first workgroup index
};
struct DiscConvArgs { DiscConvSet d[3]; };

template <int CIN, int N>
__global__ __launch_bounds__(256) void disc_conv_kernel(const DiscConvArgs args) {
  static_assert(CIN % kDiscCC == 0 && N % 32 == 0, "shape");
  constexpr int NT = N / 32;
  __shared__ float s_in[kDiscPH * kDiscPW * kDiscLd];
  __shared__ __attribute__((aligned(16))) float s_w[kDiscTaps * kDiscCC * N];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int k = blockIdx.x >= args.d[2].first_block ? 2 : blockIdx.x >= args.d[1].first_block ? 1 : 0;
  const DiscConvSet& d = args.d[k];
  const unsigned r = blockIdx.x - d.first_block;
  const int row = (int)(r / (unsigned)d.tiles), tile = (int)(r % (unsigned)d.tiles);
  const int oy0 = (tile / d.tiles_x) * kDiscTH, ox0 = (tile % d.tiles_x) * kDiscTW;
  const int iy0 = 2 * oy0 - 1, ix0 = 2 * ox0 - 1;                      // SAME, stride 2, 4 taps: 1 before on even sizes and on 1 x 1
  const int H = d.H, Ho = d.Ho;
  const float* in = d.in + (size_t)row * H * H * CIN;
  const int m = lane & 31, kh = lane >> 5;
  const int a_base = ((2 * (wave * 2 + (m >> 4))) * kDiscPW + 2 * (m & 15)) * kDiscLd + kh;        // the wave's pixel m, tap (0, 0), channel kh

  f32x16 acc[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) acc[nt] = bias_tile(kh, d.bias[nt * 32 + m]);

  for (int c0 = 0; c0 < CIN; c0 += kDiscCC) {
    if (c0 != 0) __syncthreads();
    for (int i = tid; i < kDiscPH * kDiscPW * 2; i += 256) {
      const int pix = i >> 1, half = i & 1;
      const int iy = iy0 + pix / kDiscPW, ix = ix0 + pix % kDiscPW;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (iy >= 0 && iy < H && ix >= 0 && ix < H) v = *reinterpret_cast<const f32x4*>(in + ((size_t)iy * H + ix) * CIN + c0 + half * 4);
      float* dst = s_in + pix * kDiscLd + half * 4;
      dst[0] = v[0]; dst[1] = v[1]; dst[2] = v[2]; dst[3] = v[3];
    }
    const f32x4* wsrc = reinterpret_cast<const f32x4*>(d.w + (size_t)(c0 / kDiscCC) * kDiscTaps * kDiscCC * N);
    for (int i = tid; i < kDiscTaps * kDiscCC * N / 4; i += 256) reinterpret_cast<f32x4*>(s_w)[i] = wsrc[i];
    __syncthreads();
#pragma unroll
    for (int tap = 0; tap < kDiscTaps; ++tap) {
      const float* ap = s_in + a_base + ((tap >> 2) * kDiscPW + (tap & 3)) * kDiscLd;
      const float* bp = s_w + (tap * kDiscCC + kh) * N + m;
#pragma unroll
      for (int k2 = 0; k2 < kDiscCC / 2; ++k2) {
        const float av = ap[2 * k2];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bp[2 * k2 * N + nt * 32], acc[nt], 0, 0, 0);
      }
    }
  }
  float* out = d.out + (size_t)row * Ho * Ho * N;
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    leaky_relu_tile(acc[nt], kLeakyAlpha);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int mr = (i & 3) + 8 * (i >> 2) + 4 * kh;                  // the accumulator's row: pixel mr of the wave
      const int oy = oy0 + wave * 2 + (mr >> 4), ox = ox0 + (mr & 15);
      if (oy < Ho && ox < Ho) out[((size_t)oy * Ho + ox) * N + nt * 32 + m] = acc[nt][i];
    }
  }
}

// grid (3 * 2B): workgroup (k, row).  x: the last conv's output [2B][h][h][64]; w: [16][64], then the bias.
__global__ __launch_bounds__(256) void disc_head_kernel(const float* __restrict__ blob, int B, int S, void* scratch, double* __restrict__ sums,
                                                        float* __restrict__ logits) {
#pragma clang fp contract(off)
  __shared__ float s_logit[256];
  __shared__ double s_red[4][2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int k = blockIdx.x / (2 * B), row = blockIdx.x % (2 * B);
  const int h = disc_side(S, k, kDiscLayers), hh = h * h;               // h <= 16
  const float* w = blob + (size_t)k * disc_record_floats() + disc_w_off(kDiscLayers);
  const float* x = disc_map(scratch, B, S, k, kDiscLayers) + (size_t)row * hh * 64;
  float wl[kDiscTaps];
#pragma unroll
  for (int t = 0; t < kDiscTaps; ++t) wl[t] = w[t * 64 + lane];
  const float bias = w[kDiscTaps * 64];
  for (int p = wave; p < hh; p += 4) {
    const int oy = p / h, ox = p % h;
    float a = 0.f;
#pragma unroll
    for (int t = 0; t < kDiscTaps; ++t) {
      const int iy = oy + (t >> 2) - 1, ix = ox + (t & 3) - 1;           // SAME, stride 1, 4 taps: 1 before, 2 after
      if (iy >= 0 && iy < h && ix >= 0 && ix < h) a = __builtin_fmaf(x[((size_t)iy * h + ix) * 64 + lane], wl[t], a);
    }
    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
    if (lane == 0) s_logit[p] = a + bias;
  }
  __syncthreads();
  const bool real = row < B;
  double hinge = 0.0, plain = 0.0;
  if (tid < hh) {
    const float y = s_logit[tid];
    disc_map(scratch, B, S, k, kDiscLayers + 1)[(size_t)row * hh + tid] = y;
    if (logits != nullptr) {
      size_t off = 0;
      for (int j = 0; j < k; ++j) { const size_t hj = (size_t)disc_side(S, j, kDiscLayers); off += (size_t)2 * B * hj * hj; }
      logits[off + (size_t)row * hh + tid] = y;
    }
    const float t = real ? 1.0f - y : 1.0f + y;
    hinge = (double)fmaxf(0.f, t);
    plain = (double)y;
  }
  for (int o = 32; o > 0; o >>= 1) { hinge += __shfl_xor(hinge, o); plain += __shfl_xor(plain, o); }
  if (lane == 0) { s_red[wave][0] = hinge; s_red[wave][1] = plain; }
  __syncthreads();
  if (tid == 0) {
    double* dst = sums + (size_t)(real ? row : row - B) * kDiscSums + k * 3;
    dst[real ? 0 : 1] = ((s_red[0][0] + s_red[1][0]) + s_red[2][0]) + s_red[3][0];
    if (!real) dst[2] = ((s_red[0][1] + s_red[1][1]) + s_red[2][1]) + s_red[3][1];
  }
}

__global__ __launch_bounds__(64) void disc_finish_kernel(int B, int S, const double* __restrict__ sums, float* __restrict__ losses3) {      // grid (1)
#pragma clang fp contract(off)
  __shared__ double s_t[kDiscSums];
  const int tid = threadIdx.x;
  if (tid < kDiscSums) {
    double a = 0.0;
    for (int item = 0; item < B; ++item) a = a + sums[(size_t)item * kDiscSums + tid];
    s_t[tid] = a;
  }
  __syncthreads();
  if (tid == 0) {
    double n[3];
    for (int k = 0; k < 3; ++k) { const double h = (double)disc_side(S, k, kDiscLayers); n[k] = (double)B * h * h; }
    losses3[0] = (float)((-(s_t[2] / n[0]) - s_t[5] / n[1]) - s_t[8] / n[2]);
    losses3[1] = (float)((s_t[0] / n[0] + s_t[3] / n[1]) + s_t[6] / n[2]);
    losses3[2] = (float)((s_t[1] / n[0] + s_t[4] / n[1]) + s_t[7] / n[2]);
  }
}

template <int CIN, int N>
inline hipError_t launch_disc_conv(const float* blob, int layer, int B, int S, void* scratch, hipStream_t stream) {
  DiscConvArgs a;
  unsigned blocks = 0;
  for (int k = 0; k < 3; ++k) {
    DiscConvSet& d = a.d[k];
    const float* rec = blob + (size_t)k * disc_record_floats() + disc_w_off(layer);
    d.in = disc_map(scratch, B, S, k, layer);
    d.out = disc_map(scratch, B, S, k, layer + 1);
    d.w = rec;
    d.bias = rec + (size_t)kDiscTaps * CIN * N;
    d.H = disc_side(S, k, layer);
    d.Ho = disc_side(S, k, layer + 1);
    d.tiles_x = (d.Ho + kDiscTW - 1) / kDiscTW;
    d.tiles = d.tiles_x * ((d.Ho + kDiscTH - 1) / kDiscTH);
    d.first_block = blocks;
    blocks += (unsigned)(2 * B) * (unsigned)d.tiles;
  }
  hipLaunchKernelGGL((disc_conv_kernel<CIN, N>), dim3(blocks), dim3(256), 0, stream, a);
  return hipGetLastError();
}

inline hipError_t launch_disc_losses(const float* blob, const float* gt, const float* con, const float* mask_sv, int B, int S, double* sums, float* losses3,
                                     float* logits, void* scratch, hipStream_t stream) {
  const size_t pixels = (size_t)2 * B * S * S / 16 * 21;                 // 1 + 1/4 + 1/16
  hipLaunchKernelGGL(disc_input_kernel, dim3((unsigned)((pixels + 255) / 256)), dim3(256), 0, stream, gt, con, mask_sv, B, S, disc_map(scratch, B, S, 0, 0),
                     disc_map(scratch, B, S, 1, 0), disc_map(scratch, B, S, 2, 0));
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if ((e = launch_disc_conv<8, 32>(blob, 0, B, S, scratch, stream)) != hipSuccess) return e;
  if ((e = launch_disc_conv<32, 32>(blob, 1, B, S, scratch, stream)) != hipSuccess) return e;
  if ((e = launch_disc_conv<32, 64>(blob, 2, B, S, scratch, stream)) != hipSuccess) return e;
  if ((e = launch_disc_conv<64, 64>(blob, 3, B, S, scratch, stream)) != hipSuccess) return e;
  hipLaunchKernelGGL(disc_head_kernel, dim3((unsigned)(3 * 2 * B)), dim3(256), 0, stream, blob, B, S, scratch, sums, logits);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(disc_finish_kernel, dim3(1), dim3(64), 0, stream, B, S, sums, losses3);
  return hipGetLastError();
}

}  // namespace bsr
