// The generator's backward pass below the non-local block, ON THE DEVICE, training=False: the lower half of res_stack/5 (and, with their
// weights, of blocks 3 and 4, whose shapes are the same) — conv1/bnorm1/relu1 (1x1, 261 -> 128), conv2/bnorm2/relu2 (3x3, 128 -> 128),
// conv3/bnorm3 (1x1, 128 -> 257) and the sum with what the skip carries.  Given the block's input xin, d_y3 = d loss / d (bnorm3's
// output) and d_skip (or none) it writes d_xin and the twelve variable gradients.  blindshadowremoval_amd/generator_grad.py is the host
// statement (bottleneck_grad); pack.pack_bottleneck_grad writes the blob.
//
// The chain is a template on X, the width of the block's input: 261 for blocks 3..5, and for block_chain_grad.h 257 (blocks 1, 2)
// and 99 (block 0, conv1 99 -> 128).  Where the text below says 261, 272 and 384 it speaks of X, of X rounded up to 16 and of X rounded
// up to 128; the kernels that carry X in their index arithmetic are instantiated per width, the others take it as K, n_store, strides
// and grids.
//
// The chain keeps nothing of the forward but xin: a1 and a2 are formed again from the BN-folded images, so the same entry serves blocks
// 3 and 4, whose t1/t2 slots the forward has overwritten by the time it ends.
//
// N = B h w pixels (h a multiple of 4, w of 32, so N is a multiple of 128 and every 2 x 32 tile lies inside one image).  Twelve launches
// on the caller's stream, one after the other: no host synchronisation, no second stream, no floating-point atomic; every word a launch
// reads was written by the caller or by an earlier launch of the same call, and every sum runs in a fixed order, so a call repeats its
// bits.  All matrix work is v_mfma_f32_16x16x4_f32.
//    1  bn_entry_kernel      xin -> xp [N][272] and d_y3 -> dyp [N][272] (the pads 0); per 64 rows the column sums of d_y3 in float64
//    2  bn_gemm_kernel<0>    a1 = lrelu(xp w1f + b1f)                          (K = 272, N = 128)
//    3  bn_conv3_kernel<0>   a2 = lrelu(conv3x3(a1, w2f) + b2f): a 2 x 32 pixel tile per workgroup, its 4 x 34 halo through LDS sixteen
//                            channels at a time, zero outside the image; per tap a 16 x 128 weight tile
//    4  bn_gemm_kernel<1>    gz2 = LeakyReluGrad(dyp w3t, a2)                  (K = 272, N = 128)
//    5  bn_conv3_kernel<1>   gz1 = LeakyReluGrad(conv3x3(gz2, w2t), a1): the same main loop over the turned, folded kernel
//    6  bn_wgrad3_kernel     per tap and slice of rows: a1(shifted by the tap, zero outside the image)^T gz2 -> float32 partials
//    7  nl_tn_kernel         a2^T dyp   (128 x 257): float32 partials per slice of rows (nonlocal_grad_kernels.h's kernel as it is)
//    8  nl_tn_kernel         xp^T gz1   (261 x 128): likewise
//    9  bn_gemm_kernel<2>    d_xin = d_skip + gz1 w1t                          (K = 128, N = 261)
//   10  bn_colsum_kernel     per 128 rows the column sums of [gz2 | gz1] in float64 in row order
//   11  bn_fold_kernel       a thread per kernel element: the partials in index order in float64 -> Wg (float64) and d K = inv[o] Wg
//   12  bn_finish_kernel     a wave per channel: S, KW = sum K Wg -> d beta, d bias, d gamma (grad_common.h's bn_channel_grads)
#pragma once
#include "nonlocal_grad_kernels.h"

namespace bsr {

constexpr int kBnLaunches = 12;
constexpr int kBnVars = 12;
constexpr int kBnD = 128, kBnX = 261, kBnY = 257, kBnYp = 272;
constexpr int kBnMaps = 8;
constexpr int kBnK2 = 9 * kBnD * kBnD, kBnK3 = kBnD * kBnY;
constexpr int kBnChannels = 2 * kBnD + kBnY;

// What the width X of the block's input (conv1's) gives: 261 for blocks 3..5, 257 for blocks 1 and 2, 99 for block 0.  xp = X rounded
// up to the GEMMs' 16-channel steps (272, 272, 112), w1t = X rounded up to launch 9's 128-column tiles (384, 384, 128), mp = launch
// 8's partial rows, whole 64-row tiles of xp^T (320, 320, 128).
__host__ __device__ constexpr bool bn_width_ok(int X) { return X == 261 || X == 257 || X == 99; }
__host__ __device__ constexpr int bn_xp(int X) { return (X + 15) / 16 * 16; }
__host__ __device__ constexpr int bn_w1t(int X) { return (X + 127) / 128 * 128; }
__host__ __device__ constexpr int bn_mp(int X) { return (bn_xp(X) + 63) / 64 * 64; }
__host__ __device__ constexpr int bn_k1(int X) { return X * kBnD; }
__host__ __device__ constexpr int bn_kernel_elems(int X) { return bn_k1(X) + kBnK2 + kBnK3; }
static_assert(bn_xp(261) == 272 && bn_w1t(261) == 384 && bn_mp(261) == kNlTnMp, "the colour branch's widths");
static_assert(bn_xp(257) == 272 && bn_w1t(257) == 384 && bn_mp(257) == 320, "blocks 1 and 2");
static_assert(bn_xp(99) == 112 && bn_w1t(99) == 128 && bn_mp(99) == 128, "block 0");

// float offsets inside the blob; part 13: the total
__host__ __device__ inline size_t bn_blob_off(int part, int X = kBnX) {
  // 0: w1f [xp][128]  1: b1f [128]  2: w2f [9][128][128]  3: b2f [128]  4: w3t [272][128]  5: w2t [9][128][128]  6: w1t [128][w1t]
  // 7: k1 [X][128]  8: k2 [9][128][128]  9: k3 [128][257]  10: vecs1 [4][128]  11: vecs2 [4][128]  12: vecs3 [4][257]
  const size_t n[13] = {(size_t)bn_xp(X) * kBnD, kBnD, kBnK2, kBnD, (size_t)kBnYp * kBnD, kBnK2, (size_t)kBnD * bn_w1t(X), (size_t)bn_k1(X), kBnK2,
                        kBnK3, 4 * kBnD, 4 * kBnD, 4 * kBnY};
  size_t o = 0;
  for (int i = 0; i < part && i < 13; ++i) o += n[i];
  return o;
}

// float offset of variable `index` (conv1, conv2, conv3: kernel, bias; bnorm1, bnorm2, bnorm3: gamma, beta) inside grads; 12: the total
__host__ __device__ inline size_t bn_var_offset(int index, int X = kBnX) {
  const size_t n[kBnVars] = {(size_t)bn_k1(X), kBnD, kBnK2, kBnD, kBnK3, kBnY, kBnD, kBnD, kBnD, kBnD, kBnY, kBnY};
  size_t o = 0;
  for (int v = 0; v < index && v < kBnVars; ++v) o += n[v];
  return o;
}

// Byte offsets inside the scratch.  map 0: xp [N][xp], 1: dyp [N][272], 2: a1, 3: a2, 4: gz2, 5: gz1 [N][128], 6: Wg float64
// [X x 128 | 9 x 128 x 128 | 128 x 257], 7: S float64 [128 | 128 | 257] (layers 1, 2, 3).
struct BnPlan {
  int N, P;
  size_t map[kBnMaps], szpart, bpart, part1, part2, part3, total;
};
inline BnPlan bn_plan(int B, int h, int w, int X = kBnX) {
  BnPlan pl;
  BumpBytes bump;
  pl.N = B * h * w;
  const int chunks = pl.N / 128;
  pl.P = chunks < 64 ? chunks : 64;
  const size_t N = (size_t)pl.N;
  pl.map[0] = bump.take(N * bn_xp(X) * sizeof(float));
  pl.map[1] = bump.take(N * kBnYp * sizeof(float));
  for (int m = 2; m < 6; ++m) pl.map[m] = bump.take(N * kBnD * sizeof(float));
  pl.map[6] = bump.take((size_t)bn_kernel_elems(X) * sizeof(double));
  pl.map[7] = bump.take((size_t)kBnChannels * sizeof(double));
  pl.szpart = bump.take((N / 64) * kBnYp * sizeof(double));
  pl.bpart = bump.take((N / 128) * 2 * kBnD * sizeof(double));
  pl.part1 = bump.take((size_t)pl.P * bn_mp(X) * kNlQ * sizeof(float));
  pl.part2 = bump.take((size_t)pl.P * 9 * kBnD * kBnD * sizeof(float));
  pl.part3 = bump.take((size_t)pl.P * kBnD * kNlQ * sizeof(float));
  pl.total = bump.o;
  return pl;
}

__device__ __forceinline__ float bn_lrelu(float v) { return v >= 0.f ? v : kLeakyAlpha * v; }

// ---- launch 1
struct BnEntryArgs {
  const float *xin, *d_y3;
  float *xp, *dyp;      // [N][xp], [N][272]
  double* szpart;      // [N / 64][272]
  int xin_cs;
};

// grid (N / 64).  xin is read for c < X alone: block 0's pixel ends at channel 98 of a 120-float stride
template <int X>
__global__ __launch_bounds__(256) void bn_entry_kernel(const BnEntryArgs a) {
  constexpr int Xp = bn_xp(X);
  const int tid = threadIdx.x;
  const size_t row0 = (size_t)blockIdx.x * 64;
  for (int c = tid; c < kBnYp; c += 256) {
    double s = 0.0;
    for (int i = 0; i < 64; ++i) {
      const size_t row = row0 + i;
      const float x = c < X ? a.xin[row * a.xin_cs + c] : 0.f;
      const float g = c < kBnY ? a.d_y3[row * kBnY + c] : 0.f;
      if (Xp == kBnYp || c < Xp) a.xp[row * Xp + c] = x;
      a.dyp[row * kBnYp + c] = g;
      s += (double)g;
    }
    a.szpart[(size_t)blockIdx.x * kBnYp + c] = s;
  }
}

// ---- launches 2, 4, 9: out [N][.] = epilogue(a [N][K] w [K][.]), nl_gemm_kernel's main loop
struct BnGemmArgs {
  const float* a;       // [N][a_cs], K a multiple of 16, pad columns 0
  const float* w;       // [K][w_cs], w_cs a multiple of 128
  const float* bias;    // MODE 0
  const float* act;     // MODE 1: [N][128], the LeakyReLU's kept output
  const float* res;     // MODE 2: [N][res_cs] or null
  float* out;           // [N][out_cs], columns < n_store
  int a_cs, K, w_cs, res_cs, out_cs, n_store;
};

// grid (N / 64, column tiles of 128)
template <int MODE>
__global__ __launch_bounds__(256) void bn_gemm_kernel(const BnGemmArgs a) {
  constexpr int LDA = 18, LDW = 144;
  __shared__ __attribute__((aligned(16))) float s_a[64 * LDA];
  __shared__ __attribute__((aligned(16))) float s_w[16 * LDW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, q = lane >> 4;
  const size_t row0 = (size_t)blockIdx.x * 64;
  const int c0 = (int)blockIdx.y * 128;
  f32x4 acc[8];
#pragma unroll
  for (int n = 0; n < 8; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < a.K; k0 += 16) {
    const f32x4 av4 = *reinterpret_cast<const f32x4*>(a.a + (row0 + (tid >> 2)) * a.a_cs + k0 + (tid & 3) * 4);
    f32x4 wv4[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int i = tid + j * 256;
      wv4[j] = *reinterpret_cast<const f32x4*>(a.w + (size_t)(k0 + (i >> 5)) * a.w_cs + c0 + (i & 31) * 4);
    }
    __syncthreads();                                                       // every wave is done with the previous chunk
    {
      float* d = s_a + (tid >> 2) * LDA + (tid & 3) * 4;
      *reinterpret_cast<f32x2*>(d) = f32x2{av4[0], av4[1]};
      *reinterpret_cast<f32x2*>(d + 2) = f32x2{av4[2], av4[3]};
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int i = tid + j * 256;
      *reinterpret_cast<f32x4*>(s_w + (i >> 5) * LDW + (i & 31) * 4) = wv4[j];
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const float av = s_a[(wave * 16 + r) * LDA + kk * 4 + q];
      const float* wp = s_w + (kk * 4 + q) * LDW + r;
#pragma unroll
      for (int n = 0; n < 8; ++n) acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, wp[n * 16], acc[n], 0, 0, 0);
    }
  }
#pragma unroll
  for (int n = 0; n < 8; ++n) {
    const int col = c0 + n * 16 + r;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const size_t row = row0 + wave * 16 + 4 * q + e;
      float v = acc[n][e];
      if constexpr (MODE == 0) v = bn_lrelu(v + a.bias[col]);
      if constexpr (MODE == 1) v = clr_leaky_grad(v, a.act[row * kBnD + col]);
      if constexpr (MODE == 2) {
        if (a.res != nullptr && col < a.n_store) v += a.res[row * a.res_cs + col];
      }
      if (col < a.n_store) a.out[row * a.out_cs + col] = v;
    }
  }
}

// ---- launches 3, 5: out [B,h,w,128] = epilogue(conv3x3_same(in [B,h,w,128], w [9][128][128]))
struct BnConv3Args {
  const float* in;      // [N][128]
  const float* w;       // [9][128 in][128 out], tap t = 3 a + b reads the pixel (y + a - 1, x + b - 1)
  const float* bias;    // MODE 0
  const float* act;     // MODE 1: [N][128]
  float* out;           // [N][128]
  int h, w_px;
};

// grid (w / 32, h / 2, B): the tile's rows y0, y0 + 1 and columns x0 .. x0 + 31; wave v takes row v / 2, columns 16 (v % 2) ..
template <int MODE>
__global__ __launch_bounds__(256) void bn_conv3_kernel(const BnConv3Args a) {
  constexpr int LDA = 18, LDW = 144, HW = 34, HALO = 4 * HW;
  __shared__ __attribute__((aligned(16))) float s_in[HALO * LDA];
  __shared__ __attribute__((aligned(16))) float s_w[16 * LDW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int x0 = (int)blockIdx.x * 32, y0 = (int)blockIdx.y * 2;
  const size_t img0 = (size_t)blockIdx.z * a.h * a.w_px;
  const int trow = wave >> 1, tcol = (wave & 1) * 16;
  // the halo elements this thread stages: 136 pixels x 4 quads of channels = 544, three rounds of 256
  const float* hsrc[3];
  int hdst[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int i = tid + j * 256;
    const int p = i >> 2, part = i & 3;
    const int y = y0 - 1 + p / HW, x = x0 - 1 + p % HW;
    const bool in = i < 4 * HALO && y >= 0 && y < a.h && x >= 0 && x < a.w_px;
    hsrc[j] = in ? a.in + (img0 + (size_t)y * a.w_px + x) * kBnD + part * 4 : nullptr;
    hdst[j] = i < 4 * HALO ? p * LDA + part * 4 : -1;
  }
  f32x4 acc[8];
#pragma unroll
  for (int n = 0; n < 8; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int c0 = 0; c0 < kBnD; c0 += 16) {
    f32x4 hv[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) hv[j] = hsrc[j] != nullptr ? *reinterpret_cast<const f32x4*>(hsrc[j] + c0) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int t = 0; t < 9; ++t) {
      f32x4 wv4[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int i = tid + j * 256;
        wv4[j] = *reinterpret_cast<const f32x4*>(a.w + ((size_t)t * kBnD + c0 + (i >> 5)) * kBnD + (i & 31) * 4);
      }
      __syncthreads();                                                     // every wave is done with the previous tap
      if (t == 0) {
#pragma unroll
        for (int j = 0; j < 3; ++j)
          if (hdst[j] >= 0) {
            float* d = s_in + hdst[j];
            *reinterpret_cast<f32x2*>(d) = f32x2{hv[j][0], hv[j][1]};
            *reinterpret_cast<f32x2*>(d + 2) = f32x2{hv[j][2], hv[j][3]};
          }
      }
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int i = tid + j * 256;
        *reinterpret_cast<f32x4*>(s_w + (i >> 5) * LDW + (i & 31) * 4) = wv4[j];
      }
      __syncthreads();
      const float* ap = s_in + ((trow + t / 3) * HW + tcol + r + t % 3) * LDA + q;
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        const float av = ap[kk * 4];
        const float* wp = s_w + (kk * 4 + q) * LDW + r;
#pragma unroll
        for (int n = 0; n < 8; ++n) acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, wp[n * 16], acc[n], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int n = 0; n < 8; ++n) {
    const int col = n * 16 + r;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const size_t row = img0 + (size_t)(y0 + trow) * a.w_px + x0 + tcol + 4 * q + e;
      float v = acc[n][e];
      if constexpr (MODE == 0) v = bn_lrelu(v + a.bias[col]);
      if constexpr (MODE == 1) v = clr_leaky_grad(v, a.act[row * kBnD + col]);
      a.out[row * kBnD + col] = v;
    }
  }
}

// ---- launch 6: part[p][t][c][o] = sum over the slice's rows of x(row shifted by tap t, zero outside the image)[c] g[row][o]
struct BnWgrad3Args {
  const float* x;       // [N][128]: conv2's input a1
  const float* g;       // [N][128]: gz2
  float* part;          // [P][9][128][128]
  int h, w_px, chunks, P;
};

// grid (P, 2 halves of the input channels, 9 taps): slice p takes the 128-row chunks p, p + P, ...; nl_tn_kernel's main loop
__global__ __launch_bounds__(256) void bn_wgrad3_kernel(const BnWgrad3Args a) {
  constexpr int LDL = 80, LDR = 144;
  __shared__ __attribute__((aligned(16))) float s_l[16 * LDL];
  __shared__ __attribute__((aligned(16))) float s_r[16 * LDR];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int p = (int)blockIdx.x, m0 = (int)blockIdx.y * 64, t = (int)blockIdx.z;
  const int dy = t / 3 - 1, dx = t % 3 - 1;
  f32x4 acc[8];
#pragma unroll
  for (int n = 0; n < 8; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int ch = p; ch < a.chunks; ch += a.P) {
    for (int st = 0; st < 8; ++st) {
      const size_t row0 = (size_t)ch * 128 + st * 16;
      f32x4 lv = {0.f, 0.f, 0.f, 0.f}, rv[2];
      {
        const size_t row = row0 + (tid >> 4);
        const int x = (int)(row % a.w_px) + dx, y = (int)((row / a.w_px) % a.h) + dy;
        if (x >= 0 && x < a.w_px && y >= 0 && y < a.h)
          lv = *reinterpret_cast<const f32x4*>(a.x + (size_t)((long long)row + (long long)dy * a.w_px + dx) * kBnD + m0 + (tid & 15) * 4);
      }
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int i = tid + j * 256;
        rv[j] = *reinterpret_cast<const f32x4*>(a.g + (row0 + (i >> 5)) * kBnD + (i & 31) * 4);
      }
      __syncthreads();
      *reinterpret_cast<f32x4*>(s_l + (tid >> 4) * LDL + (tid & 15) * 4) = lv;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int i = tid + j * 256;
        *reinterpret_cast<f32x4*>(s_r + (i >> 5) * LDR + (i & 31) * 4) = rv[j];
      }
      __syncthreads();
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        const float av = s_l[(kk * 4 + q) * LDL + wave * 16 + r];
        const float* bp = s_r + (kk * 4 + q) * LDR + r;
#pragma unroll
        for (int n = 0; n < 8; ++n) acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bp[n * 16], acc[n], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int n = 0; n < 8; ++n)
#pragma unroll
    for (int e = 0; e < 4; ++e) a.part[(((size_t)p * 9 + t) * kBnD + m0 + wave * 16 + 4 * q + e) * kBnD + n * 16 + r] = acc[n][e];
}

// ---- launch 10: grid (N / 128), 256 threads: columns 0..127 gz2's, 128..255 gz1's
__global__ __launch_bounds__(256) void bn_colsum_kernel(const float* gz2, const float* gz1, double* bpart) {
  const int t = threadIdx.x;
  const float* src = (t < kBnD ? gz2 : gz1) + (size_t)blockIdx.x * 128 * kBnD + (t & (kBnD - 1));
  double s = 0.0;
#pragma unroll 8
  for (int i = 0; i < 128; ++i) s += (double)src[(size_t)i * kBnD];
  bpart[(size_t)blockIdx.x * 2 * kBnD + t] = s;
}

// ---- launch 11
struct BnFoldArgs {
  const float *part1, *part2, *part3;
  const float *vecs1, *vecs2, *vecs3;
  double* Wg;
  float* grads;
  int P;
};

template <int X>
__global__ __launch_bounds__(256) void bn_fold_kernel(const BnFoldArgs a) {
  constexpr int kBnK1 = bn_k1(X);
  const int e = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (e >= bn_kernel_elems(X)) return;
  double s = 0.0, inv;
  size_t at;
  if (e < kBnK1) {
    const int c = e / kBnD, k = e % kBnD;
    const float* src = a.part1 + (size_t)c * kNlQ + k;
#pragma unroll 8
    for (int p = 0; p < a.P; ++p) s += (double)src[(size_t)p * bn_mp(X) * kNlQ];
    inv = a.vecs1[kBnD + k];
    at = bn_var_offset(0, X) + e;
  } else if (e < kBnK1 + kBnK2) {
    const int i = e - kBnK1;
    const float* src = a.part2 + i;
#pragma unroll 8
    for (int p = 0; p < a.P; ++p) s += (double)src[(size_t)p * kBnK2];
    inv = a.vecs2[kBnD + i % kBnD];
    at = bn_var_offset(2, X) + i;
  } else {
    const int i = e - kBnK1 - kBnK2, k = i / kBnY, n = i % kBnY;
    const float* src = a.part3 + (size_t)k * kNlQ + n;
#pragma unroll 8
    for (int p = 0; p < a.P; ++p) s += (double)src[(size_t)p * kBnD * kNlQ];
    inv = a.vecs3[kBnY + n];
    at = bn_var_offset(4, X) + i;
  }
  a.Wg[e] = s;
  a.grads[at] = (float)(inv * s);
}

// ---- launch 12: grid (128 + 128 + 257), one wave each: layer 1's, layer 2's, layer 3's channels
struct BnFinishArgs {
  const double *szpart, *bpart, *Wg;
  const float *k1, *k2, *k3, *vecs1, *vecs2, *vecs3;
  double* S;
  float* grads;
  int nsz, nb;
};

template <int X>
__global__ __launch_bounds__(64) void bn_finish_kernel(const BnFinishArgs a) {
  constexpr int kBnK1 = bn_k1(X);
  const int lane = threadIdx.x, b = (int)blockIdx.x;
  double s = 0.0, kw = 0.0;
  if (b < kBnD) {
    for (int i = lane; i < a.nb; i += 64) s += a.bpart[(size_t)i * 2 * kBnD + kBnD + b];
    for (int c = lane; c < X; c += 64) kw += (double)a.k1[c * kBnD + b] * a.Wg[c * kBnD + b];
  } else if (b < 2 * kBnD) {
    const int o = b - kBnD;
    for (int i = lane; i < a.nb; i += 64) s += a.bpart[(size_t)i * 2 * kBnD + o];
    for (int i = lane; i < 9 * kBnD; i += 64) kw += (double)a.k2[i * kBnD + o] * a.Wg[kBnK1 + i * kBnD + o];
  } else {
    const int n = b - 2 * kBnD;
    for (int i = lane; i < a.nsz; i += 64) s += a.szpart[(size_t)i * kBnYp + n];
    for (int k = lane; k < kBnD; k += 64) kw += (double)a.k3[k * kBnY + n] * a.Wg[kBnK1 + kBnK2 + k * kBnY + n];
  }
  s = wave_sum(s);
  kw = wave_sum(kw);
  if (lane != 0) return;
  a.S[b] = s;
  if (b < kBnD)
    bn_channel_grads(kw, s, a.vecs1, kBnD, b, a.grads[bn_var_offset(1, X) + b], a.grads[bn_var_offset(6, X) + b], a.grads[bn_var_offset(7, X) + b]);
  else if (b < 2 * kBnD)
    bn_channel_grads(kw, s, a.vecs2, kBnD, b - kBnD, a.grads[bn_var_offset(3, X) + b - kBnD], a.grads[bn_var_offset(8, X) + b - kBnD],
                     a.grads[bn_var_offset(9, X) + b - kBnD]);
  else
    bn_channel_grads(kw, s, a.vecs3, kBnY, b - 2 * kBnD, a.grads[bn_var_offset(5, X) + b - 2 * kBnD], a.grads[bn_var_offset(10, X) + b - 2 * kBnD],
                     a.grads[bn_var_offset(11, X) + b - 2 * kBnD]);
}

// The first `stop_after` of the twelve launches above (kBnLaunches: all of them; fewer are for the tests' stage-by-stage comparison).
// xin [B,h,w,X of xin_cs], d_y3 dense 257 wide, d_skip dense X wide or null, d_xin dense X wide; blob, grads and scratch are
// bn_blob_off's, bn_var_offset's and bn_plan's at this X.  A narrow input does not run the wide blocks' work on zeros: launch 2 runs
// K = xp, launch 8 covers xp^T's own 64-row tiles and launch 9 w1t's own 128-column tiles.
template <int X = kBnX>
inline hipError_t launch_bottleneck_grad(const float* blob, const float* xin, int xin_cs, const float* d_y3, const float* d_skip, int B, int h, int w,
                                         float* d_xin, float* grads, void* scratch, int stop_after, hipStream_t stream) {
  static_assert(bn_width_ok(X), "the input is 261, 257 or 99 wide");
  constexpr int Xp = bn_xp(X), W1t = bn_w1t(X), Mp = bn_mp(X);
  constexpr int kRowTiles = Mp / 64, kColTiles = W1t / 128;       // launch 8's grid.y, launch 9's grid.y
  static_assert(X != 99 || (Xp == 112 && kRowTiles == 2 && kColTiles == 1), "block 0: K = 112, two 64-row tiles, one 128-column tile");
  static_assert(X == 99 || (Xp == 272 && kRowTiles == 5 && kColTiles == 3), "the wide blocks: K = 272, five row tiles, three column tiles");
  static_assert(Xp % 16 == 0 && Xp <= Mp && X <= W1t, "the GEMMs' steps and the tiles cover the input");
  const BnPlan pl = bn_plan(B, h, w, X);
  unsigned char* base = static_cast<unsigned char*>(scratch);
  auto f = [&](size_t off) { return reinterpret_cast<float*>(base + off); };
  auto d = [&](size_t off) { return reinterpret_cast<double*>(base + off); };
  float *xp = f(pl.map[0]), *dyp = f(pl.map[1]), *a1 = f(pl.map[2]), *a2 = f(pl.map[3]), *gz2 = f(pl.map[4]), *gz1 = f(pl.map[5]);
  float *part1 = f(pl.part1), *part2 = f(pl.part2), *part3 = f(pl.part3);
  double *Wg = d(pl.map[6]), *S = d(pl.map[7]), *szpart = d(pl.szpart), *bpart = d(pl.bpart);
  const int N = pl.N;
  const dim3 tiles(w / 32, h / 2, B);
  hipError_t e;
  int done = 0;
  if (stop_after <= done++) return hipSuccess;
  {
    BnEntryArgs a{xin, d_y3, xp, dyp, szpart, xin_cs};
    hipLaunchKernelGGL(bn_entry_kernel<X>, dim3(N / 64), dim3(256), 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (stop_after <= done++) return hipSuccess;
  {
    BnGemmArgs a{};
    a.a = xp; a.a_cs = Xp; a.K = Xp; a.w = blob + bn_blob_off(0, X); a.w_cs = kBnD; a.bias = blob + bn_blob_off(1, X);
    a.out = a1; a.out_cs = kBnD; a.n_store = kBnD;
    hipLaunchKernelGGL(bn_gemm_kernel<0>, dim3(N / 64, 1), dim3(256), 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (stop_after <= done++) return hipSuccess;
  {
    BnConv3Args a{a1, blob + bn_blob_off(2, X), blob + bn_blob_off(3, X), nullptr, a2, h, w};
    hipLaunchKernelGGL(bn_conv3_kernel<0>, tiles, dim3(256), 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (stop_after <= done++) return hipSuccess;
  {
    BnGemmArgs a{};
    a.a = dyp; a.a_cs = kBnYp; a.K = kBnYp; a.w = blob + bn_blob_off(4, X); a.w_cs = kBnD; a.act = a2;
    a.out = gz2; a.out_cs = kBnD; a.n_store = kBnD;
    hipLaunchKernelGGL(bn_gemm_kernel<1>, dim3(N / 64, 1), dim3(256), 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (stop_after <= done++) return hipSuccess;
  {
    BnConv3Args a{gz2, blob + bn_blob_off(5, X), nullptr, a1, gz1, h, w};
    hipLaunchKernelGGL(bn_conv3_kernel<1>, tiles, dim3(256), 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (stop_after <= done++) return hipSuccess;
  {
    BnWgrad3Args a{a1, gz2, part2, h, w, N / 128, pl.P};
    hipLaunchKernelGGL(bn_wgrad3_kernel, dim3(pl.P, 2, 9), dim3(256), 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (stop_after <= done++) return hipSuccess;
  {
    NlTnArgs a{a2, dyp, part3, kBnD, kBnD, kBnYp, kBnYp, kBnD, N / 128, pl.P};
    hipLaunchKernelGGL(nl_tn_kernel, dim3(pl.P, 2, 3), dim3(256), 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (stop_after <= done++) return hipSuccess;
  {
    NlTnArgs a{xp, gz1, part1, Xp, Xp, kBnD, kBnD, Mp, N / 128, pl.P};
    hipLaunchKernelGGL(nl_tn_kernel, dim3(pl.P, kRowTiles, 1), dim3(256), 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (stop_after <= done++) return hipSuccess;
  {
    BnGemmArgs a{};
    a.a = gz1; a.a_cs = kBnD; a.K = kBnD; a.w = blob + bn_blob_off(6, X); a.w_cs = W1t; a.res = d_skip; a.res_cs = X;
    a.out = d_xin; a.out_cs = X; a.n_store = X;
    hipLaunchKernelGGL(bn_gemm_kernel<2>, dim3(N / 64, kColTiles), dim3(256), 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (stop_after <= done++) return hipSuccess;
  hipLaunchKernelGGL(bn_colsum_kernel, dim3(N / 128), dim3(256), 0, stream, gz2, gz1, bpart);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if (stop_after <= done++) return hipSuccess;
  {
    BnFoldArgs a{part1, part2, part3, blob + bn_blob_off(10, X), blob + bn_blob_off(11, X), blob + bn_blob_off(12, X), Wg, grads, pl.P};
    hipLaunchKernelGGL(bn_fold_kernel<X>, dim3((bn_kernel_elems(X) + 255) / 256), dim3(256), 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (stop_after <= done++) return hipSuccess;
  BnFinishArgs a{szpart, bpart, Wg, blob + bn_blob_off(7, X), blob + bn_blob_off(8, X), blob + bn_blob_off(9, X), blob + bn_blob_off(10, X),
                 blob + bn_blob_off(11, X), blob + bn_blob_off(12, X), S, grads, N / 64, N / 128};
  hipLaunchKernelGGL(bn_finish_kernel<X>, dim3(kBnChannels), dim3(64), 0, stream, a);
  return hipGetLastError();
}

}  // namespace bsr
