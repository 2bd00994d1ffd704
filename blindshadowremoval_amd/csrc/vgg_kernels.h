// The VGG19 perceptual term of the reference's train_step ON THE DEVICE: per_loss = style_content_loss(feat_extractor, d_img)
// (train_test_GSC.py:128-139, 153-160, 303; utils.py:104-114).  blindshadowremoval_amd/perceptual.py is the host statement and writes the
// arithmetic out; pack.pack_vgg writes the weight blob (vgg_layout).
//
// One chain of 20 launches on the caller's stream, no host synchronisation, no parallel branch, no floating-point atomic; every word of
// scratch that a launch reads was written by an earlier launch of the same call.
//   vgg_input_kernel     a thread per pixel: rows [0, B) from gt, rows [B, 2B) from con_rgb; x * 255, channels reversed to BGR, the
//                        ImageNet means subtracted, one float32 rounding per operation (contraction off): bit-identical to the host
//                        statement.  Writes [2B][S][S][8], channels 3..7 as zeros.
//   vgg_conv_kernel      x 13, one launch per layer.  3 x 3, stride 1, SAME (1 before, 1 after) as an implicit GEMM on
//                        v_mfma_f32_32x32x2_f32: a workgroup of four waves owns a 16 x 16 tile of output pixels and 64 output channels, a
//                        wave 4 x 16 pixels (two M tiles of 32) x two N tiles of 32 = four accumulator tiles, so every LDS fragment feeds
//                        two matrix instructions.  K = 9 C_in runs in chunks of CC = 16 input channels (8 for the first layer, whose 3
//                        channels are padded to 8): the 18 x 18 input patch of the chunk (halo included; padding and pixels outside the map
//                        are stored as 0) and the chunk's [9][CC][64] weights go to LDS, and each tap reads the patch at a shifted address.
//                        The NEXT chunk's global loads are issued into registers before the current chunk's 288 matrix instructions
//                        and land behind them.  Epilogue (the template parameter Epi, here VggBiasRelu; vgg_grad_kernels.h runs the
//                        same main loop with the data gradient's): bias (bias_tile) + ReLU (leaky_relu_tile(acc, 0): negative values
//                        leave as -0).  Output pixels outside the map are computed and not stored, so maps smaller than a tile, down to 2 x 2, take
//                        the same path.  The workgroup index runs over the 64-channel blocks fastest: the blocks of one tile run
//                        together and share its patch through L2.  LDS: 22 KB + 36 KB.
//   vgg_pool_kernel      x 4: 2 x 2 stride-2 max pool, a thread per four channels of an output pixel; exact.
//   vgg_l1_kernel        one launch over the five taps: a workgroup owns a slice of kVggSlice values of one (tap, item), forms float32
//                        |real - fake|, folds in float64 by wave butterfly, then the waves in index order, and writes its own slot.
//   vgg_finish_kernel    one workgroup: a thread per (item, tap) adds its slots in index order into sums[B][5]; then a thread per tap
//                        adds the items in order, and one thread forms the loss in float64, rounded once to float32.
//
// SCRATCH (vgg_act_offset): the input, then every conv layer's output in order, then the four pooled maps, each rounded up to 256
// bytes, then the slots.  Nothing is reused, so every activation is there afterwards (the binding's `keep`); at 32 items of 256 x 256 that
// is 5.5 GB.
#pragma once
#include "mfma_common.h"

namespace bsr {

constexpr int kVggLayers = 13, kVggTaps = 5, kVggPools = 4, kVggInC = 8, kVggNB = 64;
constexpr int kVggTH = 16, kVggTW = 16, kVggPH = kVggTH + 2, kVggPW = kVggTW + 2;
constexpr int kVggSlice = 8192;                         // float32 values per vgg_l1_kernel workgroup
constexpr int kVggMaxB = 4096;
constexpr int kVggMaps = 1 + kVggLayers + kVggPools;    // maps of vgg_act_offset: 0 the input, 1..13 the conv outputs, 14..17 the pools

// block (0..4) and output channels of conv layer i (0..12): 64,64 | 128,128 | 256 x 4 | 512 x 4 | 512
__host__ __device__ inline int vgg_block(int i) { return i < 2 ? 0 : i < 4 ? 1 : i < 8 ? 2 : i < 12 ? 3 : 4; }
__host__ __device__ inline int vgg_ch(int i) { const int b = vgg_block(i); return b < 4 ? 64 << b : 512; }
__host__ __device__ inline int vgg_cin(int i) { return i == 0 ? kVggInC : vgg_ch(i - 1); }
__host__ __device__ inline int vgg_side(int S, int i) { return S >> vgg_block(i); }
__host__ __device__ inline int vgg_tap_layer(int k) { return k == 0 ? 0 : k == 1 ? 2 : k == 2 ? 4 : k == 3 ? 8 : 12; }     // block{k+1}_conv1
__host__ __device__ inline bool vgg_first_of_block(int i) { return i == 2 || i == 4 || i == 8 || i == 12; }
// float offset of layer i's weights inside the blob (i = 13: the total): [N / 64][C_in / CC][9][CC][64], then bias [N]
__host__ __device__ inline size_t vgg_w_off(int i) {
  size_t o = 0;
  for (int j = 0; j < i; ++j) o += (size_t)9 * vgg_cin(j) * vgg_ch(j) + vgg_ch(j);
  return o;
}
__host__ __device__ inline size_t vgg_map_bytes(int B, int S, int map) {
  size_t n;
  if (map == 0) n = (size_t)S * S * kVggInC;
  else if (map <= kVggLayers) { const size_t s = (size_t)vgg_side(S, map - 1); n = s * s * vgg_ch(map - 1); }
  else { const int p = map - kVggLayers - 1; const size_t s = (size_t)(S >> (p + 1)); n = s * s * (64 << p); }       // pool p follows block p
  return ((size_t)2 * B * n * sizeof(float) + 255) & ~size_t(255);
}
__host__ __device__ inline size_t vgg_slices(int S, int k) {
  const size_t s = (size_t)(S >> k);
  return (s * s * vgg_ch(vgg_tap_layer(k)) + kVggSlice - 1) / kVggSlice;
}
__host__ __device__ inline size_t vgg_slots(int B, int S) {
  size_t n = 0;
  for (int k = 0; k < kVggTaps; ++k) n += vgg_slices(S, k);
  return n * B;
}
// byte offset of `map` inside the scratch; kVggMaps is where the slots start, kVggMaps + 1 the total
__host__ __device__ inline size_t vgg_act_offset(int B, int S, int map) {
  size_t o = 0;
  for (int j = 0; j < map && j < kVggMaps; ++j) o += vgg_map_bytes(B, S, j);
  if (map > kVggMaps) o += (vgg_slots(B, S) * sizeof(double) + 255) & ~size_t(255);
  return o;
}
__host__ __device__ inline float* vgg_map(void* scratch, int B, int S, int map) {
  return reinterpret_cast<float*>(static_cast<unsigned char*>(scratch) + vgg_act_offset(B, S, map));
}

__global__ __launch_bounds__(256) void vgg_input_kernel(const float* __restrict__ gt, const float* __restrict__ con, int B, int S, float* __restrict__ out) {
#pragma clang fp contract(off)
  const size_t per = (size_t)S * S, p = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= 2 * B * per) return;
  const size_t row = p / per, q = p % per;
  const float* im = (row < (size_t)B ? gt + row * per * 3 : con + (row - B) * per * 3) + q * 3;
  const float r = im[0] * 255.f, g = im[1] * 255.f, b = im[2] * 255.f;
  f32x4* o = reinterpret_cast<f32x4*>(out + p * kVggInC);
  o[0] = f32x4{b - 103.939f, g - 116.779f, r - 123.68f, 0.f};
  o[1] = f32x4{0.f, 0.f, 0.f, 0.f};
}

struct VggConvArgs {
  const float* in;        // [rows][H][H][CIN]
  const float* w;         // [N / 64][CIN / CC][9][CC][64]
  int H, CIN, N, tiles_x, tiles, nblk;      // tiles per row = tiles_x^2; nblk = N / 64
};

// What a wave of vgg_conv_kernel knows about its four accumulator tiles: acc[t][nt][i] is pixel (oy0 + wave * 4 + t * 2 + (mr >> 4),
// ox0 + (mr & 15)), mr = (i & 3) + 8 * (i >> 2) + 4 * kh, of network row `row`, channel nb * 64 + nt * 32 + m.
struct VggTilePos {
  int row, oy0, ox0, wave, kh, m, nb, H, N;
};

// The forward layer's epilogue: the accumulators start as the bias (bias_tile) and leave through ReLU (leaky_relu_tile(acc, 0):
// negative values leave as -0).
struct VggBiasRelu {
  float* out;             // [rows][H][H][N]
  const float* bias;      // [N]
  __device__ __forceinline__ f32x16 init(int kh, int ch) const { return bias_tile(kh, bias[ch]); }
  __device__ __forceinline__ void finish(f32x16 (&acc)[2][2], const VggTilePos& p) const {
    const int H = p.H, N = p.N, kh = p.kh, m = p.m, wave = p.wave, oy0 = p.oy0, ox0 = p.ox0;
    float* out = this->out + (size_t)p.row * H * H * N + p.nb * kVggNB;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {
        leaky_relu_tile(acc[t][nt], 0.f);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int mr = (i & 3) + 8 * (i >> 2) + 4 * kh;                  // the accumulator's row: pixel mr of the M tile
          const int oy = oy0 + wave * 4 + t * 2 + (mr >> 4), ox = ox0 + (mr & 15);
          if (oy < H && ox < H) out[((size_t)oy * H + ox) * N + nt * 32 + m] = acc[t][nt][i];
        }
      }
  }
};

// Epi: how the accumulators start and leave (VggBiasRelu here; the data gradient's, VggGradEpilogue, in vgg_grad_kernels.h).
template <int CC, class Epi>
__global__ __launch_bounds__(256) void vgg_conv_kernel(const VggConvArgs a, const Epi epi) {
  static_assert(CC == 8 || CC == 16, "chunk");
  constexpr int Ld = CC + 1, Q = CC / 4;
  constexpr int PN = kVggPH * kVggPW * Q, PIT = (PN + 255) / 256;          // f32x4 of the patch, per thread
  constexpr int WN = 9 * CC * kVggNB / 4, WIT = (WN + 255) / 256;          // f32x4 of the chunk's weights, per thread
  __shared__ float s_in[kVggPH * kVggPW * Ld];
  __shared__ __attribute__((aligned(16))) float s_w[9 * CC * kVggNB];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned r = blockIdx.x;
  const int nb = (int)(r % (unsigned)a.nblk);
  r /= (unsigned)a.nblk;
  const int tile = (int)(r % (unsigned)a.tiles), row = (int)(r / (unsigned)a.tiles);
  const int oy0 = (tile / a.tiles_x) * kVggTH, ox0 = (tile % a.tiles_x) * kVggTW;
  const int H = a.H, CIN = a.CIN, N = a.N;
  const float* in = a.in + (size_t)row * H * H * CIN;
  const float* wblk = a.w + (size_t)nb * 9 * CIN * kVggNB;
  const int m = lane & 31, kh = lane >> 5;
  int a_base[2];                                                            // the wave's pixel m of M tile t, tap (0, 0), channel kh
#pragma unroll
  for (int t = 0; t < 2; ++t) a_base[t] = ((wave * 4 + t * 2 + (m >> 4)) * kVggPW + (m & 15)) * Ld + kh;

  f32x16 acc[2][2];
#pragma unroll
  for (int nt = 0; nt < 2; ++nt) {
    acc[0][nt] = epi.init(kh, nb * kVggNB + nt * 32 + m);
    acc[1][nt] = epi.init(kh, nb * kVggNB + nt * 32 + m);
  }

  // where this thread's patch words come from (-1: padding or outside the map) — the same for every chunk but for + c0
  int poff[PIT];
#pragma unroll
  for (int j = 0; j < PIT; ++j) {
    const int i = tid + j * 256;
    const int pix = i / Q, q = i % Q;
    const int iy = oy0 - 1 + pix / kVggPW, ix = ox0 - 1 + pix % kVggPW;
    poff[j] = (i < PN && iy >= 0 && iy < H && ix >= 0 && ix < H) ? (iy * H + ix) * CIN + q * 4 : -1;
  }
  f32x4 pr[PIT], wr[WIT];
  auto fetch = [&](int c0) {                                                // global -> registers
#pragma unroll
    for (int j = 0; j < PIT; ++j) {
      pr[j] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (poff[j] >= 0) pr[j] = *reinterpret_cast<const f32x4*>(in + poff[j] + c0);
    }
    const f32x4* wsrc = reinterpret_cast<const f32x4*>(wblk + (size_t)(c0 / CC) * 9 * CC * kVggNB);
#pragma unroll
    for (int j = 0; j < WIT; ++j)
      if (WN % 256 == 0 || tid + j * 256 < WN) wr[j] = wsrc[tid + j * 256];
  };

  fetch(0);
  for (int c0 = 0; c0 < CIN; c0 += CC) {
    if (c0 != 0) __syncthreads();                                          // every wave is done with the previous chunk's LDS
#pragma unroll
    for (int j = 0; j < PIT; ++j) {
      const int i = tid + j * 256;
      if (PN % 256 == 0 || i < PN) {
        float* dst = s_in + (i / Q) * Ld + (i % Q) * 4;
        dst[0] = pr[j][0]; dst[1] = pr[j][1]; dst[2] = pr[j][2]; dst[3] = pr[j][3];
      }
    }
#pragma unroll
    for (int j = 0; j < WIT; ++j)
      if (WN % 256 == 0 || tid + j * 256 < WN) reinterpret_cast<f32x4*>(s_w)[tid + j * 256] = wr[j];
    __syncthreads();
    if (c0 + CC < CIN) fetch(c0 + CC);                                     // in flight behind this chunk's matrix work
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int sh = ((tap / 3) * kVggPW + tap % 3) * Ld;
      const float* ap0 = s_in + a_base[0] + sh;
      const float* ap1 = s_in + a_base[1] + sh;
      const float* bp = s_w + (tap * CC + kh) * kVggNB + m;
#pragma unroll
      for (int k2 = 0; k2 < CC / 2; ++k2) {
        const float av0 = ap0[2 * k2], av1 = ap1[2 * k2];
        const float b0 = bp[2 * k2 * kVggNB], b1 = bp[2 * k2 * kVggNB + 32];
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av1, b1, acc[1][1], 0, 0, 0);
      }
    }
  }
  epi.finish(acc, VggTilePos{row, oy0, ox0, wave, kh, m, nb, H, N});
}

// in [rows][2h][2h][C] -> out [rows][h][h][C]; a thread per four channels of an output pixel
__global__ __launch_bounds__(256) void vgg_pool_kernel(const float* __restrict__ in, float* __restrict__ out, size_t total4, int h, int C) {
  const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= total4) return;
  const int c4 = C / 4;
  const size_t c = p % c4, pix = p / c4;
  const size_t x = pix % h, y = (pix / h) % h, row = pix / ((size_t)h * h);
  const f32x4* src = reinterpret_cast<const f32x4*>(in) + ((row * 2 * h + 2 * y) * 2 * h + 2 * x) * c4 + c;
  const f32x4 v0 = src[0], v1 = src[c4], v2 = src[(size_t)2 * h * c4], v3 = src[(size_t)2 * h * c4 + c4];
  f32x4 o;
#pragma unroll
  for (int i = 0; i < 4; ++i) o[i] = fmaxf(fmaxf(v0[i], v1[i]), fmaxf(v2[i], v3[i]));
  reinterpret_cast<f32x4*>(out)[p] = o;
}

struct VggL1Args {
  const float* feat[kVggTaps];      // [2B][h_k][h_k][C_k]
  unsigned per_item[kVggTaps];      // float32 values of one item's map
  unsigned slices[kVggTaps];        // workgroups per (tap, item)
  unsigned first_block[kVggTaps];   // the tap's first workgroup index = its first slot
};

__global__ __launch_bounds__(256) void vgg_l1_kernel(const VggL1Args a, int B, double* __restrict__ slots) {
#pragma clang fp contract(off)
  __shared__ double s_red[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int k = 0;
#pragma unroll
  for (int j = 1; j < kVggTaps; ++j)
    if (blockIdx.x >= a.first_block[j]) k = j;
  const unsigned r = blockIdx.x - a.first_block[k];
  const unsigned item = r / a.slices[k], slice = r % a.slices[k];
  const size_t per = a.per_item[k];
  const float* real = a.feat[k] + (size_t)item * per;
  const float* fake = a.feat[k] + ((size_t)B + item) * per;
  const size_t lo = (size_t)slice * kVggSlice, hi = lo + kVggSlice < per ? lo + kVggSlice : per;      // per is a multiple of 4
  double s = 0.0;
  for (size_t i = lo + (size_t)tid * 4; i < hi; i += 1024) {
    const f32x4 x = *reinterpret_cast<const f32x4*>(real + i), y = *reinterpret_cast<const f32x4*>(fake + i);
#pragma unroll
    for (int c = 0; c < 4; ++c) s += (double)fabsf(x[c] - y[c]);
  }
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if (lane == 0) s_red[wave] = s;
  __syncthreads();
  if (tid == 0) slots[blockIdx.x] = ((s_red[0] + s_red[1]) + s_red[2]) + s_red[3];
}

__global__ __launch_bounds__(256) void vgg_finish_kernel(const VggL1Args a, int B, const double* __restrict__ slots, double* __restrict__ sums,
                                                         float* __restrict__ loss1) {      // grid (1)
#pragma clang fp contract(off)
  __shared__ double s_t[kVggTaps];
  const int tid = threadIdx.x;
  for (int p = tid; p < B * kVggTaps; p += 256) {
    const int item = p / kVggTaps, k = p % kVggTaps;
    const double* src = slots + a.first_block[k] + (size_t)item * a.slices[k];
    double s = 0.0;
    for (unsigned j = 0; j < a.slices[k]; ++j) s = s + src[j];
    sums[p] = s;
  }
  __syncthreads();
  if (tid < kVggTaps) {
    double t = 0.0;
    for (int item = 0; item < B; ++item) t = t + sums[(size_t)item * kVggTaps + tid];
    s_t[tid] = t / ((double)B * (double)a.per_item[tid]);
  }
  __syncthreads();
  if (tid == 0) loss1[0] = (float)((((s_t[0] + s_t[1]) + s_t[2]) + s_t[3]) + s_t[4]);
}

inline VggConvArgs vgg_conv_args(const float* in, const float* w, int H, int CIN, int N) {
  VggConvArgs a;
  a.in = in;
  a.w = w;
  a.H = H;
  a.CIN = CIN;
  a.N = N;
  a.tiles_x = (H + kVggTW - 1) / kVggTW;
  a.tiles = a.tiles_x * a.tiles_x;
  a.nblk = N / kVggNB;
  return a;
}

inline hipError_t launch_vgg_per_loss(const float* blob, const float* gt, const float* con, int B, int S, double* sums, float* loss1, void* scratch,
                                      hipStream_t stream) {
  const size_t pixels = (size_t)2 * B * S * S;
  hipLaunchKernelGGL(vgg_input_kernel, dim3((unsigned)((pixels + 255) / 256)), dim3(256), 0, stream, gt, con, B, S, vgg_map(scratch, B, S, 0));
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  int src = 0;                                            // the map the next layer reads
  for (int i = 0; i < kVggLayers; ++i) {
    if (vgg_first_of_block(i)) {
      const int p = vgg_block(i) - 1, h = S >> (p + 1), C = 64 << p, dst = kVggLayers + 1 + p;
      const size_t total4 = (size_t)2 * B * h * h * (C / 4);
      hipLaunchKernelGGL(vgg_pool_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, stream, vgg_map(scratch, B, S, src), vgg_map(scratch, B, S, dst),
                         total4, h, C);
      if ((e = hipGetLastError()) != hipSuccess) return e;
      src = dst;
    }
    const VggConvArgs a = vgg_conv_args(vgg_map(scratch, B, S, src), blob + vgg_w_off(i), vgg_side(S, i), vgg_cin(i), vgg_ch(i));
    const VggBiasRelu epi{vgg_map(scratch, B, S, i + 1), a.w + (size_t)9 * vgg_cin(i) * vgg_ch(i)};
    const dim3 grid((unsigned)(2 * B) * (unsigned)a.tiles * (unsigned)a.nblk);
    if (i == 0) hipLaunchKernelGGL((vgg_conv_kernel<8, VggBiasRelu>), grid, dim3(256), 0, stream, a, epi);
    else hipLaunchKernelGGL((vgg_conv_kernel<16, VggBiasRelu>), grid, dim3(256), 0, stream, a, epi);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    src = i + 1;
  }
  VggL1Args l;
  unsigned blocks = 0;
  for (int k = 0; k < kVggTaps; ++k) {
    const int layer = vgg_tap_layer(k);
    const size_t s = (size_t)vgg_side(S, layer);
    l.feat[k] = vgg_map(scratch, B, S, layer + 1);
    l.per_item[k] = (unsigned)(s * s * vgg_ch(layer));
    l.slices[k] = (unsigned)vgg_slices(S, k);
    l.first_block[k] = blocks;
    blocks += l.slices[k] * (unsigned)B;
  }
  double* slots = reinterpret_cast<double*>(vgg_map(scratch, B, S, kVggMaps));
  hipLaunchKernelGGL(vgg_l1_kernel, dim3(blocks), dim3(256), 0, stream, l, B, slots);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(vgg_finish_kernel, dim3(1), dim3(256), 0, stream, l, B, slots, sums, loss1);
  return hipGetLastError();
}

}  // namespace bsr
