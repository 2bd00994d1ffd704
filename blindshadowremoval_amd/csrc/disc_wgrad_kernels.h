// d d_total_loss / d the three discriminators' 54 trainable variables ON THE DEVICE, d_total_loss = disc_real + disc_fake, training=False.
// blindshadowremoval_amd/discriminator.py is the host statement (disc_grad) and writes the arithmetic out; pack.pack_discriminators_wgrad
// writes the chain's own blob (disc_wgrad_layout: the unfolded kernels and the per-channel vectors bias, inv, moving_mean, rstd).
//
// The forward chain of disc_kernels.h (seven launches, unchanged), then eleven more on the same stream, one after the other: no host
// synchronisation, no parallel branch, no floating-point atomic; every word a launch reads was written by an earlier launch of the same
// call.  Each launch covers all three discriminators (first_block routing).  All 2B rows are differentiated.
//    1  disc_wgrad_seed_kernel     a thread per four channels of a pixel of conv3's map, all 2B rows: the per-pixel seed read from the
//                                  logits the forward left in the scratch (a real row -w_k where the float32 term 1 - y is > 0, a fake
//                                  row +w_k where 1 + y is > 0, else 0; w_k = float32(1 / (B h_k^2))), gathered over the head's 16
//                                  taps (index order, float32, contraction off), times the slope of conv3's kept output.  Writes the
//                                  seed map as well.
//    2  disc_head_wgrad_kernel     the head's kernel gradient, narrow (64 channels x 16 taps) and not matrix work: a workgroup per
//                                  (discriminator, tap, one of 16 row chunks), a thread per channel and quarter of the chunk's pixels,
//                                  float64 products and sums in a fixed order -> [16 chunks][16][64] float64 partials.
//    3, 5, 7, 9  disc_wgrad_kernel  conv3, conv2, conv1, conv0: THE KERNEL GRADIENT on v_mfma_f32_32x32x2_f32.  A GEMM with M = 16 C_in
//                                  (tap, input channel), N = C_out and the reduction over the 2B Ho^2 output pixels, which is the
//                                  instruction's k.  The reduction is split over P workgroups per discriminator (a third of the tile
//                                  count, at most its share by tile count of 630 over the chunks: the three scales' workgroups then
//                                  walk about equally many tiles) and the rows of M over C_in / 8 channel chunks: workgroup (p, chunk) walks the 8 x 16 output
//                                  tiles p, p + P, ... of all 2B rows in order; the next tile's global loads are issued into registers
//                                  before the tile's matrix work and stored to LDS after it.  Per tile it stages the chunk's 18 x 34
//                                  input patch (halo included; padding and pixels outside the map stored as 0; 8 floats a pixel, so the
//                                  32 rows a lane group reads, four adjacent taps x 8 channels, are 32 consecutive words: no bank is
//                                  met twice) and the tile's 128 x N gz (pixels outside the map 0; a lane group reads 32 consecutive
//                                  channels).  Wave w owns the tap row a = w: M rows (b, c), NT = N / 32 accumulator tiles kept in
//                                  registers across the tiles; 64 k-steps of two pixels a tile.  Chunk 0 also adds gz per channel in
//                                  float64 (a thread per channel, pixels in order).  Writes a float32 partial [128][N] and a float64
//                                  partial [N].  LDS: 19.1 KB + 16 or 32 KB.
//    4, 6, 8  disc_dgrad_kernel    of disc_grad_kernels.h, unchanged, through its argument struct: over all 2B rows, conv3 -> conv2 ->
//                                  conv1, the slope from the kept activation's row 0 on.  conv0's input gradient is not formed.
//   10  disc_wgrad_fold_kernel     a thread per element (tap, c, o) of the twelve kernels: the partials in index order in float64 -> W
//                                  (float64, kept for d gamma) and d kernel = inv[o] W rounded once, HWIO, rows c = 6, 7 of conv0
//                                  dropped.
//   11  disc_wgrad_finish_kernel   a wave per output: per channel of the twelve layers S = sum gz (the partials in lane-strided order,
//                                  then the wave butterfly) and KW = sum_{tap, c} K W -> d beta = S, d bias = inv S, d gamma = ((KW +
//                                  bias S) - moving_mean S) rstd, since c = sum K x + bias; per (discriminator, tap) the head's kernel
//                                  gradient from its 16 partials; per discriminator the head's bias gradient, the sum of the seed.
//
// SCRATCH: the forward's (disc_map_offset, unchanged), then per discriminator the gradient maps gz at conv0..conv3's BatchNormalization
// output [2B][.][.][32, 32, 64, 64] and the seed [2B][h][h] (disc_wgrad_map_offset, layer 1..5), then the partials and W (DiscWgradPlan).
// GRADS: the 54 variables dense in their own shapes in weights.discriminator_trainable_names' order (disc_wgrad_var_offset).
#pragma once
#include "disc_grad_kernels.h"
#include "grad_common.h"

namespace bsr {

constexpr int kDiscWgradLaunches = 11;
constexpr int kDiscWgradCap = 630;             // workgroups of a kernel-gradient launch over its C_in / 8 chunks, shared among the three discriminators by tile count
constexpr int kDiscWgradMinTiles = 3;          // P = min(share, ceil(tiles / 3)): the write-out of a partial is paid by at least three tiles where there are three
constexpr int kDiscWgradLd = 8;                // floats per staged input pixel: unpadded, see above
constexpr int kDiscHeadChunks = 16;
constexpr int kDiscVars = 54, kDiscVarsPer = 18;
constexpr int kDiscRealCin0 = 6;

__host__ __device__ inline int disc_real_cin(int i) { return i == 0 ? kDiscRealCin0 : disc_cin(i); }
// float offset of layer i's record inside one discriminator's record of pack.pack_discriminators_wgrad's blob: K [16][C_in8][N], then
// bias, inv, moving_mean, rstd [4][N]; i = 4: the record's floats
__host__ __device__ inline size_t disc_wgrad_w_off(int i) {
  size_t o = 0;
  for (int j = 0; j < i; ++j) o += (size_t)kDiscTaps * disc_cin(j) * disc_ch(j) + 4 * (size_t)disc_ch(j);
  return o;
}
// float offset of trainable variable `index` (0..53) inside grads; 54: the total.  Per discriminator: conv_stack/0..3 {kernel, bias,
// gamma, beta}, then conv2 {kernel, bias}
__host__ __device__ inline size_t disc_wgrad_var_offset(int index) {
  size_t o = 0;
  for (int v = 0; v < index; ++v) {
    const int j = v % kDiscVarsPer;
    if (j < 16) o += (j & 3) == 0 ? (size_t)kDiscTaps * disc_real_cin(j >> 2) * disc_ch(j >> 2) : (size_t)disc_ch(j >> 2);
    else o += j == 16 ? (size_t)kDiscTaps * 64 : 1;
  }
  return o;
}
__host__ __device__ inline int disc_wgrad_map_ch(int l) { return l <= kDiscLayers ? disc_ch(l - 1) : 1; }
__host__ __device__ inline size_t disc_wgrad_map_bytes(int B, int S, int k, int l) {
  const size_t s = (size_t)disc_side(S, k, l);
  return ((size_t)2 * B * s * s * disc_wgrad_map_ch(l) * sizeof(float) + 255) & ~size_t(255);
}
// byte offset of gradient map l (1..4: gz at conv0..conv3; 5: the seed) of discriminator k (0-based) inside the scratch; (3, 1): the
// end of the maps
__host__ __device__ inline size_t disc_wgrad_map_offset(int B, int S, int k, int l) {
  size_t o = disc_map_offset(B, S, 3, 0);
  for (int kk = 0; kk < 3; ++kk)
    for (int ll = 1; ll <= kDiscLayers + 1; ++ll) {
      if (kk == k && ll == l) return o;
      o += disc_wgrad_map_bytes(B, S, kk, ll);
    }
  return o;
}
__host__ __device__ inline float* disc_wgrad_map(void* scratch, int B, int S, int k, int l) {
  return reinterpret_cast<float*>(static_cast<unsigned char*>(scratch) + disc_wgrad_map_offset(B, S, k, l));
}

// What follows the maps in the scratch, per (discriminator k, layer i): the float32 kernel partials [P][C_in / 8][128][N], the float64
// per-channel partials [P][N], W float64 [16][C_in8][N]; then the head's float64 partials [3][16][16][64].  Byte offsets.
struct DiscWgradPlan {
  int tiles_x[3][kDiscLayers], tiles[3][kDiscLayers], T[3][kDiscLayers], P[3][kDiscLayers];
  size_t wpart[3][kDiscLayers], spart[3][kDiscLayers], W[3][kDiscLayers], hpart, total;
};
inline DiscWgradPlan disc_wgrad_plan(int B, int S) {
  DiscWgradPlan pl;
  BumpBytes bump{disc_wgrad_map_offset(B, S, 3, 1)};
  for (int i = 0; i < kDiscLayers; ++i) {
    size_t all = 0;
    for (int k = 0; k < 3; ++k) {
      const int Ho = disc_side(S, k, i + 1);
      pl.tiles_x[k][i] = (Ho + kDiscTW - 1) / kDiscTW;
      pl.tiles[k][i] = pl.tiles_x[k][i] * ((Ho + kDiscTH - 1) / kDiscTH);
      pl.T[k][i] = 2 * B * pl.tiles[k][i];
      all += (size_t)pl.T[k][i];
    }
    for (int k = 0; k < 3; ++k) {
      const size_t cap = (size_t)(kDiscWgradCap / (disc_cin(i) / kDiscCC));
      const size_t share = (cap * (size_t)pl.T[k][i] + all - 1) / all, want = ((size_t)pl.T[k][i] + kDiscWgradMinTiles - 1) / kDiscWgradMinTiles;
      pl.P[k][i] = (int)(want < share ? want : share);
    }
  }
  for (int k = 0; k < 3; ++k)
    for (int i = 0; i < kDiscLayers; ++i) {
      const size_t mn = (size_t)kDiscTaps * disc_cin(i) * disc_ch(i);
      pl.wpart[k][i] = bump.take((size_t)pl.P[k][i] * mn * sizeof(float));
      pl.spart[k][i] = bump.take((size_t)pl.P[k][i] * disc_ch(i) * sizeof(double));
      pl.W[k][i] = bump.take(mn * sizeof(double));
    }
  pl.hpart = bump.take((size_t)3 * kDiscHeadChunks * kDiscTaps * 64 * sizeof(double));
  pl.total = bump.o;
  return pl;
}

// ---- launch 1: the seed and the head's input gradient
struct DiscSeedArgs {
  const float* w[3];       // the head's [16][64] of the forward blob
  const float* y[3];       // conv3's kept output [2B][h][h][64]
  const float* logit[3];   // [2B][h][h]
  float* g[3];             // gz at conv3 [2B][h][h][64]
  float* seed[3];          // [2B][h][h]
  float w_k[3];
  int h[3];
  unsigned first[3];       // the set's first thread
};

__device__ __forceinline__ float disc_hinge_seed(float y, bool real, float w_k) {
#pragma clang fp contract(off)
  const float t = real ? 1.0f - y : 1.0f + y;
  return t > 0.f ? (real ? -w_k : w_k) : 0.f;
}

__global__ __launch_bounds__(256) void disc_wgrad_seed_kernel(const DiscSeedArgs a, unsigned total, int B) {
#pragma clang fp contract(off)
  const unsigned p = blockIdx.x * 256u + threadIdx.x;
  if (p >= total) return;
  const int k = p >= a.first[2] ? 2 : p >= a.first[1] ? 1 : 0;
  const unsigned r = p - a.first[k];
  const int h = a.h[k];
  const int c4 = (int)(r % 16u);
  const unsigned pix = r / 16u;
  const int x = (int)(pix % (unsigned)h), y = (int)((pix / (unsigned)h) % (unsigned)h);
  const unsigned row = pix / (unsigned)(h * h);
  const bool real = row < (unsigned)B;
  const float* lg = a.logit[k] + (size_t)row * h * h;
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int t = 0; t < kDiscTaps; ++t) {
    const int oy = y - (t >> 2) + 1, ox = x - (t & 3) + 1;               // the head's output that read this pixel at tap t
    if (oy >= 0 && oy < h && ox >= 0 && ox < h) {
      const float sd = disc_hinge_seed(lg[oy * h + ox], real, a.w_k[k]);
      const f32x4 w = reinterpret_cast<const f32x4*>(a.w[k] + t * 64)[c4];
#pragma unroll
      for (int i = 0; i < 4; ++i) s[i] = s[i] + sd * w[i];
    }
  }
  const f32x4 yv = reinterpret_cast<const f32x4*>(a.y[k])[(size_t)pix * 16 + c4];
  f32x4 o;
#pragma unroll
  for (int i = 0; i < 4; ++i) o[i] = s[i] * disc_slope(yv[i]);
  reinterpret_cast<f32x4*>(a.g[k])[(size_t)pix * 16 + c4] = o;
  if (c4 == 0) a.seed[k][pix] = disc_hinge_seed(lg[y * h + x], real, a.w_k[k]);
}

// ---- launch 2: the head's kernel gradient, float64 partials
struct DiscHeadWgradArgs {
  const float* x[3];       // conv3's kept output [2B][h][h][64]
  const float* seed[3];    // [2B][h][h]
  int h[3];
  double* part;            // [3][16 chunks][16 taps][64]
};

// grid (3 * 16 * 16): workgroup (k, tap, chunk); chunk j owns the rows [j R, (j + 1) R) of the 2B, R = ceil(2B / 16)
__global__ __launch_bounds__(256) void disc_head_wgrad_kernel(const DiscHeadWgradArgs a, int B) {
  __shared__ double s_red[4][64];
  const int tid = threadIdx.x, c = tid & 63, slice = tid >> 6;
  const int k = blockIdx.x / (kDiscTaps * kDiscHeadChunks), tap = (blockIdx.x / kDiscHeadChunks) % kDiscTaps, chunk = blockIdx.x % kDiscHeadChunks;
  const int h = a.h[k], hh = h * h;
  const int R = (2 * B + kDiscHeadChunks - 1) / kDiscHeadChunks;
  const int r0 = chunk * R, r1 = min(r0 + R, 2 * B);
  const int dy = (tap >> 2) - 1, dx = (tap & 3) - 1;
  double acc = 0.0;
  for (int row = r0; row < r1; ++row) {
    const float* x = a.x[k] + (size_t)row * hh * 64;
    const float* sd = a.seed[k] + (size_t)row * hh;
    for (int p = slice; p < hh; p += 4) {
      const int iy = p / h + dy, ix = p % h + dx;
      if (iy >= 0 && iy < h && ix >= 0 && ix < h) acc += (double)sd[p] * (double)x[((size_t)iy * h + ix) * 64 + c];
    }
  }
  s_red[slice][c] = acc;
  __syncthreads();
  if (slice == 0) a.part[((size_t)(k * kDiscHeadChunks + chunk) * kDiscTaps + tap) * 64 + c] = ((s_red[0][c] + s_red[1][c]) + s_red[2][c]) + s_red[3][c];
}

// ---- launches 3, 5, 7, 9: the kernel gradient
struct DiscWgradSet {
  const float* x;         // the layer's input [2B][H][H][CIN]
  const float* gz;        // [2B][Ho][Ho][N]
  float* wpart;           // [P][CIN / 8][128][N]
  double* spart;          // [P][N]
  int H, Ho, tiles_x, tiles, T, P;    // tiles per row; T = 2B * tiles
  unsigned first_block;
};
struct DiscWgradArgs { DiscWgradSet d[3]; };

template <int CIN, int N>
__global__ __launch_bounds__(256) void disc_wgrad_kernel(const DiscWgradArgs args) {
  static_assert(CIN % kDiscCC == 0 && N % 32 == 0 && N <= 64, "shape");
  constexpr int NT = N / 32, NCH = CIN / kDiscCC;
  __shared__ __attribute__((aligned(16))) float s_in[kDiscPH * kDiscPW * kDiscWgradLd];
  __shared__ __attribute__((aligned(16))) float s_gz[kDiscTH * kDiscTW * N];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int k = blockIdx.x >= args.d[2].first_block ? 2 : blockIdx.x >= args.d[1].first_block ? 1 : 0;
  const DiscWgradSet& d = args.d[k];
  const unsigned r = blockIdx.x - d.first_block;
  const int p = (int)(r / (unsigned)NCH), cc = (int)(r % (unsigned)NCH);
  const int H = d.H, Ho = d.Ho;
  const int m = lane & 31, kh = lane >> 5;
  // the lane's row of M: tap (a = wave, b = m >> 3), channel m & 7 of the chunk; its pixel of a k-step: 2 kk + kh
  const int a_base = (wave * kDiscPW + (m >> 3)) * kDiscWgradLd + (m & 7);

  f32x16 acc[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[nt][i] = 0.f;
  double sacc = 0.0;

  constexpr int PATCH = kDiscPH * kDiscPW * 2, PV = (PATCH + 255) / 256, GV = kDiscTH * kDiscTW * N / 4 / 256;
  static_assert(kDiscTH * kDiscTW * N / 4 % 256 == 0, "gz per thread");
  f32x4 pv[PV], gv[GV];
  auto fetch = [&](int t) {
    const int row = t / d.tiles, tile = t % d.tiles;
    const int oy0 = (tile / d.tiles_x) * kDiscTH, ox0 = (tile % d.tiles_x) * kDiscTW;
    const int iy0 = 2 * oy0 - 1, ix0 = 2 * ox0 - 1;                    // SAME, stride 2, 4 taps: 1 before on even sizes and on 1 x 1
    const float* in = d.x + (size_t)row * H * H * CIN;
    const float* gz = d.gz + (size_t)row * Ho * Ho * N;
#pragma unroll
    for (int j = 0; j < PV; ++j) {
      const int i = tid + j * 256;
      const int pix = i >> 1, half = i & 1;
      const int iy = iy0 + pix / kDiscPW, ix = ix0 + pix % kDiscPW;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (i < PATCH && iy >= 0 && iy < H && ix >= 0 && ix < H) v = *reinterpret_cast<const f32x4*>(in + ((size_t)iy * H + ix) * CIN + cc * kDiscCC + half * 4);
      pv[j] = v;
    }
#pragma unroll
    for (int j = 0; j < GV; ++j) {
      const int i = tid + j * 256;
      const int q = i / (N / 4), n4 = i % (N / 4);
      const int oy = oy0 + (q >> 4), ox = ox0 + (q & 15);
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (oy < Ho && ox < Ho) v = *reinterpret_cast<const f32x4*>(gz + ((size_t)oy * Ho + ox) * N + n4 * 4);
      gv[j] = v;
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (int j = 0; j < PV; ++j) {
      const int i = tid + j * 256;
      if (i < PATCH) *reinterpret_cast<f32x4*>(s_in + (i >> 1) * kDiscWgradLd + (i & 1) * 4) = pv[j];
    }
#pragma unroll
    for (int j = 0; j < GV; ++j) reinterpret_cast<f32x4*>(s_gz)[tid + j * 256] = gv[j];
  };

  fetch(p);
  for (int t = p; t < d.T; t += d.P) {
    if (t != p) __syncthreads();                                        // every wave is done with the previous tile's LDS
    stage();
    __syncthreads();
    if (t + d.P < d.T) fetch(t + d.P);                                  // in flight behind the matrix work below
#pragma unroll 8
    for (int kk = 0; kk < kDiscTH * kDiscTW / 2; ++kk) {
      const int q = 2 * kk + kh;
      const float av = s_in[a_base + ((2 * (q >> 4)) * kDiscPW + 2 * (q & 15)) * kDiscWgradLd];
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, s_gz[q * N + nt * 32 + m], acc[nt], 0, 0, 0);
    }
    if (cc == 0 && tid < N) {
      double s = 0.0;
      for (int q = 0; q < kDiscTH * kDiscTW; ++q) s += (double)s_gz[q * N + tid];
      sacc += s;
    }
  }
  float* wp = d.wpart + ((size_t)p * NCH + cc) * (128 * N);
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int mr = (i & 3) + 8 * (i >> 2) + 4 * kh;                  // the accumulator's row: (b, c) = (mr >> 3, mr & 7) of tap row `wave`
      wp[(size_t)(wave * 32 + mr) * N + nt * 32 + m] = acc[nt][i];
    }
  if (cc == 0 && tid < N) d.spart[(size_t)p * N + tid] = sacc;
}

// ---- launch 10: the partials -> W and d kernel
struct DiscFoldSet {
  const float* wpart;     // [P][cin8 / 8][128][N]
  const float* inv;       // [N]
  double* W;              // [16][cin8][N]
  float* out;             // the variable [16][cin][N]
  int P, cin8, cin, N;
  unsigned first;         // the set's first thread
};
struct DiscFoldArgs { DiscFoldSet s[3 * kDiscLayers]; };

__global__ __launch_bounds__(256) void disc_wgrad_fold_kernel(const DiscFoldArgs args, unsigned total) {
  const unsigned e = blockIdx.x * 256u + threadIdx.x;
  if (e >= total) return;
  int j = 0;
  for (int i = 1; i < 3 * kDiscLayers; ++i)
    if (e >= args.s[i].first) j = i;
  const DiscFoldSet& s = args.s[j];
  const unsigned r = e - s.first;
  const int n = (int)(r % (unsigned)s.N), c = (int)((r / (unsigned)s.N) % (unsigned)s.cin8), tap = (int)(r / (unsigned)(s.N * s.cin8));
  const size_t per = (size_t)kDiscTaps * s.cin8 * s.N;
  const float* src = s.wpart + ((size_t)(c >> 3) * 128 + (tap >> 2) * 32 + (tap & 3) * 8 + (c & 7)) * s.N + n;
  double a = 0.0;
#pragma unroll 8
  for (int p = 0; p < s.P; ++p) a += (double)src[(size_t)p * per];      // in index order; the loads of eight partials are in flight together
  s.W[r] = a;
  if (c < s.cin) s.out[((size_t)tap * s.cin + c) * s.N + n] = (float)((double)s.inv[n] * a);
}

// ---- launch 11: the per-channel gradients and the head's
struct DiscFinishSet {
  const double* spart;    // [P][N]
  const double* W;        // [16 cin8][N]
  const float* K;         // [16 cin8][N], then bias, inv, moving_mean, rstd [4][N]
  float* bias; float* gamma; float* beta;
  int P, M, N;            // M = 16 cin8
  unsigned first;         // the set's first workgroup
};
struct DiscFinishArgs {
  DiscFinishSet s[3 * kDiscLayers];
  const double* hpart;    // [3][16][16][64]
  const float* seed[3];
  unsigned n_seed[3];     // 2B h^2
  float* head_kernel[3]; float* head_bias[3];
  unsigned channels;      // the twelve layers' channels: 576
};

// grid (576 + 48 + 3), one wave each
__global__ __launch_bounds__(64) void disc_wgrad_finish_kernel(const DiscFinishArgs args) {
  const int lane = threadIdx.x;
  const unsigned b = blockIdx.x;
  if (b < args.channels) {
    int j = 0;
    for (int i = 1; i < 3 * kDiscLayers; ++i)
      if (b >= args.s[i].first) j = i;
    const DiscFinishSet& s = args.s[j];
    const int o = (int)(b - s.first);
    double S = 0.0, KW = 0.0;
    for (int p = lane; p < s.P; p += 64) S += s.spart[(size_t)p * s.N + o];
    for (int mm = lane; mm < s.M; mm += 64) KW += (double)s.K[(size_t)mm * s.N + o] * s.W[(size_t)mm * s.N + o];
    S = wave_sum(S);
    KW = wave_sum(KW);
    if (lane == 0) bn_channel_grads(KW, S, s.K + (size_t)s.M * s.N, s.N, o, s.bias[o], s.gamma[o], s.beta[o]);
  } else if (b < args.channels + 3 * kDiscTaps) {
    const int k = (int)(b - args.channels) / kDiscTaps, tap = (int)(b - args.channels) % kDiscTaps;
    double a = 0.0;
    for (int ch = 0; ch < kDiscHeadChunks; ++ch) a += args.hpart[((size_t)(k * kDiscHeadChunks + ch) * kDiscTaps + tap) * 64 + lane];
    args.head_kernel[k][tap * 64 + lane] = (float)a;
  } else {
    const int k = (int)(b - args.channels - 3 * kDiscTaps);
    double a = 0.0;
    for (unsigned i = lane; i < args.n_seed[k]; i += 64) a += (double)args.seed[k][i];
    a = wave_sum(a);
    if (lane == 0) args.head_bias[k][0] = (float)a;
  }
}

template <int CIN, int N>
inline hipError_t launch_disc_wgrad_layer(const DiscWgradPlan& pl, int layer, int B, int S, void* scratch, hipStream_t stream) {
  unsigned char* base = static_cast<unsigned char*>(scratch);
  DiscWgradArgs a;
  unsigned blocks = 0;
  for (int k = 0; k < 3; ++k) {
    DiscWgradSet& d = a.d[k];
    d.x = disc_map(scratch, B, S, k, layer);
    d.gz = disc_wgrad_map(scratch, B, S, k, layer + 1);
    d.wpart = reinterpret_cast<float*>(base + pl.wpart[k][layer]);
    d.spart = reinterpret_cast<double*>(base + pl.spart[k][layer]);
    d.H = disc_side(S, k, layer);
    d.Ho = disc_side(S, k, layer + 1);
    d.tiles_x = pl.tiles_x[k][layer];
    d.tiles = pl.tiles[k][layer];
    d.T = pl.T[k][layer];
    d.P = pl.P[k][layer];
    d.first_block = blocks;
    blocks += (unsigned)d.P * (unsigned)(CIN / kDiscCC);
  }
  hipLaunchKernelGGL((disc_wgrad_kernel<CIN, N>), dim3(blocks), dim3(256), 0, stream, a);
  return hipGetLastError();
}

// disc_dgrad_kernel over all 2B rows: gz at `layer` -> gz at `layer - 1`, the slope from the kept activation of the layer below
template <int C_OUT, int C_IN>
inline hipError_t launch_disc_wgrad_dgrad(const float* dblob, int layer, int B, int S, void* scratch, hipStream_t stream) {
  DiscDgradArgs a;
  unsigned blocks = 0;
  for (int k = 0; k < 3; ++k) {
    DiscDgradSet& d = a.d[k];
    d.H = disc_side(S, k, layer);
    d.Ho = disc_side(S, k, layer + 1);
    d.gy = disc_wgrad_map(scratch, B, S, k, layer + 1);
    d.gx = disc_wgrad_map(scratch, B, S, k, layer);
    d.y = disc_map(scratch, B, S, k, layer);
    d.w = dblob + (size_t)k * disc_dgrad_w_off(kDiscLayers) + disc_dgrad_w_off(layer);
    d.tiles_x = (d.Ho + kDiscQW - 1) / kDiscQW;
    d.tiles = d.tiles_x * ((d.Ho + kDiscQH - 1) / kDiscQH);
    d.first_block = blocks;
    blocks += (unsigned)(2 * B) * (unsigned)d.tiles;
  }
  hipLaunchKernelGGL((disc_dgrad_kernel<C_OUT, C_IN>), dim3(blocks), dim3(256), 0, stream, a);
  return hipGetLastError();
}

// The forward chain, then the first `stop_after` of the eleven launches above (kDiscWgradLaunches: all of them; fewer are for the tests'
// stage-by-stage comparison).
inline hipError_t launch_disc_wgrad(const float* blob, const float* dblob, const float* wblob, const float* gt, const float* con, const float* mask_sv, int B,
                                    int S, double* sums, float* losses3, float* logits, float* grads, void* scratch, int stop_after, hipStream_t stream) {
  hipError_t e = launch_disc_losses(blob, gt, con, mask_sv, B, S, sums, losses3, logits, scratch, stream);
  if (e != hipSuccess) return e;
  const DiscWgradPlan pl = disc_wgrad_plan(B, S);
  unsigned char* base = static_cast<unsigned char*>(scratch);
  if (stop_after < 1) return hipSuccess;
  {
    DiscSeedArgs a;
    unsigned total = 0;
    for (int k = 0; k < 3; ++k) {
      const int h = disc_side(S, k, kDiscLayers);
      a.w[k] = blob + (size_t)k * disc_record_floats() + disc_w_off(kDiscLayers);
      a.y[k] = disc_map(scratch, B, S, k, kDiscLayers);
      a.logit[k] = disc_map(scratch, B, S, k, kDiscLayers + 1);
      a.g[k] = disc_wgrad_map(scratch, B, S, k, kDiscLayers);
      a.seed[k] = disc_wgrad_map(scratch, B, S, k, kDiscLayers + 1);
      a.w_k[k] = disc_seed_w(B, S, k);
      a.h[k] = h;
      a.first[k] = total;
      total += (unsigned)(2 * B) * (unsigned)(h * h) * 16u;
    }
    hipLaunchKernelGGL(disc_wgrad_seed_kernel, dim3((total + 255) / 256), dim3(256), 0, stream, a, total, B);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (stop_after < 2) return hipSuccess;
  {
    DiscHeadWgradArgs a;
    for (int k = 0; k < 3; ++k) {
      a.x[k] = disc_map(scratch, B, S, k, kDiscLayers);
      a.seed[k] = disc_wgrad_map(scratch, B, S, k, kDiscLayers + 1);
      a.h[k] = disc_side(S, k, kDiscLayers);
    }
    a.part = reinterpret_cast<double*>(base + pl.hpart);
    hipLaunchKernelGGL(disc_head_wgrad_kernel, dim3(3 * kDiscTaps * kDiscHeadChunks), dim3(256), 0, stream, a, B);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (stop_after < 3) return hipSuccess;
  if ((e = launch_disc_wgrad_layer<64, 64>(pl, 3, B, S, scratch, stream)) != hipSuccess) return e;
  if (stop_after < 4) return hipSuccess;
  if ((e = launch_disc_wgrad_dgrad<64, 64>(dblob, 3, B, S, scratch, stream)) != hipSuccess) return e;
  if (stop_after < 5) return hipSuccess;
  if ((e = launch_disc_wgrad_layer<32, 64>(pl, 2, B, S, scratch, stream)) != hipSuccess) return e;
  if (stop_after < 6) return hipSuccess;
  if ((e = launch_disc_wgrad_dgrad<64, 32>(dblob, 2, B, S, scratch, stream)) != hipSuccess) return e;
  if (stop_after < 7) return hipSuccess;
  if ((e = launch_disc_wgrad_layer<32, 32>(pl, 1, B, S, scratch, stream)) != hipSuccess) return e;
  if (stop_after < 8) return hipSuccess;
  if ((e = launch_disc_wgrad_dgrad<32, 32>(dblob, 1, B, S, scratch, stream)) != hipSuccess) return e;
  if (stop_after < 9) return hipSuccess;
  if ((e = launch_disc_wgrad_layer<8, 32>(pl, 0, B, S, scratch, stream)) != hipSuccess) return e;
  if (stop_after < 10) return hipSuccess;
  {
    DiscFoldArgs a;
    unsigned total = 0;
    for (int k = 0; k < 3; ++k)
      for (int i = 0; i < kDiscLayers; ++i) {
        DiscFoldSet& s = a.s[k * kDiscLayers + i];
        s.wpart = reinterpret_cast<const float*>(base + pl.wpart[k][i]);
        s.inv = wblob + (size_t)k * disc_wgrad_w_off(kDiscLayers) + disc_wgrad_w_off(i) + (size_t)kDiscTaps * disc_cin(i) * disc_ch(i) + disc_ch(i);
        s.W = reinterpret_cast<double*>(base + pl.W[k][i]);
        s.out = grads + disc_wgrad_var_offset(k * kDiscVarsPer + 4 * i);
        s.P = pl.P[k][i];
        s.cin8 = disc_cin(i);
        s.cin = disc_real_cin(i);
        s.N = disc_ch(i);
        s.first = total;
        total += (unsigned)(kDiscTaps * disc_cin(i) * disc_ch(i));
      }
    hipLaunchKernelGGL(disc_wgrad_fold_kernel, dim3((total + 255) / 256), dim3(256), 0, stream, a, total);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (stop_after < 11) return hipSuccess;
  DiscFinishArgs a;
  unsigned blocks = 0;
  for (int k = 0; k < 3; ++k) {
    for (int i = 0; i < kDiscLayers; ++i) {
      DiscFinishSet& s = a.s[k * kDiscLayers + i];
      s.spart = reinterpret_cast<const double*>(base + pl.spart[k][i]);
      s.W = reinterpret_cast<const double*>(base + pl.W[k][i]);
      s.K = wblob + (size_t)k * disc_wgrad_w_off(kDiscLayers) + disc_wgrad_w_off(i);
      s.bias = grads + disc_wgrad_var_offset(k * kDiscVarsPer + 4 * i + 1);
      s.gamma = grads + disc_wgrad_var_offset(k * kDiscVarsPer + 4 * i + 2);
      s.beta = grads + disc_wgrad_var_offset(k * kDiscVarsPer + 4 * i + 3);
      s.P = pl.P[k][i];
      s.M = kDiscTaps * disc_cin(i);
      s.N = disc_ch(i);
      s.first = blocks;
      blocks += (unsigned)disc_ch(i);
    }
    const int h = disc_side(S, k, kDiscLayers);
    a.seed[k] = disc_wgrad_map(scratch, B, S, k, kDiscLayers + 1);
    a.n_seed[k] = (unsigned)(2 * B) * (unsigned)(h * h);
    a.head_kernel[k] = grads + disc_wgrad_var_offset(k * kDiscVarsPer + 16);
    a.head_bias[k] = grads + disc_wgrad_var_offset(k * kDiscVarsPer + 17);
  }
  a.hpart = reinterpret_cast<const double*>(base + pl.hpart);
  a.channels = blocks;
  hipLaunchKernelGGL(disc_wgrad_finish_kernel, dim3(blocks + 3 * kDiscTaps + 3), dim3(64), 0, stream, a);
  return hipGetLastError();
}

}  // namespace bsr
