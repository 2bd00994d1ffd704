// The generator's backward pass from the output down, ON THE DEVICE, training=False: the colour tail clr_conv1 (3x3, cat[gs, f] 65 -> 16,
// BN, LeakyReLU), clr_conv2 (1x1, 16 -> 16, BN, LeakyReLU), clr_conv3 (1x1, 16 -> 3).  Given g_con = d loss / d con_rgb (and g_gs, what
// reaches gs directly) it writes the ten variable gradients, d_f at clr_up3's output and the complete d_gs.
// blindshadowremoval_amd/generator_grad.py is the host statement (tail_grad); pack.pack_clr_tail_grad writes the blob (clr_tail_grad_layout).
//
// Six launches on the caller's stream, one after the other: no host synchronisation, no second stream, no floating-point atomic; every
// word a launch reads was written by an earlier launch of the same call, so a call repeats its bits.
//    1  conv_n16_kernel<3,3,GS,!TAIL,2>   of conv_n16.h, unchanged, through its argument struct: a1 [B,H,W,16], the forward's arithmetic
//                                  (the fused forward never stores the tail's intermediates).
//    2  clr_tail_pixel_kernel      a thread per pixel, a workgroup per 256 consecutive pixels, persistent over chunks g, g + grid, ...:
//                                  reads a1[16] and g_con[3], re-forms z2 = a1 k2f + b2f and a2, forms gz2 = LeakyReluGrad(G K3^T, a2) and
//                                  gz1 = LeakyReluGrad(gz2 k2f^T, a1) in float32; writes gz1 (and a2 when kept).  The 339 sums a1 (x) gz2
//                                  (16 x 16), a2 (x) G (16 x 3), sum G, sum gz1, sum gz2 go through LDS (20 floats a pixel: a thread's
//                                  four 16-byte stores meet no bank twice; a summing thread reads one word all its wave's lanes share
//                                  or 16 consecutive ones): thread j owns one sum and adds the chunk's 256 pixels in order in float64
//                                  (a product of two floats is exact there), kept in a register across the chunks -> [grid][344] float64.
//    3  clr_wgrad_kernel           clr_conv1's KERNEL GRADIENT on v_mfma_f32_16x16x4_f32: a GEMM with M = 9 taps x 65 channels, N = 16
//                                  (exactly one tile) and the reduction over the B H W output pixels, which is the instruction's k.
//                                  Workgroup (p, cc) owns the 16 f channels [16 cc, 16 cc + 16) and walks the 8 x 32 output tiles p, p + P,
//                                  ... of all B images in order; the next tile's global loads are issued into registers before the
//                                  tile's matrix work and stored to LDS after it.  Per tile it stages the chunk's 10 x 34 input patch
//                                  (halo included, zero outside the image; 16 floats a pixel UNPADDED: the A operand of a k-step is
//                                  channel r of four consecutive pixels = 64 consecutive words, no bank met twice), the tile's 256 x 16
//                                  gz1 (the B operand: 64 consecutive words likewise) and the 10 x 34 gs patch.  Wave w owns the tile's
//                                  rows 2w, 2w + 1 as its 16 k-steps and ALL nine tap tiles (nine accumulators: one B read serves nine
//                                  instructions); chunk 0 adds a tenth, the gs channel's nine rows (row r = tap r, rows 9..15 fed 0).
//                                  At the end the four waves' accumulators are added through LDS in wave order -> float32 partial
//                                  [P][4][160][16] (rows 16 tap + c; 144 + tap for gs).
//    4  clr_dgrad_kernel           clr_conv1's DATA GRADIENT, same instruction: d_f[pixel][c] = sum_{tap, o} gz1[pixel + tap - 1][o]
//                                  k1f[2 - ta, 2 - tb, 1 + c, o] (the BN factor inv1 is inside the folded kernel, so gz1 is read as it
//                                  is), M = 64 channels in four tiles, N = 16 pixels, k = 9 x 16 with nothing padded.  Persistent
//                                  workgroups keep the flipped kernel in LDS (20 floats a row: the 16-byte operand reads of 16 rows
//                                  meet every bank once) and walk 8 x 32 tiles, staging the 10 x 34 gz1 patch (20 floats a pixel) with
//                                  the next tile's loads in flight behind the matrix work.  The accumulator is four consecutive
//                                  channels of a pixel: one 16-byte store.  The 65th output, d_gs, is a dot product of 144 a pixel on
//                                  the vector pipe, a thread per pixel, from the same LDS patch, g_gs added last in float32.
//    5  clr_fold_kernel            a thread per element (tap, c, o) of K1: the P partials in index order in float64 -> W1 (float64,
//                                  kept for d gamma1) and d K1 = inv1[o] W1 rounded once; a wave per sum of launch 2: the partials in
//                                  lane-strided order, then the wave butterfly -> S [344] float64.
//    6  clr_finish_kernel          per channel of clr_conv1 / clr_conv2: S = sum gz, KW = sum K W -> d beta = S, d bias = inv S,
//                                  d gamma = ((KW + bias S) - moving_mean S) rstd, since c = sum K x + bias; d K2 = inv2 (a1 (x) gz2),
//                                  d K3 = a2 (x) G, d b3 = sum G.
//
// SCRATCH (ClrTailPlan): a1, a2, gz1 [B,H,W,16], then the float64 partials of launch 2, the float32 partials of launch 3, W1 and S.
// GRADS: the ten variables dense in their own shapes in weights.generator_tail_trainable_names' order (clr_tail_var_offset).
#pragma once
#include "conv_n16.h"
#include "grad_common.h"

namespace bsr {

constexpr int kClrTailLaunches = 6;
constexpr int kClrVars = 10;
constexpr int kClrTH = 8, kClrTW = 32, kClrPH = 10, kClrPW = 34, kClrPatch = kClrPH * kClrPW;    // conv_n16_kernel<3,3,..,RW=2>'s tile, and its patch with halo
constexpr int kClrLd = 20;                     // floats per pixel / weight row where 16-byte accesses must spread over the banks
constexpr int kClrSums = 339, kClrSumsLd = 344;        // launch 2's sums: [0,256) a1 (x) gz2, [256,304) a2 (x) G, [304,307) G, [307,323) gz1, [323,339) gz2
constexpr int kClrPixCap = 1024;               // workgroups of launch 2
constexpr int kClrWgradCap = 640;              // workgroups of launch 3 over its four channel chunks
constexpr int kClrWgradMinTiles = 4;           // P = min(cap / 4, ceil(tiles / 4)): a partial's write-out is paid by four tiles where there are four
constexpr int kClrWRows = 160;                 // rows of a launch-3 partial: 9 x 16 (tap, channel), then the gs channel's 16 (9 used)
constexpr int kClrDgradCap = 512;              // persistent workgroups of launch 4
constexpr int kClrK1 = 9 * 65 * 16;

// float offsets inside pack.pack_clr_tail_grad's blob (clr_tail_grad_layout)
constexpr size_t kClrOffFwdW = 0, kClrOffFwdB = 10368, kClrOffFwdGs = 10384, kClrOffTail = 10640, kClrOffDgradW = 10976, kClrOffDgradGs = 20192,
                 kClrOffK1 = 20336, kClrOffK2 = 29696, kClrOffVecs1 = 29952, kClrOffVecs2 = 30016, kClrBlobFloats = 30080;
constexpr int kClrTailFloats = 336;            // k2f [16][16] | b2f [16] | k3 [16][4]

// float offset of variable `index` (0..9) inside grads; 10: the total
__host__ __device__ inline size_t clr_tail_var_offset(int index) {
  const int n[kClrVars] = {kClrK1, 16, 16, 16, 256, 16, 16, 16, 48, 3};
  size_t o = 0;
  for (int v = 0; v < index && v < kClrVars; ++v) o += (size_t)n[v];
  return o;
}

inline bool clr_tail_size_ok(int B, int H, int W) {
  return B > 0 && H > 0 && W > 0 && H % kClrTH == 0 && W % kClrTW == 0 && (long long)B * H * W <= (1ll << 26);
}

// Byte offsets inside the scratch.  map[0..2]: a1, a2, gz1 [B,H,W,16]; map[3]: launch 2's partials [G][344] float64; map[4]: launch 3's
// [P][4][160][16] float32; map[5]: W1 [9][65][16] float64; map[6]: S [344] float64
struct ClrTailPlan {
  size_t npix;
  int tiles_x, tiles_per_img, T, P, G;
  size_t map[7], total;
};
inline ClrTailPlan clr_tail_plan(int B, int H, int W) {
  ClrTailPlan pl;
  pl.npix = (size_t)B * H * W;
  pl.tiles_x = W / kClrTW;
  pl.tiles_per_img = pl.tiles_x * (H / kClrTH);
  pl.T = B * pl.tiles_per_img;
  const int want = (pl.T + kClrWgradMinTiles - 1) / kClrWgradMinTiles;
  pl.P = want < kClrWgradCap / 4 ? want : kClrWgradCap / 4;
  const size_t chunks = pl.npix / 256;
  pl.G = (int)(chunks < (size_t)kClrPixCap ? chunks : (size_t)kClrPixCap);
  BumpBytes bump;
  for (int m = 0; m < 3; ++m) pl.map[m] = bump.take(pl.npix * 16 * sizeof(float));
  pl.map[3] = bump.take((size_t)pl.G * kClrSumsLd * sizeof(double));
  pl.map[4] = bump.take((size_t)pl.P * 4 * kClrWRows * 16 * sizeof(float));
  pl.map[5] = bump.take((size_t)kClrK1 * sizeof(double));
  pl.map[6] = bump.take((size_t)kClrSumsLd * sizeof(double));
  pl.total = bump.o;
  return pl;
}

__device__ __forceinline__ float clr_leaky_grad(float g, float a) { return a > 0.f ? g : kLeakyAlpha * g; }

// ---- launch 2: the two 1x1 layers' backward per pixel, and their sums
struct ClrPixelArgs {
  const float* a1;        // [npix][16]
  const float* g_con;     // [npix][3]
  const float* tail;      // k2f [16][16] | b2f [16] | k3 [16][4]
  float* gz1;             // [npix][16]
  float* a2;              // [npix][16], or null
  double* part;           // [grid][344]
  unsigned chunks;        // npix / 256
};

__global__ __launch_bounds__(256) void clr_tail_pixel_kernel(const ClrPixelArgs p) {
  __shared__ __attribute__((aligned(16))) float s_w[kClrTailFloats];
  __shared__ __attribute__((aligned(16))) float s_a[256 * kClrLd];        // a1, then a2
  __shared__ __attribute__((aligned(16))) float s_g[256 * kClrLd];        // gz2, then gz1
  __shared__ __attribute__((aligned(16))) float s_G[256 * 4 + 4];         // the last word holds 1
  const int tid = threadIdx.x;
  for (int i = tid; i < kClrTailFloats; i += 256) s_w[i] = p.tail[i];
  if (tid == 0) s_G[256 * 4] = 1.f;
  __syncthreads();
  // the second group of sums, thread j < 67: a2 (x) G for j < 48 (k = j / 3, c = j % 3), sum G for j < 51, sum gz1 for the rest
  const float* bx = tid < 48 ? s_a + tid / 3 : tid < 51 ? s_G + (tid - 48) : s_g + (tid - 51);
  const float* by = tid < 48 ? s_G + tid % 3 : s_G + 256 * 4;
  const int bxs = tid >= 48 && tid < 51 ? 4 : kClrLd, bys = tid < 48 ? 4 : 0;
  const float* k2f = s_w;
  const float* b2f = s_w + 256;
  const float* k3 = s_w + 272;
  double acc_a = 0.0, acc_b = 0.0, acc_c = 0.0;
  const int ak = tid >> 4, an = tid & 15;
  for (unsigned ch = blockIdx.x; ch < p.chunks; ch += gridDim.x) {
    // The two 16 x 16 products below read their weights from LDS row by row, and the empty statements keep it so.  Left alone the compiler
    // vectorises the transposed product across its rows, reads all 256 weights first and keeps them: 256 VGPRs + 36 AGPRs and one wave a
    // SIMD, against 108 registers and three (the LDS's limit) with the rows pinned.
    asm volatile("" ::: "memory");
    const size_t pix = (size_t)ch * 256 + tid;
    float a1[16], a2[16], gz2[16], gz1[16];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const f32x4 v = reinterpret_cast<const f32x4*>(p.a1)[pix * 4 + i];
#pragma unroll
      for (int e = 0; e < 4; ++e) a1[4 * i + e] = v[e];
    }
    const float G0 = p.g_con[pix * 3], G1 = p.g_con[pix * 3 + 1], G2 = p.g_con[pix * 3 + 2];
#pragma unroll
    for (int n = 0; n < 16; ++n) a2[n] = b2f[n];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
#pragma unroll
      for (int n = 0; n < 16; ++n) a2[n] = __builtin_fmaf(a1[k], k2f[k * 16 + n], a2[n]);
      asm volatile("" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int n = 0; n < 16; ++n) {
      a2[n] = leaky_relu(a2[n]);
      const float gy = __builtin_fmaf(G2, k3[n * 4 + 2], __builtin_fmaf(G1, k3[n * 4 + 1], G0 * k3[n * 4]));
      gz2[n] = clr_leaky_grad(gy, a2[n]);
    }
    asm volatile("" ::: "memory");
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      float s = 0.f;
#pragma unroll
      for (int n = 0; n < 16; ++n) s = __builtin_fmaf(gz2[n], k2f[k * 16 + n], s);
      asm volatile("" : "+v"(s));               // the row's sum is complete here, before the next row's weights are read
      gz1[k] = clr_leaky_grad(s, a1[k]);
      asm volatile("" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const f32x4 v1 = {gz1[4 * i], gz1[4 * i + 1], gz1[4 * i + 2], gz1[4 * i + 3]};
      const f32x4 v2 = {a2[4 * i], a2[4 * i + 1], a2[4 * i + 2], a2[4 * i + 3]};
      reinterpret_cast<f32x4*>(p.gz1)[pix * 4 + i] = v1;
      if (p.a2 != nullptr) reinterpret_cast<f32x4*>(p.a2)[pix * 4 + i] = v2;
      *reinterpret_cast<f32x4*>(s_a + tid * kClrLd + 4 * i) = f32x4{a1[4 * i], a1[4 * i + 1], a1[4 * i + 2], a1[4 * i + 3]};
      *reinterpret_cast<f32x4*>(s_g + tid * kClrLd + 4 * i) = f32x4{gz2[4 * i], gz2[4 * i + 1], gz2[4 * i + 2], gz2[4 * i + 3]};
    }
    *reinterpret_cast<f32x4*>(s_G + tid * 4) = f32x4{G0, G1, G2, 0.f};
    __syncthreads();
    {
      double s = 0.0;
#pragma unroll 8
      for (int q = 0; q < 256; ++q) s += (double)s_a[q * kClrLd + ak] * (double)s_g[q * kClrLd + an];        // a1 (x) gz2
      acc_a += s;
      if (tid < 16) {
        double s2 = 0.0;
#pragma unroll 8
        for (int q = 0; q < 256; ++q) s2 += (double)s_g[q * kClrLd + tid];                                      // sum gz2
        acc_c += s2;
      }
    }
    __syncthreads();                                                     // a1 and gz2 have been read: a2 and gz1 take their place
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      *reinterpret_cast<f32x4*>(s_a + tid * kClrLd + 4 * i) = f32x4{a2[4 * i], a2[4 * i + 1], a2[4 * i + 2], a2[4 * i + 3]};
      *reinterpret_cast<f32x4*>(s_g + tid * kClrLd + 4 * i) = f32x4{gz1[4 * i], gz1[4 * i + 1], gz1[4 * i + 2], gz1[4 * i + 3]};
    }
    __syncthreads();
    if (tid < 67) {
      // one loop for the three kinds of sum: x[q xs] y[q ys], with y the constant 1 (stride 0) for the plain sums
      double s = 0.0;
#pragma unroll 8
      for (int q = 0; q < 256; ++q) s += (double)bx[q * bxs] * (double)by[q * bys];
      acc_b += s;
    }
    __syncthreads();                                                     // the sums are done: the next chunk may overwrite
  }
  double* out = p.part + (size_t)blockIdx.x * kClrSumsLd;
  out[tid] = acc_a;
  if (tid < 67) out[256 + tid] = acc_b;
  if (tid < 16) out[323 + tid] = acc_c;
}

// ---- launch 3: clr_conv1's kernel gradient
struct ClrWgradArgs {
  const float* f;         // [B,H,W,.], channel stride f_cs
  const float* gs;        // [B,H,W]
  const float* gz1;       // [B,H,W,16]
  float* wpart;           // [P][4][160][16]
  int f_cs, H, W, tiles_x, tiles_per_img, T, P;
};

// grid (4 P): workgroup (p, cc)
__global__ __launch_bounds__(256) void clr_wgrad_kernel(const ClrWgradArgs a) {
  constexpr int IN_F = kClrPatch * 16, GZ_F = 256 * 16, GS_F = 344, RED_F = 4 * kClrWRows * 16;
  constexpr int SM_F = IN_F + GZ_F + GS_F > RED_F ? IN_F + GZ_F + GS_F : RED_F;
  __shared__ __attribute__((aligned(16))) float smem[SM_F];
  float* s_in = smem;
  float* s_gz = smem + IN_F;
  float* s_gs = s_gz + GZ_F;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int p = (int)(blockIdx.x >> 2), cc = (int)(blockIdx.x & 3);

  f32x4 acc[10];
#pragma unroll
  for (int t = 0; t < 10; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};

  constexpr int PV = (kClrPatch * 4 + 255) / 256, GV = 4, SV = 2;
  f32x4 pv[PV], gv[GV];
  float sv[SV];
  auto fetch = [&](int t) {
    const int img = t / a.tiles_per_img, tile = t % a.tiles_per_img;
    const int y0 = (tile / a.tiles_x) * kClrTH, x0 = (tile % a.tiles_x) * kClrTW;
    const size_t img_pix = (size_t)img * a.H * a.W;
#pragma unroll
    for (int j = 0; j < PV; ++j) {
      const int i = tid + j * 256;
      const int pix = i >> 2, c4 = i & 3;
      const int iy = y0 - 1 + pix / kClrPW, ix = x0 - 1 + pix % kClrPW;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (i < kClrPatch * 4 && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W)
        v = *reinterpret_cast<const f32x4*>(a.f + (img_pix + (size_t)iy * a.W + ix) * a.f_cs + cc * 16 + c4 * 4);
      pv[j] = v;
    }
#pragma unroll
    for (int j = 0; j < GV; ++j) {
      const int i = tid + j * 256;
      const int pq = i >> 2, c4 = i & 3;
      gv[j] = *reinterpret_cast<const f32x4*>(a.gz1 + (img_pix + (size_t)(y0 + (pq >> 5)) * a.W + x0 + (pq & 31)) * 16 + c4 * 4);
    }
#pragma unroll
    for (int j = 0; j < SV; ++j) {
      const int i = tid + j * 256;
      const int iy = y0 - 1 + i / kClrPW, ix = x0 - 1 + i % kClrPW;
      sv[j] = (i < kClrPatch && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) ? a.gs[img_pix + (size_t)iy * a.W + ix] : 0.f;
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (int j = 0; j < PV; ++j) {
      const int i = tid + j * 256;
      if (i < kClrPatch * 4) reinterpret_cast<f32x4*>(s_in)[i] = pv[j];
    }
#pragma unroll
    for (int j = 0; j < GV; ++j) reinterpret_cast<f32x4*>(s_gz)[tid + j * 256] = gv[j];
#pragma unroll
    for (int j = 0; j < SV; ++j) {
      const int i = tid + j * 256;
      if (i < kClrPatch) s_gs[i] = sv[j];
    }
  };

  const int gs_tap = r < 9 ? (r / 3) * kClrPW + r % 3 : 0;
  fetch(p);
  for (int t = p; t < a.T; t += a.P) {
    if (t != p) __syncthreads();                                          // every wave is done with the previous tile's LDS
    stage();
    __syncthreads();
    if (t + a.P < a.T) fetch(t + a.P);                                    // in flight behind the matrix work below
#pragma unroll 4
    for (int kk = 0; kk < 16; ++kk) {
      const int ty = 2 * wave + (kk >> 3), tx = (kk & 7) * 4 + q;        // the lane's pixel of this k-step
      const float bv = s_gz[(ty * kClrTW + tx) * 16 + r];
      const float* ap = s_in + (ty * kClrPW + tx) * 16 + r;
#pragma unroll
      for (int tap = 0; tap < 9; ++tap)
        acc[tap] = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[((tap / 3) * kClrPW + tap % 3) * 16], bv, acc[tap], 0, 0, 0);
      if (cc == 0) {
        const float gv0 = s_gs[ty * kClrPW + tx + gs_tap];
        acc[9] = __builtin_amdgcn_mfma_f32_16x16x4f32(r < 9 ? gv0 : 0.f, bv, acc[9], 0, 0, 0);
      }
    }
  }
  __syncthreads();                                                        // the staged tile is done with: the waves' accumulators take its place
#pragma unroll
  for (int t = 0; t < 10; ++t)
#pragma unroll
    for (int e = 0; e < 4; ++e) smem[(wave * kClrWRows + t * 16 + 4 * q + e) * 16 + r] = acc[t][e];
  __syncthreads();
  float* wp = a.wpart + (size_t)blockIdx.x * (kClrWRows * 16);
  for (int i = tid; i < kClrWRows * 16; i += 256)
    wp[i] = ((smem[i] + smem[kClrWRows * 16 + i]) + smem[2 * kClrWRows * 16 + i]) + smem[3 * kClrWRows * 16 + i];
}

// ---- launch 4: clr_conv1's data gradient
struct ClrDgradArgs {
  const float* gz1;       // [B,H,W,16]
  const float* w;         // dgrad/w [9][64][16], then dgrad/gs [9][16]
  const float* g_gs;      // [B,H,W], or null
  float* d_f;             // [B,H,W,64]
  float* d_gs;            // [B,H,W]
  int H, W, tiles_x, tiles_per_img, T;
};

constexpr int kClrDgradSmemFloats = 9 * 64 * kClrLd + 9 * 16 + kClrPatch * kClrLd;

__global__ __launch_bounds__(256) void clr_dgrad_kernel(const ClrDgradArgs a) {
  extern __shared__ __attribute__((aligned(16))) float dsm[];
  float* s_w = dsm;                                  // [9][64][20]
  float* s_wgs = dsm + 9 * 64 * kClrLd;              // [9][16]
  float* s_p = s_wgs + 9 * 16;                       // [340][20]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, q = lane >> 4;
  for (int i = tid; i < 9 * 64 * 4; i += 256) *reinterpret_cast<f32x4*>(s_w + (i >> 2) * kClrLd + (i & 3) * 4) = reinterpret_cast<const f32x4*>(a.w)[i];
  if (tid < 9 * 16) s_wgs[tid] = a.w[9 * 64 * 16 + tid];

  constexpr int PV = (kClrPatch * 4 + 255) / 256;
  f32x4 pv[PV];
  auto fetch = [&](int t) {
    const int img = t / a.tiles_per_img, tile = t % a.tiles_per_img;
    const int y0 = (tile / a.tiles_x) * kClrTH, x0 = (tile % a.tiles_x) * kClrTW;
#pragma unroll
    for (int j = 0; j < PV; ++j) {
      const int i = tid + j * 256;
      const int pix = i >> 2, c4 = i & 3;
      const int iy = y0 - 1 + pix / kClrPW, ix = x0 - 1 + pix % kClrPW;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (i < kClrPatch * 4 && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W)
        v = *reinterpret_cast<const f32x4*>(a.gz1 + (((size_t)img * a.H + iy) * a.W + ix) * 16 + c4 * 4);
      pv[j] = v;
    }
  };
  int t = (int)blockIdx.x;
  if (t < a.T) fetch(t);
  for (; t < a.T; t += (int)gridDim.x) {
    __syncthreads();                                                      // the weights are staged / every wave is done with the previous patch
#pragma unroll
    for (int j = 0; j < PV; ++j) {
      const int i = tid + j * 256;
      if (i < kClrPatch * 4) *reinterpret_cast<f32x4*>(s_p + (i >> 2) * kClrLd + (i & 3) * 4) = pv[j];
    }
    __syncthreads();
    const int img = t / a.tiles_per_img, tile = t % a.tiles_per_img;
    const int y0 = (tile / a.tiles_x) * kClrTH, x0 = (tile % a.tiles_x) * kClrTW;
    if (t + (int)gridDim.x < a.T) fetch(t + (int)gridDim.x);             // in flight behind the matrix work below
    f32x4 acc[4][4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
      for (int pt = 0; pt < 4; ++pt) acc[mt][pt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      f32x4 wa[4], xb[4];
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) wa[mt] = *reinterpret_cast<const f32x4*>(s_w + (tap * 64 + 16 * mt + r) * kClrLd + 4 * q);
#pragma unroll
      for (int pt = 0; pt < 4; ++pt)
        xb[pt] = *reinterpret_cast<const f32x4*>(s_p + ((2 * wave + (pt >> 1) + tap / 3) * kClrPW + (pt & 1) * 16 + r + tap % 3) * kClrLd + 4 * q);
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
          for (int pt = 0; pt < 4; ++pt) acc[mt][pt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[mt][j], xb[pt][j], acc[mt][pt], 0, 0, 0);
    }
    const size_t img_pix = (size_t)img * a.H * a.W;
#pragma unroll
    for (int pt = 0; pt < 4; ++pt) {
      const size_t pix = img_pix + (size_t)(y0 + 2 * wave + (pt >> 1)) * a.W + x0 + (pt & 1) * 16 + r;
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) *reinterpret_cast<f32x4*>(a.d_f + pix * 64 + 16 * mt + 4 * q) = acc[mt][pt];
    }
    {
      // d_gs: the thread's own pixel, taps and channels in index order
      const int ty = tid >> 5, tx = tid & 31;
      float s = 0.f;
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
        const float* src = s_p + ((ty + tap / 3) * kClrPW + tx + tap % 3) * kClrLd;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const f32x4 v = *reinterpret_cast<const f32x4*>(src + 4 * i), w = *reinterpret_cast<const f32x4*>(s_wgs + tap * 16 + 4 * i);
#pragma unroll
          for (int e = 0; e < 4; ++e) s = __builtin_fmaf(v[e], w[e], s);
        }
      }
      const size_t pix = img_pix + (size_t)(y0 + ty) * a.W + x0 + tx;
      a.d_gs[pix] = a.g_gs != nullptr ? s + a.g_gs[pix] : s;
    }
  }
}

// ---- launch 5: the partials -> W1, d K1 and S
struct ClrFoldArgs {
  const float* wpart;     // [P][4][160][16]
  const double* ppart;    // [G][344]
  const float* inv1;      // [16]
  double* W1;             // [9][65][16]
  double* S;              // [344]
  float* dk1;             // [9][65][16]
  int P, G;
};
constexpr int kClrFoldK1Blocks = (kClrK1 + 255) / 256;

// grid (37 + 85): the first 37 workgroups a thread per element of K1, the rest a wave per sum
__global__ __launch_bounds__(256) void clr_fold_kernel(const ClrFoldArgs a) {
  const int tid = threadIdx.x;
  if (blockIdx.x < (unsigned)kClrFoldK1Blocks) {
    const int e = (int)blockIdx.x * 256 + tid;
    if (e >= kClrK1) return;
    const int o = e & 15, c = (e >> 4) % 65, tap = e / (65 * 16);
    const size_t per = (size_t)4 * kClrWRows * 16;
    const float* src = a.wpart + (c == 0 ? (size_t)(144 + tap) * 16 : (size_t)((c - 1) >> 4) * (kClrWRows * 16) + (size_t)(tap * 16 + ((c - 1) & 15)) * 16) + o;
    double s = 0.0;
#pragma unroll 8
    for (int p = 0; p < a.P; ++p) s += (double)src[(size_t)p * per];      // in index order
    a.W1[e] = s;
    a.dk1[e] = (float)((double)a.inv1[o] * s);
  } else {
    const int j = ((int)blockIdx.x - kClrFoldK1Blocks) * 4 + (tid >> 6), lane = tid & 63;
    if (j >= kClrSums) return;
    double s = 0.0;
    for (int g = lane; g < a.G; g += 64) s += a.ppart[(size_t)g * kClrSumsLd + j];
    s = wave_sum(s);
    if (lane == 0) a.S[j] = s;
  }
}

// ---- launch 6: the per-channel gradients and the 1x1 kernels'
struct ClrFinishArgs {
  const double* W1;       // [585][16]
  const double* S;        // [344]
  const float* k1;        // [585][16]
  const float* k2;        // [16][16]
  const float* vecs1;     // bias, inv, moving_mean, rstd [4][16]
  const float* vecs2;
  float* grads;
};

// grid (17), one wave each: workgroup o < 16 the channel o of both layers, workgroup 16 the 1x1 kernels and b3
__global__ __launch_bounds__(64) void clr_finish_kernel(const ClrFinishArgs a) {
  const int lane = threadIdx.x, o = (int)blockIdx.x;
  if (o < 16) {
    double kw1 = 0.0;
    for (int m = lane; m < 9 * 65; m += 64) kw1 += (double)a.k1[m * 16 + o] * a.W1[m * 16 + o];
    kw1 = wave_sum(kw1);
    double kw2 = lane < 16 ? (double)a.k2[lane * 16 + o] * a.S[lane * 16 + o] : 0.0;
    kw2 = wave_sum(kw2);
    if (lane < 2) {
      const float* v = lane == 0 ? a.vecs1 : a.vecs2;
      const double KW = lane == 0 ? kw1 : kw2, S = a.S[(lane == 0 ? 307 : 323) + o];
      const int first = lane == 0 ? 1 : 5;
      bn_channel_grads(KW, S, v, 16, o, a.grads[clr_tail_var_offset(first) + o], a.grads[clr_tail_var_offset(first + 1) + o],
                       a.grads[clr_tail_var_offset(first + 2) + o]);
    }
  } else {
    for (int i = lane; i < 256; i += 64) a.grads[clr_tail_var_offset(4) + i] = (float)((double)a.vecs2[16 + (i & 15)] * a.S[i]);
    if (lane < 48) a.grads[clr_tail_var_offset(8) + lane] = (float)a.S[256 + lane];
    if (lane < 3) a.grads[clr_tail_var_offset(9) + lane] = (float)a.S[304 + lane];
  }
}

// The first `stop_after` of the six launches above (kClrTailLaunches: all of them; fewer are for the tests' stage-by-stage comparison).
inline hipError_t launch_clr_tail_grad(const float* blob, const float* gs, const float* f, int f_cs, const float* g_con, const float* g_gs, int B, int H, int W,
                                       float* d_f, float* d_gs, float* grads, bool keep, void* scratch, int stop_after, hipStream_t stream) {
  const ClrTailPlan pl = clr_tail_plan(B, H, W);
  unsigned char* base = static_cast<unsigned char*>(scratch);
  float* a1 = reinterpret_cast<float*>(base + pl.map[0]);
  float* a2 = reinterpret_cast<float*>(base + pl.map[1]);
  float* gz1 = reinterpret_cast<float*>(base + pl.map[2]);
  double* ppart = reinterpret_cast<double*>(base + pl.map[3]);
  float* wpart = reinterpret_cast<float*>(base + pl.map[4]);
  double* W1 = reinterpret_cast<double*>(base + pl.map[5]);
  double* S = reinterpret_cast<double*>(base + pl.map[6]);
  hipError_t e;
  if (stop_after < 1) return hipSuccess;
  {
    ConvN16Args a{};
    a.in = f; a.in_cs = f_cs; a.H = H; a.W = W;
    a.w = blob + kClrOffFwdW; a.bias = blob + kClrOffFwdB; a.out = a1; a.out_cs = 16; a.act = 1;
    a.pad_t = 1; a.pad_l = 1; a.gs = gs; a.w_gs = blob + kClrOffFwdGs;
    if ((e = launch_conv_n16<3, 3, true, false, 2>(a, B, stream)) != hipSuccess) return e;
  }
  if (stop_after < 2) return hipSuccess;
  {
    ClrPixelArgs a;
    a.a1 = a1; a.g_con = g_con; a.tail = blob + kClrOffTail; a.gz1 = gz1; a.a2 = keep ? a2 : nullptr; a.part = ppart;
    a.chunks = (unsigned)(pl.npix / 256);
    hipLaunchKernelGGL(clr_tail_pixel_kernel, dim3(pl.G), dim3(256), 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (stop_after < 3) return hipSuccess;
  {
    ClrWgradArgs a;
    a.f = f; a.gs = gs; a.gz1 = gz1; a.wpart = wpart; a.f_cs = f_cs; a.H = H; a.W = W;
    a.tiles_x = pl.tiles_x; a.tiles_per_img = pl.tiles_per_img; a.T = pl.T; a.P = pl.P;
    hipLaunchKernelGGL(clr_wgrad_kernel, dim3(4 * pl.P), dim3(256), 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (stop_after < 4) return hipSuccess;
  {
    static PerDeviceOnce once;               // the dynamic LDS limit is set once per device
    constexpr int bytes = kClrDgradSmemFloats * (int)sizeof(float);
    if ((e = dynamic_lds_once(clr_dgrad_kernel, bytes, once)) != hipSuccess) return e;
    ClrDgradArgs a;
    a.gz1 = gz1; a.w = blob + kClrOffDgradW; a.g_gs = g_gs; a.d_f = d_f; a.d_gs = d_gs; a.H = H; a.W = W;
    a.tiles_x = pl.tiles_x; a.tiles_per_img = pl.tiles_per_img; a.T = pl.T;
    hipLaunchKernelGGL(clr_dgrad_kernel, dim3(pl.T < kClrDgradCap ? pl.T : kClrDgradCap), dim3(256), bytes, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (stop_after < 5) return hipSuccess;
  {
    ClrFoldArgs a;
    a.wpart = wpart; a.ppart = ppart; a.inv1 = blob + kClrOffVecs1 + 16; a.W1 = W1; a.S = S; a.dk1 = grads + clr_tail_var_offset(0); a.P = pl.P; a.G = pl.G;
    hipLaunchKernelGGL(clr_fold_kernel, dim3(kClrFoldK1Blocks + (kClrSums + 3) / 4), dim3(256), 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (stop_after < 6) return hipSuccess;
  ClrFinishArgs a;
  a.W1 = W1; a.S = S; a.k1 = blob + kClrOffK1; a.k2 = blob + kClrOffK2; a.vecs1 = blob + kClrOffVecs1; a.vecs2 = blob + kClrOffVecs2; a.grads = grads;
  hipLaunchKernelGGL(clr_finish_kernel, dim3(17), dim3(64), 0, stream, a);
  return hipGetLastError();
}

}  // namespace bsr
