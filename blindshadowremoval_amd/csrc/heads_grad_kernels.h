// The generator's backward pass through the grey heads, ON THE DEVICE, training=False (the reference's model.py:246-250): conv2
// ('tconv3', 7x7, 64 -> 1, tanh) gives mask, conv3 ('tconv4', 7x7, 64 -> 1) gives con, gs = gray(inputs) (1 + mask) + con.  Given the
// complete d_gs = d loss / d gs (ColourTail's), the forward's inputs and mask22 and the heads' input y (up3's output) it writes d_y and
// the four variable gradients.  blindshadowremoval_amd/generator_grad.py is the host statement (heads_grad); pack.pack_heads_grad
// writes the blob.
//
// N = B H W pixels (H a multiple of 8, W of 32, so every 8 x 32 tile lies inside one image and N is a multiple of 256).  The two heads
// are one convolution with two output channels: row k = 2 (7 a + b) + j of the 98 holds tap (a, b) of head j (0 mask, 1 con), and
//    A[p, k] = g2[p - (a - 3, b - 3)][j], zero outside p's own image,    g2[p] = (g_m, g_con)[p]
// is never written out: a workgroup keeps its tile's g2 with a 3-pixel halo in LDS (14 x 38 pixels, 4.2 KB) and reads the operand there.
// The border test is on the staged pixel's own (row, column) inside the tile's image, so nothing is read across an image seam.
//
// Five launches on the caller's stream, one after the other: no host synchronisation, no second stream, no floating-point atomic; every
// word a launch reads was written by the caller or by an earlier launch of the same call, and every sum runs in a fixed order, so a
// call repeats its bits.  All matrix work is v_mfma_f32_16x16x4_f32.
//    1  hg_entry_kernel   mask = mask22[.., 0] - mask22[.., 2] (tanh(m) as the forward rounded it), gray = gray3(inputs),
//                         g_con = d_gs, g_m = (d_gs * gray) * (1 - mask * mask) in float32 with fp contraction off -> g2 [N][2], mask [N];
//                         per 256 pixels the float64 sums of g_m and g_con in row order
//    2  hg_dgrad_kernel   d_y = A Kt (M = N, K = 98 -> 100, N = 64): up to 512 workgroups that each walk 8 x 32 tiles, Kt in registers
//                         (25 k-steps x 4 column tiles per lane, loaded once), the operand out of the LDS halo, the next tile's halo
//                         fetched under this tile's matrix work; MFMA column r of tile n is channel 4 r + n, so Kt loads and d_y stores
//                         are 16 bytes per lane and a store instruction writes whole 256-byte pixels
//    3  hg_wgrad_kernel   Wg = A^T y (M = 98 -> 112, N = 64, K = the pixels): slice p takes the tiles p, p + P, ...; each of its four waves
//                         takes two of a tile's eight rows and keeps all 7 x 4 accumulator tiles, y as one 16-byte load per lane and four
//                         pixels; the next tile's y and halo are fetched into registers under this tile's matrix work; the float32
//                         partials go out per wave, straight from the accumulators: part [4 P][112][64]
//    4  hg_fold_kernel    a thread per kernel element: the 4 P partials in index order in float64 -> Wg (float64 [2][49][64]) and the two
//                         kernels rounded once
//    5  hg_finish_kernel  a workgroup per head: the column sums' partials -> S (float64 [2]) and the two biases
#pragma once
#include "clr_tail_grad_kernels.h"
#include "glue_kernels.h"

namespace bsr {

constexpr int kHgLaunches = 5;
constexpr int kHgVars = 4;
constexpr int kHgC = 64, kHgTaps = 49, kHgK = 98, kHgKp = 100, kHgMp = 112;
constexpr int kHgTH = 8, kHgTW = 32, kHgTile = kHgTH * kHgTW;
constexpr int kHgHaloH = kHgTH + 6, kHgHaloW = kHgTW + 6;
constexpr int kHgMaps = 4;
constexpr int kHgKernel = kHgTaps * kHgC;                 // floats of one head's kernel [7][7][64][1]
constexpr int kHgBlobFloats = kHgKp * kHgC;
constexpr int kHgMaxSlices = 256;
constexpr int kHgDgradGroups = 512;       // two resident workgroups a CU: each loads the 25.6 KB image once and walks its tiles

// float offset of variable `index` (conv2: kernel, bias; conv3: kernel, bias) inside grads; 4: the total
__host__ __device__ inline size_t hg_var_offset(int index) {
  const size_t n[kHgVars] = {kHgKernel, 1, kHgKernel, 1};
  size_t o = 0;
  for (int v = 0; v < index && v < kHgVars; ++v) o += n[v];
  return o;
}

inline bool hg_size_ok(int B, int H, int W) { return clr_tail_size_ok(B, H, W); }

// Byte offsets inside the scratch.  map 0: g2 [N][2], 1: mask [N], 2: Wg float64 [2][49][64], 3: S float64 [2].  P slices of whole tiles:
// half as many as there are tiles (a slice's partials, 4 x 28 KB, are written once for at least two tiles), at most kHgMaxSlices.
struct HgPlan {
  int N, tiles, P;
  size_t map[kHgMaps], colpart, part, total;
};
inline HgPlan hg_plan(int B, int H, int W) {
  HgPlan pl;
  BumpBytes bump;
  pl.N = B * H * W;
  pl.tiles = pl.N / kHgTile;
  const int half = (pl.tiles + 1) / 2;
  pl.P = half < kHgMaxSlices ? half : kHgMaxSlices;
  const size_t N = (size_t)pl.N;
  pl.map[0] = bump.take(N * 2 * sizeof(float));
  pl.map[1] = bump.take(N * sizeof(float));
  pl.map[2] = bump.take((size_t)2 * kHgKernel * sizeof(double));
  pl.map[3] = bump.take(2 * sizeof(double));
  pl.colpart = bump.take((size_t)pl.tiles * 2 * sizeof(double));
  pl.part = bump.take((size_t)pl.P * 4 * kHgMp * kHgC * sizeof(float));
  pl.total = bump.o;
  return pl;
}

// ---- launch 1: grid (N / 256)
struct HgEntryArgs {
  const float *inputs, *mask22, *d_gs;
  float *g2, *mask;
  double* colpart;      // [N / 256][2]
};

// the declared float32 order of g_m: four rounded operations, nothing contracted
__device__ __forceinline__ float hg_g_m(float d, float gray, float mask) {
#pragma clang fp contract(off)
  const float dg = d * gray, mm = mask * mask;
  const float om = 1.f - mm;
  return dg * om;
}

__global__ __launch_bounds__(256) void hg_entry_kernel(const HgEntryArgs a) {
  __shared__ float s_v[2 * 256];
  const int tid = threadIdx.x;
  const size_t p = (size_t)blockIdx.x * 256 + tid;
  const float gray = gray3(a.inputs[p * 3], a.inputs[p * 3 + 1], a.inputs[p * 3 + 2]);
  const float mask = a.mask22[p * 3] - a.mask22[p * 3 + 2];
  const float d = a.d_gs[p];
  const float gm = hg_g_m(d, gray, mask);
  *reinterpret_cast<f32x2*>(a.g2 + p * 2) = f32x2{gm, d};
  a.mask[p] = mask;
  s_v[tid] = gm;
  s_v[256 + tid] = d;
  __syncthreads();
  if (tid < 2) {
    double s = 0.0;
    for (int i = 0; i < 256; ++i) s += (double)s_v[tid * 256 + i];
    a.colpart[(size_t)blockIdx.x * 2 + tid] = s;
  }
}

// tile t of the N / 256 (row-major over an image's 8 x 32 tiles, image after image): the pixel index of its image and its corner
struct HgTileAt {
  size_t img0;
  int y0, x0;
};
__device__ __forceinline__ HgTileAt hg_tile_at(int t, int H, int W) {
  const int tx_n = W / kHgTW, ty_n = H / kHgTH;
  return HgTileAt{(size_t)(t / (tx_n * ty_n)) * H * W, ((t / tx_n) % ty_n) * kHgTH, (t % tx_n) * kHgTW};
}

// a tile's g2 with the 3-pixel halo, [14][38][2] floats: a thread fetches three of the 532 pixels into registers ahead of their use
// (zero outside the image: the test is on the pixel's own row and column) and puts them into LDS when the tile's turn comes
__device__ __forceinline__ void hg_fetch_halo(f32x2 (&hv)[3], const float* g2, const HgTileAt at, int H, int W, int tid) {
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int i = tid + j * 256;
    const int y = at.y0 - 3 + i / kHgHaloW, x = at.x0 - 3 + i % kHgHaloW;
    hv[j] = f32x2{0.f, 0.f};
    if (i < kHgHaloH * kHgHaloW && y >= 0 && y < H && x >= 0 && x < W) hv[j] = *reinterpret_cast<const f32x2*>(g2 + (at.img0 + (size_t)y * W + x) * 2);
  }
}
__device__ __forceinline__ void hg_put_halo(float* s_g, const f32x2 (&hv)[3], int tid) {
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int i = tid + j * 256;
    if (i < kHgHaloH * kHgHaloW) *reinterpret_cast<f32x2*>(s_g + i * 2) = hv[j];
  }
}

// where row k = 2 (7 a + b) + j of the operand lies in the halo, relative to the pixel's own slot: the pixel (i, x) of the tile is halo
// slot (i + 3, x + 3) and reads (i + 6 - a, x + 6 - b); k must be below 98
__device__ __forceinline__ int hg_tap_off(int k) {
  const int t = k >> 1, ta = t / 7, tb = t - 7 * ta;
  return ((6 - ta) * kHgHaloW + (6 - tb)) * 2 + (k & 1);
}

// ---- launch 2: grid (min(tiles, kHgDgradGroups)): workgroup g takes the tiles g, g + grid, ...  Wave v takes a tile's rows 2 v, 2 v + 1
// as four groups of 16 pixels.
struct HgDgradArgs {
  const float* g2;      // [N][2]
  const float* kt;      // [100][64], rows 98, 99 zero
  float* d_y;           // [N][64]
  int H, W, tiles;
};

__global__ __launch_bounds__(256) void hg_dgrad_kernel(const HgDgradArgs a) {
  __shared__ __attribute__((aligned(16))) float s_g[kHgHaloH * kHgHaloW * 2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, q = lane >> 4;
  f32x2 hv[3];
  hg_fetch_halo(hv, a.g2, hg_tile_at((int)blockIdx.x, a.H, a.W), a.H, a.W, tid);         // the grid is at most the tiles
  f32x4 kt[kHgKp / 4];
  int off[kHgKp / 4];
#pragma unroll
  for (int s = 0; s < kHgKp / 4; ++s) {
    const int k = 4 * s + q;
    kt[s] = *reinterpret_cast<const f32x4*>(a.kt + (size_t)k * kHgC + 4 * r);
    off[s] = k < kHgK ? hg_tap_off(k) : 0;
  }
  const bool live = q < 2;         // the last k-step's rows 98, 99 are the pad
#pragma unroll 1
  for (int t = (int)blockIdx.x; t < a.tiles; t += (int)gridDim.x) {
    const HgTileAt at = hg_tile_at(t, a.H, a.W);
    __syncthreads();                                                       // every wave is done with the previous tile
    hg_put_halo(s_g, hv, tid);
    __syncthreads();
    if (t + (int)gridDim.x < a.tiles) hg_fetch_halo(hv, a.g2, hg_tile_at(t + (int)gridDim.x, a.H, a.W), a.H, a.W, tid);
#pragma unroll 1
    for (int g = 0; g < 4; ++g) {
      const int i = wave * 2 + (g >> 1), x = (g & 1) * 16;
      const float* ap = s_g + (i * kHgHaloW + x + r) * 2;
      f32x4 acc[4];
#pragma unroll
      for (int n = 0; n < 4; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < kHgKp / 4; ++s) {
        float av = ap[off[s]];
        if (s == kHgKp / 4 - 1) av = live ? av : 0.f;
#pragma unroll
        for (int n = 0; n < 4; ++n) acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, kt[s][n], acc[n], 0, 0, 0);
      }
      const size_t pix0 = at.img0 + (size_t)(at.y0 + i) * a.W + at.x0 + x + 4 * q;
#pragma unroll
      for (int e = 0; e < 4; ++e)
        *reinterpret_cast<f32x4*>(a.d_y + (pix0 + e) * kHgC + 4 * r) = f32x4{acc[0][e], acc[1][e], acc[2][e], acc[3][e]};
    }
  }
}

// ---- launch 3: grid (P).  part[(4 p + wave)][k][c] = sum over the wave's pixels of the slice's tiles of A[pixel][k] y[pixel][c]
struct HgWgradArgs {
  const float* g2;      // [N][2]
  const float* y;       // [N][64 of y_cs]
  float* part;          // [4 P][112][64]
  int y_cs, H, W, tiles, P;
};

// what a thread fetches of a tile ahead of its use: its three halo pixels (zero outside the image) and, per lane, the sixteen 16-byte
// pieces of y its wave multiplies (k-step s: row 2 wave + s / 8, columns 4 (s % 8) + q, channels 4 r ..)
struct HgTileRegs {
  f32x2 hv[3];
  f32x4 yv[16];
};

__device__ __forceinline__ void hg_fetch_tile(HgTileRegs& regs, const HgWgradArgs& a, int t, int tid) {
  const int lane = tid & 63, wave = tid >> 6, r = lane & 15, q = lane >> 4;
  const HgTileAt at = hg_tile_at(t, a.H, a.W);
  hg_fetch_halo(regs.hv, a.g2, at, a.H, a.W, tid);
#pragma unroll
  for (int s = 0; s < 16; ++s) {
    const int i = wave * 2 + (s >> 3), x = (s & 7) * 4 + q;
    regs.yv[s] = *reinterpret_cast<const f32x4*>(a.y + (at.img0 + (size_t)(at.y0 + i) * a.W + at.x0 + x) * a.y_cs + 4 * r);
  }
}

__global__ __launch_bounds__(256) void hg_wgrad_kernel(const HgWgradArgs a) {
  __shared__ __attribute__((aligned(16))) float s_g[kHgHaloH * kHgHaloW * 2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int p = (int)blockIdx.x;
  int off[kHgMp / 16];
#pragma unroll
  for (int mt = 0; mt < kHgMp / 16; ++mt) off[mt] = mt * 16 + r < kHgK ? hg_tap_off(mt * 16 + r) : 0;
  const bool live = 96 + r < kHgK;         // the last row tile holds rows 96, 97 and the pad
  f32x4 acc[kHgMp / 16][4];
#pragma unroll
  for (int mt = 0; mt < kHgMp / 16; ++mt)
#pragma unroll
    for (int n = 0; n < 4; ++n) acc[mt][n] = f32x4{0.f, 0.f, 0.f, 0.f};
  HgTileRegs cur, nxt;
  hg_fetch_tile(cur, a, p, tid);           // P <= tiles: every slice has a first tile
#pragma unroll 1
  for (int t = p; t < a.tiles; t += a.P) {
    __syncthreads();                                                       // every wave is done with the previous tile
    hg_put_halo(s_g, cur.hv, tid);
    __syncthreads();
    const bool more = t + a.P < a.tiles;
    if (more) hg_fetch_tile(nxt, a, t + a.P, tid);                         // in flight under this tile's matrix work
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      const int i = wave * 2 + (s >> 3), x = (s & 7) * 4 + q;
      const float* ap = s_g + (i * kHgHaloW + x) * 2;
#pragma unroll
      for (int mt = 0; mt < kHgMp / 16; ++mt) {
        float av = ap[off[mt]];
        if (mt == kHgMp / 16 - 1) av = live ? av : 0.f;
#pragma unroll
        for (int n = 0; n < 4; ++n) acc[mt][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, cur.yv[s][n], acc[mt][n], 0, 0, 0);
      }
    }
    if (more) cur = nxt;
  }
  float* dst = a.part + (size_t)(p * 4 + wave) * kHgMp * kHgC;
#pragma unroll
  for (int mt = 0; mt < kHgMp / 16; ++mt)
#pragma unroll
    for (int e = 0; e < 4; ++e)
      *reinterpret_cast<f32x4*>(dst + (mt * 16 + 4 * q + e) * kHgC + 4 * r) = f32x4{acc[mt][0][e], acc[mt][1][e], acc[mt][2][e], acc[mt][3][e]};
}

// ---- launch 4: grid (98 x 64 / 256 rounded up)
__global__ __launch_bounds__(256) void hg_fold_kernel(const float* part, int slices, double* Wg, float* grads) {
  const int e = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (e >= kHgK * kHgC) return;
  const float* src = part + e;
  double s = 0.0;
#pragma unroll 16
  for (int i = 0; i < slices; ++i) s += (double)src[(size_t)i * kHgMp * kHgC];
  const int k = e / kHgC, c = e % kHgC, j = k & 1, t = k >> 1;
  Wg[(size_t)j * kHgKernel + t * kHgC + c] = s;
  grads[hg_var_offset(2 * j) + t * kHgC + c] = (float)s;
}

// ---- launch 5: grid (2), sixteen waves each: head j's bias.  A thread takes the chunks tid, tid + 1024, ...; the wave's butterfly, then
// the sixteen wave sums in wave order
__global__ __launch_bounds__(1024) void hg_finish_kernel(const double* colpart, int chunks, double* S, float* grads) {
  __shared__ double s_w[16];
  const int tid = threadIdx.x, j = (int)blockIdx.x;
  double s = 0.0;
#pragma unroll 4
  for (int i = tid; i < chunks; i += 1024) s += colpart[(size_t)i * 2 + j];
  s = wave_sum(s);
  if ((tid & 63) == 0) s_w[tid >> 6] = s;
  __syncthreads();
  if (tid != 0) return;
  s = 0.0;
  for (int w = 0; w < 16; ++w) s += s_w[w];
  S[j] = s;
  grads[hg_var_offset(2 * j + 1)] = (float)s;
}

// The first `stop_after` of the five launches above (kHgLaunches: all of them; fewer are for the tests' stage-by-stage comparison).
// inputs, mask22 dense 3 wide, y [B,H,W,64 of y_cs], d_gs dense 1 wide, d_y dense 64 wide.
inline hipError_t launch_heads_grad(const float* blob, const float* inputs, const float* mask22, const float* y, int y_cs, const float* d_gs, int B,
                                    int H, int W, float* d_y, float* grads, void* scratch, int stop_after, hipStream_t stream) {
  const HgPlan pl = hg_plan(B, H, W);
  unsigned char* base = static_cast<unsigned char*>(scratch);
  float *g2 = reinterpret_cast<float*>(base + pl.map[0]), *mask = reinterpret_cast<float*>(base + pl.map[1]);
  float* part = reinterpret_cast<float*>(base + pl.part);
  double *Wg = reinterpret_cast<double*>(base + pl.map[2]), *S = reinterpret_cast<double*>(base + pl.map[3]);
  double* colpart = reinterpret_cast<double*>(base + pl.colpart);
  hipError_t e;
  int done = 0;
  if (stop_after <= done++) return hipSuccess;
  {
    HgEntryArgs a{inputs, mask22, d_gs, g2, mask, colpart};
    hipLaunchKernelGGL(hg_entry_kernel, dim3(pl.tiles), dim3(256), 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (stop_after <= done++) return hipSuccess;
  {
    HgDgradArgs a{g2, blob, d_y, H, W, pl.tiles};
    hipLaunchKernelGGL(hg_dgrad_kernel, dim3(pl.tiles < kHgDgradGroups ? pl.tiles : kHgDgradGroups), dim3(256), 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (stop_after <= done++) return hipSuccess;
  {
    HgWgradArgs a{g2, y, part, y_cs, H, W, pl.tiles, pl.P};
    hipLaunchKernelGGL(hg_wgrad_kernel, dim3(pl.P), dim3(256), 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (stop_after <= done++) return hipSuccess;
  hipLaunchKernelGGL(hg_fold_kernel, dim3((kHgK * kHgC + 255) / 256), dim3(256), 0, stream, part, pl.P * 4, Wg, grads);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if (stop_after <= done++) return hipSuccess;
  hipLaunchKernelGGL(hg_finish_kernel, dim3(2), dim3(1024), 0, stream, colpart, pl.tiles, S, grads);
  return hipGetLastError();
}

}  // namespace bsr
