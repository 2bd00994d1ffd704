// ConvT(3x3, stride 2, TF SAME) Cin -> 64 (+ folded BN + LeakyReLU) in a Winograd-style minimal form on the fp32 matrix cores:
// up2, up3 and clr_up3 of the fp32 GSC forward.
//
// Per axis the layer is (igemm_conv.h: tap a feeds phase (a == 1) from input pixel i - (a == 2); x(-1) = 0)
//   out(2i) = w0 x(i) + w2 x(i-1),   out(2i+1) = w1 x(i).
// For the patch i = 2p with [xm, x0, x1] = [x(i-1), x(i), x(i+1)] the four outputs out(2i) .. out(2i+3) are
//   t = [x0, x1, xm - x0, x0, x0 - x1],  u = [w1, w1, w2, w0 + w2, w0],  m = t . u  (5 products instead of 6),
//   out = [m2 + m3, m0, m3 - m4, m1].
// In 2D a 2x2 input patch gives a 4x4 output patch from 25 products per (cin, cout) instead of 36, and the sum over cin at each of the
// 25 positions (r, s) is a GEMM [patches x Cin] x [Cin x 64] on v_mfma_f32_32x32x2_f32: 1.44x fewer matrix instructions than the
// implicit GEMM of igemm_conv.h.  t has only 4 distinct values per axis, so the transformed input V has 16 images, not 25.
//  * U = G g G^T is computed once per handle in fp64 and rounded once (bsr_create, from the blob's direct image: bsr_api.hip
//    wino_convt_filter_transform; pack.py: pack_wino_convt states the same), stored in the order the B fragments are read:
//    [16-channel chunk][position 5 r + s][cout half][K group g][lane 32 h + n][4 j] = channel 16 chunk + 8 g + 4 h + j, cout 32 half + n.
//  * A workgroup of eight waves owns a tile of 2 x 16 patches (4 x 32 input pixels, 8 x 64 output pixels) = ONE 32-row M block, and
//    all 64 output channels.  The 50 (position, cout half) accumulator tiles are split over the waves BY POSITION so that the output
//    transform stays inside a wave:
//      role 0: (r, s) in {2,3,4} x {2,3,4} without (4,4)  (8 tiles) -> output rows 0, 2 x columns 0, 2 of the 4x4 patch
//      role 1: (r, s) in {2,3,4} x {0,1} and (4,4)        (7 tiles) -> output rows 0, 2 x columns 1, 3; hands (4,4) to role 0 through LDS
//              (written before the tile's last barrier, read behind it; two buffers by tile parity)
//      role 2: r = 0, all s                               (5 tiles) -> output row 1
//      role 3: r = 1, all s                               (5 tiles) -> output row 3
//    Waves 0-3 are roles 0, 0, 1, 1 (cout half = wave & 1), waves 4-7 roles 2, 2, 3, 3: a heavy and a light owner share each SIMD
//    (13 / 13 / 12 / 12 tiles), at most 128 accumulator registers per wave, two waves per SIMD.
//  * A (position, half) tile belongs to ONE wave, so the weights never need to be shared: a wave loads its B fragments straight from
//    the stream (one coalesced 1-KB load per K group, L2 hits) into a small register ring a few tiles ahead.  No LDS ring for U.
//  * The input transform V = B^T d B is done once per workgroup and 16-channel chunk: a thread owns (patch, channel), loads its 3x3
//    pixels (out-of-image pixels through the raw-buffer out-of-range-returns-zero rule), and writes 16 values to LDS
//    ([image][patch][16 + 4 pad]).  V is a ring of three 40-KB images: chunk c + 2 is written late in chunk c and published by the
//    barrier that ends it, so the first fragments of chunk c + 1 are read BEFORE that barrier.  One barrier per chunk.
//  * Persistent: one workgroup per compute unit walks the tiles t, t + grid, ...  The staging side runs two chunks ahead of the matrix
//    side THROUGH tile boundaries (the chunk after a tile's last one is the next tile's first), so only a workgroup's first tile pays
//    the input latency, and a tile's epilogue is followed at once by the next tile's matrix work.  Measured (profiles/HISTORY.md,
//    round 11): up3 at B = 32 539 us with one tile per workgroup, 500 us this way (direct kernel: 583 us).
//  * Per output element the operations and their order are the same at every batch, tile position, grid and image size.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mfma_common.h"

namespace bsr {

struct WinoTArgs {
  const float* in;      // NHWC, Cin = 16 nchunk channels at stride in_cs
  float* out;           // NHWC at twice the input size, 64 channels at stride out_cs
  const float* w;       // [nchunk][25][2][2][64][4]: see above
  const float* bias;    // [64]
  int H, W;             // INPUT feature map (both even)
  int in_cs, out_cs, nchunk;
  int tiles_x, tiles_y, ntiles;
  int act;              // 1: LeakyReLU(0.3)
};

struct WinoTCfg {
  static constexpr int NT = 512;
  static constexpr int CC = 16, LDP = CC + 4;
  static constexpr int N = 64;
  static constexpr int V_POS = 32 * LDP;            // floats of one image's [32 patches][LDP]
  static constexpr int V_FLOATS = 16 * V_POS;
  static constexpr int X_FLOATS = 2 * 16 * 64;      // the hand-over of position (4,4): [half][register][lane], one per tile parity
  static constexpr int SMEM_BYTES = (3 * V_FLOATS + 2 * X_FLOATS) * 4;
  static constexpr unsigned kUnitBytes = 2 * 64 * 16;                 // one (chunk, position, half): two K groups of 64 lanes x 16 bytes
  static constexpr unsigned kChunkBytes = 25 * 2 * kUnitBytes;
  static_assert(SMEM_BYTES <= 160 * 1024 && X_FLOATS * 4 <= SMEM_BYTES, "LDS budget");
};

// The positions a role owns, and how far ahead it keeps B fragments (PF tiles; NU % PF == 0 so that a tile's ring slot is fixed).
template <int ROLE>
struct WinoTRole;
template <>
struct WinoTRole<0> {
  static constexpr int NU = 8, PF = 4;
  static constexpr int pos(int u) { return 5 * (2 + u / 3) + 2 + u % 3; }
};
template <>
struct WinoTRole<1> {
  static constexpr int NU = 7, PF = 7;
  static constexpr int pos(int u) { return u == 6 ? 24 : 5 * (2 + u / 2) + u % 2; }
};
template <>
struct WinoTRole<2> {
  static constexpr int NU = 5, PF = 5;
  static constexpr int pos(int u) { return u; }
};
template <>
struct WinoTRole<3> {
  static constexpr int NU = 5, PF = 5;
  static constexpr int pos(int u) { return 5 + u; }
};
// position (r, s) reads image 4 d(r) + d(s): t = [x0, x1, xm - x0, x0, x0 - x1] has the distinct values d = 0, 1, 2, 0, 3
constexpr int wino_convt_image(int pos) {
  constexpr int d[5] = {0, 1, 2, 0, 3};
  return 4 * d[pos / 5] + d[pos % 5];
}

template <int ROLE>
__device__ __forceinline__ void wino_convt_body(const WinoTArgs& p, float* smem, const int half) {
  using C = WinoTCfg;
  using R = WinoTRole<ROLE>;
  constexpr int NU = R::NU, PF = R::PF, LDP = C::LDP;
  static_assert(NU % PF == 0, "a tile's ring slot must not move");
  typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int h = lane >> 5, r = lane & 31;
  const int nchunk = p.nchunk, ntiles = p.ntiles;
  const int tile_step = (int)gridDim.x;

  // ---- the staging side: a cursor (tile, chunk) runs two chunks ahead of the matrix side through this workgroup's tiles, tile after
  // tile, so a tile's first chunks are staged during the previous tile's last ones.  Per tile: the 3x3 input pixels of this thread's
  // (patch, channel) item as byte offsets from the image start (kLaneOff = zero padding, and everything past the last tile) ----
  unsigned in_goff[9];
  const int patch = tid >> 4, cn = tid & 15;
  const int v_loff = patch * LDP + cn;
  int f_tile = (int)blockIdx.x, f_ch = 0;
  __amdgpu_buffer_rsrc_t in_rsrc = make_rsrc(p.in);
  auto stage_tile = [&](int tile) {
    const bool live = tile < ntiles;
    const int t = live ? tile : 0;
    const int tile_x = t % p.tiles_x, tile_y = (t / p.tiles_x) % p.tiles_y, img = t / (p.tiles_x * p.tiles_y);
    in_rsrc = make_rsrc(p.in + (size_t)img * p.H * p.W * p.in_cs);
    const int iy0 = 2 * (2 * tile_y + (patch >> 4)), ix0 = 2 * (16 * tile_x + (patch & 15));
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b) {
        const int iy = iy0 - 1 + a, ix = ix0 - 1 + b;
        const bool ok = live && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W;
        in_goff[3 * a + b] = ok ? (unsigned)(((iy * p.W + ix) * p.in_cs + cn) * 4) : kLaneOff;
      }
  };
  // loads the cursor's chunk and moves the cursor on
  auto fetch_in = [&](float (&d)[9]) {
    const unsigned soff = (unsigned)(f_ch * C::CC * 4);
#pragma unroll
    for (int i = 0; i < 9; ++i) d[i] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(in_rsrc, in_goff[i], soff, 0));
    if (++f_ch == nchunk) {
      f_ch = 0;
      f_tile += tile_step;
      stage_tile(f_tile);
    }
  };
  // V = B^T d B: rows first (d[3 a + b], a / b = 0, 1, 2 for the pixel before, at and after the patch origin), then columns; image 4 k + l
  auto transform_store = [&](const float (&d)[9], int v_off) {
    float c[4][3];
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      c[0][b] = d[3 + b];
      c[1][b] = d[6 + b];
      c[2][b] = d[b] - d[3 + b];
      c[3][b] = d[3 + b] - d[6 + b];
    }
    float* dst = smem + v_off + v_loff;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      dst[(4 * k + 0) * C::V_POS] = c[k][1];
      dst[(4 * k + 1) * C::V_POS] = c[k][2];
      dst[(4 * k + 2) * C::V_POS] = c[k][0] - c[k][1];
      dst[(4 * k + 3) * C::V_POS] = c[k][1] - c[k][2];
    }
  };
  const __amdgpu_buffer_rsrc_t w_rsrc = make_rsrc(p.w);
  const unsigned w_voff = (unsigned)(lane * 16);
  const unsigned w_half = (unsigned)half * C::kUnitBytes;
  f32x4 bfr[PF][2];
  auto fetch_b = [&](int chunk, int u, int slot) {
    const unsigned soff = (unsigned)chunk * C::kChunkBytes + (unsigned)(R::pos(u) * 2) * C::kUnitBytes + w_half;
#pragma unroll
    for (int g = 0; g < 2; ++g)
      bfr[slot][g] = __builtin_bit_cast(f32x4, (u32x4_t)__builtin_amdgcn_raw_buffer_load_b128(w_rsrc, w_voff, soff + (unsigned)g * 1024u, 0));
  };

  // ---- prologue, once per workgroup: the first two chunks of the input to LDS, the first PF tiles' weights in flight ----
  float d[9];
  stage_tile(f_tile);
  {
    float d1[9];
    fetch_in(d);
    fetch_in(d1);
#pragma unroll
    for (int u = 0; u < PF; ++u) fetch_b(0, u, u);
    transform_store(d, 0);
    transform_store(d1, C::V_FLOATS);
  }
  int v_cur = 0, v_n1 = C::V_FLOATS, v_n2 = 2 * C::V_FLOATS;
  __syncthreads();

  f32x16 acc[NU];
#pragma unroll
  for (int u = 0; u < NU; ++u)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[u][i] = 0.f;

  const int a_base = r * LDP + 4 * h;
  f32x4 af[2][2];
  auto read_frags = [&](int slot, int v_off, int u) {
    const float* src = smem + v_off + wino_convt_image(R::pos(u)) * C::V_POS + a_base;
    af[slot][0] = *reinterpret_cast<const f32x4*>(src);
    af[slot][1] = *reinterpret_cast<const f32x4*>(src + 8);
  };
  read_frags(0, v_cur, 0);

  const float alpha = p.act ? kLeakyAlpha : 1.f;
  const float bias_n = p.bias[half * 32 + r];
  const int Wo = 2 * p.W;
  const unsigned cs4 = (unsigned)p.out_cs * 4u;
  const unsigned lane_out = (unsigned)(16 * h) * cs4 + (unsigned)r * 4u;      // patch column 4h = pixel column 16h
  float* x_base = smem + 3 * C::V_FLOATS + half * (16 * 64) + lane;           // the hand-over of position (4,4): [tile parity][half][register][lane]
  int x_par = 0;

#pragma unroll 1
  for (int tile = (int)blockIdx.x; tile < ntiles; tile += tile_step) {
#pragma unroll 1
    for (int ch = 0; ch < nchunk; ++ch) {
      // The chunk after this tile's last one is the next tile's first: same weights (chunk 0 again), its V already in the ring.  Past
      // the workgroup's last tile the input loads fall outside their buffer and the staged images are never read.
      const int ch1 = ch + 1 < nchunk ? ch + 1 : 0;
      fetch_in(d);
#pragma unroll
      for (int u = 0; u < NU; ++u) {
        const int cur = u & 1, nxt = cur ^ 1;
        if (u + 1 < NU) read_frags(nxt, v_cur, u + 1);
        else read_frags(nxt, v_n1, 0);                    // the next chunk's image was published one barrier ago
        if (u == NU - 1) transform_store(d, v_n2);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            acc[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[cur][g][j], bfr[u % PF][g][j], acc[u], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        // the ring slot is free: it takes the tile PF further on (of the next chunk past this one's end)
        if (u + PF < NU) fetch_b(ch, u + PF, u % PF);
        else fetch_b(ch1, u + PF - NU, u % PF);
      }
      if constexpr (ROLE == 1) {
        // position (4,4) goes to role 0 behind the tile's last barrier
        if (ch == nchunk - 1) {
#pragma unroll
          for (int v = 0; v < 16; ++v) x_base[x_par * C::X_FLOATS + v * 64] = acc[6][v];
        }
      }
      __syncthreads();
      { const int tv = v_cur; v_cur = v_n1; v_n1 = v_n2; v_n2 = tv; }
      if (NU & 1) { af[0][0] = af[1][0]; af[0][1] = af[1][1]; }      // odd tile count: restore fragment parity 0
    }

    // ---- the tile's epilogue: output transform in registers, bias, LeakyReLU, NHWC stores; then the accumulators start again ----
    // Register v of a tile is patch 8 (v / 4) + 4 h + (v % 4) of the tile (patch = 16 py + px), channel r of the wave's 32.
    float x44[16];
    if constexpr (ROLE == 0) {
#pragma unroll
      for (int v = 0; v < 16; ++v) x44[v] = x_base[x_par * C::X_FLOATS + v * 64];
    }
    x_par ^= 1;      // the next tile's hand-over may be written before a slow reader is done with this one

    const int tile_x = tile % p.tiles_x, tile_y = (tile / p.tiles_x) % p.tiles_y, img = tile / (p.tiles_x * p.tiles_y);
    const int py0 = tile_y * 2, px0 = tile_x * 16;      // the tile's first patch row / column
    const __amdgpu_buffer_rsrc_t orsrc =
        make_rsrc(p.out + (((size_t)img * 2 * p.H + 4 * py0) * Wo + 4 * px0) * p.out_cs + half * 32);
    const int npy = p.H / 2 - py0, npx = p.W / 2 - px0 - 4 * h;                // patches of the image from this tile's / lane's first one on
    // an empty statement, only to have the 64 scalar store offsets computed here, per tile, instead of kept (and spilled) across the loop
    unsigned row4 = (unsigned)Wo * cs4, pix4 = cs4;
    asm volatile("" : "+s"(row4), "+s"(pix4));
    auto store = [&](int v, int a, int b, float y) {
      const int ppy = v >> 3, ppx = 8 * ((v >> 2) & 1) + (v & 3);
      const unsigned voff = (ppy < npy && ppx < npx) ? lane_out : kLaneOff;
      const unsigned soff = (unsigned)(4 * ppy + a) * row4 + (unsigned)(4 * ppx + b) * pix4;
      const float x = y + bias_n;
      __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(__builtin_amdgcn_fmed3f(x, x * alpha, 3.4028234664e38f)), orsrc, voff, soff, 0);
    };
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      if constexpr (ROLE == 0) {
        // tiles: 0 (2,2) 1 (2,3) 2 (2,4) 3 (3,2) 4 (3,3) 5 (3,4) 6 (4,2) 7 (4,3), x44 = (4,4)
        const float p02 = acc[0][v] + acc[3][v], p03 = acc[1][v] + acc[4][v], p04 = acc[2][v] + acc[5][v];
        const float p22 = acc[3][v] - acc[6][v], p23 = acc[4][v] - acc[7][v], p24 = acc[5][v] - x44[v];
        store(v, 0, 0, p02 + p03);
        store(v, 0, 2, p03 - p04);
        store(v, 2, 0, p22 + p23);
        store(v, 2, 2, p23 - p24);
      } else if constexpr (ROLE == 1) {
        // tiles: 0 (2,0) 1 (2,1) 2 (3,0) 3 (3,1) 4 (4,0) 5 (4,1)
        store(v, 0, 1, acc[0][v] + acc[2][v]);
        store(v, 0, 3, acc[1][v] + acc[3][v]);
        store(v, 2, 1, acc[2][v] - acc[4][v]);
        store(v, 2, 3, acc[3][v] - acc[5][v]);
      } else {
        // tiles: s = 0 .. 4 of r = 0 (output row 1) or r = 1 (output row 3)
        constexpr int a = ROLE == 2 ? 1 : 3;
        store(v, a, 0, acc[2][v] + acc[3][v]);
        store(v, a, 1, acc[0][v]);
        store(v, a, 2, acc[3][v] - acc[4][v]);
        store(v, a, 3, acc[1][v]);
      }
    }
    (void)x44;
#pragma unroll
    for (int u = 0; u < NU; ++u)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[u][i] = 0.f;
  }
}

__global__ __launch_bounds__(512, 2) void wino_convt_kernel(WinoTArgs p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int half = wave & 1;
  const int role = (wave >> 1) & 3;                 // waves 0-3: roles 0, 0, 1, 1; waves 4-7: roles 2, 2, 3, 3
  // Each role is its own instruction stream; all of them pass the same number of barriers (one before the first tile, one per chunk).
  if (role == 0) wino_convt_body<0>(p, smem, half);
  else if (role == 1) wino_convt_body<1>(p, smem, half);
  else if (role == 2) wino_convt_body<2>(p, smem, half);
  else wino_convt_body<3>(p, smem, half);
}

// nullptr when the launcher takes the layer; else why not (the caller reports it BEFORE any launch)
inline const char* wino_convt_refusal(int batch, int H, int W, int cin, int cout, int in_cs, int out_cs) {
  if (batch <= 0 || H <= 0 || W <= 0) return "empty tensor";
  if (H % 2 != 0 || W % 2 != 0) return "H and W must be even";
  if (cin <= 0 || cin % WinoTCfg::CC != 0) return "Cin must be a positive multiple of 16";
  if (cout != WinoTCfg::N) return "Cout must be 64";
  if (in_cs < cin || out_cs < cout) return "channel stride below the channel count";
  if ((long long)H * W * in_cs * 4 >= (1LL << 31) || (long long)4 * H * W * out_cs * 4 >= (1LL << 31)) return "image too large for 32-bit offsets";
  return nullptr;
}

// The caller has checked wino_convt_refusal().
inline hipError_t launch_wino_convt(WinoTArgs a, int batch, hipStream_t stream) {
  using C = WinoTCfg;
  static PerDeviceOnce once;
  const int dev = PerDeviceOnce::current();
  if (dev < 0 || !once.done[dev]) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(wino_convt_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, C::SMEM_BYTES);
    if (e != hipSuccess) return e;
    if (dev >= 0) once.done[dev] = true;
  }
  a.tiles_x = (a.W / 2 + 15) / 16;
  a.tiles_y = (a.H / 2 + 1) / 2;
  a.ntiles = a.tiles_x * a.tiles_y * batch;
  // one resident workgroup per compute unit walks its tiles t, t + grid, ...: the same tile code whatever the grid, so the bits do not depend on it
  const int grid = a.ntiles < device_cu_count() ? a.ntiles : device_cu_count();
  hipLaunchKernelGGL(wino_convt_kernel, dim3(grid), dim3(C::NT), C::SMEM_BYTES, stream, a);
  return hipGetLastError();
}

}  // namespace bsr
