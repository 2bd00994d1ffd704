// res*.conv2 (3x3, 128 -> 128, stride 1, TF SAME, + folded BN + LeakyReLU) in Winograd F(2x2, 3x3) form on the fp32 matrix cores.
//
// A 2x2 output patch costs 16 multiplies per (cin, cout) instead of 36:  Y = A^T [ sum_cin (G g G^T) . (B^T d B) ] A  with the 4x4 input
// tile d of the patch (Lavin & Gray 2016).  The sum over cin at each of the 16 transform positions is a GEMM
//   [patches x 128 cin] x [128 cin x 128 cout],
// so the layer is 16 independent GEMMs on v_mfma_f32_32x32x2_f32: 2.25x fewer matrix instructions than the implicit GEMM of
// igemm_conv.h, which is bound by their issue rate.
//  * U = G g G^T is computed once per handle in fp64 and rounded once (bsr_create, from the blob's direct image: bsr_api.hip
//    wino_filter_transform; pack.py: pack_wino states the same), [K chunk][position][cout][16 channels].
//  * A workgroup owns one 4x32-pixel output tile = 2x16 patches = ONE 32-row M block, and 32 * NW output channels; each of its NW waves
//    owns 32 output channels at all 16 positions: 16 accumulator tiles = 256 registers, one wave per SIMD.  The output transform then
//    stays in registers: the 16 values of one (patch, cout) are the same register of the 16 tiles of one lane.
//  * The input transform V = B^T d B is done ONCE per workgroup and 16-channel chunk: a thread owns (patch, channel pair), loads its 4x4
//    pixels straight from global memory (out-of-image pixels through the raw-buffer out-of-range-returns-zero rule: TF SAME padding
//    without selects), and writes the 16 positions to LDS ([position][patch][16 + 4 pad]); the chunk after the current one is loaded
//    at its first step and transformed a few instructions per matrix group late in the chunk (double-buffered V).
//  * U flows through a 3-slot LDS ring in steps of two positions; the loads of step t+3 are issued in step t and written to LDS
//    during step t+1, one 16-byte store per matrix group; one barrier per step.
//  * NW = 4 (all 128 channels per workgroup) when the tiles fill the device, NW = 2 (two workgroups per tile) below that.  Per output
//    element the operations and their order are the same in both and at every tile position, so an image gets the same bits in any batch.
//  * Since round 10 the full grids run wino_conv2_pairs_kernel below (eight waves, two per SIMD, the same bits); NW = 4 stays as the
//    form it is measured and tested against.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mfma_common.h"

namespace bsr {

struct WinoArgs {
  const float* in;      // NHWC, 128 channels at stride in_cs
  float* out;           // NHWC, 128 channels at stride out_cs
  const float* w;       // [8][16][128][16]: K chunk, transform position 4 xi + nu, cout, channel
  const float* bias;    // [128]
  int H, W;             // feature map (input = output size)
  int in_cs, out_cs;
  int tiles_x, tiles_y;
  int act;              // 1: LeakyReLU(0.3)
};

template <int NW>
struct WinoCfg {
  static constexpr int NT = NW * 64;
  static constexpr int CC = 16;                   // channels per K chunk
  static constexpr int LDP = CC + 4;              // LDS row pitch (floats): conflict-free ds_read_b128 over 16 rows
  static constexpr int K = 128, N = 128, NCHUNK = K / CC;
  static constexpr int SPC = 8;                   // steps per chunk: two transform positions each
  static constexpr int NSTEPS = NCHUNK * SPC;
  static constexpr int BN = NW * 32;              // output channels per workgroup
  static constexpr int V_POS = 32 * LDP;          // floats of one position's [32 patches][LDP] image
  static constexpr int V_FLOATS = 16 * V_POS;
  static constexpr int U_POS = BN * LDP;
  static constexpr int U_FLOATS = 2 * U_POS;
  static constexpr int SMEM_BYTES = (2 * V_FLOATS + 3 * U_FLOATS) * 4;
  static constexpr int IT = 256 / NT;             // (patch, channel pair) items per thread: 32 x 8 per chunk
  static_assert(NW == 4 || NW == 2, "4 waves (128 channels) or 2 waves (64 channels) per workgroup");
  static_assert(SMEM_BYTES <= 160 * 1024, "LDS budget");
};

template <int NW>
__global__ __launch_bounds__(NW * 64, 1) void wino_conv2_kernel(WinoArgs p) {
  using C = WinoCfg<NW>;
  constexpr int NT = C::NT, LDP = C::LDP, IT = C::IT, SPC = C::SPC, NSTEPS = C::NSTEPS;
  typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
  typedef unsigned u32x2_t __attribute__((ext_vector_type(2)));
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* s_v = smem;
  float* s_u = smem + 2 * C::V_FLOATS;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = lane >> 5, r = lane & 31;

  int bid = blockIdx.x;
  const int tile_x = bid % p.tiles_x;
  bid /= p.tiles_x;
  const int tile_y = bid % p.tiles_y;
  const int img = bid / p.tiles_y;
  const int n0 = blockIdx.y * C::BN;
  const int y0 = tile_y * 4, x0 = tile_x * 32;
  const float* in_img = p.in + (size_t)img * p.H * p.W * p.in_cs;
  const __amdgpu_buffer_rsrc_t in_rsrc = make_rsrc(in_img);

  // ---- per-thread constants: the 4x4 input pixels of this thread's items (byte offsets from the image start, kLaneOff = zero padding),
  // its LDS destination, its share of a weight step ----
  unsigned in_goff[IT][16];
  int v_loff[IT];
#pragma unroll
  for (int it = 0; it < IT; ++it) {
    const int item = tid + it * NT;
    const int patch = item >> 3, cp = item & 7;
    const int py = patch >> 4, px = patch & 15;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int iy = y0 + 2 * py - 1 + a, ix = x0 + 2 * px - 1 + b;
        const bool ok = iy >= 0 && iy < p.H && ix >= 0 && ix < p.W;
        in_goff[it][4 * a + b] = ok ? (unsigned)(((iy * p.W + ix) * p.in_cs + 2 * cp) * 4) : kLaneOff;
      }
    v_loff[it] = patch * LDP + 2 * cp;
  }
  // a position's [BN cout][16] block is contiguous in the weight stream: element e (16 bytes) of it is cout e / 4, channels 4 (e % 4) ..
  unsigned w_goff[2];
  int w_loff[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int e = tid + j * NT;
    w_goff[j] = (unsigned)(e * 16);
    w_loff[j] = (e >> 2) * LDP + (e & 3) * 4;
  }
  const __amdgpu_buffer_rsrc_t w_rsrc = make_rsrc(p.w + (size_t)n0 * C::CC);
  constexpr unsigned kPosBytes = (unsigned)(C::N * C::CC * 4);       // one (chunk, position) block of all 128 couts
  const float bias_n = p.bias[n0 + wave * 32 + r];

  auto fetch_in = [&](int chunk, f32x2 (&d)[IT][16]) {
    const unsigned soff = (unsigned)(chunk * C::CC * 4);
#pragma unroll
    for (int it = 0; it < IT; ++it)
#pragma unroll
      for (int i = 0; i < 16; ++i)
        d[it][i] = __builtin_bit_cast(f32x2, (u32x2_t)__builtin_amdgcn_raw_buffer_load_b64(in_rsrc, in_goff[it][i], soff, 0));
  };
  // B^T d: column b of the row combinations (w[a][b], a = 0..3), in place
  auto in_rows = [&](f32x2 (&d)[IT][16], int b) {
#pragma unroll
    for (int it = 0; it < IT; ++it) {
      const f32x2 d0 = d[it][b], d1 = d[it][4 + b], d2 = d[it][8 + b], d3 = d[it][12 + b];
      d[it][b] = d0 - d2;
      d[it][4 + b] = d1 + d2;
      d[it][8 + b] = d2 - d1;
      d[it][12 + b] = d1 - d3;
    }
  };
  // (B^T d) B: row a of V -> positions 4a .. 4a + 3 of the LDS image
  auto in_cols_store = [&](int v_off, const f32x2 (&d)[IT][16], int a) {
#pragma unroll
    for (int it = 0; it < IT; ++it) {
      const f32x2 w0 = d[it][4 * a], w1 = d[it][4 * a + 1], w2 = d[it][4 * a + 2], w3 = d[it][4 * a + 3];
      float* dst = s_v + v_off + v_loff[it] + 4 * a * C::V_POS;
      *reinterpret_cast<f32x2*>(dst) = w0 - w2;
      *reinterpret_cast<f32x2*>(dst + C::V_POS) = w1 + w2;
      *reinterpret_cast<f32x2*>(dst + 2 * C::V_POS) = w2 - w1;
      *reinterpret_cast<f32x2*>(dst + 3 * C::V_POS) = w1 - w3;
    }
  };
  // step t = positions 2 (t % 8), + 1 of chunk t / 8 = blocks 2t, 2t + 1 of the stream
  auto fetch_w = [&](int t, f32x4 (&regs)[4]) {
#pragma unroll
    for (int pl = 0; pl < 2; ++pl)
#pragma unroll
      for (int j = 0; j < 2; ++j)
        regs[2 * pl + j] = __builtin_bit_cast(f32x4, (u32x4_t)__builtin_amdgcn_raw_buffer_load_b128(w_rsrc, w_goff[j], (unsigned)(2 * t + pl) * kPosBytes, 0));
  };
  auto store_w1 = [&](int u_off, const f32x4 (&regs)[4], int i) {
    *reinterpret_cast<f32x4*>(s_u + u_off + (i >> 1) * C::U_POS + w_loff[i & 1]) = regs[i];
  };

  // ---- prologue: chunk 0 of the input, weight steps 0 and 1 to LDS, step 2 in flight ----
  f32x2 d[IT][16];
  f32x4 w_regs[2][4];
  int u_cur = 0, u_n1 = C::U_FLOATS, u_n2 = 2 * C::U_FLOATS;
  int v_cur = 0, v_nxt = C::V_FLOATS;
  fetch_in(0, d);
  fetch_w(0, w_regs[0]);
  fetch_w(1, w_regs[1]);
#pragma unroll
  for (int b = 0; b < 4; ++b) in_rows(d, b);
#pragma unroll
  for (int a = 0; a < 4; ++a) in_cols_store(0, d, a);
#pragma unroll
  for (int i = 0; i < 4; ++i) store_w1(u_cur, w_regs[0], i);
#pragma unroll
  for (int i = 0; i < 4; ++i) store_w1(u_n1, w_regs[1], i);
  fetch_w(2, w_regs[1]);                                    // as if issued in "step -1": written to LDS during step 0
  __syncthreads();

  f32x16 acc[16];
#pragma unroll
  for (int q = 0; q < 16; ++q)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[q][i] = 0.f;
  // the bias is a constant over the patch: in the transform domain that is position (1, 1) alone (A^T e11 A = all ones)
  acc[5] = bias_tile(h, bias_n);

  const int a_base = r * LDP + 4 * h;
  const int b_base = (wave * 32 + r) * LDP + 4 * h;
  f32x4 af[2], bf[2];
  auto read_frags = [&](int slot, int v_off, int u_off) {
    af[slot] = *reinterpret_cast<const f32x4*>(s_v + a_base + v_off);
    bf[slot] = *reinterpret_cast<const f32x4*>(s_u + b_base + u_off);
  };
  read_frags(0, v_cur, u_cur);

  for (int ch = 0; ch < C::NCHUNK; ++ch) {
    // No branches inside the matrix loop: past the last chunk / step the loads repeat the last one (clamped index) and the staging
    // writes go to the free LDS slots, where nothing reads them.
    const int ch1 = ch + 1 < C::NCHUNK ? ch + 1 : C::NCHUNK - 1;
#pragma unroll
    for (int s = 0; s < SPC; ++s) {
      const int t = ch * SPC + s;
      // (1) global loads: weights of step t + 3; at the chunk's first step the next chunk's input pixels
      fetch_w(t + 3 < NSTEPS ? t + 3 : NSTEPS - 1, w_regs[s & 1]);
      if (s == 0) fetch_in(ch1, d);
      __builtin_amdgcn_sched_barrier(0);
      // (2) four groups of four matrix instructions: position 2s (channels 0-7, 8-15), position 2s + 1
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int cur = q & 1, nxt = cur ^ 1;
        const int pl = q >> 1;
        if (q < 3) {
          const int pl1 = (q + 1) >> 1, g1 = (q + 1) & 1;
          read_frags(nxt, v_cur + (2 * s + pl1) * C::V_POS + g1 * 8, u_cur + pl1 * C::U_POS + g1 * 8);
        } else if (s + 1 < SPC) {
          read_frags(nxt, v_cur + (2 * s + 2) * C::V_POS, u_n1);        // next step, same chunk (published one barrier ago)
        } else {
          read_frags(nxt, v_nxt, u_n1);                                 // next chunk's V was published two barriers ago
        }
        // staging, a few instructions per group: weights of step t + 2 (loaded during step t - 1); the next chunk's input transform
        store_w1(u_n2, w_regs[(s + 1) & 1], q);
        if (s == SPC - 3) in_rows(d, q);
        if (s == SPC - 2) in_cols_store(v_nxt, d, q);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[2 * s + pl] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[cur][j], bf[cur][j], acc[2 * s + pl], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
      // (3) one barrier per step publishes what was staged and frees the slots read in this step
      __syncthreads();
      { const int tu = u_cur; u_cur = u_n1; u_n1 = u_n2; u_n2 = tu; }
      if (s == SPC - 1) { const int tv = v_cur; v_cur = v_nxt; v_nxt = tv; }
    }
  }

  // ---- epilogue: output transform Y = A^T m A in registers, LeakyReLU, NHWC stores ----
  // Register v of a tile is patch 8 (v / 4) + 4 h + (v % 4) of the tile (patch = 16 py + px), channel r of the wave's 32.
  const float alpha = p.act ? kLeakyAlpha : 1.f;
  const unsigned cs4 = (unsigned)p.out_cs * 4u;
  const __amdgpu_buffer_rsrc_t orsrc =
      make_rsrc(p.out + ((size_t)img * p.H * p.W + (size_t)y0 * p.W + x0) * p.out_cs + n0 + wave * 32);
  const unsigned lane_out = (unsigned)(8 * h) * cs4 + (unsigned)r * 4u;      // patch column 4h = pixel column 8h
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    float t0[4], t1[4];
#pragma unroll
    for (int nu = 0; nu < 4; ++nu) {
      t0[nu] = (acc[nu][v] + acc[4 + nu][v]) + acc[8 + nu][v];
      t1[nu] = (acc[4 + nu][v] - acc[8 + nu][v]) - acc[12 + nu][v];
    }
    f32x2 y0v = f32x2{(t0[0] + t0[1]) + t0[2], (t0[1] - t0[2]) - t0[3]};
    f32x2 y1v = f32x2{(t1[0] + t1[1]) + t1[2], (t1[1] - t1[2]) - t1[3]};
    const f32x2 s0 = y0v * alpha, s1 = y1v * alpha;
    const int prow = 2 * (v >> 3), pcol = 2 * (8 * ((v >> 2) & 1) + (v & 3));
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const float x = i ? y1v[j] : y0v[j], ax = i ? s1[j] : s0[j];
        const unsigned soff = (unsigned)((prow + i) * p.W + pcol + j) * cs4;
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(__builtin_amdgcn_fmed3f(x, ax, 3.4028234664e38f)), orsrc, lane_out, soff, 0);
      }
  }
}

// ---- the wave-pair form: eight waves per workgroup, two per SIMD ----
// Same tile (4x32 pixels, 32 patches, all 128 output channels), same matrix instructions in the same order into every accumulator, but a
// wave is (channel quarter w, column half c) and holds only the transform positions 4 xi + nu with nu in {2c, 2c + 1}: 8 accumulator
// tiles = 128 registers, so two waves fit a SIMD and one issues matrix instructions while the other reads fragments, stages or waits.
//  * A step is the four positions 4 xi .. 4 xi + 3 of a chunk (contiguous in the stream, a 40-KB U slot): 16 matrix instructions per
//    wave, 32 per SIMD and barrier; four steps per chunk.  U flows through a 3-slot ring as above, from ONE register set: a group
//    writes one 16-byte element of step t+2 to LDS and reloads its registers with the same element of step t+3.
//  * V is ONE 40-KB image written in place: step xi reads row xi (positions 4 xi .. 4 xi + 3) only, so row xi of the next chunk is
//    written once the barrier that ends step xi has passed, and is published at least one barrier before its first fragment read.
//    All 512 threads stage alike: an input-transform item is (patch, ONE channel), which halves the registers of the pair form
//    above and keeps every branch out of the loop; the weights of a step are four 16-byte elements per thread.
//  * Waves 4-7 run the loop at a static priority 1 (they are the arbitration losers of their SIMD otherwise).
//  * Output transform: the row combinations t0, t1 are local to a wave (it holds all xi of its nu); the column combination needs the
//    partner's t0, t1 at ONE nu (half 0 needs nu = 2, half 1 needs nu = 1): 32 floats per lane each way through LDS, which is dead
//    after the loop's last barrier.  Each half stores its own pixel column of the 2x2 patches.  Every sum keeps the operand order of the
//    kernel above, so the output bits are the same.
struct WinoPairCfg {
  static constexpr int NT = 512;
  static constexpr int CC = 16, LDP = CC + 4;
  static constexpr int K = 128, N = 128, NCHUNK = K / CC;
  static constexpr int SPC = 4;                   // steps per chunk: four transform positions (one xi) each
  static constexpr int NSTEPS = NCHUNK * SPC;
  static constexpr int V_POS = 32 * LDP;
  static constexpr int V_FLOATS = 16 * V_POS;
  static constexpr int U_POS = N * LDP;
  static constexpr int U_FLOATS = 4 * U_POS;
  static constexpr int SMEM_BYTES = (V_FLOATS + 3 * U_FLOATS) * 4;
  static constexpr int X_FLOATS = 8 * 32 * 64;    // the epilogue's exchange: [wave][32 values][lane]
  static_assert(SMEM_BYTES <= 160 * 1024 && X_FLOATS * 4 <= SMEM_BYTES, "LDS budget");
};

__global__ __launch_bounds__(512, 2) void wino_conv2_pairs_kernel(WinoArgs p) {
  using C = WinoPairCfg;
  constexpr int LDP = C::LDP, SPC = C::SPC, NSTEPS = C::NSTEPS;
  typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* s_v = smem;
  float* s_u = smem + C::V_FLOATS;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wq = wave & 3, c = wave >> 2;           // channel quarter, column half: waves wq and wq + 4 share the channels (and a SIMD)
  const int h = lane >> 5, r = lane & 31;

  int bid = blockIdx.x;
  const int tile_x = bid % p.tiles_x;
  bid /= p.tiles_x;
  const int tile_y = bid % p.tiles_y;
  const int img = bid / p.tiles_y;
  const int y0 = tile_y * 4, x0 = tile_x * 32;
  const float* in_img = p.in + (size_t)img * p.H * p.W * p.in_cs;
  const __amdgpu_buffer_rsrc_t in_rsrc = make_rsrc(in_img);

  // ---- per-thread constants, as in the kernel above, but an input-transform item is (patch, ONE channel): 512 items, one per thread ----
  unsigned in_goff[16];
  const int patch = tid >> 4, cn = tid & 15;
  {
    const int py = patch >> 4, px = patch & 15;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int iy = y0 + 2 * py - 1 + a, ix = x0 + 2 * px - 1 + b;
        const bool ok = iy >= 0 && iy < p.H && ix >= 0 && ix < p.W;
        in_goff[4 * a + b] = ok ? (unsigned)(((iy * p.W + ix) * p.in_cs + cn) * 4) : kLaneOff;
      }
  }
  const int v_loff = patch * LDP + cn;
  // a step is four (chunk, position) blocks of [128 cout][16]: a thread moves element tid (16 bytes: cout tid / 4, channels 4 (tid % 4) ..) of each
  const unsigned w_goff = (unsigned)(tid * 16);
  const int w_loff = (tid >> 2) * LDP + (tid & 3) * 4;
  const __amdgpu_buffer_rsrc_t w_rsrc = make_rsrc(p.w);
  constexpr unsigned kPosBytes = (unsigned)(C::N * C::CC * 4);
  const float bias_n = c == 0 ? p.bias[wq * 32 + r] : 0.f;         // position 5 = (xi 1, nu 1) belongs to half 0

  auto fetch_in = [&](int chunk, float (&d)[16]) {
    const unsigned soff = (unsigned)(chunk * C::CC * 4);
#pragma unroll
    for (int i = 0; i < 16; ++i)
      d[i] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(in_rsrc, in_goff[i], soff, 0));
  };
  auto in_rows = [&](float (&d)[16], int b) {
    const float d0 = d[b], d1 = d[4 + b], d2 = d[8 + b], d3 = d[12 + b];
    d[b] = d0 - d2;
    d[4 + b] = d1 + d2;
    d[8 + b] = d2 - d1;
    d[12 + b] = d1 - d3;
  };
  auto in_cols_store = [&](const float (&d)[16], int a) {
    const float w0 = d[4 * a], w1 = d[4 * a + 1], w2 = d[4 * a + 2], w3 = d[4 * a + 3];
    float* dst = s_v + v_loff + 4 * a * C::V_POS;
    dst[0] = w0 - w2;
    dst[C::V_POS] = w1 + w2;
    dst[2 * C::V_POS] = w2 - w1;
    dst[3 * C::V_POS] = w1 - w3;
  };
  // step t = positions 4 (t % 4) .. + 3 of chunk t / 4 = blocks 4t .. 4t + 3 of the stream
  auto fetch_w1 = [&](int t, f32x4 (&regs)[4], int j) {
    regs[j] = __builtin_bit_cast(f32x4, (u32x4_t)__builtin_amdgcn_raw_buffer_load_b128(w_rsrc, w_goff, (unsigned)(4 * t + j) * kPosBytes, 0));
  };
  auto store_w1 = [&](int u_off, const f32x4 (&regs)[4], int i) {
    *reinterpret_cast<f32x4*>(s_u + u_off + i * C::U_POS + w_loff) = regs[i];
  };

  // ---- prologue: chunk 0 of the input (rows 0-2 to LDS; row 3 goes at step 0, as in every chunk), weight steps 0 and 1 to LDS,
  // step 2 in flight ----
  float d[16];
  f32x4 w_regs[4];
  int u_cur = 0, u_n1 = C::U_FLOATS, u_n2 = 2 * C::U_FLOATS;
  fetch_in(0, d);
#pragma unroll
  for (int t = 0; t < 2; ++t) {
#pragma unroll
    for (int i = 0; i < 4; ++i) fetch_w1(t, w_regs, i);
#pragma unroll
    for (int i = 0; i < 4; ++i) store_w1(t * C::U_FLOATS, w_regs, i);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) fetch_w1(2, w_regs, i);
#pragma unroll
  for (int b = 0; b < 4; ++b) in_rows(d, b);
#pragma unroll
  for (int a = 0; a < 3; ++a) in_cols_store(d, a);
  __syncthreads();

  // acc[2 xi + pl] = position 4 xi + 2c + pl
  f32x16 acc[8];
#pragma unroll
  for (int q = 0; q < 8; ++q)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[q][i] = 0.f;
  acc[3] = bias_tile(h, bias_n);                    // half 0: the bias at position (1, 1); half 1: 1 * 0 + 0 * 0 + 0 = +0, the same start as the others

  const int a_base = 2 * c * C::V_POS + r * LDP + 4 * h;
  const int b_base = 2 * c * C::U_POS + (wq * 32 + r) * LDP + 4 * h;
  f32x4 af[2], bf[2];
  auto read_frags = [&](int slot, int v_off, int u_off) {
    af[slot] = *reinterpret_cast<const f32x4*>(s_v + a_base + v_off);
    bf[slot] = *reinterpret_cast<const f32x4*>(s_u + b_base + u_off);
  };
  read_frags(0, 0, u_cur);

  // Waves 4-7 are dispatched second and lose the issue arbitration against their SIMD partner at equal priority: one static priority
  // for that half, no per-group flips (measured: profiles/HISTORY.md round 10).
  if (c) __builtin_amdgcn_s_setprio(1);
#pragma unroll 1
  for (int ch = 0; ch < C::NCHUNK; ++ch) {
    // No data-dependent branches in the matrix loop: past the last chunk / step the loads repeat the last one (clamped index), the weight
    // staging goes to free slots, and the last chunk's V rows are rewritten with their own values after their last use.
    const int ch1 = ch + 1 < C::NCHUNK ? ch + 1 : C::NCHUNK - 1;
#pragma unroll
    for (int s = 0; s < SPC; ++s) {
      const int t = ch * SPC + s;
      const int t3 = t + 3 < NSTEPS ? t + 3 : NSTEPS - 1;
      // four groups of four matrix instructions: position 4s + 2c (channels 0-7, 8-15), position 4s + 2c + 1
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int cur = q & 1, nxt = cur ^ 1;
        const int pl = q >> 1;
        if (q < 3) {
          const int pl1 = (q + 1) >> 1, g1 = (q + 1) & 1;
          read_frags(nxt, (4 * s + pl1) * C::V_POS + g1 * 8, u_cur + pl1 * C::U_POS + g1 * 8);
        } else {
          read_frags(nxt, (4 * ((s + 1) % SPC)) * C::V_POS, u_n1);      // next step: both published at least one barrier ago
        }
        // staging, a few instructions per group: position q of the weights of step t + 2 (loaded during step t - 1) goes to LDS and its
        // registers take the same position of step t + 3
        store_w1(u_n2, w_regs, q);
        fetch_w1(t3, w_regs, q);
        // the input transform, V row by row behind the step that read the row last (row xi is free once step xi's barrier has passed):
        //   step 0: row 3 of THIS chunk (read first at the end of step 2), then the next chunk's pixels are loaded;
        //   step 2: the next chunk's row combinations, its rows 0 and 1;  step 3: its row 2
        if (s == 0 && q == 0) in_cols_store(d, 3);
        if (s == 0 && q == 1) fetch_in(ch1, d);
        if (s == 2 && q == 0) { in_rows(d, 0); in_rows(d, 1); }
        if (s == 2 && q == 1) { in_rows(d, 2); in_rows(d, 3); }
        if (s == 2 && q == 2) in_cols_store(d, 0);
        if (s == 2 && q == 3) in_cols_store(d, 1);
        if (s == 3 && q == 0) in_cols_store(d, 2);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[2 * s + pl] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[cur][j], bf[cur][j], acc[2 * s + pl], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
      // one barrier per step publishes what was staged and frees the U slot and the V row read in this step
      __syncthreads();
      { const int tu = u_cur; u_cur = u_n1; u_n1 = u_n2; u_n2 = tu; }
    }
  }

  __builtin_amdgcn_s_setprio(0);
  // ---- epilogue: row combinations in registers, one value pair per (patch, cout) exchanged with the partner half through LDS (every
  // fragment read and staging write is behind the loop's last barrier), column combination, LeakyReLU, NHWC stores of pixel column c ----
  // Register v of a tile is patch 8 (v / 4) + 4 h + (v % 4) of the tile (patch = 16 py + px), channel r of the wave's 32.
  float t0[2][16], t1[2][16];
#pragma unroll
  for (int pl = 0; pl < 2; ++pl)
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      t0[pl][v] = (acc[pl][v] + acc[2 + pl][v]) + acc[4 + pl][v];
      t1[pl][v] = (acc[2 + pl][v] - acc[4 + pl][v]) - acc[6 + pl][v];
    }
  // half 0 sends nu = 1 (its pl 1), half 1 sends nu = 2 (its pl 0): [wave][k][lane], k = v for t0 and 16 + v for t1
  float* x_mine = smem + (wave * 32) * 64 + lane;
  const float* x_theirs = smem + ((wave ^ 4) * 32) * 64 + lane;
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    x_mine[v * 64] = c ? t0[0][v] : t0[1][v];
    x_mine[(16 + v) * 64] = c ? t1[0][v] : t1[1][v];
  }
  __syncthreads();
  float y0v[16], y1v[16];
  if (c == 0) {
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      y0v[v] = (t0[0][v] + t0[1][v]) + x_theirs[v * 64];
      y1v[v] = (t1[0][v] + t1[1][v]) + x_theirs[(16 + v) * 64];
    }
  } else {
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      y0v[v] = (x_theirs[v * 64] - t0[0][v]) - t0[1][v];
      y1v[v] = (x_theirs[(16 + v) * 64] - t1[0][v]) - t1[1][v];
    }
  }
  const float alpha = p.act ? kLeakyAlpha : 1.f;
  const unsigned cs4 = (unsigned)p.out_cs * 4u;
  const __amdgpu_buffer_rsrc_t orsrc =
      make_rsrc(p.out + ((size_t)img * p.H * p.W + (size_t)y0 * p.W + x0) * p.out_cs + wq * 32);
  const unsigned lane_out = (unsigned)(8 * h) * cs4 + (unsigned)r * 4u;      // patch column 4h = pixel column 8h
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    const int prow = 2 * (v >> 3), pcol = 2 * (8 * ((v >> 2) & 1) + (v & 3));
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const float x = i ? y1v[v] : y0v[v];
      const unsigned soff = (unsigned)((prow + i) * p.W + pcol + c) * cs4;
      __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(__builtin_amdgcn_fmed3f(x, x * alpha, 3.4028234664e38f)), orsrc, lane_out, soff, 0);
    }
  }
}

// NW = 4 unless the tiles cover at most half of the compute units (then two workgroups per tile)
inline int wino_conv2_auto_nw(int batch, int H, int W) {
  const long long tiles = (long long)batch * (H / 4) * (W / 32);
  return 2 * tiles <= device_cu_count() ? 2 : 4;
}

inline hipError_t launch_wino_conv2_pairs(WinoArgs a, int batch, hipStream_t stream) {
  using C = WinoPairCfg;
  static PerDeviceOnce once;
  const int dev = PerDeviceOnce::current();
  if (dev < 0 || !once.done[dev]) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(wino_conv2_pairs_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, C::SMEM_BYTES);
    if (e != hipSuccess) return e;
    if (dev >= 0) once.done[dev] = true;
  }
  a.tiles_x = a.W / 32;
  a.tiles_y = a.H / 4;
  hipLaunchKernelGGL(wino_conv2_pairs_kernel, dim3(a.tiles_x * a.tiles_y * batch), dim3(C::NT), C::SMEM_BYTES, stream, a);
  return hipGetLastError();
}

template <int NW>
inline hipError_t launch_wino_conv2_nw(WinoArgs a, int batch, hipStream_t stream) {
  using C = WinoCfg<NW>;
  auto kern = wino_conv2_kernel<NW>;
  static PerDeviceOnce once;
  const int dev = PerDeviceOnce::current();
  if (dev < 0 || !once.done[dev]) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, C::SMEM_BYTES);
    if (e != hipSuccess) return e;
    if (dev >= 0) once.done[dev] = true;
  }
  a.tiles_x = a.W / 32;
  a.tiles_y = a.H / 4;
  dim3 grid(a.tiles_x * a.tiles_y * batch, 4 / NW);
  hipLaunchKernelGGL(kern, grid, dim3(C::NT), C::SMEM_BYTES, stream, a);
  return hipGetLastError();
}

// H a multiple of 4, W a multiple of 32 (the caller checks); nw = 0: by the grid, where a full grid takes the wave-pair form (nw = 8)
// unless `pairs` is off
inline hipError_t launch_wino_conv2(const WinoArgs& a, int batch, hipStream_t stream, int nw = 0, bool pairs = true) {
  if (nw == 0) {
    nw = wino_conv2_auto_nw(batch, a.H, a.W);
    if (nw == 4 && pairs) nw = 8;
  }
  if (nw == 8) return launch_wino_conv2_pairs(a, batch, stream);
  return nw == 2 ? launch_wino_conv2_nw<2>(a, batch, stream) : launch_wino_conv2_nw<4>(a, batch, stream);
}

}  // namespace bsr
