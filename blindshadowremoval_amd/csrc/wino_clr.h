// The fp32 colour tail with clr_conv1 in Winograd F(2x2, 3x3) form on v_mfma_f32_16x16x4_f32, the transformed input held in registers:
// clr_conv1 = Conv(16, 3x3) over cat[gs, f] (65 -> 16, + BN + LeakyReLU) with clr_conv2, clr_conv3 and dif fused behind it — the launch
// conv_n16_kernel<3, 3, true, true, 2> does in direct form (conv_n16.h), 16 products per 2x2 output patch instead of 36.
//
// Standard transforms (Lavin & Gray 2016, as wino_conv2.h): V = B^T d B over the patch's 4x4 input pixels, M = sum_c U_c . V_c at each of
// the 16 positions 4 xi + nu, Y = A^T M A.  U = G g G^T is computed once per handle in fp64 and rounded once (bsr_api.hip:
// wino_clr_filter_transform; pack.py: pack_wino_clr states the same).
//
// The GEMM is conv_n16.h's TRANSPOSED one: A = weights (M = 16 output channels), B = 16 PATCHES (one patch row of a 32-pixel-wide strip),
// K = 4 per instruction.  The B operand of lane (r = lane & 15, q = lane >> 4) is element (k = q, n = r), so the lane that owns patch r
// and channels 4q .. 4q + 3 of a 16-channel K group
//   * loads its patch's input pixels as 16-byte raw-buffer loads (out-of-image columns through the out-of-range-returns-zero rule,
//     out-of-image rows through a resource of no records: the same zero, no branch) — its own two columns of the four, the other two
//     come from the neighbouring patches' lanes by DPP behind the transform's row pass (see fetch_f),
//   * computes V for its four channels in registers (32 four-wide adds, 64 values), and
//   * holds exactly the B operands of that K group's 16 positions x 4 matrix instructions.
// V never goes through LDS, no wave reads another wave's V, and the matrix loop has no barrier.
//  * The 16 position accumulators of a wave (64 registers) are one patch tile; the output transform is in-lane (24 four-wide adds) and
//    leaves channels 4q .. 4q + 3 of each of the patch's four pixels in the lane — the layout of conv_n16.h's fused tail, which runs here
//    once per pixel of the patch with its operations and their order unchanged.
//  * gs is one more K group with a single live k: the lanes with q = 0 load and transform the patch's 4x4 gs scalars, the others are
//    masked and supply the zeros they loaded.  16 matrix instructions per patch tile.
//  * U ([16 positions][4 K groups][64 lanes][4] in A-fragment order, then [16 positions][16 cout] of the gs channel: 65 KB) is the same for
//    every tile: a persistent workgroup stages it ONCE into LDS and reads fragments as ds_read_b128.  With the fused tail's weights the
//    workgroup holds 68 KB, two workgroups per compute unit, two waves per SIMD.
//  * Persistent workgroups of 4 waves = 4 patch rows = an 8x32-pixel tile, tiles blockIdx.x, + gridDim.x, ...  The input loads of the next
//    K group — across a tile boundary those of the next tile — are in flight while the current group is multiplied.
//  * Per output element the operations and their order do not depend on batch, grid, tile position or image size.
#pragma once
#include <hip/hip_runtime.h>

#include "conv_n16.h"

namespace bsr {

struct WinoClrCfg {
  static constexpr int TH = 8, TW = 32;
  static constexpr int U_FLOATS = 16 * 4 * 64 * 4;      // [position][K group][lane 16 q + r][j]: U[position][cout r][channel 16 g + 4 q + j]
  static constexpr int UGS_FLOATS = 16 * 16;            // [position][cout]
  static constexpr int W_FLOATS = U_FLOATS + UGS_FLOATS;
  static constexpr int TAIL_FLOATS = 340 + 16;          // conv_n16.h's tail_w (337 floats), then clr_conv1's bias
  static constexpr int SMEM_BYTES = (W_FLOATS + TAIL_FLOATS) * 4;
  static_assert(2 * SMEM_BYTES <= 160 * 1024, "two workgroups per compute unit");
};

// `src` of the lane the DPP control names (within the 16 lanes of one q); a lane that has no such neighbour keeps `old`
template <int CTRL>
__device__ __forceinline__ float wino_clr_from_lane(float old, float src) {
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(old), __float_as_int(src), CTRL, 0xf, 0xf, false));
}
template <int CTRL>
__device__ __forceinline__ f32x4 wino_clr_from_lane(const f32x4& old, const f32x4& src) {
  return f32x4{wino_clr_from_lane<CTRL>(old[0], src[0]), wino_clr_from_lane<CTRL>(old[1], src[1]), wino_clr_from_lane<CTRL>(old[2], src[2]),
               wino_clr_from_lane<CTRL>(old[3], src[3])};
}

// p.w = the handle's transformed image (WinoClrCfg::W_FLOATS floats); the other fields as conv_n16_kernel<3, 3, true, true, 2> reads them.
__global__ __launch_bounds__(256, 2) void wino_clr_kernel(ConvN16Args p) {
  using C = WinoClrCfg;
  typedef unsigned u32x2_t __attribute__((ext_vector_type(2)));
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* s_u = smem;
  float* s_ugs = smem + C::U_FLOATS;
  float* s_tail = smem + C::W_FLOATS;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15, q = lane >> 4;

  struct Tile { int img, y0, x0; };
  const int ntiles = p.tiles_x * p.tiles_y * p.batch;
  auto decode = [&](int t) {
    Tile d;
    d.x0 = (t % p.tiles_x) * C::TW;
    t /= p.tiles_x;
    d.y0 = (t % p.tiles_y) * C::TH;
    d.img = t / p.tiles_y;
    return d;
  };

  // The 4x4 input pixels of this lane's patch are rows y0 + 2 wave - 1 + a, columns x0 + 2 r - 1 + b.  Neighbouring patches share two
  // of their four columns, and the lanes of one q are a DPP row: a lane LOADS only its own two columns b = 1, 2 (always inside the image)
  // and takes column b = 0 from lane r - 1 and b = 3 from lane r + 1 after the row pass of the transform (row_shr:1 / row_shl:1; a lane
  // without a neighbour keeps `old`).  The strip's outer columns x0 - 1 and x0 + 32 are one more load per row, live in the lanes
  // r = 0 and r = 15 only (kLaneOff in the others and outside the image).  Half the vector-memory instructions and cache-line requests
  // of sixteen full loads.  Measured at B = 32 (profiles/HISTORY.md, round 12): 286 us with sixteen loads, 238 us this way (direct kernel: 355 us).
  // The resource starts at pixel (row 0, column 0) of the window; the row and the K group are the wave-uniform offset.  Rows a = 0 and
  // a = 3 can lie outside the image (the first / last patch row): they read through a resource of no records, which returns zeros.
  const __amdgpu_buffer_rsrc_t no_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.in), 0, 0, 0x00020000);
  auto pick = [&](bool ok, const __amdgpu_buffer_rsrc_t& a) { return ok ? a : no_rsrc; };
  auto edge_col = [&](const Tile& d) { return r == 0 && d.x0 > 0 ? 0 : r == 15 && d.x0 + C::TW < p.W ? C::TW + 1 : -1; };      // window column of this lane's outer pixel
  auto fetch_f = [&](const Tile& d, int g, f32x4 (&regs)[12]) {      // [3 a + 0, 1]: columns b = 1, 2; [3 a + 2]: the outer column
    const int iy0 = d.y0 + 2 * wave - 1, ix0 = d.x0 - 1;
    const __amdgpu_buffer_rsrc_t rs = make_rsrc(p.in + (((ptrdiff_t)d.img * p.H + iy0) * p.W + ix0) * p.in_cs);
    const __amdgpu_buffer_rsrc_t rs0 = pick(iy0 >= 0, rs), rs3 = pick(iy0 + 3 < p.H, rs);
    const int ec = edge_col(d);
    const unsigned voff[3] = {(unsigned)((2 * r + 1) * p.in_cs + 4 * q) * 4u, (unsigned)((2 * r + 2) * p.in_cs + 4 * q) * 4u,
                              ec >= 0 ? (unsigned)(ec * p.in_cs + 4 * q) * 4u : kLaneOff};
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b)
        regs[3 * a + b] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(a == 0 ? rs0 : a == 3 ? rs3 : rs, voff[b],
                                                                                           (unsigned)(a * p.W * p.in_cs + g * 16) * 4u, 0));
  };
  const __amdgpu_buffer_rsrc_t no_gs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.gs), 0, 0, 0x00020000);
  auto fetch_gs = [&](const Tile& d, float (&regs)[12]) {
    const int iy0 = d.y0 + 2 * wave - 1, ix0 = d.x0 - 1;
    const __amdgpu_buffer_rsrc_t rs = make_rsrc(p.gs + ((ptrdiff_t)d.img * p.H + iy0) * p.W + ix0);
    const __amdgpu_buffer_rsrc_t rs0 = iy0 >= 0 ? rs : no_gs, rs3 = iy0 + 3 < p.H ? rs : no_gs;
    const int ec = edge_col(d);
    // q != 0: masked, the lane supplies the zeros it loads
    const unsigned voff[3] = {q == 0 ? (unsigned)(2 * r + 1) * 4u : kLaneOff, q == 0 ? (unsigned)(2 * r + 2) * 4u : kLaneOff,
                              q == 0 && ec >= 0 ? (unsigned)ec * 4u : kLaneOff};
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b)
        regs[3 * a + b] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(a == 0 ? rs0 : a == 3 ? rs3 : rs, voff[b], (unsigned)(a * p.W) * 4u, 0));
  };
  // V = B^T d B, B^T = rows (1 0 -1 0), (0 1 1 0), (0 -1 1 0), (0 1 0 -1): rows first (on the lane's own columns and its outer one), then
  // columns, with the row-transformed columns 0 and 3 taken from the neighbouring lanes; position 4 xi + nu
  auto transform = [&](const auto (&d)[12], auto (&v)[16]) {
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      v[b] = d[b] - d[6 + b];
      v[4 + b] = d[3 + b] + d[6 + b];
      v[8 + b] = d[6 + b] - d[3 + b];
      v[12 + b] = d[3 + b] - d[9 + b];
    }
#pragma unroll
    for (int x = 0; x < 4; ++x) {
      const auto c1 = v[4 * x], c2 = v[4 * x + 1], ce = v[4 * x + 2];
      const auto c0 = wino_clr_from_lane<0x111>(ce, c2), c3 = wino_clr_from_lane<0x101>(ce, c1);      // row_shr:1, row_shl:1
      v[4 * x] = c0 - c2; v[4 * x + 1] = c1 + c2; v[4 * x + 2] = c2 - c1; v[4 * x + 3] = c1 - c3;
    }
  };

  // ---- prologue, once per workgroup: the first tile's first K group in flight, then U and the tail's weights into LDS ----
  int tile = (int)blockIdx.x;
  Tile cur = decode(tile < ntiles ? tile : 0);
  f32x4 ld[12];
  fetch_f(cur, 0, ld);
  for (int i = tid; i < C::W_FLOATS / 4; i += 256) reinterpret_cast<f32x4*>(smem)[i] = reinterpret_cast<const f32x4*>(p.w)[i];
  for (int i = tid; i < 337; i += 256) s_tail[i] = p.tail_w[i];
  if (tid < 16) s_tail[340 + tid] = p.bias[tid];
  __syncthreads();

  const float* u_lane = s_u + lane * 4;
  auto read_u = [&](int pos, int g) { return *reinterpret_cast<const f32x4*>(u_lane + (pos * 4 + g) * 256); };

  for (; tile < ntiles; tile += (int)gridDim.x) {
    const int tile_n = tile + (int)gridDim.x;
    const bool has_next = tile_n < ntiles;
    const Tile nxt = decode(has_next ? tile_n : tile);
    f32x4 acc[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    float gl[12];

#pragma unroll
    for (int g = 0; g < 4; ++g) {
      f32x4 v[16];
      transform(ld, v);
      // the next K group goes into the registers the transform has just read; behind the last group the gs scalars, then the next tile
      if (g < 3) {
        fetch_f(cur, g + 1, ld);
      } else {
        fetch_gs(cur, gl);
        if (has_next) fetch_f(nxt, 0, ld);
      }
      __builtin_amdgcn_sched_barrier(0);
      // positions in pairs, so that an accumulator's next instruction is two issue slots away; fragments read one pair ahead
      f32x4 af[2][2];
      af[0][0] = read_u(0, g);
      af[0][1] = read_u(1, g);
#pragma unroll
      for (int pp = 0; pp < 8; ++pp) {
        const int cu = pp & 1, nx = cu ^ 1;
        if (pp + 1 < 8) {
          af[nx][0] = read_u(2 * pp + 2, g);
          af[nx][1] = read_u(2 * pp + 3, g);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int hh = 0; hh < 2; ++hh)
            acc[2 * pp + hh] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[cu][hh][j], v[2 * pp + hh][j], acc[2 * pp + hh], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    {   // the gs channel: k = q, live in the lanes with q = 0
      float vg[16];
      transform(gl, vg);
      float ag[16];
#pragma unroll
      for (int pos = 0; pos < 16; ++pos) ag[pos] = s_ugs[pos * 16 + r];
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int pos = 0; pos < 16; ++pos) acc[pos] = __builtin_amdgcn_mfma_f32_16x16x4f32(ag[pos], vg[pos], acc[pos], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }

    // ---- epilogue.  The input pixels of the grayscale difference are requested now and used behind the tail's matrix instructions ----
    const size_t pix0 = ((size_t)cur.img * p.H + cur.y0 + 2 * wave) * p.W + cur.x0;      // the patch row's first pixel
    u32x2_t tin[2][3];
    {
      const __amdgpu_buffer_rsrc_t rs = make_rsrc(p.inputs + pix0 * 3);
      const unsigned voff = q == 0 ? (unsigned)(2 * r * 3) * 4u : kLaneOff;
#pragma unroll
      for (int dy = 0; dy < 2; ++dy)
#pragma unroll
        for (int e = 0; e < 3; ++e) tin[dy][e] = __builtin_amdgcn_raw_buffer_load_b64(rs, voff, (unsigned)(dy * p.W * 3 + 2 * e) * 4u, 0);
    }
    float tw2[4], tw3[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      tw2[e] = s_tail[(4 * q + e) * 16 + r];
      tw3[e] = s_tail[272 + (4 * q + e) * 3 + (r < 3 ? r : 0)];
    }
    const f32x4 tb2 = *reinterpret_cast<const f32x4*>(s_tail + 256 + 4 * q);
    const f32x4 b4 = *reinterpret_cast<const f32x4*>(s_tail + 340 + 4 * q);
    float tb3[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) tb3[c] = s_tail[320 + c];

    // Y = A^T M A, A^T = rows (1 1 1 0), (0 1 -1 -1): y[2 dy + dx]
    f32x4 y[4];
    {
      f32x4 t[2][4];
#pragma unroll
      for (int nu = 0; nu < 4; ++nu) {
        t[0][nu] = (acc[nu] + acc[4 + nu]) + acc[8 + nu];
        t[1][nu] = (acc[4 + nu] - acc[8 + nu]) - acc[12 + nu];
      }
#pragma unroll
      for (int dy = 0; dy < 2; ++dy) {
        y[2 * dy] = (t[dy][0] + t[dy][1]) + t[dy][2];
        y[2 * dy + 1] = (t[dy][1] - t[dy][2]) - t[dy][3];
      }
    }
    f32x4 a3[4];
#pragma unroll
    for (int px = 0; px < 4; ++px) {
      f32x4 v = y[px] + b4;
      if (p.act) {
#pragma unroll
        for (int e = 0; e < 4; e += 2) {
          const f32x2 z = leaky_relu2(f32x2{v[e], v[e + 1]});
          v[e] = z[0];
          v[e + 1] = z[1];
        }
      }
      // clr_conv2: y2^T[c2][px] = sum_c W2^T[c2][c] * y1^T[c][px]; register e of v is channel c = 4q + e (k index q)
      f32x4 a2 = tb2;
#pragma unroll
      for (int e = 0; e < 4; ++e) a2 = __builtin_amdgcn_mfma_f32_16x16x4f32(tw2[e], v[e], a2, 0, 0, 0);
#pragma unroll
      for (int e = 0; e < 4; e += 2) {
        const f32x2 z = leaky_relu2(f32x2{a2[e], a2[e + 1]});
        a2[e] = z[0];
        a2[e + 1] = z[1];
      }
      // clr_conv3: rows c3 = 0..2 (lanes r < 3 carry the weights, the rest multiply by 0)
      a3[px] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int e = 0; e < 4; ++e) a3[px] = __builtin_amdgcn_mfma_f32_16x16x4f32(r < 3 ? tw3[e] : 0.f, a2[e], a3[px], 0, 0, 0);
    }
    if (q == 0) {   // rows 0..2 = R,G,B of the patch's pixels (dy, dx)
#pragma clang fp contract(off)
#pragma unroll
      for (int px = 0; px < 4; ++px) {
        const int dy = px >> 1, dx = px & 1;
        const size_t pix = pix0 + (size_t)dy * p.W + 2 * r + dx;
        // the row's six input floats: pixel dx = words 3 dx .. 3 dx + 2
        const float in0 = __uint_as_float(dx ? tin[dy][1][1] : tin[dy][0][0]);
        const float in1 = __uint_as_float(dx ? tin[dy][2][0] : tin[dy][0][1]);
        const float in2 = __uint_as_float(dx ? tin[dy][2][1] : tin[dy][1][0]);
        const float cr = a3[px][0] + tb3[0], cg = a3[px][1] + tb3[1], cb = a3[px][2] + tb3[2];
        const float g1 = (cr * 0.2989f + cg * 0.5870f) + cb * 0.1140f;
        const float g0 = (in0 * 0.2989f + in1 * 0.5870f) + in2 * 0.1140f;
        if (p.packed != nullptr) {
          *reinterpret_cast<f32x4*>(p.packed + pix * 4) = f32x4{cr, cg, cb, g1 - g0};
        } else {
          p.con_rgb[pix * 3 + 0] = cr;
          p.con_rgb[pix * 3 + 1] = cg;
          p.con_rgb[pix * 3 + 2] = cb;
          p.dif[pix] = g1 - g0;
        }
      }
    }
    cur = nxt;
  }
}

// nullptr when the launcher takes the layer; else why not (the caller reports it BEFORE any launch)
inline const char* wino_clr_refusal(int batch, int H, int W, int in_cs) {
  if (batch <= 0 || H <= 0 || W <= 0) return "empty tensor";
  if (H % WinoClrCfg::TH != 0 || W % WinoClrCfg::TW != 0) return "image is not a multiple of its 8x32 tile";
  if (in_cs < 64 || in_cs % 4 != 0) return "channel stride must be a multiple of 4, at least 64";
  if ((long long)4 * (W + 2) * in_cs * 4 >= (1LL << 31)) return "image too wide for 32-bit offsets";
  if ((long long)batch * (H / WinoClrCfg::TH) * (W / WinoClrCfg::TW) >= (1LL << 31)) return "too many tiles";
  return nullptr;
}

// The caller has checked wino_clr_refusal().
inline hipError_t launch_wino_clr(ConvN16Args a, int batch, hipStream_t stream) {
  using C = WinoClrCfg;
  static PerDeviceOnce once;
  const int dev = PerDeviceOnce::current();
  if (dev < 0 || !once.done[dev]) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(wino_clr_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, C::SMEM_BYTES);
    if (e != hipSuccess) return e;
    if (dev >= 0) once.done[dev] = true;
  }
  a.tiles_x = a.W / C::TW;
  a.tiles_y = a.H / C::TH;
  a.batch = batch;
  const int ntiles = a.tiles_x * a.tiles_y * batch;
  const int resident = 2 * device_cu_count();      // two workgroups per compute unit (LDS)
  hipLaunchKernelGGL(wino_clr_kernel, dim3(ntiles < resident ? ntiles : resident), dim3(256), C::SMEM_BYTES, stream, a);
  return hipGetLastError();
}

}  // namespace bsr
