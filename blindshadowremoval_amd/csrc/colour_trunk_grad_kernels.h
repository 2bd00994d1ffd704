// The generator's backward pass between res_stack/5's input and res_stack/2's output, ON THE DEVICE, training=False: res_stack/4,
// res_stack/3 and the hole (model.py:256-262) — x_hole = x (1 - bmask), xh = cat[x_hole 257 | bmask | uv 3] with bmask under
// stop_gradient.  Given d_xin = d loss / d (res_stack/5's input) (bsr_bottleneck_grad's d_xin) and, optionally, the grey branch's
// gradient d_x at res_stack/2's output (bsr_grey_decoder_grad's d_x), it writes d_res2, the complete gradient at res_stack/2's output,
// and the 44 variable gradients of blocks 3 and 4.  blindshadowremoval_amd/generator_grad.py is the host statement
// (colour_trunk_grad); pack.pack_colour_trunk_grad writes the blob.
//
// The chain is the two existing chains as they are, with blocks 4's and 3's weights, and one kernel of its own.  49 launches on the
// caller's stream, one after the other: no host synchronisation, no second stream, no floating-point atomic; every word a launch reads
// was written by the caller or by an earlier launch of the same call, so a call repeats its bits.
//    1..12   launch_nonlocal_grad, block 4     d_out = d_xin, xin = out3            -> d_y3_4, d_skip_4, block 4's ten
//   13..24   launch_bottleneck_grad, block 4   xin = out3, d_y3_4, d_skip_4         -> d_xin4, block 4's twelve
//   25..36   launch_nonlocal_grad, block 3     d_out = d_xin4, xin = xh             -> d_y3_3, d_skip_3, block 3's ten
//   37..48   launch_bottleneck_grad, block 3   xin = xh, d_y3_3, d_skip_3           -> d_xin3, block 3's twelve
//   49       hole_grad_kernel                  d_res2 = d_xin3[..., :257] (1 - bmask) + d_x, bmask = xh[..., 257]
// Channel 257 of d_xin3 (bmask: constant under stop_gradient) and channels 258..260 (uv: an input) reach nothing.
//
// Each of the four sub-chains has a scratch region of its own, so that after a call the maps of both blocks can be read, and the six
// intermediate data gradients lie behind them.
#pragma once
#include "bottleneck_grad_kernels.h"

namespace bsr {

constexpr int kCtBlockLaunches = kNlLaunches + kBnLaunches;
constexpr int kCtLaunches = 2 * kCtBlockLaunches + 1;
constexpr int kCtBlockVars = kBnVars + kNlVars;
constexpr int kCtVars = 2 * kCtBlockVars;
constexpr int kCtC = 257, kCtX = 261;
constexpr int kCtData = 6;                                   // d_y3_4, d_skip_4, d_xin4, d_y3_3, d_skip_3, d_xin3
constexpr int kCtMaps = 2 * (kNlMaps + kBnMaps) + kCtData;

// float offsets inside the blob, the four existing blobs end to end in the order of the launches; part 4: the total.  Each part is a
// multiple of four floats, so every sub-blob keeps the 16-byte alignment of the whole.
inline size_t ct_blob_off(int part) {
  const size_t n[4] = {nl_blob_off(6), bn_blob_off(13), nl_blob_off(6), bn_blob_off(13)};      // block 4: non-local, bottleneck; block 3
  size_t o = 0;
  for (int i = 0; i < part && i < 4; ++i) o += n[i];
  return o;
}

// float offset of variable `index` inside grads, in weights.generator_colour_trunk_trainable_names' order: block 3's twelve bottleneck
// variables, its ten non-local ones, then block 4's; 44: the total
inline size_t ct_var_offset(int index) {
  const size_t bn = bn_var_offset(kBnVars), nl = nl_var_offset(kNlVars);
  size_t o = 0;
  if (index >= kCtVars) return 2 * (bn + nl);
  if (index >= kCtBlockVars) {
    o = bn + nl;
    index -= kCtBlockVars;
  }
  return index < kBnVars ? o + bn_var_offset(index) : o + bn + nl_var_offset(index - kBnVars);
}

// Byte offsets inside the scratch.  region: the sub-chains' scratches in the order of the launches (block 4's non-local chain, its
// bottleneck chain, block 3's two).  map 0..9 nl_plan's of block 4, 10..17 bn_plan's of block 4, 18..27 and 28..35 block 3's, 36 d_y3_4
// [N][257], 37 d_skip_4 [N][261], 38 d_xin4 [N][261], 39 d_y3_3, 40 d_skip_3, 41 d_xin3.
struct CtPlan {
  int N;
  size_t region[4], map[kCtMaps], total;
};
inline CtPlan ct_plan(int B, int h, int w) {
  CtPlan pl;
  BumpBytes bump;
  const NlPlan nl = nl_plan(B, h, w);
  const BnPlan bn = bn_plan(B, h, w);
  pl.N = nl.N;
  int m = 0;
  for (int r = 0; r < 4; ++r) {
    if (r % 2 == 0) {
      pl.region[r] = bump.take(nl.total);
      for (int i = 0; i < kNlMaps; ++i) pl.map[m++] = pl.region[r] + nl.map[i];
    } else {
      pl.region[r] = bump.take(bn.total);
      for (int i = 0; i < kBnMaps; ++i) pl.map[m++] = pl.region[r] + bn.map[i];
    }
  }
  const size_t N = (size_t)pl.N;
  for (int b = 0; b < 2; ++b) {
    pl.map[m++] = bump.take(N * kCtC * sizeof(float));
    pl.map[m++] = bump.take(N * kCtX * sizeof(float));
    pl.map[m++] = bump.take(N * kCtX * sizeof(float));
  }
  pl.total = bump.o;
  return pl;
}

// ---- launch 49: out [N][257] = g [N][261][:257] (1 - bmask[N]) + add [N][257], bmask = xh[n xh_cs + 257] in {0, 1}, so the product is
// exact and there is at most one rounding.  Bandwidth-bound glue: a thread per four consecutive floats of the dense output.  N is a
// multiple of 128, so 257 N is a multiple of 4 and the output and `add` go as aligned 16-byte accesses; output float i of pixel n lies
// at g[i + 4 n], so a quad inside one pixel is an aligned 16-byte load of g as well.  Three of four pixel boundaries fall inside a quad:
// those three quads in 257 load g by the float.  Consecutive lanes take consecutive quads: a wave's stores cover 1 KB without a gap.
struct HoleGradArgs {
  const float *g, *xh, *add;      // add: null for none
  float* out;
  int xh_cs;
  unsigned quads;                 // 257 N / 4
};

// grid (ceil(quads / 256))
__global__ __launch_bounds__(256) void hole_grad_kernel(const HoleGradArgs a) {
  const unsigned q = blockIdx.x * 256u + threadIdx.x;
  if (q >= a.quads) return;
  const unsigned i = 4u * q;                      // 257 N <= 257 * 2^21 < 2^32
  const unsigned n = i / kCtC, c = i - n * kCtC;
  const int first = kCtC - (int)c;                // how many of the quad's floats lie in pixel n: 1..4 of them when first < 4
  float4 v;
  float keep0 = 1.f - a.xh[(size_t)n * a.xh_cs + kCtC], keep1 = keep0;
  if (first >= 4) {
    v = *reinterpret_cast<const float4*>(a.g + (size_t)i + 4u * n);
  } else {
    keep1 = 1.f - a.xh[(size_t)(n + 1) * a.xh_cs + kCtC];
    float e[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) e[j] = a.g[(size_t)i + j + 4u * (j < first ? n : n + 1)];
    v = make_float4(e[0], e[1], e[2], e[3]);
  }
  v.x *= keep0;
  v.y *= first > 1 ? keep0 : keep1;
  v.z *= first > 2 ? keep0 : keep1;
  v.w *= first > 3 ? keep0 : keep1;
  if (a.add != nullptr) {
    const float4 d = *reinterpret_cast<const float4*>(a.add + i);
    v.x += d.x; v.y += d.y; v.z += d.z; v.w += d.w;
  }
  *reinterpret_cast<float4*>(a.out + i) = v;
}

// N pixels, a multiple of 4: g and out 16-byte aligned, add 16-byte aligned or null
inline hipError_t launch_hole_grad(const float* g, const float* xh, int xh_cs, const float* add, int N, float* out, hipStream_t stream) {
  HoleGradArgs a{g, xh, add, out, xh_cs, (unsigned)((size_t)N * kCtC / 4)};
  hipLaunchKernelGGL(hole_grad_kernel, dim3((a.quads + 255) / 256), dim3(256), 0, stream, a);
  return hipGetLastError();
}

// The first `stop_after` of the 49 launches above (kCtLaunches: all of them; fewer are for the tests' stage-by-stage comparison): one
// running budget across the four sub-chains and the hole.  y3x4, out4, y3x3, out3, xh [B,h,w,.] with their floats between pixels (block
// 4's input is out3, block 3's is xh), d_xin dense 261 wide, d_x dense 257 wide or null, d_res2 dense 257 wide; d_x and d_res2 16-byte
// aligned.
inline hipError_t launch_colour_trunk_grad(const float* blob, const float* y3x4, int y3x4_cs, const float* out4, int out4_cs, const float* y3x3,
                                           int y3x3_cs, const float* out3, int out3_cs, const float* xh, int xh_cs, const float* d_xin, const float* d_x,
                                           int B, int h, int w, float* d_res2, float* grads, void* scratch, int stop_after, hipStream_t stream) {
  const CtPlan pl = ct_plan(B, h, w);
  unsigned char* base = static_cast<unsigned char*>(scratch);
  auto f = [&](int map) { return reinterpret_cast<float*>(base + pl.map[map]); };
  const int data = kCtMaps - kCtData;
  const size_t block_floats = ct_var_offset(kCtBlockVars), bn_floats = bn_var_offset(kBnVars);
  const float* d_out = d_xin;
  hipError_t e;
  int left = stop_after;
  for (int k = 0; k < 2; ++k) {                   // block 4, then block 3
    const float *y3x = k == 0 ? y3x4 : y3x3, *xin = k == 0 ? out3 : xh, *out = k == 0 ? out4 : out3;
    const int y3x_cs = k == 0 ? y3x4_cs : y3x3_cs, xin_cs = k == 0 ? out3_cs : xh_cs, out_cs = k == 0 ? out4_cs : out3_cs;
    float *d_y3 = f(data + 3 * k), *d_skip = f(data + 3 * k + 1), *d_in = f(data + 3 * k + 2);
    float* g = grads + (k == 0 ? block_floats : 0);
    if (left <= 0) return hipSuccess;
    e = launch_nonlocal_grad(blob + ct_blob_off(2 * k), y3x, y3x_cs, xin, xin_cs, out, out_cs, d_out, B, h, w, d_y3, d_skip, g + bn_floats,
                             base + pl.region[2 * k], left < kNlLaunches ? left : kNlLaunches, stream);
    if (e != hipSuccess) return e;
    left -= kNlLaunches;
    if (left <= 0) return hipSuccess;
    e = launch_bottleneck_grad(blob + ct_blob_off(2 * k + 1), xin, xin_cs, d_y3, d_skip, B, h, w, d_in, g, base + pl.region[2 * k + 1],
                               left < kBnLaunches ? left : kBnLaunches, stream);
    if (e != hipSuccess) return e;
    left -= kBnLaunches;
    d_out = d_in;
  }
  if (left <= 0) return hipSuccess;
  return launch_hole_grad(d_out, xh, xh_cs, d_x, pl.N, d_res2, stream);
}

}  // namespace bsr
