// The generator's backward pass between res_stack/5's input and res_stack/2's output, ON THE DEVICE, training=False: res_stack/4,
// res_stack/3 and the hole (model.py:256-262) — x_hole = x (1 - bmask), xh = cat[x_hole 257 | bmask | uv 3] with bmask under
// stop_gradient.  Given d_xin = d loss / d (res_stack/5's input) (bsr_bottleneck_grad's d_xin) and, optionally, the grey branch's
// gradient d_x at res_stack/2's output (bsr_grey_decoder_grad's d_x), it writes d_res2, the complete gradient at res_stack/2's output,
// and the 44 variable gradients of blocks 3 and 4.  blindshadowremoval_amd/generator_grad.py is the host statement
// (colour_trunk_grad); pack.pack_colour_trunk_grad writes the blob.
//
// The chain is block_chain_grad.h's kColourChain, whose header lists its 48 launches, and one kernel of its own as the tail:
//   49       hole_grad_kernel                  d_res2 = d_xin3[..., :257] (1 - bmask) + d_x, bmask = xh[..., 257]
// Channel 257 of d_xin3 (bmask: constant under stop_gradient) and channels 258..260 (uv: an input) reach nothing.
#pragma once
#include "block_chain_grad.h"

namespace bsr {

constexpr int kCtC = kChainC;

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

// The first `stop_after` of the 49 launches (kColourChain.launches(): all of them; fewer are for the tests' stage-by-stage comparison):
// one running budget across the four sub-chains and the hole.  y3x4, out4, y3x3, out3, xh [B,h,w,.] with their floats between pixels
// (block 4's input is out3, block 3's is xh), d_xin dense 261 wide, d_x dense 257 wide or null, d_res2 dense 257 wide; d_x and d_res2
// 16-byte aligned.
inline hipError_t launch_colour_trunk_grad(const float* blob, const float* y3x4, int y3x4_cs, const float* out4, int out4_cs, const float* y3x3,
                                           int y3x3_cs, const float* out3, int out3_cs, const float* xh, int xh_cs, const float* d_xin, const float* d_x,
                                           int B, int h, int w, float* d_res2, float* grads, void* scratch, int stop_after, hipStream_t stream) {
  const ChainBlockIn in[2] = {{y3x4, out3, out4, y3x4_cs, out3_cs, out4_cs}, {y3x3, xh, out3, y3x3_cs, xh_cs, out3_cs}};
  float* d_xin3 = nullptr;
  int left = stop_after;
  const hipError_t e = launch_block_chain(kColourChain, blob, in, d_xin, B, h, w, &d_xin3, grads, scratch, left, stream);
  if (e != hipSuccess || left <= 0) return e;
  return launch_hole_grad(d_xin3, xh, xh_cs, d_x, B * h * w, d_res2, stream);
}

}  // namespace bsr
