// The generator's backward pass between res_stack/2's output and the trunk's input, ON THE DEVICE, training=False: res_stack/2,
// res_stack/1 and res_stack/0, the three blocks both branches share (model.py: x = cat[down3 96 | uv 3], then for i in
// range(n_res // 2)).  Given d_res2 = d loss / d (res_stack/2's output) (bsr_colour_trunk_grad's d_res2) it writes d_x0, the gradient at
// x0 = cat[down3's output 96 | the resized uv 3] (channels 96..98 belong to an input and reach nothing), and the 66 variable gradients
// of blocks 0, 1 and 2.  blindshadowremoval_amd/generator_grad.py is the host statement (lower_trunk_grad);
// pack.pack_lower_trunk_grad writes the blob.
//
// The chain is the two existing chains at the widths of these blocks' inputs: 257 for blocks 2 and 1 (the input is the block below's
// output, no channels of the skip's own) and 99 for block 0, whose skip reaches the first 99 of the 257 output channels only and
// whose conv1 is 99 -> 128 (nl_entry_kernel<X>, bn_entry_kernel<X>, bn_fold_kernel<X>, bn_finish_kernel<X>, and the launchers'
// K, tiles and strides).  72 launches on the caller's stream, one after the other: no host synchronisation, no second stream, no
// floating-point atomic; every word a launch reads was written by the caller or by an earlier launch of the same call, so a call
// repeats its bits.
//    1..12   launch_nonlocal_grad<257>, block 2     d_out = d_res2, xin = out1        -> d_y3_2, d_skip_2, block 2's ten
//   13..24   launch_bottleneck_grad<257>, block 2   xin = out1, d_y3_2, d_skip_2      -> d_xin2, block 2's twelve
//   25..36   launch_nonlocal_grad<257>, block 1     d_out = d_xin2, xin = out0        -> d_y3_1, d_skip_1, block 1's ten
//   37..48   launch_bottleneck_grad<257>, block 1   xin = out0, d_y3_1, d_skip_1      -> d_xin1, block 1's twelve
//   49..60   launch_nonlocal_grad<99>, block 0      d_out = d_xin1, xin = x0          -> d_y3_0, d_skip_0 (99 wide), block 0's ten
//   61..72   launch_bottleneck_grad<99>, block 0    xin = x0, d_y3_0, d_skip_0        -> d_x0 (99 wide), block 0's twelve
//
// Each of the six sub-chains has a scratch region of its own, so that after a call the maps of all three blocks can be read, and the
// eight intermediate data gradients lie behind them.
#pragma once
#include "bottleneck_grad_kernels.h"

namespace bsr {

constexpr int kLtBlocks = 3;
constexpr int kLtBlockLaunches = kNlLaunches + kBnLaunches;
constexpr int kLtLaunches = kLtBlocks * kLtBlockLaunches;
constexpr int kLtBlockVars = kBnVars + kNlVars;
constexpr int kLtVars = kLtBlocks * kLtBlockVars;
constexpr int kLtC = 257, kLtX0 = 99;
constexpr int kLtData = 8;                                   // d_y3_2, d_skip_2, d_xin2, d_y3_1, d_skip_1, d_xin1, d_y3_0, d_skip_0
constexpr int kLtBlockMaps = kNlMaps + kBnMaps;
constexpr int kLtMaps = kLtBlocks * kLtBlockMaps + kLtData;
static_assert(kLtLaunches == 72 && kLtVars == 66, "three blocks of twelve and twelve launches, of twelve and ten variables");

// the width of block b's input
constexpr int lt_width(int block) { return block == 0 ? kLtX0 : kLtC; }

// float offsets inside the blob, the six sub-blobs end to end in the order of the launches (block 2's non-local blob, its bottleneck
// blob, block 1's two, block 0's two); part 6: the total.  Each part is a multiple of four floats, so every sub-blob keeps the 16-byte
// alignment of the whole.
inline size_t lt_blob_off(int part) {
  size_t o = 0;
  for (int i = 0; i < part && i < 2 * kLtBlocks; ++i) o += i % 2 == 0 ? nl_blob_off(6) : bn_blob_off(13, lt_width(2 - i / 2));
  return o;
}

// the floats of block b's 22 variable gradients
inline size_t lt_block_floats(int block) { return bn_var_offset(kBnVars, lt_width(block)) + nl_var_offset(kNlVars); }

// float offset of variable `index` inside grads, in weights.generator_lower_trunk_trainable_names' order: block 0's twelve bottleneck
// variables, its ten non-local ones, then block 1's, then block 2's; 66: the total
inline size_t lt_var_offset(int index) {
  size_t o = 0;
  int block = 0;
  for (; block < kLtBlocks && index >= kLtBlockVars; ++block, index -= kLtBlockVars) o += lt_block_floats(block);
  if (block == kLtBlocks) return o;
  const int X = lt_width(block);
  return index < kBnVars ? o + bn_var_offset(index, X) : o + bn_var_offset(kBnVars, X) + nl_var_offset(index - kBnVars);
}

// Byte offsets inside the scratch.  region: the sub-chains' scratches in the order of the launches.  map 0..9 nl_plan's of block 2,
// 10..17 bn_plan's of block 2, 18..35 block 1's, 36..53 block 0's (its bn_plan at the width 99), 54 d_y3_2 [N][257], 55 d_skip_2
// [N][257], 56 d_xin2 [N][257], 57..59 the same of block 1, 60 d_y3_0 [N][257], 61 d_skip_0 [N][99].
struct LtPlan {
  int N;
  size_t region[2 * kLtBlocks], map[kLtMaps], total;
};
inline LtPlan lt_plan(int B, int h, int w) {
  LtPlan pl;
  BumpBytes bump;
  const NlPlan nl = nl_plan(B, h, w);
  pl.N = nl.N;
  int m = 0;
  for (int k = 0; k < kLtBlocks; ++k) {           // block 2, 1, 0
    const BnPlan bn = bn_plan(B, h, w, lt_width(2 - k));
    pl.region[2 * k] = bump.take(nl.total);
    for (int i = 0; i < kNlMaps; ++i) pl.map[m++] = pl.region[2 * k] + nl.map[i];
    pl.region[2 * k + 1] = bump.take(bn.total);
    for (int i = 0; i < kBnMaps; ++i) pl.map[m++] = pl.region[2 * k + 1] + bn.map[i];
  }
  const size_t N = (size_t)pl.N;
  for (int k = 0; k < kLtBlocks; ++k) {
    const int X = lt_width(2 - k);
    pl.map[m++] = bump.take(N * kLtC * sizeof(float));
    pl.map[m++] = bump.take(N * X * sizeof(float));
    if (k < kLtBlocks - 1) pl.map[m++] = bump.take(N * X * sizeof(float));      // block 0's d_xin is the call's output d_x0
  }
  pl.total = bump.o;
  return pl;
}

// one block of the chain: the non-local sub-chain, then the bottleneck's, under the running budget `left`
template <int X>
inline hipError_t lt_block(const float* nl_blob, const float* bn_blob, const float* y3x, int y3x_cs, const float* xin, int xin_cs, const float* out,
                           int out_cs, const float* d_out, int B, int h, int w, float* d_y3, float* d_skip, float* d_in, float* grads, void* nl_scratch,
                           void* bn_scratch, int& left, hipStream_t stream) {
  if (left <= 0) return hipSuccess;
  hipError_t e = launch_nonlocal_grad<X>(nl_blob, y3x, y3x_cs, xin, xin_cs, out, out_cs, d_out, B, h, w, d_y3, d_skip,
                                         grads + bn_var_offset(kBnVars, X), nl_scratch, left < kNlLaunches ? left : kNlLaunches, stream);
  if (e != hipSuccess) return e;
  left -= kNlLaunches;
  if (left <= 0) return hipSuccess;
  e = launch_bottleneck_grad<X>(bn_blob, xin, xin_cs, d_y3, d_skip, B, h, w, d_in, grads, bn_scratch, left < kBnLaunches ? left : kBnLaunches, stream);
  left -= kBnLaunches;
  return e;
}

// The first `stop_after` of the 72 launches above (kLtLaunches: all of them; fewer are for the tests' stage-by-stage comparison): one
// running budget across the six sub-chains.  y3x<b>, out<b> [B,h,w,257 of their strides] of blocks 2, 1, 0 and x0 [B,h,w,99 of x0_cs]
// (block 2's input is out1, block 1's is out0, block 0's is x0), d_res2 dense 257 wide, d_x0 dense 99 wide.
inline hipError_t launch_lower_trunk_grad(const float* blob, const float* y3x2, int y3x2_cs, const float* out2, int out2_cs, const float* y3x1,
                                          int y3x1_cs, const float* out1, int out1_cs, const float* y3x0, int y3x0_cs, const float* out0, int out0_cs,
                                          const float* x0, int x0_cs, const float* d_res2, int B, int h, int w, float* d_x0, float* grads,
                                          void* scratch, int stop_after, hipStream_t stream) {
  const LtPlan pl = lt_plan(B, h, w);
  unsigned char* base = static_cast<unsigned char*>(scratch);
  auto f = [&](int map) { return reinterpret_cast<float*>(base + pl.map[map]); };
  const int data = kLtMaps - kLtData;
  float* g0 = grads;
  float* g1 = g0 + lt_block_floats(0);
  float* g2 = g1 + lt_block_floats(1);
  int left = stop_after;
  hipError_t e = lt_block<kLtC>(blob + lt_blob_off(0), blob + lt_blob_off(1), y3x2, y3x2_cs, out1, out1_cs, out2, out2_cs, d_res2, B, h, w, f(data),
                                f(data + 1), f(data + 2), g2, base + pl.region[0], base + pl.region[1], left, stream);
  if (e != hipSuccess || left <= 0) return e;
  e = lt_block<kLtC>(blob + lt_blob_off(2), blob + lt_blob_off(3), y3x1, y3x1_cs, out0, out0_cs, out1, out1_cs, f(data + 2), B, h, w, f(data + 3),
                     f(data + 4), f(data + 5), g1, base + pl.region[2], base + pl.region[3], left, stream);
  if (e != hipSuccess || left <= 0) return e;
  return lt_block<kLtX0>(blob + lt_blob_off(4), blob + lt_blob_off(5), y3x0, y3x0_cs, x0, x0_cs, out0, out0_cs, f(data + 5), B, h, w, f(data + 6),
                         f(data + 7), d_x0, g0, base + pl.region[4], base + pl.region[5], left, stream);
}

}  // namespace bsr
