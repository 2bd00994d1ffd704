// The generator's backward pass through a chain of residual blocks, ON THE DEVICE, training=False: a list of res_stack's blocks walked
// from the top down.  Each block is launch_nonlocal_grad<X> followed by launch_bottleneck_grad<X> at the width X of the block's input
// (nl_entry_kernel<X>, bn_entry_kernel<X>, bn_fold_kernel<X>, bn_finish_kernel<X>, and the launchers' K, tiles and strides), each
// block's d_xin is the next block's d_out, and one running launch budget covers the whole chain.  A chain is a BlockChain: the blocks
// in the order of the launches, each block's input width, and whether a launch of the caller's follows the last block.  There are two:
//
// kColourChain — between res_stack/5's input and res_stack/2's output: res_stack/4, res_stack/3 and, as its tail, the hole
// (colour_trunk_grad_kernels.h).  Both inputs are 261 wide.  48 launches and the tail's one:
//    1..12   launch_nonlocal_grad<261>, block 4     d_out = d_xin, xin = out3            -> d_y3_4, d_skip_4, block 4's ten
//   13..24   launch_bottleneck_grad<261>, block 4   xin = out3, d_y3_4, d_skip_4         -> d_xin4, block 4's twelve
//   25..36   launch_nonlocal_grad<261>, block 3     d_out = d_xin4, xin = xh             -> d_y3_3, d_skip_3, block 3's ten
//   37..48   launch_bottleneck_grad<261>, block 3   xin = xh, d_y3_3, d_skip_3           -> d_xin3, block 3's twelve
//
// kLowerChain — between res_stack/2's output and the trunk's input: res_stack/2, res_stack/1 and res_stack/0, the three blocks both
// branches share (model.py: x = cat[down3 96 | uv 3], then for i in range(n_res // 2)).  Given d_res2 = d loss / d (res_stack/2's
// output) (bsr_colour_trunk_grad's d_res2) it writes d_x0, the gradient at x0 = cat[down3's output 96 | the resized uv 3] (channels
// 96..98 belong to an input and reach nothing), and the 66 variable gradients of blocks 0, 1 and 2.  The widths are 257 for blocks 2
// and 1 (the input is the block below's output, no channels of the skip's own) and 99 for block 0, whose skip reaches the first 99 of
// the 257 output channels only and whose conv1 is 99 -> 128.  blindshadowremoval_amd/generator_grad.py is the host statement
// (lower_trunk_grad); pack.pack_lower_trunk_grad writes the blob.  72 launches, no tail:
//    1..12   launch_nonlocal_grad<257>, block 2     d_out = d_res2, xin = out1        -> d_y3_2, d_skip_2, block 2's ten
//   13..24   launch_bottleneck_grad<257>, block 2   xin = out1, d_y3_2, d_skip_2      -> d_xin2, block 2's twelve
//   25..36   launch_nonlocal_grad<257>, block 1     d_out = d_xin2, xin = out0        -> d_y3_1, d_skip_1, block 1's ten
//   37..48   launch_bottleneck_grad<257>, block 1   xin = out0, d_y3_1, d_skip_1      -> d_xin1, block 1's twelve
//   49..60   launch_nonlocal_grad<99>, block 0      d_out = d_xin1, xin = x0          -> d_y3_0, d_skip_0 (99 wide), block 0's ten
//   61..72   launch_bottleneck_grad<99>, block 0    xin = x0, d_y3_0, d_skip_0        -> d_x0 (99 wide), block 0's twelve
//
// The launches go to the caller's stream, one after the other: no host synchronisation, no second stream, no floating-point atomic;
// every word a launch reads was written by the caller or by an earlier launch of the same call, so a call repeats its bits.  Each
// sub-chain has a scratch region of its own, so that after a call the maps of every block can be read, and the intermediate data
// gradients lie behind those regions.
#pragma once
#include "bottleneck_grad_kernels.h"

namespace bsr {

constexpr int kChainMaxBlocks = 3;
constexpr int kChainBlockLaunches = kNlLaunches + kBnLaunches;
constexpr int kChainBlockVars = kBnVars + kNlVars;
constexpr int kChainBlockMaps = kNlMaps + kBnMaps;
constexpr int kChainC = 257;                                 // every block's output, and so every d_y3, is 257 wide

struct BlockChain {
  int n;                              // blocks
  int block[kChainMaxBlocks];         // res_stack's index, in the order of the launches: descending
  int width[kChainMaxBlocks];         // the block's input width X
  bool tail;                          // a launch of the caller's follows and reads the last block's d_xin
  constexpr int launches() const { return n * kChainBlockLaunches + (tail ? 1 : 0); }
  constexpr int vars() const { return n * kChainBlockVars; }
  constexpr int data() const { return 3 * n - (tail ? 0 : 1); }      // d_y3, d_skip, d_xin per block; without a tail the last d_xin is the caller's output
  constexpr int maps() const { return n * kChainBlockMaps + data(); }
};
constexpr BlockChain kColourChain{2, {4, 3}, {261, 261}, true};
constexpr BlockChain kLowerChain{3, {2, 1, 0}, {257, 257, 99}, false};
static_assert(kColourChain.launches() == 49 && kColourChain.vars() == 44 && kColourChain.maps() == 42, "two blocks and the hole");
static_assert(kLowerChain.launches() == 72 && kLowerChain.vars() == 66 && kLowerChain.maps() == 62, "three blocks, the last d_xin the caller's");

// float offsets inside the blob, the sub-blobs end to end in the order of the launches (per block the non-local blob, then the
// bottleneck blob at the block's width); part 2 n: the total.  Each part is a multiple of four floats, so every sub-blob keeps the
// 16-byte alignment of the whole.
inline size_t chain_blob_off(const BlockChain& c, int part) {
  size_t o = 0;
  for (int i = 0; i < part && i < 2 * c.n; ++i) o += i % 2 == 0 ? nl_blob_off(6) : bn_blob_off(13, c.width[i / 2]);
  return o;
}

// the floats of the 22 variable gradients of the k-th block launched
inline size_t chain_block_floats(const BlockChain& c, int k) { return bn_var_offset(kBnVars, c.width[k]) + nl_var_offset(kNlVars); }

// float offset of variable `index` inside grads, in ascending block order (the reverse of the launches'; weights.py's
// generator_colour_trunk_trainable_names and generator_lower_trunk_trainable_names): per block its twelve bottleneck variables, then its
// ten non-local ones; c.vars(): the total
inline size_t chain_var_offset(const BlockChain& c, int index) {
  size_t o = 0;
  int k = c.n - 1;
  for (; k >= 0 && index >= kChainBlockVars; --k, index -= kChainBlockVars) o += chain_block_floats(c, k);
  if (k < 0) return o;
  const int X = c.width[k];
  return index < kBnVars ? o + bn_var_offset(index, X) : o + bn_var_offset(kBnVars, X) + nl_var_offset(index - kBnVars);
}

// Byte offsets inside the scratch.  region: the sub-chains' scratches in the order of the launches.  map: per block in that order
// nl_plan's ten and bn_plan's eight at the block's width (18 k .. 18 k + 17), then behind all regions per block d_y3 [N][257], d_skip
// [N][X] and d_xin [N][X]; the last block's d_xin is a map only when a tail follows.  So kColourChain's 36..41 are d_y3_4, d_skip_4,
// d_xin4, d_y3_3, d_skip_3, d_xin3 and kLowerChain's 54..61 d_y3_2, d_skip_2, d_xin2, the same of block 1, d_y3_0, d_skip_0 [N][99].
struct ChainPlan {
  int N;
  size_t region[2 * kChainMaxBlocks], map[kChainMaxBlocks * (kChainBlockMaps + 3)], total;
};
inline ChainPlan chain_plan(const BlockChain& c, int B, int h, int w) {
  ChainPlan pl;
  BumpBytes bump;
  const NlPlan nl = nl_plan(B, h, w);
  pl.N = nl.N;
  int m = 0;
  for (int k = 0; k < c.n; ++k) {
    const BnPlan bn = bn_plan(B, h, w, c.width[k]);
    pl.region[2 * k] = bump.take(nl.total);
    for (int i = 0; i < kNlMaps; ++i) pl.map[m++] = pl.region[2 * k] + nl.map[i];
    pl.region[2 * k + 1] = bump.take(bn.total);
    for (int i = 0; i < kBnMaps; ++i) pl.map[m++] = pl.region[2 * k + 1] + bn.map[i];
  }
  const size_t N = (size_t)pl.N;
  for (int k = 0; k < c.n; ++k) {
    pl.map[m++] = bump.take(N * kChainC * sizeof(float));
    pl.map[m++] = bump.take(N * c.width[k] * sizeof(float));
    if (k < c.n - 1 || c.tail) pl.map[m++] = bump.take(N * c.width[k] * sizeof(float));
  }
  pl.total = bump.o;
  return pl;
}

// what a block reads of the forward: y3x and out [B,h,w,257 or more of their strides], xin [B,h,w,X of xin_cs]
struct ChainBlockIn {
  const float *y3x, *xin, *out;
  int y3x_cs, xin_cs, out_cs;
};

// one block's launch: its two sub-blobs and scratch regions, its gradients' first float, d_out in, d_y3 and d_skip between the
// sub-chains, d_in out
struct ChainBlockArgs {
  const float *nl_blob, *bn_blob;
  ChainBlockIn in;
  const float* d_out;
  int B, h, w;
  float *d_y3, *d_skip, *d_in, *grads;
  void *nl_scratch, *bn_scratch;
};

// one block of a chain: the non-local sub-chain, then the bottleneck's, under the running budget `left`
template <int X>
inline hipError_t chain_block(const ChainBlockArgs& a, int& left, hipStream_t stream) {
  if (left <= 0) return hipSuccess;
  hipError_t e = launch_nonlocal_grad<X>(a.nl_blob, a.in.y3x, a.in.y3x_cs, a.in.xin, a.in.xin_cs, a.in.out, a.in.out_cs, a.d_out, a.B, a.h, a.w, a.d_y3,
                                         a.d_skip, a.grads + bn_var_offset(kBnVars, X), a.nl_scratch, left < kNlLaunches ? left : kNlLaunches, stream);
  if (e != hipSuccess) return e;
  left -= kNlLaunches;
  if (left <= 0) return hipSuccess;
  e = launch_bottleneck_grad<X>(a.bn_blob, a.in.xin, a.in.xin_cs, a.d_y3, a.d_skip, a.B, a.h, a.w, a.d_in, a.grads, a.bn_scratch,
                                left < kBnLaunches ? left : kBnLaunches, stream);
  left -= kBnLaunches;
  return e;
}

// The blocks of `c` under the budget `left`, which comes back as what the blocks did not use (positive: all of them ran).  in[k]: the
// k-th block launched; d_out dense, as wide as the first block's output or, where its input is wider (261), as that; grads:
// chain_var_offset's.  *d_last: where the last block's d_xin goes, dense X wide — the caller's output, or null for the chain's own map,
// and then it comes back as that map's address for the tail.  Here, and nowhere else, a width becomes an instantiation.
inline hipError_t launch_block_chain(const BlockChain& c, const float* blob, const ChainBlockIn* in, const float* d_out, int B, int h, int w, float** d_last,
                                     float* grads, void* scratch, int& left, hipStream_t stream) {
  const ChainPlan pl = chain_plan(c, B, h, w);
  unsigned char* base = static_cast<unsigned char*>(scratch);
  auto f = [&](int map) { return reinterpret_cast<float*>(base + pl.map[map]); };
  const int data = c.n * kChainBlockMaps;
  if (*d_last == nullptr) *d_last = f(data + 3 * c.n - 1);
  size_t g_off = chain_var_offset(c, c.vars());
  for (int k = 0; k < c.n && left > 0; ++k) {
    g_off -= chain_block_floats(c, k);
    const ChainBlockArgs a{blob + chain_blob_off(c, 2 * k), blob + chain_blob_off(c, 2 * k + 1), in[k], d_out, B, h, w, f(data + 3 * k), f(data + 3 * k + 1),
                           k < c.n - 1 ? f(data + 3 * k + 2) : *d_last, grads + g_off, base + pl.region[2 * k], base + pl.region[2 * k + 1]};
    hipError_t e = hipErrorInvalidValue;
    switch (c.width[k]) {
      case 261: e = chain_block<261>(a, left, stream); break;
      case 257: e = chain_block<257>(a, left, stream); break;
      case 99: e = chain_block<99>(a, left, stream); break;
    }
    if (e != hipSuccess) return e;
    d_out = a.d_in;
  }
  return hipSuccess;
}

}  // namespace bsr
