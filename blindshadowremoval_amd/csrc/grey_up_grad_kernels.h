// The generator's backward pass through the GREY decoder, ON THE DEVICE, training=False: up1 (257 -> 96, H/8 -> H/4), up2 (cat[up1, x3] 160 ->
// 64, -> H/2), up3 (cat[up2, x2] 128 -> 64, -> H), each Conv2DTranspose(3, stride 2, SAME) + BN + LeakyReLU (the reference's model.py:243-245).
// Given d_y = d loss / d y at up3's output and what the forward kept — x (res_stack/2's output), c2 = [up1 | x3], c3 = [up2 | x2], y — it
// writes the twelve variable gradients, d_x and the skip gradients d_x3, d_x2.  generator_grad.grey_decoder_grad is the host statement,
// pack.pack_grey_decoder_grad writes the blob.
//
// The layers are clr_up_grad_kernels.h's, at other widths, and the nine launches are that chain's in its order: the entry mask (only when
// maps are kept), per layer from up3 down a kernel gradient and a data gradient (the slope on load where d_y and y are read), the fold, the
// finish; one line on the caller's stream, no host synchronisation, no second stream, no floating-point atomic, every sum in a fixed
// order.  What differs:
//    the layer input of up3 and up2 is the whole concatenation as the forward laid it out, so the kernels' C index is the cat order;
//    up_dgrad_kernel's SPLIT: of up3's 128 (up2's 160) data-gradient channels the first 64 (96) take the slope of up2's (up1's) output,
//    read from c3 (c2), and are the next gz; the other 64 go unmasked to d_x2 (d_x3), a dense tensor of their own.  Both counts are whole
//    16-channel tiles: the split is the unrolled store loop's tile index.  up3 is one column block of NT = 8, so d_y and y are read once
//    by its data gradient; up2 is two of NT = 5 (one block of NT = 10 needs more than 256 registers: it spills), the first all masked,
//    the second with one masked tile and four of d_x3;
//    up_wgrad_kernel at C = 128 is clr_up2's instantiation (CTW = 2, two chunks of 64); at C = 160 it is CTW = 1, five chunks of 32 real
//    channels, no column of zeros; at C = 257 it is clr_up1's (CTW = 3, three chunks of 96, channels 257..287 staged as 0 by the kernel
//    itself, scalar loads at any stride: the pad lanes of a caller's x are never read).
#pragma once
#include "clr_up_grad_kernels.h"

namespace bsr {

// index 0: up1, 1: up2, 2: up3.  The largest P per layer: 9 P = 765 workgroups are three rounds of the 256 CUs' one place (up1, scalar
// loads); 10 P = 510 and 4 P = 512 are one round of their two places (up2, up3).
constexpr UpShape kGreyUp = {{96, 64, 64}, {257, 160, 128}, {288, 160, 128}, {3, 1, 2}, {85, 51, 128}};
constexpr int kGreySplit[3] = {0, 6, 4};         // the data gradient's first 16-channel tile that belongs to the skip: 96 / 16, 64 / 16

// H, W: the image's.  x [B,H/8,W/8,257 of x_cs], c2 [B,H/4,W/4,160 of c2_cs], c3 [B,H/2,W/2,128 of c3_cs], y [B,H,W,64 of y_cs], d_y dense.
inline hipError_t launch_grey_decoder_grad(const float* blob, const float* x, int x_cs, const float* c2, int c2_cs, const float* c3, int c3_cs,
                                           const float* y, int y_cs, const float* d_y, int B, int H, int W, float* d_x, float* d_x3, float* d_x2,
                                           float* grads, bool keep, void* scratch, int stop_after, hipStream_t stream) {
  const UpShape& sh = kGreyUp;
  const UpPlan pl = up_plan(sh, B, H, W, keep);
  unsigned char* base = static_cast<unsigned char*>(scratch);
  float* gz[3];
  for (int l = 0; l < 3; ++l) gz[l] = reinterpret_cast<float*>(base + pl.map[l]);
  hipError_t e;
  int done = 0;
  if (stop_after <= done++) return hipSuccess;
  if (keep) {
    const size_t n4 = (size_t)B * H * W * 16;
    hipLaunchKernelGGL(up_mask_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, stream, d_y, y, y_cs, gz[2], n4);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  const float* in[3] = {x, c2, c3};
  const int in_cs[3] = {x_cs, c2_cs, c3_cs};
  float* skip[3] = {nullptr, d_x3, d_x2};
  for (int l = 2; l >= 0; --l) {
    const float* g = l == 2 ? d_y : gz[l];            // gz[l] is the gradient at layer l's BN output: gz[2] is formed on load
    if (stop_after <= done++) return hipSuccess;
    {
      UpWgradArgs a;
      a.x = in[l]; a.g = g; a.act = l == 2 ? y : nullptr; a.wpart = reinterpret_cast<float*>(base + pl.wpart[l]);
      a.spart = reinterpret_cast<double*>(base + pl.spart[l]);
      a.x_cs = in_cs[l]; a.act_cs = y_cs; a.h = pl.h[l]; a.w = pl.w[l]; a.C = sh.C[l]; a.O = sh.O[l];
      a.tiles_x = pl.w[l] / 16; a.tiles_per_img = a.tiles_x * (pl.h[l] / 4); a.T = pl.T[l]; a.P = pl.P[l];
      e = l == 2 ? launch_up_wgrad<2, true>(a, sh.Cp[l], stream) : l == 1 ? launch_up_wgrad<1, true>(a, sh.Cp[l], stream) : launch_up_wgrad<3, false>(a, sh.Cp[l], stream);
      if (e != hipSuccess) return e;
    }
    if (stop_after <= done++) return hipSuccess;
    {
      UpDgradArgs a;
      a.g = g; a.act = l == 2 ? y : nullptr; a.wf = blob + up_blob_off(sh, l, 1);
      a.below = l == 0 ? nullptr : in[l]; a.below_cs = in_cs[l];           // the decoder's own half comes first in c3 and c2
      a.out = l == 0 ? d_x : gz[l - 1]; a.out2 = skip[l]; a.out_cs = l == 0 ? sh.C[0] : sh.O[l - 1];
      a.act_cs = y_cs; a.h = pl.h[l]; a.w = pl.w[l]; a.C = sh.C[l]; a.Cp = sh.Cp[l]; a.O = sh.O[l];
      a.tiles_x = pl.w[l] / 32; a.tiles_per_img = a.tiles_x * (pl.h[l] / 4);
      e = l == 2 ? launch_up_dgrad<8, true, kGreySplit[2]>(a, B, stream)
          : l == 1 ? launch_up_dgrad<5, true, kGreySplit[1]>(a, B, stream) : launch_up_dgrad<6, false>(a, B, stream);
      if (e != hipSuccess) return e;
    }
  }
  if (stop_after <= done++) return hipSuccess;
  if ((e = launch_up_fold(sh, blob, pl, base, grads, stream)) != hipSuccess) return e;
  if (stop_after <= done++) return hipSuccess;
  return launch_up_finish(sh, blob, pl, base, grads, stream);
}

}  // namespace bsr
