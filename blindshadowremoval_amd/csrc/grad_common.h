// What the four gradient chains share (disc_wgrad_kernels.h, clr_tail_grad_kernels.h, clr_up_grad_kernels.h, nonlocal_grad_kernels.h):
// the wave's float64 sum, the batch-norm channel's three gradients, the scratch plans' 256-byte bump allocation and the one-time
// dynamic-LDS limit of a kernel.  The fold kernels and the plans themselves stay with their chains: their partial layouts differ.
#pragma once
#include <hip/hip_runtime.h>

#include "mfma_common.h"

namespace bsr {

// the sum of `v` over the wave's 64 lanes, in every lane: the xor butterfly 32, 16, .., 1
__device__ __forceinline__ double wave_sum(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// The gradients of channel o's bias, gamma and beta of a convolution followed by batch norm (training=False), in float64, each rounded
// once: d beta = S, d bias = inv S, d gamma = ((KW + bias S) - moving_mean S) rstd, since c = sum K x + bias.  S = sum gz, KW = sum K W
// (the kernel times its gradient before the BN factor); vecs: bias, inv, moving_mean, rstd [4][N] of the chain's blob.
__device__ __forceinline__ void bn_channel_grads(double KW, double S, const float* vecs, int N, int o, float& d_bias, float& d_gamma, float& d_beta) {
  const double bias = vecs[o], inv = vecs[N + o], mean = vecs[2 * N + o], rstd = vecs[3 * N + o];
  d_bias = (float)(inv * S);
  d_gamma = (float)(((KW + bias * S) - mean * S) * rstd);
  d_beta = (float)S;
}

// the byte offsets of a scratch plan: every part starts on a multiple of 256 bytes
struct BumpBytes {
  size_t o = 0;
  size_t take(size_t bytes) {
    const size_t at = o;
    o += (bytes + 255) & ~size_t(255);
    return at;
  }
};

// raises `kernel`'s dynamic LDS limit to `bytes`, once per device (`once` is the launcher's static)
template <typename K>
inline hipError_t dynamic_lds_once(K kernel, int bytes, PerDeviceOnce& once) {
  const int dev = PerDeviceOnce::current();
  if (dev < 0 || !once.done[dev]) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e != hipSuccess) return e;
    if (dev >= 0) once.done[dev] = true;
  }
  return hipSuccess;
}

}  // namespace bsr
