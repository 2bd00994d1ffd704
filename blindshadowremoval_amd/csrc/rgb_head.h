// The RGB baseline's output head (/root/reference/model_RGB.py:253-254): conv2 = Conv(3, 7x7, no BN, no activation) on the 128-channel
// up3 output, then conv3 = Conv(3, 7x7, no BN, no activation) on conv2's output.
//
// conv2 runs on the matrix cores as a 7x1 convolution (igemm_conv_kernel<7, 1, ..>, the approach of the GSC heads in conv_n16.h):
// taps = ky, K = the 128 input channels, N = (kx, co) = 21 of 32 columns; its output qh[pixel][kx * 3 + co] is the partial sum of
// column kx.  rgb_hsum_kernel adds the seven horizontal taps (TF SAME: zero outside the row) and the bias -> y [pixel][3].
// conv3 (3 -> 3, 441 MACs per pixel, 0.2 % of the forward) is direct fp32 arithmetic in rgb_conv7_kernel: a 16 x 16 output tile,
// its 22 x 22 input halo and the 444 weights in LDS.
#pragma once
#include <hip/hip_runtime.h>

namespace bsr {

// y[p][c] = bias[c] + sum_kx qh[row, x + kx - 3][kx * 3 + c]; one thread per (pixel, c)
__global__ void rgb_hsum_kernel(const float* __restrict__ qh, int qh_cs, const float* __restrict__ bias, int W, float* __restrict__ y,
                                size_t npix) {
  const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= npix * 3) return;
  const size_t pix = gid / 3;
  const int c = (int)(gid % 3);
  const int x = (int)(pix % W);
  float acc = bias[c];
#pragma unroll
  for (int kx = 0; kx < 7; ++kx) {
    const int xx = x + kx - 3;
    if (xx >= 0 && xx < W) acc += qh[(pix + kx - 3) * qh_cs + kx * 3 + c];
  }
  y[gid] = acc;
}

// con[b][i][j][co] = b3[co] + sum_{ky,kx,ci} y[b][i+ky-3][j+kx-3][ci] * w3[ky][kx][ci][co]  (zero outside the image).
// w: 441 HWIO weights then 3 biases.  Grid: (W / 16, H / 16, B), 256 threads.  out2 (may be null): a second copy of con.
__global__ __launch_bounds__(256) void rgb_conv7_kernel(const float* __restrict__ y, const float* __restrict__ w, int H, int W,
                                                       float* __restrict__ con, float* __restrict__ out2) {
  __shared__ float s_w[444];
  __shared__ float s_in[22 * 22 * 3];
  const int tid = threadIdx.x;
  const int b = blockIdx.z, i0 = blockIdx.y * 16, j0 = blockIdx.x * 16;
  for (int k = tid; k < 444; k += 256) s_w[k] = w[k];
  const float* yb = y + (size_t)b * H * W * 3;
  for (int k = tid; k < 22 * 22 * 3; k += 256) {
    const int c = k % 3, p = k / 3, ii = i0 - 3 + p / 22, jj = j0 - 3 + p % 22;
    s_in[k] = (ii >= 0 && ii < H && jj >= 0 && jj < W) ? yb[((size_t)ii * W + jj) * 3 + c] : 0.f;
  }
  __syncthreads();
  const int ti = tid / 16, tj = tid % 16;
  float a0 = s_w[441], a1 = s_w[442], a2 = s_w[443];
  for (int ky = 0; ky < 7; ++ky) {
#pragma unroll
    for (int kx = 0; kx < 7; ++kx) {
      const float* src = s_in + ((ti + ky) * 22 + tj + kx) * 3;
      const float* wk = s_w + (ky * 7 + kx) * 9;
#pragma unroll
      for (int ci = 0; ci < 3; ++ci) {
        const float v = src[ci];
        a0 += v * wk[ci * 3 + 0];
        a1 += v * wk[ci * 3 + 1];
        a2 += v * wk[ci * 3 + 2];
      }
    }
  }
  const size_t o = (((size_t)b * H + i0 + ti) * W + j0 + tj) * 3;
  con[o] = a0; con[o + 1] = a1; con[o + 2] = a2;
  if (out2 != nullptr) { out2[o] = a0; out2[o + 1] = a1; out2[o + 2] = a2; }
}

inline hipError_t launch_rgb_conv7(const float* y, const float* w, int B, int H, int W, float* con, float* out2, hipStream_t s) {
  if (H % 16 != 0 || W % 16 != 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(rgb_conv7_kernel, dim3((unsigned)(W / 16), (unsigned)(H / 16), (unsigned)B), dim3(256), 0, s, y, w, H, W, con, out2);
  return hipGetLastError();
}

}  // namespace bsr
