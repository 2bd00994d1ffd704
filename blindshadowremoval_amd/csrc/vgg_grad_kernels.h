// d per_loss / d con_rgb of train_step's VGG19 perceptual term ON THE DEVICE.  blindshadowremoval_amd/perceptual.py is the host statement
// (per_loss_grad) and writes the arithmetic out; pack.pack_vgg_dgrad writes the gradient layers' weight blob (vgg_dgrad_layout).
//
// The forward chain of vgg_kernels.h, then 18 more launches on the same stream, one after the other: no host synchronisation, no parallel
// branch, no floating-point atomic; every word a launch reads was written by an earlier launch of the same call.  Only the network's
// rows [B, 2B) (con_rgb) are differentiated; the frozen network and gt are constants.
//   vgg_seed_kernel      d per / d block5_conv1's pre-activation: sign(fake - real) w_5 [fake > 0], a thread per four channels, from the
//                        kept feature.  w_k = float32(1 / (B h_k^2 C_k)); sign(0) = 0.
//   vgg_conv_kernel      x 13 with VggGradEpilogue, layer 12 down to 0: the data gradient of a 3 x 3 stride-1 SAME convolution is such a
//                        convolution with the taps turned by 180 degrees and the channel roles swapped, so the main loop is the forward
//                        kernel's on the re-packed blob, on B rows, always in chunks of 16 (C' = the forward layer's C_out >= 64).  The
//                        accumulators start at 0.  Epilogue, per accumulator element, where the forward layer's input y is a
//                        convolution's output: + the tap's seed if y is a tapped feature (block{k}_conv1, k = 1..4), then * [y > 0]
//                        (ReluGrad: nothing passes at y == 0, and the forward's -0 is 0); where it is a pooled map the value passes.
//                        y is read from the forward's kept activation with the store's own addressing, once per element after the main
//                        loop: the loop's LDS traffic is the forward's.  The last launch (block1_conv1, its 3 input channels padded to
//                        one 64-block of zeros weights) writes grad[c] = (255 g_bgr[2 - c]) upstream instead.
//   vgg_unpool_kernel    x 4: a thread per four channels of a pooled pixel reads the window's four kept inputs x, sends the gradient to
//                        the first maximum in row-major order (strict >, so -0 and 0 tie), times [x > 0] of that convolution output, and
//                        writes all four positions, zeros included: every input pixel lies in exactly one window.
//
// SCRATCH: the forward's (vgg_act_offset, unchanged) followed by two gradient buffers of B S^2 64 floats, the largest gradient map;
// backward launch j = 1..17 writes buffer (j - 1) & 1 and reads the other; launch 18 writes grad.
#pragma once
#include "vgg_kernels.h"

namespace bsr {

constexpr int kVggGradLaunches = 1 + kVggLayers + kVggPools;

// the gradient layer of forward layer i: N' = C_in (block1_conv1: one 64-block), C' = C_out
__host__ __device__ inline int vgg_dgrad_n(int i) { return i == 0 ? kVggNB : vgg_ch(i - 1); }
// float offset of gradient layer i inside pack.pack_vgg_dgrad's blob (i = 13: the total): [N' / 64][C' / 16][9][16][64], no bias
__host__ __device__ inline size_t vgg_dgrad_w_off(int i) {
  size_t o = 0;
  for (int j = 0; j < i; ++j) o += (size_t)9 * vgg_ch(j) * vgg_dgrad_n(j);
  return o;
}
__host__ __device__ inline size_t vgg_grad_buf_bytes(int B, int S) { return ((size_t)B * S * S * kVggNB * sizeof(float) + 255) & ~size_t(255); }
// byte offset of gradient buffer `which` (0, 1) inside the scratch; 2: the total
__host__ __device__ inline size_t vgg_grad_offset(int B, int S, int which) { return vgg_act_offset(B, S, kVggMaps + 1) + (size_t)which * vgg_grad_buf_bytes(B, S); }
// w_k of tap k = 0..4
inline float vgg_seed_w(int B, int S, int k) {
  const double h = (double)(S >> k);
  return (float)(1.0 / ((double)B * h * h * (double)vgg_ch(vgg_tap_layer(k))));
}

__device__ __forceinline__ float vgg_sign_seed(float fake, float real, float w) {
  const float d = fake - real;
  return d > 0.f ? w : d < 0.f ? -w : 0.f;
}

// feat [2B][h][h][C] (rows [0, B) real, [B, 2B) fake) -> g [B][h][h][C]; total4 = B h h C / 4
__global__ __launch_bounds__(256) void vgg_seed_kernel(const float* __restrict__ feat, float* __restrict__ g, size_t total4, float w) {
  const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= total4) return;
  const f32x4 real = reinterpret_cast<const f32x4*>(feat)[p], fake = reinterpret_cast<const f32x4*>(feat)[total4 + p];
  f32x4 o;
#pragma unroll
  for (int i = 0; i < 4; ++i) o[i] = fake[i] > 0.f ? vgg_sign_seed(fake[i], real[i], w) : 0.f;
  reinterpret_cast<f32x4*>(g)[p] = o;
}

struct VggGradEpilogue {
  float* out;              // [B][H][H][N]: the gradient at the forward layer's input (its pre-activation where that is a conv output)
  const float* y;          // the kept activation the forward layer read, [2B][H][H][N]; null where it is a pooled map or the image
  float seed_w;            // w_k where y is a tapped feature, else 0
  int B;
  float* grad;             // the last launch: [B][H][H][3], out and y null
  const float* upstream;   // device float[1] or null
  __device__ __forceinline__ f32x16 init(int, int) const {
    return f32x16{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  }
  __device__ __forceinline__ void finish(f32x16 (&acc)[2][2], const VggTilePos& p) const {
#pragma clang fp contract(off)
    const int H = p.H, N = p.N;
    const size_t map = (size_t)H * H * N;
    const float up = grad != nullptr && upstream != nullptr ? upstream[0] : 1.f;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int mr = (i & 3) + 8 * (i >> 2) + 4 * p.kh;
          const int oy = p.oy0 + p.wave * 4 + t * 2 + (mr >> 4), ox = p.ox0 + (mr & 15);
          if (oy >= H || ox >= H) continue;
          float v = acc[t][nt][i];
          if (grad != nullptr) {                                            // channels 0..2 of the one block are B, G, R
            if (nt == 0 && p.m < 3) grad[(((size_t)p.row * H + oy) * H + ox) * 3 + (2 - p.m)] = (255.f * v) * up;
            continue;
          }
          const size_t at = (size_t)p.row * map + ((size_t)oy * H + ox) * N + p.nb * kVggNB + nt * 32 + p.m;
          if (y != nullptr) {
            const float fake = y[(size_t)B * map + at];
            if (seed_w != 0.f) v = v + vgg_sign_seed(fake, y[at], seed_w);
            v = fake > 0.f ? v : 0.f;
          }
          out[at] = v;
        }
  }
};

// g [B][h][h][C], x [B][2h][2h][C] (the fake rows of the block's last conv output) -> out [B][2h][2h][C]; a thread per four channels of
// a pooled pixel
__global__ __launch_bounds__(256) void vgg_unpool_kernel(const float* __restrict__ g, const float* __restrict__ x, float* __restrict__ out, size_t total4,
                                                         int h, int C) {
  const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= total4) return;
  const int c4 = C / 4;
  const size_t c = p % c4, pix = p / c4;
  const size_t px = pix % h, py = (pix / h) % h, row = pix / ((size_t)h * h);
  const size_t first = ((row * 2 * h + 2 * py) * 2 * h + 2 * px) * c4 + c;
  const size_t off[4] = {first, first + c4, first + (size_t)2 * h * c4, first + (size_t)2 * h * c4 + c4};
  const f32x4 gv = reinterpret_cast<const f32x4*>(g)[p];
  f32x4 v[4], o[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = reinterpret_cast<const f32x4*>(x)[off[j]];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int win = 0;
    float best = v[0][i];
#pragma unroll
    for (int j = 1; j < 4; ++j)
      if (v[j][i] > best) { best = v[j][i]; win = j; }
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j][i] = (j == win && best > 0.f) ? gv[i] : 0.f;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) reinterpret_cast<f32x4*>(out)[off[j]] = o[j];
}

// The forward chain, then the first `stop_after` backward launches (kVggGradLaunches: all of them; fewer leave the latest gradient in
// buffer (stop_after - 1) & 1 and are for the tests' stage-by-stage comparison).
inline hipError_t launch_vgg_per_loss_grad(const float* blob, const float* dblob, const float* gt, const float* con, const float* upstream, int B, int S,
                                           double* sums, float* loss1, float* grad, void* scratch, int stop_after, hipStream_t stream) {
  hipError_t e = launch_vgg_per_loss(blob, gt, con, B, S, sums, loss1, scratch, stream);
  if (e != hipSuccess) return e;
  unsigned char* base = static_cast<unsigned char*>(scratch);
  float* buf[2] = {reinterpret_cast<float*>(base + vgg_grad_offset(B, S, 0)), reinterpret_cast<float*>(base + vgg_grad_offset(B, S, 1))};
  int done = 0;
  if (done >= stop_after) return hipSuccess;
  {
    const int h = S >> 4, C = vgg_ch(kVggLayers - 1);
    const size_t total4 = (size_t)B * h * h * (C / 4);
    hipLaunchKernelGGL(vgg_seed_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, stream, vgg_map(scratch, B, S, kVggLayers), buf[0], total4,
                       vgg_seed_w(B, S, kVggTaps - 1));
    if ((e = hipGetLastError()) != hipSuccess) return e;
    ++done;
  }
  for (int i = kVggLayers - 1; i >= 0; --i) {
    if (done >= stop_after) return hipSuccess;
    const int H = vgg_side(S, i);
    const VggConvArgs a = vgg_conv_args(buf[(done - 1) & 1], dblob + vgg_dgrad_w_off(i), H, vgg_ch(i), vgg_dgrad_n(i));
    VggGradEpilogue epi;
    epi.out = buf[done & 1];
    epi.y = nullptr;
    epi.seed_w = 0.f;
    epi.B = B;
    epi.grad = nullptr;
    epi.upstream = upstream;
    if (i == 0) {
      epi.out = nullptr;
      epi.grad = grad;
    } else if (!vgg_first_of_block(i)) {                                    // the layer read conv layer i - 1's output, map i
      epi.y = vgg_map(scratch, B, S, i);
      for (int k = 0; k < kVggTaps - 1; ++k)
        if (vgg_tap_layer(k) == i - 1) epi.seed_w = vgg_seed_w(B, S, k);
    }
    const dim3 grid((unsigned)B * (unsigned)a.tiles * (unsigned)a.nblk);
    hipLaunchKernelGGL((vgg_conv_kernel<16, VggGradEpilogue>), grid, dim3(256), 0, stream, a, epi);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    ++done;
    if (vgg_first_of_block(i)) {                                            // through pool vgg_block(i) - 1 into conv layer i - 1's output
      if (done >= stop_after) return hipSuccess;
      const int h = H, C = vgg_ch(i - 1);
      const size_t total4 = (size_t)B * h * h * (C / 4);
      const float* x = vgg_map(scratch, B, S, i) + (size_t)B * 4 * h * h * C;
      hipLaunchKernelGGL(vgg_unpool_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, stream, buf[(done - 1) & 1], x, buf[done & 1], total4, h, C);
      if ((e = hipGetLastError()) != hipSuccess) return e;
      ++done;
    }
  }
  return hipSuccess;
}

}  // namespace bsr
