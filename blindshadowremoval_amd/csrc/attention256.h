// Non-local attention at head dimension 256: the NonLocalBlock of the RGB baseline's 513-channel bottleneck
// (/root/reference/model_RGB.py:224-225, model.py:10-13,51-53):
//   f = theta . phi^T  [HW x HW]   (NO 1/sqrt(d) scaling),  P = softmax(f, -1),  y = P . g
// on the fp32 matrix cores, flash-style with the online softmax of attention.h.  Layout of the qkv buffer: [B][HW][3*256] rows =
// tokens, channels [0,256) = theta, [256,512) = phi, [512,768) = g.  Output y: [B][HW][256].
//
// Why not attention.h with kAttD = 256: its two key streams stage 4 x (32 keys x (d+4) + 32 keys x d) floats, 264 KB at d = 256, over
// the 160 KB of LDS.  Here ONE key stream runs per workgroup: 4 waves x 32 queries = 128 queries, every 32-key tile staged once for all
// four waves, double-buffered — 2 x (32 x 260 + 32 x 256) floats = 129 KB, so one workgroup per CU, one wave per SIMD.
// Per wave and lane: theta fragment 32 x float4 (128 VGPRs), O^T accumulators 8 tiles x 16 (128), S^T 16, the next tile's staging
// registers 16 x float4 (64): ~340 of the 512 registers one wave per SIMD may use (launch_bounds(256, 1)).
// The d index of the eight O^T tiles is interleaved (tile dt, row i  <->  d = 8*i + dt): two ds_read_b128 of g[key][8i .. 8i+7] feed
// the eight matrix instructions of a key pair.
// Queries: a workgroup's last block may run past `tokens` (tokens % 128 != 0, e.g. 64): those lanes read the last token's theta and
// store nothing.  Keys: tokens % 32 == 0.
#pragma once
#include <hip/hip_runtime.h>

#include "mfma_common.h"

namespace bsr {

constexpr int kAtt2D = 256;                    // C/2 of the 513-channel NonLocalBlock
constexpr int kAtt2KT = 32;                    // keys per LDS stage
constexpr int kAtt2LdK = kAtt2D + 4;           // phi rows, padded (the S^T A-fragment reads of 32 different rows)
constexpr int kAtt2StageFloats = kAtt2KT * kAtt2LdK + kAtt2KT * kAtt2D;
constexpr int kAtt2SmemBytes = 2 * kAtt2StageFloats * 4;
constexpr float kAtt2RescaleThreshold = 8.f;   // log2 units, as attention.h
static_assert(kAtt2SmemBytes <= 160 * 1024, "LDS budget");

__global__ __launch_bounds__(256, 1) void nonlocal_attention256_kernel(const float* __restrict__ qkv, float* __restrict__ out, int tokens) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int NT = 256;
  constexpr int V4_PER_TILE = kAtt2KT * kAtt2D / 4;            // 2048 float4 per operand and tile
  constexpr int SV = V4_PER_TILE / NT;                         // 8 per thread
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = lane >> 5, r = lane & 31;
  const int qblocks = (tokens + 127) / 128;
  const int img = blockIdx.x / qblocks, qb = blockIdx.x % qblocks;
  const float* base = qkv + (size_t)img * tokens * (3 * kAtt2D);
  const int q = qb * 128 + wave * 32 + r;
  const bool q_ok = q < tokens;
  const int ql = q_ok ? q : tokens - 1;

  // theta fragment of this lane's query: element j of group g is channel 8g + 4h + j, pre-scaled by log2 e (softmax in base 2)
  f32x4 qf[kAtt2D / 8];
#pragma unroll
  for (int g = 0; g < kAtt2D / 8; ++g)
    qf[g] = *reinterpret_cast<const f32x4*>(base + (size_t)ql * (3 * kAtt2D) + g * 8 + 4 * h) * 1.4426950408889634f;

  f32x16 o[8];
#pragma unroll
  for (int dt = 0; dt < 8; ++dt)
#pragma unroll
    for (int i = 0; i < 16; ++i) o[dt][i] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;

  // staging: float4 i of a thread is key (tid >> 6) + 4 i, channels 4 (tid & 63) .. +3 of phi and of g
  typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
  const __amdgpu_buffer_rsrc_t kv_rsrc = make_rsrc(base);
  const unsigned kv_voff = (unsigned)(((tid >> 6) * (3 * kAtt2D) + (tid & 63) * 4) * 4);
  f32x4 kreg[SV], vreg[SV];
  auto fetch = [&](int t) {
#pragma unroll
    for (int i = 0; i < SV; ++i) {
      const unsigned soff = (unsigned)((t * kAtt2KT + 4 * i) * (3 * kAtt2D) * 4);
      kreg[i] = __builtin_bit_cast(f32x4, (u32x4_t)__builtin_amdgcn_raw_buffer_load_b128(kv_rsrc, kv_voff + (unsigned)(kAtt2D * 4), soff, 0));
      vreg[i] = __builtin_bit_cast(f32x4, (u32x4_t)__builtin_amdgcn_raw_buffer_load_b128(kv_rsrc, kv_voff + (unsigned)(2 * kAtt2D * 4), soff, 0));
    }
  };
  auto publish = [&](int buf) {
    float* sk = smem + buf * kAtt2StageFloats;
    float* sv = sk + kAtt2KT * kAtt2LdK;
#pragma unroll
    for (int i = 0; i < SV; ++i) {
      const int key = (tid >> 6) + 4 * i, c = (tid & 63) * 4;
      *reinterpret_cast<f32x4*>(sk + key * kAtt2LdK + c) = kreg[i];
      *reinterpret_cast<f32x4*>(sv + key * kAtt2D + c) = vreg[i];
    }
  };

  const int ntiles = tokens / kAtt2KT;
  fetch(0);
  publish(0);
  __syncthreads();
  for (int t = 0; t < ntiles; ++t) {
    const int buf = t & 1;
    if (t + 1 < ntiles) fetch(t + 1);
    const float* sk = smem + buf * kAtt2StageFloats;
    const float* sv = sk + kAtt2KT * kAtt2LdK;

    // S^T tile: rows = keys (A from LDS), cols = queries (B from registers)
    f32x16 s;
#pragma unroll
    for (int i = 0; i < 16; ++i) s[i] = 0.f;
#pragma unroll
    for (int g = 0; g < kAtt2D / 8; ++g) {
      const f32x4 kf = *reinterpret_cast<const f32x4*>(sk + r * kAtt2LdK + g * 8 + 4 * h);
#pragma unroll
      for (int j = 0; j < 4; ++j) s = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[j], qf[g][j], s, 0, 0, 0);
    }

    // online softmax of this lane's query (attention.h): 16 keys here + 16 in lane ^ 32; the running maximum is raised — and O^T, l
    // rescaled — only when a query's tile maximum exceeds it by more than the threshold
    float mx = s[0];
#pragma unroll
    for (int i = 1; i < 16; ++i) mx = fmaxf(mx, s[i]);
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    if (__any(mx > m_run + kAtt2RescaleThreshold)) {
      const float m_new = fmaxf(m_run, mx);
      const float scale = __builtin_amdgcn_exp2f(m_run - m_new);
      l_run *= scale;
      m_run = m_new;
#pragma unroll
      for (int dt = 0; dt < 8; ++dt)
#pragma unroll
        for (int i = 0; i < 16; ++i) o[dt][i] *= scale;
    }
    float psum = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      s[i] = __builtin_amdgcn_exp2f(s[i] - m_run);
      psum += s[i];
    }
    l_run += psum;

    // O^T += g^T . P^T : register i of s holds key (i&3) + 8*(i>>2) + 4h; O^T tile dt row r is d = 8r + dt
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int key = (i & 3) + 8 * (i >> 2) + 4 * h;
      const f32x4 v0 = *reinterpret_cast<const f32x4*>(sv + key * kAtt2D + 8 * r);
      const f32x4 v1 = *reinterpret_cast<const f32x4*>(sv + key * kAtt2D + 8 * r + 4);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) o[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(v0[dt], s[i], o[dt], 0, 0, 0);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) o[4 + dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(v1[dt], s[i], o[4 + dt], 0, 0, 0);
    }

    if (t + 1 < ntiles) {
      publish(buf ^ 1);      // the buffer of tile t - 1: every wave finished with it before the barrier that ended step t - 1
      __syncthreads();
    }
  }

  const float l_tot = l_run + __shfl_xor(l_run, 32);
  const float inv = 1.f / l_tot;
  if (!q_ok) return;
  float* orow = out + ((size_t)img * tokens + q) * kAtt2D;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int row = (i & 3) + 8 * (i >> 2) + 4 * h;
    const f32x4 a = {o[0][i] * inv, o[1][i] * inv, o[2][i] * inv, o[3][i] * inv};
    const f32x4 b = {o[4][i] * inv, o[5][i] * inv, o[6][i] * inv, o[7][i] * inv};
    *reinterpret_cast<f32x4*>(orow + 8 * row) = a;
    *reinterpret_cast<f32x4*>(orow + 8 * row + 4) = b;
  }
}

inline hipError_t launch_nonlocal_attention256(const float* qkv, float* out, int batch, int tokens, hipStream_t stream) {
  if (batch <= 0 || tokens <= 0 || tokens % kAtt2KT != 0) return hipErrorInvalidValue;
  auto kern = nonlocal_attention256_kernel;
  static PerDeviceOnce once;
  const int dev = PerDeviceOnce::current();
  if (dev < 0 || !once.done[dev]) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, kAtt2SmemBytes);
    if (e != hipSuccess) return e;
    if (dev >= 0) once.done[dev] = true;
  }
  hipLaunchKernelGGL(kern, dim3((unsigned)(batch * ((tokens + 127) / 128))), dim3(256), kAtt2SmemBytes, stream, qkv, out, tokens);
  return hipGetLastError();
}

}  // namespace bsr
