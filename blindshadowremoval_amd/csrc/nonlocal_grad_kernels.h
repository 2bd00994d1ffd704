// The generator's backward pass below the colour decoder, ON THE DEVICE, training=False: the upper half of res_stack/5 — relu3, the
// block's zero-padded skip and the NonLocalBlock (theta, phi, g: 1x1 257 -> 128; softmax(theta phi^T) g; w: 1x1 128 -> 257; BN;
// z = y3 + w_y).  Given d_out = d loss / d (the block's output) and the forward's kept y3x = y3 + pad(xin), xin and out it writes d_y3 (at
// bnorm3's output), d_skip (what the skip carries to the block's input) and the ten variable gradients of the non-local block.
// blindshadowremoval_amd/generator_grad.py is the host statement (nonlocal_grad); pack.pack_nonlocal_grad writes the blob.
//
// N = B T rows (T = h w tokens per image, a multiple of 128).  Twelve launches on the caller's stream, one after the other: no host
// synchronisation, no second stream, no floating-point atomic; every word a launch reads was written by the caller or by an earlier
// launch of the same call, and every sum runs in a fixed order, so a call repeats its bits.  All matrix work is v_mfma_f32_16x16x4_f32.
//    1  nl_entry_kernel<X>   gz = LeakyReluGrad(d_out, out) where d_out is loaded -> d_skip (all X = 261 channels) and dz (the first 257, row
//                            stride 272, the pad 0); y3 = y3x - pad(xin) -> X (stride 272, pad 0); per 64 rows the column sums of dz in
//                            float64 in row order.
//    2  nl_gemm_kernel<0>    proj = [theta | phi | g] = X Wqkv + b            (K = 272, N = 384): the forward composes them away
//    3  nl_att_stats_kernel  per 64 queries, walking the image's keys twice: the row log-sum-exp L (running maximum), then
//                            A = exp(S - L) g.  L is kept as its two parts (m, r): the row maximum and r = 1 / sum exp(S - m), and a
//                            weight is exp(S - m) r everywhere: a float32 L of magnitude 250 would carry 2^-17 of relative error into
//                            every weight of its row, which the rows' sums sum dS = 0 (d phi/bias) do not forgive.  theta stays in
//                            registers; S is formed TRANSPOSED (keys x queries), so the lane that holds P[query r][keys 4q..4q+3]
//                            feeds them to the P g product as its A operand with no shuffle: k-slot q of step j stands for key
//                            4q + j, on both operands.
//    4  nl_gemm_kernel<1>    dA = dz (inv Ww)^T (K = 272, N = 128) and D = rowsum(dA o A) in the epilogue
//    5  nl_att_bwd_key_kernel   KEY-stationary: 64 keys (phi, g in registers), walking the image's queries (theta, dA, L, D through
//                            LDS): S, dP = dA g^T, P = exp(S - m) r, dS = P o (dP - D);  d_g += P^T dA,  d_phi += dS^T theta
//    6  nl_att_bwd_query_kernel QUERY-stationary: 64 queries (theta, dA in registers), walking the keys (phi, g through LDS), S and dP
//                            transposed as in launch 3;  d_theta += dS phi.     Neither writes a T x T matrix anywhere.
//    7  nl_tn_kernel         X^T [d_theta | d_phi | d_g]  (257 x 384): float32 partials per slice of rows
//    8  nl_tn_kernel         A^T dz                       (128 x 257): likewise
//    9  nl_colsum_kernel     per 128 rows the column sums of [d_theta | d_phi | d_g] in float64 in row order
//   10  nl_gemm_kernel<2>    d_y3 = dz + [d_theta | d_phi | d_g] Wqkv^T (K = 384, N = 257)
//   11  nl_fold_kernel       a thread per kernel element: the partials in index order in float64 -> d Wg, d Wp, d Wt; Wgd (float64) and
//                            d Ww = inv[n] Wgd rounded once
//   12  nl_finish_kernel     a wave per channel: Sz, KW = sum_k Ww Wgd -> d beta = Sz, d bw = inv Sz, d gamma = ((KW + bw Sz) - mean Sz) rstd;
//                            a wave per projection column: its bias gradient
#pragma once
#include "clr_up_grad_kernels.h"

namespace bsr {

constexpr int kNlLaunches = 12;
constexpr int kNlVars = 10;
constexpr int kNlC = 257, kNlCp = 272, kNlD = 128, kNlQ = 384, kNlX = 261;
constexpr int kNlLd = 132;                 // floats per row of a 128-wide LDS tile
constexpr int kNlMaps = 10;
constexpr int kNlTnMp = 320;               // launch 7's partial rows (5 tiles of 64)

// float offsets inside the blob; part 6: the total
__host__ __device__ inline size_t nl_blob_off(int part) {
  // 0: wqkv [272][384]   1: bqkv [384]   2: wwf [272][128] = inv[n] Ww[k][n]   3: wqkvT [384][384]   4: ww [128][257]   5: vecs [4][257]
  const size_t n[6] = {(size_t)kNlCp * kNlQ, (size_t)kNlQ, (size_t)kNlCp * kNlD, (size_t)kNlQ * kNlQ, (size_t)kNlD * kNlC, (size_t)4 * kNlC};
  size_t o = 0;
  for (int i = 0; i < part && i < 6; ++i) o += n[i];
  return o;
}

// float offset of variable `index` (g, phi, theta: kernel, bias; w: kernel, bias; bnorm: gamma, beta) inside grads; 10: the total
__host__ __device__ inline size_t nl_var_offset(int index) {
  const size_t n[kNlVars] = {(size_t)kNlC * kNlD, kNlD, (size_t)kNlC * kNlD, kNlD, (size_t)kNlC * kNlD, kNlD, (size_t)kNlD * kNlC, kNlC, kNlC, kNlC};
  size_t o = 0;
  for (int v = 0; v < index && v < kNlVars; ++v) o += n[v];
  return o;
}

inline bool nl_size_ok(int B, int h, int w) {
  return B > 0 && h > 0 && w > 0 && h % 4 == 0 && w % 32 == 0 && (long long)B * h * w <= (1ll << 21);
}

// Byte offsets inside the scratch.  map 0: X = y3 [N][272], 1: dz [N][272], 2: proj [N][384], 3: A [N][128], 4: L = (m, r) [N][2], 5: dA [N][128],
// 6: D [N], 7: [d_theta | d_phi | d_g] [N][384], 8: Wgd [128][257] float64, 9: Sz [257] float64.
struct NlPlan {
  int N, T, P;
  size_t map[kNlMaps], szpart, bpart, part1, part2, total;
};
inline NlPlan nl_plan(int B, int h, int w) {
  NlPlan pl;
  BumpBytes bump;
  pl.T = h * w;
  pl.N = B * pl.T;
  const int chunks = pl.N / 128;
  pl.P = chunks < 64 ? chunks : 64;
  const size_t N = (size_t)pl.N;
  pl.map[0] = bump.take(N * kNlCp * sizeof(float));
  pl.map[1] = bump.take(N * kNlCp * sizeof(float));
  pl.map[2] = bump.take(N * kNlQ * sizeof(float));
  pl.map[3] = bump.take(N * kNlD * sizeof(float));
  pl.map[4] = bump.take(N * 2 * sizeof(float));
  pl.map[5] = bump.take(N * kNlD * sizeof(float));
  pl.map[6] = bump.take(N * sizeof(float));
  pl.map[7] = bump.take(N * kNlQ * sizeof(float));
  pl.map[8] = bump.take((size_t)kNlD * kNlC * sizeof(double));
  pl.map[9] = bump.take((size_t)kNlC * sizeof(double));
  pl.szpart = bump.take((N / 64) * kNlCp * sizeof(double));
  pl.bpart = bump.take((N / 128) * kNlQ * sizeof(double));
  pl.part1 = bump.take((size_t)pl.P * kNlTnMp * kNlQ * sizeof(float));
  pl.part2 = bump.take((size_t)pl.P * kNlD * kNlQ * sizeof(float));
  pl.total = bump.o;
  return pl;
}

// ---- launch 1
struct NlEntryArgs {
  const float *y3x, *xin, *out, *d_out;
  float *d_skip, *X, *dz;
  double* szpart;      // [N / 64][272]
  int y3x_cs, xin_cs, out_cs;
};

// grid (N / 64).  X: the width of the block's input and so of the skip — 261 (blocks 3..5), 257 (blocks 1, 2: nothing beyond the block's own
// channels) or 99 (block 0: the skip reaches the first 99 channels only, out = lrelu(z + pad_257(xin))).  d_out and out are read
// max(X, 257) wide, xin for c < X alone, d_skip is written X wide.
template <int X>
__global__ __launch_bounds__(256) void nl_entry_kernel(const NlEntryArgs a) {
  constexpr int G = X > kNlC ? X : kNlC;    // d_out's dense width
  const int tid = threadIdx.x;
  const size_t row0 = (size_t)blockIdx.x * 64;
  for (int c = tid; c < kNlCp; c += 256) {
    double s = 0.0;
    for (int i = 0; i < 64; ++i) {
      const size_t row = row0 + i;
      float g = 0.f, x = 0.f;
      if (c < kNlC) {
        g = clr_leaky_grad(a.d_out[row * G + c], a.out[row * a.out_cs + c]);
        x = a.y3x[row * a.y3x_cs + c];
        if (X >= kNlC || c < X) {
          x -= a.xin[row * a.xin_cs + c];
          a.d_skip[row * X + c] = g;
        }
      }
      a.dz[row * kNlCp + c] = g;
      a.X[row * kNlCp + c] = x;
      s += (double)g;
    }
    a.szpart[(size_t)blockIdx.x * kNlCp + c] = s;
  }
  if constexpr (X > kNlC) {
    constexpr int E = X - kNlC;             // the skip's own channels 257..260
    for (int i = tid; i < 64 * E; i += 256) {
      const size_t row = row0 + i / E;
      const int c = kNlC + i % E;
      a.d_skip[row * X + c] = clr_leaky_grad(a.d_out[row * X + c], a.out[row * a.out_cs + c]);
    }
  }
}

// ---- launches 2, 4, 10: out [N][.] = a [N][K] w [K][.]
struct NlGemmArgs {
  const float* a;       // [N][a_cs], K a multiple of 16, pad columns 0
  const float* w;       // [K][w_cs], w_cs a multiple of 128
  const float* bias;    // MODE 0
  const float* mul;     // MODE 1: [N][128], D = rowsum(out o mul)
  const float* res;     // MODE 2: [N][res_cs]
  float* out;           // [N][out_cs], columns < n_store
  float* D;             // MODE 1
  int a_cs, K, w_cs, res_cs, out_cs, n_store;
};

// grid (N / 64, column tiles of 128)
template <int MODE>
__global__ __launch_bounds__(256) void nl_gemm_kernel(const NlGemmArgs a) {
  constexpr int LDA = 18, LDW = 144;
  __shared__ __attribute__((aligned(16))) float s_a[64 * LDA];
  __shared__ __attribute__((aligned(16))) float s_w[16 * LDW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, q = lane >> 4;
  const size_t row0 = (size_t)blockIdx.x * 64;
  const int c0 = (int)blockIdx.y * 128;
  f32x4 acc[8];
#pragma unroll
  for (int n = 0; n < 8; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < a.K; k0 += 16) {
    const f32x4 av4 = *reinterpret_cast<const f32x4*>(a.a + (row0 + (tid >> 2)) * a.a_cs + k0 + (tid & 3) * 4);
    f32x4 wv4[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int i = tid + j * 256;
      wv4[j] = *reinterpret_cast<const f32x4*>(a.w + (size_t)(k0 + (i >> 5)) * a.w_cs + c0 + (i & 31) * 4);
    }
    __syncthreads();                                                       // every wave is done with the previous chunk
    {
      float* d = s_a + (tid >> 2) * LDA + (tid & 3) * 4;
      *reinterpret_cast<f32x2*>(d) = f32x2{av4[0], av4[1]};
      *reinterpret_cast<f32x2*>(d + 2) = f32x2{av4[2], av4[3]};
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int i = tid + j * 256;
      *reinterpret_cast<f32x4*>(s_w + (i >> 5) * LDW + (i & 31) * 4) = wv4[j];
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const float av = s_a[(wave * 16 + r) * LDA + kk * 4 + q];
      const float* wp = s_w + (kk * 4 + q) * LDW + r;
#pragma unroll
      for (int n = 0; n < 8; ++n) acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, wp[n * 16], acc[n], 0, 0, 0);
    }
  }
  float d[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int n = 0; n < 8; ++n) {
    const int col = c0 + n * 16 + r;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const size_t row = row0 + wave * 16 + 4 * q + e;
      float v = acc[n][e];
      if constexpr (MODE == 0) v += a.bias[col];
      if constexpr (MODE == 1) d[e] += v * a.mul[row * kNlD + col];
      if constexpr (MODE == 2) {
        if (col < a.n_store) v += a.res[row * a.res_cs + col];
      }
      if (col < a.n_store) a.out[row * a.out_cs + col] = v;
    }
  }
  if constexpr (MODE == 1) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float v = d[e];
      for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o);
      if (r == 0) a.D[row0 + wave * 16 + 4 * q + e] = v;
    }
  }
}

// ---- the attention kernels
struct NlAttArgs {
  const float* proj;    // [N][384] = theta | phi | g
  const float* dA;      // [N][128]
  float* A;             // [N][128]
  float* L;             // [N][2]: the row maximum m and r = 1 / sum exp(S - m)
  const float* D;       // [N]
  float* dproj;         // [N][384] = d_theta | d_phi | d_g
  int T;
};

constexpr int kNlAttSmemFloats = 2 * 64 * kNlLd + 192;

// 64 rows x 128 floats from src (row stride cs) into an LDS tile
__device__ __forceinline__ void nl_stage_tile(float* dst, const float* src, int cs, int tid) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int i = tid + j * 256;
    *reinterpret_cast<f32x4*>(dst + (i >> 5) * kNlLd + (i & 31) * 4) = *reinterpret_cast<const f32x4*>(src + (size_t)(i >> 5) * cs + (i & 31) * 4);
  }
}

// acc[e] = sum_k tile[16 sub + r][k] reg[k] over the wave's 16 stationary rows: element (tile row 4q + e, stationary row r)
__device__ __forceinline__ f32x4 nl_tile_dot_t(const float* tile, int sub, int r, int q, const float (&reg)[32]) {
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  const float* p = tile + (sub * 16 + r) * kNlLd + q;
#pragma unroll
  for (int ks = 0; ks < 32; ++ks) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(p[4 * ks], reg[ks], acc, 0, 0, 0);
  return acc;
}

// acc[n] += sum_j p[j] tile[16 sub + 4q + j][16 n + r]
__device__ __forceinline__ void nl_tile_acc(f32x4 (&acc)[8], const f32x4 p, const float* tile, int sub, int r, int q) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float* b = tile + (sub * 16 + 4 * q + j) * kNlLd + r;
#pragma unroll
    for (int n = 0; n < 8; ++n) acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(p[j], b[n * 16], acc[n], 0, 0, 0);
  }
}

// grid (N / 64)
__global__ __launch_bounds__(256) void nl_att_stats_kernel(const NlAttArgs a) {
  extern __shared__ __attribute__((aligned(16))) float nsm[];
  float* s_k = nsm;
  float* s_v = nsm + 64 * kNlLd;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, q = lane >> 4;
  const size_t row0 = (size_t)blockIdx.x * 64;
  const size_t img0 = (row0 / a.T) * a.T;
  float th[32];
  {
    const float* src = a.proj + (row0 + wave * 16 + r) * kNlQ + q;
#pragma unroll
    for (int ks = 0; ks < 32; ++ks) th[ks] = src[4 * ks];
  }
  float m = -INFINITY, l = 0.f;
  for (int kt = 0; kt < a.T; kt += 64) {
    __syncthreads();
    nl_stage_tile(s_k, a.proj + (img0 + kt) * kNlQ + kNlD, kNlQ, tid);
    __syncthreads();
#pragma unroll 1
    for (int sub = 0; sub < 4; ++sub) {
      const f32x4 s = nl_tile_dot_t(s_k, sub, r, q, th);
      const float mx = fmaxf(fmaxf(s[0], s[1]), fmaxf(s[2], s[3]));
      if (mx > m) {
        l *= expf(m - mx);
        m = mx;
      }
      l += (expf(s[0] - m) + expf(s[1] - m)) + (expf(s[2] - m) + expf(s[3] - m));
    }
  }
  for (int o = 16; o < 64; o <<= 1) {
    const float m2 = __shfl_xor(m, o), l2 = __shfl_xor(l, o);
    const float M = fmaxf(m, m2);
    const float x = l * expf(m - M), y = l2 * expf(m2 - M);
    l = (lane & o) ? y + x : x + y;                  // the pair's lower lane's term first on both
    m = M;
  }
  const float rinv = 1.f / l;
  if (q == 0) *reinterpret_cast<f32x2*>(a.L + 2 * (row0 + wave * 16 + r)) = f32x2{m, rinv};
  f32x4 acc[8];
#pragma unroll
  for (int n = 0; n < 8; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int kt = 0; kt < a.T; kt += 64) {
    __syncthreads();
    nl_stage_tile(s_k, a.proj + (img0 + kt) * kNlQ + kNlD, kNlQ, tid);
    nl_stage_tile(s_v, a.proj + (img0 + kt) * kNlQ + 2 * kNlD, kNlQ, tid);
    __syncthreads();
#pragma unroll 1
    for (int sub = 0; sub < 4; ++sub) {
      f32x4 p = nl_tile_dot_t(s_k, sub, r, q, th);
#pragma unroll
      for (int e = 0; e < 4; ++e) p[e] = expf(p[e] - m) * rinv;
      nl_tile_acc(acc, p, s_v, sub, r, q);
    }
  }
#pragma unroll
  for (int n = 0; n < 8; ++n)
#pragma unroll
    for (int e = 0; e < 4; ++e) a.A[(row0 + wave * 16 + 4 * q + e) * kNlD + n * 16 + r] = acc[n][e];
}

// grid (N / 64): the block's 64 QUERIES are stationary
__global__ __launch_bounds__(256) void nl_att_bwd_query_kernel(const NlAttArgs a) {
  extern __shared__ __attribute__((aligned(16))) float nsm[];
  float* s_k = nsm;
  float* s_v = nsm + 64 * kNlLd;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, q = lane >> 4;
  const size_t row0 = (size_t)blockIdx.x * 64;
  const size_t img0 = (row0 / a.T) * a.T;
  const size_t mine = row0 + wave * 16 + r;
  float th[32], da[32];
#pragma unroll
  for (int ks = 0; ks < 32; ++ks) {
    th[ks] = a.proj[mine * kNlQ + 4 * ks + q];
    da[ks] = a.dA[mine * kNlD + 4 * ks + q];
  }
  const float mq = a.L[2 * mine], rq = a.L[2 * mine + 1], dd = a.D[mine];
  f32x4 acc[8];
#pragma unroll
  for (int n = 0; n < 8; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int kt = 0; kt < a.T; kt += 64) {
    __syncthreads();
    nl_stage_tile(s_k, a.proj + (img0 + kt) * kNlQ + kNlD, kNlQ, tid);
    nl_stage_tile(s_v, a.proj + (img0 + kt) * kNlQ + 2 * kNlD, kNlQ, tid);
    __syncthreads();
#pragma unroll 1
    for (int sub = 0; sub < 4; ++sub) {
      const f32x4 s = nl_tile_dot_t(s_k, sub, r, q, th);
      const f32x4 dp = nl_tile_dot_t(s_v, sub, r, q, da);
      f32x4 ds;
#pragma unroll
      for (int e = 0; e < 4; ++e) ds[e] = expf(s[e] - mq) * rq * (dp[e] - dd);
      nl_tile_acc(acc, ds, s_k, sub, r, q);
    }
  }
#pragma unroll
  for (int n = 0; n < 8; ++n)
#pragma unroll
    for (int e = 0; e < 4; ++e) a.dproj[(row0 + wave * 16 + 4 * q + e) * kNlQ + n * 16 + r] = acc[n][e];
}

// grid (N / 64): the block's 64 KEYS are stationary
__global__ __launch_bounds__(256) void nl_att_bwd_key_kernel(const NlAttArgs a) {
  extern __shared__ __attribute__((aligned(16))) float nsm[];
  float* s_q = nsm;
  float* s_d = nsm + 64 * kNlLd;
  float* s_L = nsm + 2 * 64 * kNlLd;
  float* s_D = s_L + 128;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, q = lane >> 4;
  const size_t row0 = (size_t)blockIdx.x * 64;
  const size_t img0 = (row0 / a.T) * a.T;
  const size_t mine = row0 + wave * 16 + r;
  float ph[32], gg[32];
#pragma unroll
  for (int ks = 0; ks < 32; ++ks) {
    ph[ks] = a.proj[mine * kNlQ + kNlD + 4 * ks + q];
    gg[ks] = a.proj[mine * kNlQ + 2 * kNlD + 4 * ks + q];
  }
  f32x4 dph[8], dg[8];
#pragma unroll
  for (int n = 0; n < 8; ++n) dph[n] = dg[n] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int qt = 0; qt < a.T; qt += 64) {
    __syncthreads();
    nl_stage_tile(s_q, a.proj + (img0 + qt) * kNlQ, kNlQ, tid);
    nl_stage_tile(s_d, a.dA + (img0 + qt) * kNlD, kNlD, tid);
    if (tid < 128) s_L[tid] = a.L[2 * (img0 + qt) + tid];
    else if (tid < 192) s_D[tid - 128] = a.D[img0 + qt + tid - 128];
    __syncthreads();
#pragma unroll 1
    for (int sub = 0; sub < 4; ++sub) {
      // here the TILE rows are queries: element (query 4q + e, key r)
      const f32x4 s = nl_tile_dot_t(s_q, sub, r, q, ph);
      const f32x4 dp = nl_tile_dot_t(s_d, sub, r, q, gg);
      f32x4 p, ds;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const f32x2 mr = *reinterpret_cast<const f32x2*>(s_L + 2 * (sub * 16 + 4 * q + e));
        p[e] = expf(s[e] - mr[0]) * mr[1];
        ds[e] = p[e] * (dp[e] - s_D[sub * 16 + 4 * q + e]);
      }
      nl_tile_acc(dg, p, s_d, sub, r, q);
      nl_tile_acc(dph, ds, s_q, sub, r, q);
    }
  }
#pragma unroll
  for (int n = 0; n < 8; ++n)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float* dst = a.dproj + (row0 + wave * 16 + 4 * q + e) * kNlQ + n * 16 + r;
      dst[kNlD] = dph[n][e];
      dst[2 * kNlD] = dg[n][e];
    }
}

// ---- launches 7, 8: part[p][m][n] = sum over the slice's rows of l[row][m] r[row][n]
struct NlTnArgs {
  const float* l;       // [N][l_cs], columns < M
  const float* r;       // [N][r_cs], columns < Nn
  float* part;          // [P][Mp][384]
  int l_cs, M, r_cs, Nn, Mp, chunks, P;
};

// grid (P, row tiles of 64, column tiles of 128): slice p takes the 128-row chunks p, p + P, ...
__global__ __launch_bounds__(256) void nl_tn_kernel(const NlTnArgs a) {
  constexpr int LDL = 80, LDR = 144;
  __shared__ __attribute__((aligned(16))) float s_l[16 * LDL];
  __shared__ __attribute__((aligned(16))) float s_r[16 * LDR];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int p = (int)blockIdx.x, m0 = (int)blockIdx.y * 64, n0 = (int)blockIdx.z * 128;
  f32x4 acc[8];
#pragma unroll
  for (int n = 0; n < 8; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int ch = p; ch < a.chunks; ch += a.P) {
    for (int st = 0; st < 8; ++st) {
      const size_t row0 = (size_t)ch * 128 + st * 16;
      f32x4 lv = {0.f, 0.f, 0.f, 0.f}, rv[2];
      {
        const int m = m0 + (tid & 15) * 4;
        if (m < a.M) lv = *reinterpret_cast<const f32x4*>(a.l + (row0 + (tid >> 4)) * a.l_cs + m);
      }
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int i = tid + j * 256;
        const int n = n0 + (i & 31) * 4;
        rv[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (n < a.Nn) rv[j] = *reinterpret_cast<const f32x4*>(a.r + (row0 + (i >> 5)) * a.r_cs + n);
      }
      __syncthreads();
      *reinterpret_cast<f32x4*>(s_l + (tid >> 4) * LDL + (tid & 15) * 4) = lv;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int i = tid + j * 256;
        *reinterpret_cast<f32x4*>(s_r + (i >> 5) * LDR + (i & 31) * 4) = rv[j];
      }
      __syncthreads();
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        const float av = s_l[(kk * 4 + q) * LDL + wave * 16 + r];
        const float* bp = s_r + (kk * 4 + q) * LDR + r;
#pragma unroll
        for (int n = 0; n < 8; ++n) acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bp[n * 16], acc[n], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int n = 0; n < 8; ++n)
#pragma unroll
    for (int e = 0; e < 4; ++e) a.part[((size_t)p * a.Mp + m0 + wave * 16 + 4 * q + e) * kNlQ + n0 + n * 16 + r] = acc[n][e];
}

// ---- launch 9: grid (N / 128), 384 threads
__global__ __launch_bounds__(384) void nl_colsum_kernel(const float* dproj, double* bpart) {
  const float* src = dproj + (size_t)blockIdx.x * 128 * kNlQ + threadIdx.x;
  double s = 0.0;
#pragma unroll 8
  for (int i = 0; i < 128; ++i) s += (double)src[(size_t)i * kNlQ];
  bpart[(size_t)blockIdx.x * kNlQ + threadIdx.x] = s;
}

// ---- launch 11
struct NlFoldArgs {
  const float *part1, *part2, *inv;
  double* Wgd;
  float* grads;
  int P;
};
constexpr int kNlFoldElems = 3 * kNlC * kNlD + kNlD * kNlC;

__global__ __launch_bounds__(256) void nl_fold_kernel(const NlFoldArgs a) {
  const int e = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (e >= kNlFoldElems) return;
  constexpr int per = kNlC * kNlD;
  double s = 0.0;
  if (e < 3 * per) {
    const int v = e / per, c = (e % per) / kNlD, j = e % kNlD;       // v: g, phi, theta, the variables' order; the rows hold theta | phi | g
    const float* src = a.part1 + (size_t)c * kNlQ + (2 - v) * kNlD + j;
#pragma unroll 8
    for (int p = 0; p < a.P; ++p) s += (double)src[(size_t)p * kNlTnMp * kNlQ];
    a.grads[nl_var_offset(2 * v) + (size_t)c * kNlD + j] = (float)s;
  } else {
    const int i = e - 3 * per, k = i / kNlC, n = i % kNlC;
    const float* src = a.part2 + (size_t)k * kNlQ + n;
#pragma unroll 8
    for (int p = 0; p < a.P; ++p) s += (double)src[(size_t)p * kNlD * kNlQ];
    a.Wgd[i] = s;
    a.grads[nl_var_offset(6) + i] = (float)((double)a.inv[n] * s);
  }
}

// ---- launch 12: grid (257 + 384), one wave each
struct NlFinishArgs {
  const double *szpart, *bpart, *Wgd;
  const float *ww, *vecs;
  double* Sz;
  float* grads;
  int nsz, nb;
};

__global__ __launch_bounds__(64) void nl_finish_kernel(const NlFinishArgs a) {
  const int lane = threadIdx.x, b = (int)blockIdx.x;
  if (b < kNlC) {
    double sz = 0.0, kw = 0.0;
    for (int i = lane; i < a.nsz; i += 64) sz += a.szpart[(size_t)i * kNlCp + b];
    for (int k = lane; k < kNlD; k += 64) kw += (double)a.ww[k * kNlC + b] * a.Wgd[k * kNlC + b];
    sz = wave_sum(sz);
    kw = wave_sum(kw);
    if (lane == 0) {
      a.Sz[b] = sz;
      bn_channel_grads(kw, sz, a.vecs, kNlC, b, a.grads[nl_var_offset(7) + b], a.grads[nl_var_offset(8) + b], a.grads[nl_var_offset(9) + b]);
    }
  } else {
    const int col = b - kNlC, slot = col / kNlD, j = col % kNlD;     // slot: theta, phi, g
    double s = 0.0;
    for (int i = lane; i < a.nb; i += 64) s += a.bpart[(size_t)i * kNlQ + col];
    s = wave_sum(s);
    if (lane == 0) a.grads[nl_var_offset(2 * (2 - slot) + 1) + j] = (float)s;
  }
}

template <typename K>
inline hipError_t launch_nl_att(K kernel, PerDeviceOnce& once, const NlAttArgs& a, int N, hipStream_t stream) {
  constexpr int bytes = kNlAttSmemFloats * (int)sizeof(float);
  const hipError_t e = dynamic_lds_once(kernel, bytes, once);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kernel, dim3(N / 64), dim3(256), bytes, stream, a);
  return hipGetLastError();
}

// The first `stop_after` of the twelve launches above (kNlLaunches: all of them; fewer are for the tests' stage-by-stage comparison).
// h, w: the 1/8-resolution grid's, so every tensor is [B,h,w,.]: d_out dense max(X, 257) wide, d_skip dense X wide, d_y3 dense 257 wide.
// X: the width of the block's input (nl_entry_kernel); nothing else of the chain, its blob or its scratch carries it.
template <int X = kNlX>
inline hipError_t launch_nonlocal_grad(const float* blob, const float* y3x, int y3x_cs, const float* xin, int xin_cs, const float* out, int out_cs,
                                       const float* d_out, int B, int h, int w, float* d_y3, float* d_skip, float* grads, void* scratch, int stop_after,
                                       hipStream_t stream) {
  const NlPlan pl = nl_plan(B, h, w);
  unsigned char* base = static_cast<unsigned char*>(scratch);
  auto f = [&](size_t off) { return reinterpret_cast<float*>(base + off); };
  auto d = [&](size_t off) { return reinterpret_cast<double*>(base + off); };
  float *y3 = f(pl.map[0]), *dz = f(pl.map[1]), *proj = f(pl.map[2]), *A = f(pl.map[3]), *L = f(pl.map[4]), *dA = f(pl.map[5]), *D = f(pl.map[6]);
  float *dproj = f(pl.map[7]), *part1 = f(pl.part1), *part2 = f(pl.part2);
  double *Wgd = d(pl.map[8]), *Sz = d(pl.map[9]), *szpart = d(pl.szpart), *bpart = d(pl.bpart);
  const int N = pl.N;
  hipError_t e;
  int done = 0;
  if (stop_after <= done++) return hipSuccess;
  {
    NlEntryArgs a{y3x, xin, out, d_out, d_skip, y3, dz, szpart, y3x_cs, xin_cs, out_cs};
    hipLaunchKernelGGL(nl_entry_kernel<X>, dim3(N / 64), dim3(256), 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (stop_after <= done++) return hipSuccess;
  {
    NlGemmArgs a{};
    a.a = y3; a.a_cs = kNlCp; a.K = kNlCp; a.w = blob + nl_blob_off(0); a.w_cs = kNlQ; a.bias = blob + nl_blob_off(1);
    a.out = proj; a.out_cs = kNlQ; a.n_store = kNlQ;
    hipLaunchKernelGGL(nl_gemm_kernel<0>, dim3(N / 64, 3), dim3(256), 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  NlAttArgs at{proj, dA, A, L, D, dproj, pl.T};
  if (stop_after <= done++) return hipSuccess;
  {
    static PerDeviceOnce once;
    if ((e = launch_nl_att(nl_att_stats_kernel, once, at, N, stream)) != hipSuccess) return e;
  }
  if (stop_after <= done++) return hipSuccess;
  {
    NlGemmArgs a{};
    a.a = dz; a.a_cs = kNlCp; a.K = kNlCp; a.w = blob + nl_blob_off(2); a.w_cs = kNlD; a.mul = A;
    a.out = dA; a.out_cs = kNlD; a.n_store = kNlD; a.D = D;
    hipLaunchKernelGGL(nl_gemm_kernel<1>, dim3(N / 64, 1), dim3(256), 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (stop_after <= done++) return hipSuccess;
  {
    static PerDeviceOnce once;
    if ((e = launch_nl_att(nl_att_bwd_key_kernel, once, at, N, stream)) != hipSuccess) return e;
  }
  if (stop_after <= done++) return hipSuccess;
  {
    static PerDeviceOnce once;
    if ((e = launch_nl_att(nl_att_bwd_query_kernel, once, at, N, stream)) != hipSuccess) return e;
  }
  if (stop_after <= done++) return hipSuccess;
  {
    NlTnArgs a{y3, dproj, part1, kNlCp, kNlCp, kNlQ, kNlQ, kNlTnMp, N / 128, pl.P};
    hipLaunchKernelGGL(nl_tn_kernel, dim3(pl.P, kNlTnMp / 64, 3), dim3(256), 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (stop_after <= done++) return hipSuccess;
  {
    NlTnArgs a{A, dz, part2, kNlD, kNlD, kNlCp, kNlCp, kNlD, N / 128, pl.P};
    hipLaunchKernelGGL(nl_tn_kernel, dim3(pl.P, 2, 3), dim3(256), 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (stop_after <= done++) return hipSuccess;
  hipLaunchKernelGGL(nl_colsum_kernel, dim3(N / 128), dim3(384), 0, stream, dproj, bpart);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if (stop_after <= done++) return hipSuccess;
  {
    NlGemmArgs a{};
    a.a = dproj; a.a_cs = kNlQ; a.K = kNlQ; a.w = blob + nl_blob_off(3); a.w_cs = kNlQ; a.res = dz; a.res_cs = kNlCp;
    a.out = d_y3; a.out_cs = kNlC; a.n_store = kNlC;
    hipLaunchKernelGGL(nl_gemm_kernel<2>, dim3(N / 64, 3), dim3(256), 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (stop_after <= done++) return hipSuccess;
  {
    NlFoldArgs a{part1, part2, blob + nl_blob_off(5) + kNlC, Wgd, grads, pl.P};
    hipLaunchKernelGGL(nl_fold_kernel, dim3((kNlFoldElems + 255) / 256), dim3(256), 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (stop_after <= done++) return hipSuccess;
  NlFinishArgs a{szpart, bpart, Wgd, blob + nl_blob_off(4), blob + nl_blob_off(5), Sz, grads, N / 64, N / 128};
  hipLaunchKernelGGL(nl_finish_kernel, dim3(kNlC + kNlQ), dim3(64), 0, stream, a);
  return hipGetLastError();
}

}  // namespace bsr
