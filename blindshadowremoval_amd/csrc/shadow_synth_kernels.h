// The reference's training-shadow synthesis ON THE DEVICE: process_mask (train_test_GSC.py:81-105) and what it calls in utils.py
// (render_perlin_mask, render_shadow_from_mask, apply_disc_filter, apply_spatially_varying_blur, apply_ss_shadow_map, get_brightness_mask).
// blindshadowremoval_amd/shadow_synth.py is the host statement and writes the arithmetic out; every random draw is an ARGUMENT (the
// per-item draws record of kShadowWords 32-bit words, packed by shadow_synth.pack_draws), the device never calls sin, cos or exp: the
// Perlin gradients and the Gaussian taps come in the record.
//
// One chain of four launches on the caller's stream, no host synchronisation, no parallel branches:
//   shadow_init_kernel     item stage, grid (B): checks the record's integers (a bad one gives SHADOW_BAD_DRAWS and the item is skipped by
//                          every later stage: no index can leave its array) and RESETS the three reduction words of the item — on every
//                          call, so a second call never sees the first one's extrema.
//   shadow_perlin_kernel   pixel stage, grid (N/256, B): the 4-octave Perlin map and its > 0.15 threshold (a byte per pixel), the blend
//                          guidance (1 octave) with its min / max folded per wave and posted by vector atomics on order-preserving
//                          unsigned keys, and the brightness mask (2 octaves).  float32 in the host statement's operation order,
//                          contraction off: these planes are bit-identical to the host statement.
//   shadow_disc_kernel     pixel stage, grid (S/8, B): the disc blur(s) of the thresholded map.  A disc is a set of horizontal runs:
//                          the workgroup builds per-row prefix sums of the source rows of its 8 output rows in LDS, an output is then
//                          2r+1 run sums.  The reference's FFT form is a circular convolution of period S + r cropped at offset r - 1:
//                          the taps land on source pixels (y - 1 + dy, x - 1 + dx) and exactly one wrapped term reaches row 0 and
//                          column 0 (source row / column S - 1); both are index arithmetic here, no padded image exists.  The source is
//                          0 / 1, so a run sum is an exact integer and blur = float(count) * (1 / taps) is bit-identical to the host's
//                          float64 direct sum.  The spatially varying route blurs at r = b, 2b, 4b and blends with the guidance; the
//                          blurred plane's max is folded per wave and posted by atomicMax on the float's bits (values are >= 0).
//   shadow_ss_kernel       pixel stage, grid (S/8, B): _mask = face * blur / max (or the given mask), the six separable Gaussians of
//                          1 - _mask for a strip of 8 columns x S rows — x pass from 32-row LDS tiles of the source into an LDS strip,
//                          y pass down the strip (radius up to 82: the halo is larger than any tile, so the strip spans all rows) —
//                          accumulated into the three channels IN REGISTERS, then min(1, ./0.6), the composite
//                          clip(gt * mask_ss + img_dark * mask_sv * intensity, 0, 1), mask_sv, mask_edge and the status word.
//                          REFLECT padding is index arithmetic (radius <= S - 1 is checked by the init stage).
#pragma once
#include "post_common.h"

namespace bsr {

enum { SHADOW_OK = 0, SHADOW_EMPTY_MASK = 1, SHADOW_BAD_DRAWS = 2 };

// ---- the draws record (32-bit words; shadow_synth.py's DRAW_* constants state the same layout)
constexpr int kShadowWords = 4096;
constexpr int kSwU = 0;          // float[4]: u_mask, u_ss, u_bright, u_sv
constexpr int kSwDisc = 4;       // int: disc_filter_sz 1..11
constexpr int kSwBlur = 5;       // int: SV blur_size 1..2
constexpr int kSwPers = 6;       // float[3]: persistence of the shadow pattern, the blend guidance, the brightness mask
constexpr int kSwGain = 10;      // float[6]: red gains (word 9 is the SS scale r, read by the host only: the taps below come from it)
constexpr int kSwRad = 16;       // int[6]: Gaussian radii
constexpr int kSwGradShadow = 32;                       // lattices 5, 9, 17, 33: [side][side][2] (cos, sin)
constexpr int kSwGradGuide = 3000;                      // lattice 3
constexpr int kSwGradBright = 3018;                     // lattices 3, 5
constexpr int kSwTaps = 3088;                           // [6][kShadowMaxTaps]
constexpr int kShadowMaxRadius = 82, kShadowMaxTaps = 2 * kShadowMaxRadius + 1;
static_assert(kSwGradShadow + 2 * (25 + 81 + 289 + 1089) <= kSwGradGuide && kSwGradGuide + 18 <= kSwGradBright && kSwGradBright + 2 * (9 + 25) <= kSwTaps &&
                  kSwTaps + 6 * kShadowMaxTaps <= kShadowWords, "draws record layout");

struct ShadowVars { unsigned gmin, gmax; int bmax; int bad; };      // guidance extrema as ordered keys, the blurred max as float bits

struct ShadowScratch {                   // per item, in layout order
  ShadowVars* vars;
  float* guide;                          // [N] blend guidance
  float* bright;                         // [N] brightness mask
  float* blur;                           // [N] blurred mask before / max
  unsigned char* thre;                   // [N] thresholded Perlin map
  __host__ __device__ static ShadowScratch carve(ScratchCarver& c, int S) {
    const size_t N = (size_t)S * S;
    ShadowScratch s;
    s.vars = c.take_block<ShadowVars, 256>();
    s.guide = c.take<float>(N);
    s.bright = c.take<float>(N);
    s.blur = c.take<float>(N);
    s.thre = c.take<unsigned char>(N);
    return s;
  }
};
__host__ __device__ inline size_t shadow_item_scratch_bytes(int S) { return item_scratch_bytes<ShadowScratch>(S); }

__device__ inline const float* shadow_f(const uint32_t* rec, int w) { return reinterpret_cast<const float*>(rec + w); }
__device__ inline bool shadow_perlin_branch(const uint32_t* rec) { return !(shadow_f(rec, kSwU)[0] > 0.4f); }
__device__ inline bool shadow_ss_branch(const uint32_t* rec) { return shadow_f(rec, kSwU)[1] > 0.25f; }
__device__ inline bool shadow_sv_branch(const uint32_t* rec) { return shadow_f(rec, kSwU)[3] > 0.5f; }

// an order-preserving unsigned key of a float (NaN aside) and back
__device__ inline unsigned shadow_key(float f) { const unsigned b = __float_as_uint(f); return (b & 0x80000000u) ? ~b : (b | 0x80000000u); }
__device__ inline float shadow_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// ---- one Perlin octave at pixel (y, x): lattice of n x n cells, grads [n+1][n+1][2].  The sample positions are tf.linspace(0, n, S)
// stated as i * (n / (S - 1)); the cell is the NEAREST resize's floor((i + 0.5) n / S) = i n / S (S and n are powers of two).
__device__ inline void perlin_axis(int i, int S, int n, float& t, float& fade, int& cell) {
  #pragma clang fp contract(off)
  const float step = (float)n / (float)(S - 1);
  const float v = (float)i * step;
  t = v - floorf(v);
  const float t2 = t * t, t3 = t2 * t, t4 = t3 * t, t5 = t4 * t;
  fade = (6.0f * t5 - 15.0f * t4) + 10.0f * t3;
  cell = min((i * n) / S, n - 1);
}
__device__ inline float perlin_at(int y, int x, int S, int n, const float* __restrict__ g) {
  #pragma clang fp contract(off)
  float ty, fy, tx, fx;
  int cy, cx;
  perlin_axis(y, S, n, ty, fy, cy);
  perlin_axis(x, S, n, tx, fx, cx);
  const int side = n + 1;
  const float* g00 = g + ((size_t)cy * side + cx) * 2;
  const float* g10 = g00 + side * 2;          // next lattice row
  const float* g01 = g00 + 2;                 // next lattice column
  const float* g11 = g10 + 2;
  const float d1 = g00[0] * ty + g00[1] * tx;
  const float d2 = g10[0] * (ty - 1.0f) + g10[1] * tx;
  const float d3 = g01[0] * ty + g01[1] * (tx - 1.0f);
  const float d4 = g11[0] * (ty - 1.0f) + g11[1] * (tx - 1.0f);
  const float i1 = d1 * (1.0f - fy) + d2 * fy;
  const float i2 = d3 * (1.0f - fy) + d4 * fy;
  const float i3 = i1 * (1.0f - fx) + i2 * fx;
  return 1.41421356237309515f * i3;
}
// perlin_collection: octaves of doubling resolution from n0, amplitudes 1, p, p p, ...
__device__ inline float perlin_sum(int y, int x, int S, int n0, int octaves, float pers, const float* __restrict__ g) {
  #pragma clang fp contract(off)
  float noise = 0.f, amp = 1.0f;
  int n = n0;
  for (int o = 0; o < octaves; ++o) {
    noise = noise + amp * perlin_at(y, x, S, n, g);
    amp = amp * pers;
    g += (n + 1) * (n + 1) * 2;
    n *= 2;
  }
  return noise;
}

__global__ __launch_bounds__(64) void shadow_init_kernel(const uint32_t* __restrict__ draws, int S, void* scratch) {      // grid (B)
  if (threadIdx.x != 0) return;
  const int item = blockIdx.x;
  const uint32_t* rec = draws + (size_t)item * kShadowWords;
  const ShadowScratch sc = item_scratch<ShadowScratch>(scratch, item, S);
  const int disc = (int)rec[kSwDisc], blur = (int)rec[kSwBlur];
  bool bad = disc < 1 || disc > 11 || blur < 1 || blur > 2;
  for (int l = 0; l < 6; ++l) {
    const int R = (int)rec[kSwRad + l];
    bad = bad || R < 0 || R > kShadowMaxRadius || R > S - 1;
  }
  ShadowVars v;
  v.gmin = 0xffffffffu; v.gmax = 0u; v.bmax = 0; v.bad = bad ? 1 : 0;
  *sc.vars = v;
}

// aux: optional [B][3][S][S] float32 — the Perlin map (0 for an item with a given mask), the brightness mask, _mask (written by the last stage)
__global__ __launch_bounds__(256) void shadow_perlin_kernel(const uint32_t* __restrict__ draws, int S, void* scratch, float* __restrict__ aux) {
  #pragma clang fp contract(off)
  const int item = blockIdx.y;
  const int N = S * S;
  const int p = blockIdx.x * 256 + threadIdx.x;            // N is a multiple of 256
  const uint32_t* rec = draws + (size_t)item * kShadowWords;
  const ShadowScratch sc = item_scratch<ShadowScratch>(scratch, item, S);
  if (sc.vars->bad) return;
  const int y = p / S, x = p % S;
  const float* pers = shadow_f(rec, kSwPers);
  float map = 0.f;
  if (shadow_perlin_branch(rec)) {
    map = perlin_sum(y, x, S, 4, 4, pers[0], shadow_f(rec, kSwGradShadow));
    sc.thre[p] = map > 0.15f ? 1 : 0;
    if (shadow_sv_branch(rec)) {
      const float g = perlin_sum(y, x, S, 2, 1, pers[1], shadow_f(rec, kSwGradGuide));
      sc.guide[p] = g;
      unsigned lo = shadow_key(g), hi = lo;
      for (int o = 32; o > 0; o >>= 1) { lo = min(lo, (unsigned)__shfl_xor((int)lo, o)); hi = max(hi, (unsigned)__shfl_xor((int)hi, o)); }
      if ((threadIdx.x & 63) == 0) { atomicMin(&sc.vars->gmin, lo); atomicMax(&sc.vars->gmax, hi); }
    }
  }
  // get_brightness_mask: perlin / (1 / (min_val + 1e-6)) + min_val, min(., 1); min_val 0.3 when u_bright > 0.5, else 0.5
  const bool low = shadow_f(rec, kSwU)[2] > 0.5f;
  const float min_val = low ? 0.3f : 0.5f;
  const float inv = low ? (float)(1.0 / (0.3 + 1e-6)) : (float)(1.0 / (0.5 + 1e-6));
  const float b = fminf(perlin_sum(y, x, S, 2, 2, pers[2], shadow_f(rec, kSwGradBright)) / inv + min_val, 1.0f);
  sc.bright[p] = b;
  if (aux != nullptr) {
    aux[((size_t)item * 3 + 0) * N + p] = map;
    aux[((size_t)item * 3 + 1) * N + p] = b;
  }
}

// ---- the disc blur.  8 output rows per workgroup; s_pre[j][i] = number of lit pixels left of column i in source row row0 + j.
constexpr int kDiscRows = 8, kDiscMaxR = 11, kDiscSrcRows = kDiscRows + 2 * kDiscMaxR;

// half-width of the disc's row dy: the largest h with h h + dy dy <= r r
__device__ inline int disc_half_width(int r, int dy) {
  const int q = r * r - dy * dy;
  int h = (int)sqrtf((float)q);
  while (h * h > q) --h;
  while ((h + 1) * (h + 1) <= q) ++h;
  return h;
}

// apply_disc_filter at output (y, x): taps at source (y - 1 + dy, x - 1 + dx) over the disc, plus the one wrapped term of row 0 / column 0
__device__ inline float disc_at(const int (*s_pre)[257], const unsigned char* __restrict__ thre, int row0, int S, int r, int y, int x) {
  #pragma clang fp contract(off)
  int count = 0, taps = 0;
  for (int dy = -r; dy <= r; ++dy) {
    const int h = disc_half_width(r, dy);
    taps += 2 * h + 1;
    const int sy = y - 1 + dy;
    if (sy < 0 || sy >= S) continue;
    const int lo = max(x - 1 - h, 0), hi = min(x - 1 + h, S - 1);
    if (hi >= lo) count += s_pre[sy - row0][hi + 1] - s_pre[sy - row0][lo];
  }
  if (y == 0 && x >= 1) count += thre[(size_t)(S - 1) * S + (x - 1)];        // disc row 2r (one tap) wraps to source row S - 1
  if (x == 0 && y >= 1) count += thre[(size_t)(y - 1) * S + (S - 1)];        // disc column 2r wraps to source column S - 1
  return (float)count * (1.0f / (float)taps);
}

__global__ __launch_bounds__(256) void shadow_disc_kernel(const uint32_t* __restrict__ draws, int S, void* scratch) {      // grid (S / 8, B)
  __shared__ int s_pre[kDiscSrcRows][257];
  const int item = blockIdx.y;
  const uint32_t* rec = draws + (size_t)item * kShadowWords;
  const ShadowScratch sc = item_scratch<ShadowScratch>(scratch, item, S);
  if (sc.vars->bad || !shadow_perlin_branch(rec)) return;            // workgroup-uniform
  const bool sv = shadow_sv_branch(rec);
  const int rb = sv ? (int)rec[kSwBlur] : (int)rec[kSwDisc];
  const int rmax = sv ? 4 * rb : rb;                                 // <= 11
  const int y0 = blockIdx.x * kDiscRows;
  const int row0 = y0 - 1 - rmax, nrows = kDiscRows + 2 * rmax;      // source rows row0 .. row0 + nrows - 1
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int j = wave; j < nrows; j += 4) {
  #pragma clang fp contract(off)
    const int sy = row0 + j;
    int carry = 0;
    if (lane == 0) s_pre[j][0] = 0;
    for (int c0 = 0; c0 < S; c0 += 64) {
      const int c = c0 + lane;
      int v = (sy >= 0 && sy < S && c < S) ? (int)sc.thre[(size_t)sy * S + c] : 0;
      for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(v, o); if (lane >= o) v += u; }
      if (c < S) s_pre[j][c + 1] = carry + v;
      carry += __shfl(v, 63);
    }
  }
  __syncthreads();
  float gmin = 0.f, span = 1.f;
  if (sv) { gmin = shadow_unkey(sc.vars->gmin); span = shadow_unkey(sc.vars->gmax) - gmin; }
  float wmax = 0.f;
  for (int i = threadIdx.x; i < kDiscRows * S; i += 256) {
    const int y = y0 + i / S, x = i % S;
    const size_t p = (size_t)y * S + x;
    float v;
    if (!sv) {
      v = disc_at(s_pre, sc.thre, row0, S, rb, y, x);
    } else {
      const float p0 = disc_at(s_pre, sc.thre, row0, S, rb, y, x);
      const float p1 = disc_at(s_pre, sc.thre, row0, S, 2 * rb, y, x);
      const float p2 = disc_at(s_pre, sc.thre, row0, S, 4 * rb, y, x);
      // apply_pyramid_blend: guidance to [0, 3], two lerps from the coarsest level down
      float g = sc.guide[p] - gmin;
      g = span > 0.f ? g / span : 0.f;                                // rule 3: a constant guidance selects the finest level
      const float gb = fminf(fmaxf(g / (float)(1.0 / 3.0), 0.f), 3.0f);
      const float a1 = fminf(fmaxf(gb - 1.0f, 0.f), 1.0f);
      const float r1 = p1 + a1 * (p2 - p1);
      const float a0 = fminf(fmaxf(gb, 0.f), 1.0f);
      v = p0 + a0 * (r1 - p0);
    }
    sc.blur[p] = v;
    wmax = fmaxf(wmax, v);                                            // every v is finite: counts over tap counts, lerped with weights in [0, 1]
  }
  for (int o = 32; o > 0; o >>= 1) wmax = fmaxf(wmax, __shfl_xor(wmax, o));
  if (lane == 0 && wmax > 0.f) atomicMax(&sc.vars->bmax, __float_as_int(wmax));
}

// ---- subsurface scattering and the composite.  A strip of kSsCols columns x S rows per workgroup.
constexpr int kSsCols = 8, kSsChunk = 32, kSsStride = 256 + 8, kSsOuts = 256 * kSsCols / 256;      // outputs per thread at S = 256

__device__ inline int reflect_index(int i, int S) { return i < 0 ? -i : (i >= S ? 2 * (S - 1) - i : i); }      // REFLECT, |overhang| <= S - 1

__global__ __launch_bounds__(256) void shadow_ss_kernel(const float* __restrict__ mask, const float* __restrict__ gt, const float* __restrict__ img_dark,
                                                        const float* __restrict__ face, const uint32_t* __restrict__ draws, int S, void* scratch,
                                                        float* __restrict__ img, float* __restrict__ mask_sv, float* __restrict__ mask_edge,
                                                        int* __restrict__ status, float* __restrict__ aux) {      // grid (S / 8, B)
  __shared__ float s_in[kSsChunk][kSsStride];          // 32 source rows of 1 - _mask
  __shared__ float s_h[256][kSsCols];                  // the x pass of the strip, all rows
  const int item = blockIdx.y, tid = threadIdx.x;
  const int N = S * S;
  const uint32_t* rec = draws + (size_t)item * kShadowWords;
  const ShadowScratch sc = item_scratch<ShadowScratch>(scratch, item, S);
  const bool bad = sc.vars->bad != 0;
  const bool perlin = !bad && shadow_perlin_branch(rec);
  const float bmax = __int_as_float(sc.vars->bmax);
  const bool empty = perlin && !(bmax > 0.f);
  if (blockIdx.x == 0 && tid == 0) status[item] = bad ? SHADOW_BAD_DRAWS : (empty ? SHADOW_EMPTY_MASK : SHADOW_OK);
  const int x0 = blockIdx.x * kSsCols;
  const size_t base = (size_t)item * N;
  const int nout = S * kSsCols / 256;                  // 1, 2, 4 or 8 outputs per thread: pixel (j * 256 + tid) / 8, column x0 + tid % 8
  const int xx = tid % kSsCols;
  if (bad || empty) {                                  // our rule: the clipped ground truth and zero masks
    for (int j = 0; j < nout; ++j) {
  #pragma clang fp contract(off)
      const size_t q = (base + (size_t)((j * 256 + tid) / kSsCols) * S + x0 + xx) * 3;
      for (int c = 0; c < 3; ++c) { img[q + c] = fminf(fmaxf(gt[q + c], 0.f), 1.0f); mask_sv[q + c] = 0.f; mask_edge[q + c] = 0.f; }
    }
    return;
  }
  auto mask_at = [&](size_t q) -> float { return perlin ? face[base + q] * (sc.blur[q] / bmax) : mask[base + q]; };
  float acc[kSsOuts][3];
#pragma unroll
  for (int j = 0; j < kSsOuts; ++j) acc[j][0] = acc[j][1] = acc[j][2] = 0.f;
  const bool ss = shadow_ss_branch(rec);
  if (ss) {
    const float* gain = shadow_f(rec, kSwGain);
    // utils.py:695-700, columns 1..3 (column 0, the sigmas, went into the taps on the host)
    const float wr[6] = {0.22f, 0.101f, 0.119f, 0.114f, 0.364f, 0.080f}, wg[6] = {0.437f, 0.355f, 0.208f, 0.f, 0.f, 0.f}, wb[6] = {0.635f, 0.365f, 0.f, 0.f, 0.f, 0.f};
    for (int l = 0; l < 6; ++l) {
      const int R = (int)rec[kSwRad + l];
      const float* taps = shadow_f(rec, kSwTaps + l * kShadowMaxTaps);
      for (int c0 = 0; c0 < S; c0 += kSsChunk) {       // x pass, 32 rows at a time
        __syncthreads();
        for (int i = tid; i < kSsChunk * S; i += 256) {
          const int ry = i / S, cx = i % S;
          s_in[ry][cx] = 1.0f - mask_at((size_t)(c0 + ry) * S + cx);
        }
        __syncthreads();
        const int ry = tid / kSsCols;
        float a = 0.f;
        for (int k = 0; k <= 2 * R; ++k) a = a + taps[k] * s_in[ry][reflect_index(x0 + xx - R + k, S)];
        s_h[c0 + ry][xx] = a;
      }
      __syncthreads();
#pragma unroll
      for (int j = 0; j < kSsOuts; ++j) {
        if (j < nout) {
          const int y = (j * 256 + tid) / kSsCols;
          float a = 0.f;
          for (int k = 0; k <= 2 * R; ++k) a = a + taps[k] * s_h[reflect_index(y - R + k, S)][xx];
          acc[j][0] = acc[j][0] + (a * wr[l]) * gain[l];
          acc[j][1] = acc[j][1] + a * wg[l];
          acc[j][2] = acc[j][2] + a * wb[l];
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < kSsOuts; ++j) {
    if (j < nout) {
      const size_t q1 = (size_t)((j * 256 + tid) / kSsCols) * S + x0 + xx;
      const float m = mask_at(q1);
      const float inten = sc.bright[q1];
      const size_t q = (base + q1) * 3;
      if (aux != nullptr) aux[((size_t)item * 3 + 2) * N + q1] = m;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float m_ss = ss ? fminf(1.0f, acc[j][c] / 0.6f) : 1.0f - m;
        const float m_sv = 1.0f - m_ss;
        img[q + c] = fminf(fmaxf(gt[q + c] * m_ss + (img_dark[q + c] * m_sv) * inten, 0.f), 1.0f);
        mask_sv[q + c] = m_sv;
        mask_edge[q + c] = fabsf(m_sv - m);
      }
    }
  }
}

inline hipError_t launch_shadow_synth(const float* mask, const float* gt, const float* img_dark, const float* face, const uint32_t* draws, int B, int S,
                                      float* img, float* mask_sv, float* mask_edge, int* status, float* aux, void* scratch, hipStream_t stream) {
  const int N = S * S;
  hipLaunchKernelGGL(shadow_init_kernel, dim3((unsigned)B), dim3(64), 0, stream, draws, S, scratch);
  hipLaunchKernelGGL(shadow_perlin_kernel, dim3((unsigned)(N / 256), (unsigned)B), dim3(256), 0, stream, draws, S, scratch, aux);
  hipLaunchKernelGGL(shadow_disc_kernel, dim3((unsigned)(S / kDiscRows), (unsigned)B), dim3(256), 0, stream, draws, S, scratch);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(shadow_ss_kernel, dim3((unsigned)(S / kSsCols), (unsigned)B), dim3(256), 0, stream, mask, gt, img_dark, face, draws, S, scratch, img,
                     mask_sv, mask_edge, status, aux);
  return hipGetLastError();
}

}  // namespace bsr
