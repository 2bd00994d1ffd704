// UCB post-processing of the temporal-sharing model's FSRNet.test_step (/root/reference/train_with_TSM.py:418-618) ON THE DEVICE.
//
// Everything after the generator call, for a batch of B items, every decision and figure bit-identical to the host statement
// (blindshadowremoval_amd/ucb_post_tsm.py).  Unlike the GSC step (ucb_kernels.h) the decisions are taken at full size on the unrounded
// masks: mask_pred = dif0 * face_hair (:493), a flat threshold 0.01 (:497-519), 4-connected components kept when their size is >= 0.6 x
// the largest and their hair fraction (face_hair - face, unrounded) < 0.8 (:527-546), the nose rule with this script's four windows
// (:548-565); then the composites of both generator rows (:579-580), clip -> resize -> pad of row 0's composite, SSIM / PSNR against
// the resized ground truth (:588-600), and the eight figures (:614) as one uint8 strip.
//
// The machinery is post_common.h's, shared with the GSC chain: the connected components (cc_seed / cc_join / cc_root_sums / cc_largest
// over agent-scope atomics), numpy's pairwise order for the two float64 sums that feed decisions (ucb_leaf_sum / ucb_tree_sum: the nose
// mask's sum and the shadow intensity), py_slice, BilinearTap, put_figure, ucb_ssim_tile / ucb_ssim_finish.  The hair sums of the
// components are exact: every hair value is a float32 multiple of 2^-31 of magnitude <= 1, so they are summed as int64 multiples of
// 2^-31 by atomics, in any order.
// Pixel stages: grid (S*S/256, B), 256 threads, pixel p = blockIdx.x * 256 + tid.  Item stages: grid (B).
#pragma once
#include "post_common.h"

namespace bsr {

constexpr int kUcbTsmFigs = 8;
constexpr int kUcbTsmRowCh = 13;         // img0 3 | gt0 3 | con0 3 | con1 3 | dif0 1
constexpr int kUcbTsmMasks = 3;          // face_hair | face | nose

enum { TSM_NOSE_R0, TSM_NOSE_R1, TSM_NOSE_C0, TSM_NOSE_C1, TSM_NOSE_CNT, TSM_MAX_SIZE, TSM_KEEP_CNT, TSM_NOSE_SH, TSM_NVARS };

struct UcbTsmVars {
  int v[TSM_NVARS];
  int fail, size, nose_hit, ra, rb, ca, cb;
};

struct UcbTsmVarRule {                   // which of v are min / max targets (post_common.h: vars_init, wg_vars_begin / wg_vars_end)
  static constexpr int kCount = TSM_NVARS, kMaxSize = TSM_MAX_SIZE;
  __device__ static bool is_min(int k) { return k == TSM_NOSE_R0 || k == TSM_NOSE_C0; }
  __device__ static bool is_max(int k) { return k == TSM_NOSE_R1 || k == TSM_NOSE_C1 || k == TSM_MAX_SIZE; }
};

struct UcbTsmScratch {                   // per item, inside the caller's scratch block (N = S*S), in layout order
  double* ssim_part;                     // [2][nblk]
  double* leaf_sh;                       // [N / 128] leaf sums of the shadow intensity
  double* leaf_nose;                     // [N / 128] leaf sums of the nose mask
  long long* chair;                      // [N] hair sum per component (at the root), in units of 2^-31
  float* gt;                             // [N][3] gt_sc
  float* out;                            // [N][3] output (resized clipped composite, padded)
  float* comp;                           // [N][3] clip(orig composite)
  unsigned* label;                       // [N] union-find parents
  unsigned* csize;                       // [N] component sizes (at the root)
  unsigned char* keep;                   // [N] detected, then kept
  UcbTsmVars* vars;
  __host__ __device__ static UcbTsmScratch carve(ScratchCarver& c, int S) {
    const size_t N = (size_t)S * S;
    UcbTsmScratch s;
    s.ssim_part = c.take<double>(2 * (size_t)ssim_tiles(S));
    s.leaf_sh = c.take<double>(N / 128);
    s.leaf_nose = c.take<double>(N / 128);
    s.chair = c.take<long long>(N);
    s.gt = c.take<float>(N * 3);
    s.out = c.take<float>(N * 3);
    s.comp = c.take<float>(N * 3);
    s.label = c.take<unsigned>(N);
    s.csize = c.take<unsigned>(N);
    s.keep = c.take<unsigned char>(N);
    c.align(8);
    s.vars = c.take_block<UcbTsmVars, 256>();
    return s;
  }
};
__host__ __device__ inline size_t ucb_tsm_item_scratch_bytes(int S) { return item_scratch_bytes<UcbTsmScratch>(S); }
__host__ __device__ inline UcbTsmScratch ucb_tsm_scratch(void* base, int item, int S) { return item_scratch<UcbTsmScratch>(base, item, S); }

// rows: [B][S][S][13] float32; masks: [B][3][S][S] uint8 grey levels (face_hair, face, nose: one of cv2.imread's three equal channels);
// boxes: [B][4] float32
__global__ void ucb_tsm_init_kernel(const float* __restrict__ boxes, int S, void* scratch) {       // grid (B), 64 threads
  const int item = blockIdx.x, tid = threadIdx.x;
  UcbTsmVars* g = ucb_tsm_scratch(scratch, item, S).vars;
  vars_init<UcbTsmVarRule>(g, tid);
  if (tid == 0) {
    const int size = ucb_box_size(boxes + 4 * item);
    g->size = size;
    g->fail = (size <= 0 || size > S) ? UCB_BAD_BOX : UCB_OK;
    g->nose_hit = 0;
  }
}

// stage 1: the flat threshold on the gated magnitude (:493-519) and the union-find initialisation; the nose mask's bounding box, count of
// pixels equal to 1 and float64 sum (:552-560)
__global__ __launch_bounds__(256) void ucb_tsm_s1_kernel(const float* __restrict__ rows, const unsigned char* __restrict__ masks, int S, void* scratch) {
#pragma clang fp contract(off)
  __shared__ int s_v[TSM_NVARS];
  __shared__ double s_d[256];
  const int item = blockIdx.y, tid = threadIdx.x, p = blockIdx.x * 256 + tid;
  const int N = S * S;
  const UcbTsmScratch sc = ucb_tsm_scratch(scratch, item, S);
  if (sc.vars->fail) return;
  wg_vars_begin<UcbTsmVarRule>(s_v, tid);
  const int y = p / S, x = p % S;
  const unsigned char* m = masks + (size_t)item * kUcbTsmMasks * N;
  const float mp = rows[((size_t)item * N + p) * kUcbTsmRowCh + 12] * mask_level(m[p]);
  const bool det = mp > 0.01f;
  sc.keep[p] = det ? 1 : 0;
  const unsigned char nose = m[2 * (size_t)N + p];
  ucb_wave_box(s_v, nose == 255, y, x, TSM_NOSE_R0, TSM_NOSE_R1, TSM_NOSE_C0, TSM_NOSE_C1, TSM_NOSE_CNT);
  s_d[tid] = (double)nose / 255.0;
  cc_seed(det, p, x, sc.label, sc.csize, sc.chair);
  wg_vars_end<UcbTsmVarRule>(s_v, sc.vars, tid);                            // (its barrier also publishes s_d)
  if (tid < 2) sc.leaf_nose[blockIdx.x * 2 + tid] = ucb_leaf_sum<double>(s_d + 128 * tid);
}

// stage 2: 4-connected components (:524): join runs with their left and upper neighbours ...
__global__ __launch_bounds__(256) void ucb_tsm_s2a_kernel(int S, void* scratch) {
  const int item = blockIdx.y, p = blockIdx.x * 256 + threadIdx.x;
  const UcbTsmScratch sc = ucb_tsm_scratch(scratch, item, S);
  if (sc.vars->fail) return;
  cc_join(sc.label, sc.keep, p, S);
}

// ... then sizes and hair sums at the roots
__global__ __launch_bounds__(256) void ucb_tsm_s2b_kernel(const unsigned char* __restrict__ masks, int S, void* scratch) {
  const int item = blockIdx.y, p = blockIdx.x * 256 + threadIdx.x;
  const int N = S * S;
  const UcbTsmScratch sc = ucb_tsm_scratch(scratch, item, S);
  if (sc.vars->fail) return;
  const unsigned char* m = masks + (size_t)item * kUcbTsmMasks * N;
  cc_root_sums(sc.label, sc.csize, sc.chair, sc.keep[p] != 0, p, [&] {
    const float h = (float)((double)m[p] / 255.0 - (double)m[(size_t)N + p] / 255.0);         // tf.cast(curr_mask - curr_mask_no_hair, float32)
    return (long long)((double)h * 2147483648.0);                                              // exact: h is a multiple of 2^-31
  });
}

__global__ __launch_bounds__(256) void ucb_tsm_s2c_kernel(int S, void* scratch) {       // the largest component
  __shared__ int s_v[TSM_NVARS];
  const int item = blockIdx.y, tid = threadIdx.x, p = blockIdx.x * 256 + tid;
  const UcbTsmScratch sc = ucb_tsm_scratch(scratch, item, S);
  if (sc.vars->fail) return;
  cc_largest<UcbTsmVarRule>(s_v, sc.vars, sc.label, sc.csize, sc.keep, p, tid);
}

// stage 3: the keep filter (:533-546) and the sums of the nose rule (:549-552)
__global__ __launch_bounds__(256) void ucb_tsm_s3_kernel(const float* __restrict__ rows, const unsigned char* __restrict__ masks, int S, void* scratch) {
#pragma clang fp contract(off)
  __shared__ int s_v[TSM_NVARS];
  __shared__ double s_d[256];
  const int item = blockIdx.y, tid = threadIdx.x, p = blockIdx.x * 256 + tid;
  const int N = S * S;
  const UcbTsmScratch sc = ucb_tsm_scratch(scratch, item, S);
  if (sc.vars->fail) return;
  wg_vars_begin<UcbTsmVarRule>(s_v, tid);
  const double min_size = 0.6 * (double)sc.vars->v[TSM_MAX_SIZE];
  unsigned char k = 0;
  if (sc.keep[p]) {
    const unsigned root = uf_load(sc.label + p);
    const unsigned sz = uf_load(sc.csize + root);
    const long long hs = uf_load(sc.chair + root);
    if ((double)sz >= min_size && ((double)hs * 4.656612873077392578125e-10) / (double)sz < 0.8) k = 1;      // hs * 2^-31
  }
  sc.keep[p] = k;                                               // only this thread reads keep[p] in this launch
  const float* r = rows + ((size_t)item * N + p) * kUcbTsmRowCh;
  const float mean3 = ((r[0] + r[1]) + r[2]) / 3.f;            // np.mean(tmp, 2): float32
  const double sh = (double)k * (double)mean3;                 // img2 is a float64 array in the reference
  s_d[tid] = sh;
  const double nose = (double)masks[((size_t)item * kUcbTsmMasks + 2) * N + p] / 255.0;
  const unsigned long long m_k = __ballot(k != 0), m_n = __ballot(nose * sh > 0.0);
  if ((tid & 63) == 0) {
    if (m_k) atomicAdd(&s_v[TSM_KEEP_CNT], __popcll(m_k));
    if (m_n) atomicAdd(&s_v[TSM_NOSE_SH], __popcll(m_n));
  }
  wg_vars_end<UcbTsmVarRule>(s_v, sc.vars, tid);                            // (its barrier also publishes s_d)
  if (tid < 2) sc.leaf_sh[blockIdx.x * 2 + tid] = ucb_leaf_sum<double>(s_d + 128 * tid);
}

// the nose rule's verdict (:550-565).  nose_stats: [B][2] float64 = frac_nose_in_shadow, mean_intensity (NaN both for a failed item)
__global__ __launch_bounds__(512) void ucb_tsm_a3_kernel(int S, void* scratch, double* __restrict__ nose_stats) {      // grid (B), 512 threads
#pragma clang fp contract(off)
  __shared__ double s_tree[512], s_tree2[512];
  const int tid = threadIdx.x;
  const UcbTsmScratch sc = ucb_tsm_scratch(scratch, blockIdx.x, S);
  UcbTsmVars* g = sc.vars;
  double* ns = nose_stats + 2 * blockIdx.x;
  if (g->fail) {
    if (tid == 0) ns[0] = ns[1] = __builtin_nan("");
    return;
  }
  const double sum_sh = ucb_tree_sum<double>(sc.leaf_sh, S * S / 128, s_tree, tid, 512);
  const double sum_nose = ucb_tree_sum<double>(sc.leaf_nose, S * S / 128, s_tree2, tid, 512);
  if (tid != 0) return;
  if (g->v[TSM_NOSE_CNT] == 0) {                                // the reference's np.max of an empty row list
    g->fail = UCB_EMPTY_MASK;
    ns[0] = ns[1] = __builtin_nan("");
    return;
  }
  const double mean_intensity = sum_sh / (double)g->v[TSM_KEEP_CNT];
  const double frac = (double)g->v[TSM_NOSE_SH] / sum_nose;
  ns[0] = frac;
  ns[1] = mean_intensity;
  g->nose_hit = 0;
  if ((0.423 < frac && frac < 0.425) || (0.53 < frac && frac < 0.56) || (0.35 < frac && frac < 0.38) || (0.58 < frac && frac < 0.605)) {
    const double mid_nose_height = (g->v[TSM_NOSE_R1] + g->v[TSM_NOSE_R0]) / 2.0, mid_nose_width = (g->v[TSM_NOSE_C1] + g->v[TSM_NOSE_C0]) / 2.0;
    const int reach = mean_intensity < 0.15 ? 5 : 65;
    g->nose_hit = 1;
    py_slice((int)mid_nose_height, g->v[TSM_NOSE_R1] + reach, S, g->ra, g->rb);
    py_slice((int)(mid_nose_width - 35), (int)(mid_nose_width + 35), S, g->ca, g->cb);
  }
}

__device__ inline float tsm_max(float a, float b) { return (isnan(a) || a >= b) ? a : b; }        // np.maximum

// stage 4: the nose rule applied, the composites of both rows (:579-580) and the six figures that are not resized (:614).
// strips: [B][S][8 S][3] uint8; figs: optional [B][8][S][S][3] float32; status: [B]
__global__ __launch_bounds__(256) void ucb_tsm_s4_kernel(const float* __restrict__ rows, const unsigned char* __restrict__ masks, int S, void* scratch,
                                                         unsigned char* __restrict__ strips, float* __restrict__ figs, int* __restrict__ status) {
#pragma clang fp contract(off)
  const int item = blockIdx.y, p = blockIdx.x * 256 + threadIdx.x;
  const int N = S * S;
  const UcbTsmScratch sc = ucb_tsm_scratch(scratch, item, S);
  const UcbTsmVars* g = sc.vars;
  unsigned char* strip = strips + (size_t)item * N * kUcbTsmFigs * 3;
  const int y = p / S, x = p % S;
  if (p == 0) status[item] = g->fail;
  if (g->fail) {                                                // a black strip; NaN losses are left to the finish kernel
    const float zero[3] = {0.f, 0.f, 0.f};
    for (int k = 0; k < kUcbTsmFigs; ++k) put_figure<kUcbTsmFigs>(strip, figs, S, item, k, y, x, zero);
    return;
  }
  const int xm = S - 1 - x, pm = y * S + xm;                    // the mirrored pixel
  auto final_keep = [&](int q, int qx) {
    return sc.keep[q] != 0 && !(g->nose_hit && y >= g->ra && y < g->rb && qx >= g->ca && qx < g->cb);
  };
  const float d = final_keep(p, x) ? 1.f : 0.f, dm = final_keep(pm, xm) ? 1.f : 0.f;
  const float* r = rows + ((size_t)item * N + p) * kUcbTsmRowCh;
  const float* rm = rows + ((size_t)item * N + pm) * kUcbTsmRowCh;
  const float mp2 = (r[12] * mask_level(masks[(size_t)item * kUcbTsmMasks * N + p])) * 2.f;
  float f0[3], f2[3], f4[3], f5[3], f6[3], f7[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float tmp = r[c];
    const float orig = r[6 + c] * d + tmp * (1.f - d);
    const float flipped = r[9 + c] * dm + rm[c] * (1.f - dm);         // flipped at p
    const float flipflip = rm[9 + c] * d + tmp * (1.f - d);           // flipped at the mirrored pixel = flip(flipped) at p
    sc.comp[(size_t)p * 3 + c] = fminf(fmaxf(orig, 0.f), 1.f);
    f0[c] = tmp; f2[c] = mp2; f4[c] = d; f5[c] = flipped; f6[c] = flipflip; f7[c] = tsm_max(orig, flipflip);
  }
  put_figure<kUcbTsmFigs>(strip, figs, S, item, 0, y, x, f0);
  put_figure<kUcbTsmFigs>(strip, figs, S, item, 2, y, x, f2);
  put_figure<kUcbTsmFigs>(strip, figs, S, item, 4, y, x, f4);
  put_figure<kUcbTsmFigs>(strip, figs, S, item, 5, y, x, f5);
  put_figure<kUcbTsmFigs>(strip, figs, S, item, 6, y, x, f6);
  put_figure<kUcbTsmFigs>(strip, figs, S, item, 7, y, x, f7);
}

// stage 5: output = pad(resize(clip(orig))), gt_sc = pad(resize(gt0)) (:441,454,588-590, BilinearTap), the SSIM operands and
// figures 1 and 3
__global__ __launch_bounds__(256) void ucb_tsm_s5_kernel(const float* __restrict__ rows, int S, void* scratch,
                                                         unsigned char* __restrict__ strips, float* __restrict__ figs) {
#pragma clang fp contract(off)
  const int item = blockIdx.y, p = blockIdx.x * 256 + threadIdx.x;
  const int N = S * S;
  const UcbTsmScratch sc = ucb_tsm_scratch(scratch, item, S);
  const UcbTsmVars* g = sc.vars;
  unsigned char* strip = strips + (size_t)item * N * kUcbTsmFigs * 3;
  const int oy = p / S, ox = p % S;
  const int size = g->size;
  float o[3] = {0.f, 0.f, 0.f}, gt[3] = {0.f, 0.f, 0.f};
  if (!g->fail && oy < size && ox < size) {
    const BilinearTap t(oy, ox, size, S);
    const float* r = rows + (size_t)item * N * kUcbTsmRowCh;
    const size_t q00 = (size_t)t.y0 * S + t.x0, q01 = (size_t)t.y0 * S + t.x1, q10 = (size_t)t.y1 * S + t.x0, q11 = (size_t)t.y1 * S + t.x1;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      o[c] = t.lerp(sc.comp[q00 * 3 + c], sc.comp[q01 * 3 + c], sc.comp[q10 * 3 + c], sc.comp[q11 * 3 + c]);
      gt[c] = t.lerp(r[q00 * kUcbTsmRowCh + 3 + c], r[q01 * kUcbTsmRowCh + 3 + c], r[q10 * kUcbTsmRowCh + 3 + c], r[q11 * kUcbTsmRowCh + 3 + c]);
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) { sc.gt[(size_t)p * 3 + c] = gt[c]; sc.out[(size_t)p * 3 + c] = o[c]; }
  put_figure<kUcbTsmFigs>(strip, figs, S, item, 1, oy, ox, o);
  put_figure<kUcbTsmFigs>(strip, figs, S, item, 3, oy, ox, gt);
}

inline hipError_t launch_ucb_post_tsm(const float* rows, const unsigned char* masks, const float* boxes, int B, int S, float* losses,
                                      double* nose_stats, unsigned char* strips, float* figs, int* status, void* scratch, hipStream_t stream) {
  const int N = S * S;
  const dim3 px((unsigned)(N / 256), (unsigned)B), it((unsigned)B);
  hipLaunchKernelGGL(ucb_tsm_init_kernel, it, dim3(64), 0, stream, boxes, S, scratch);
  hipLaunchKernelGGL(ucb_tsm_s1_kernel, px, dim3(256), 0, stream, rows, masks, S, scratch);
  hipLaunchKernelGGL(ucb_tsm_s2a_kernel, px, dim3(256), 0, stream, S, scratch);
  hipLaunchKernelGGL(ucb_tsm_s2b_kernel, px, dim3(256), 0, stream, masks, S, scratch);
  hipLaunchKernelGGL(ucb_tsm_s2c_kernel, px, dim3(256), 0, stream, S, scratch);
  hipLaunchKernelGGL(ucb_tsm_s3_kernel, px, dim3(256), 0, stream, rows, masks, S, scratch);
  hipLaunchKernelGGL(ucb_tsm_a3_kernel, it, dim3(512), 0, stream, S, scratch, nose_stats);
  hipLaunchKernelGGL(ucb_tsm_s4_kernel, px, dim3(256), 0, stream, rows, masks, S, scratch, strips, figs, status);
  hipLaunchKernelGGL(ucb_tsm_s5_kernel, px, dim3(256), 0, stream, rows, S, scratch, strips, figs);
  return launch_ssim_tail(
      B, S, [&](dim3 grid, dim3 block) { hipLaunchKernelGGL(ssim_pair_kernel<UcbTsmScratch>, grid, block, 0, stream, S, scratch); },
      [&](dim3 grid, dim3 block) { hipLaunchKernelGGL(ssim_finish_kernel<UcbTsmScratch>, grid, block, 0, stream, S, scratch, status, losses); });
}

}  // namespace bsr
