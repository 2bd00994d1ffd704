// UCB post-processing of FSRNet.test_step (/root/reference/train_test_GSC.py:411-748) ON THE DEVICE (round 5).
//
// What the reference does per item on the host with TensorFlow eager ops, numpy and cv2 — resize the generator outputs, the input, the
// ground truth and seven segmentation masks to the crop-box size and zero-pad them back (:437-477), gate the predicted shadow magnitude
// by per-region thresholds (:479-590), keep the large 4-connected components that are not hair (:594-615), apply the nose rule
// (:650-666), composite (:711-722), score SSIM / PSNR (:724-725) and lay the seven figures out as one strip (:744) — cost 26 ms of
// CPU per item in rounds 2-4 (blindshadowremoval_amd/ucb_post.py, the host statement of the same steps) and set the rate of
// FSRNet.test.  Here: three kernels per batch, every DECISION (thresholds, rounded masks, components, rules) bit-identical to
// ucb_post.ucb_postprocess:
//   * all arithmetic that feeds a comparison is done in the host statement's type and operation order with fp contraction off —
//     the bilinear resize is TensorFlow's CPU kernel's (compute_lerp: top = tl + (tr - tl) * xl; ... ; out = top + (bottom - top) * yl,
//     float32), means over the three channels are ((a + b) + c) / 3, counts are integers, float sums over the image use numpy's
//     pairwise order (128-element leaves with eight interleaved accumulators, then a balanced binary tree);
//   * region slices follow Python's slice rules (a negative start counts from the end).
// ucb_resize_kernel: one thread per output pixel.  The per-item work — round 5: ONE workgroup of 1024 threads per item walking its 65 536 pixels
// stage by stage (16 of 256 CUs busy for 1.2 ms per batch of 16) — is, since round 6, a CHAIN of small launches: every stage that is a map
// over pixels (mask boxes / counts, the gates, the per-pixel threshold, union, root sizes, the keep filter, the composite and the strip)
// covers all items with S*S/256 workgroups each, integer reductions by atomics into a per-item variable block in the scratch (a workgroup
// folds its own contribution in LDS first), the two float sums that feed comparisons keep numpy's pairwise order (a workgroup of 256
// pixels owns exactly two 128-element leaves; a one-workgroup-per-item launch folds the 512 leaf sums in the balanced tree and derives the
// scalars of the next stage).  Same arithmetic, same decisions, same bytes; what a stage reads of another workgroup's results crosses a
// kernel boundary (union-find parents: agent-scope atomics, as before).
// ucb_ssim_kernel: tf.image.ssim's 11x11 Gaussian window as two separable float32 passes through LDS + the squared error for PSNR,
// one partial sum per workgroup, folded in a fixed order (deterministic).
// What this chain shares with the TSM chain, the RGB baseline and the SFW scoring — the scratch carver, the bilinear tap, the figure
// writer, the variable block, the connected components, the pairwise sum, the SSIM tile routine and its fold — is in post_common.h.
#pragma once
#include "post_common.h"

namespace bsr {

constexpr int kUcbCh = 17;                // resized planes per pixel: gt 3 | pred 3 | tmp 3 | mp 1 | masks 7 (face_hair face mouth nose eyebrow eye glasses)
constexpr int kUcbFigs = 7;

// integer variables of an item (atomic min / max / add targets of the pixel stages)
enum { NOSE_R0, NOSE_R1, NOSE_C0, NOSE_C1, MOUTH_R0, MOUTH_R1, MOUTH_C0, MOUTH_C1, BROW_CNT, BROW_R0, BROW_C0, FACE_C0, FACE_C1, FACE_CNT,
       FH_R0, FH_C0, FH_C1, FH_CNT, NOSE_CNT, MOUTH_CNT, CNT_SR, CNT_ROI, CNT_DEN, MAX_SIZE, KEEP_CNT, NOSE_SH, UCB_NVARS };
constexpr int kUcbMinVars[] = {NOSE_R0, NOSE_C0, MOUTH_R0, MOUTH_C0, BROW_R0, BROW_C0, FACE_C0, FH_R0, FH_C0};
constexpr int kUcbMaxVars[] = {NOSE_R1, NOSE_C1, MOUTH_R1, MOUTH_C1, FACE_C1, FH_C1, MAX_SIZE};

struct UcbItemVars {
  int v[UCB_NVARS];
  int fail;                                  // UCB_OK, or why the item gets a black strip (every later stage skips it)
  int size;
  int forehead_rule, roi_off, left_rule, nose_hit;
  int r1a, r1b, c1a, c1b, r2a, r2b, below_lo, below_hi, fr0, fr1, fc0, fc1, left_hi, ra, rb, ca, cb;
  double min_size;
};

struct UcbVarRule {                          // which of them are min / max targets (post_common.h: vars_init, wg_vars_begin / wg_vars_end)
  static constexpr int kCount = UCB_NVARS, kMaxSize = MAX_SIZE;
  __device__ static bool is_min(int k) { for (int i : kUcbMinVars) if (i == k) return true; return false; }
  __device__ static bool is_max(int k) { for (int i : kUcbMaxVars) if (i == k) return true; return false; }
};

struct UcbScratch {                      // per-item arrays inside the caller's scratch block (all sized for N = S*S pixels), in layout order
  double* dval;                          // [N] float64 values of a pairwise sum
  double* ssim_part;                     // [2][nblk] partial sums of the SSIM map and of the squared error
  float* w;                              // [N][17]
  float* mp;                             // [N] gated magnitude
  float* out;                            // [N][3] composite
  float* fval;                           // [N] float32 values of a pairwise sum
  unsigned* label;                       // [N] union-find parents
  unsigned* csize;                       // [N] component sizes (at the root)
  int* chair;                            // [N] signed hair sum per component (at the root)
  unsigned char* keep;                   // [N]
  UcbItemVars* vars;                     // per-item variables of the stage chain (round 6)
  double* leaf_d;                        // [N / 128] leaf sums of a float64 pairwise sum
  float* leaf_f;                         // [N / 128] leaf sums of a float32 pairwise sum
  __host__ __device__ static UcbScratch carve(ScratchCarver& c, int S) {
    const size_t N = (size_t)S * S;
    UcbScratch s;
    s.dval = c.take<double>(N);
    s.ssim_part = c.take<double>(2 * (size_t)ssim_tiles(S));
    s.w = c.take<float>(N * kUcbCh);
    s.mp = c.take<float>(N);
    s.out = c.take<float>(N * 3);
    s.fval = c.take<float>(N);
    s.label = c.take<unsigned>(N);
    s.csize = c.take<unsigned>(N);
    s.chair = c.take<int>(N);
    s.keep = c.take<unsigned char>(N);
    c.align(8);
    s.vars = c.take_block<UcbItemVars, 512>();
    s.leaf_d = c.take<double>(N / 128);
    s.leaf_f = c.take<float>(N / 128);
    return s;
  }
};
__host__ __device__ inline size_t ucb_item_scratch_bytes(int S) { return item_scratch_bytes<UcbScratch>(S); }
__host__ __device__ inline UcbScratch ucb_scratch(void* base, int item, int S) { return item_scratch<UcbScratch>(base, item, S); }

// rows10: [B][S][S][10] float32 = input 3 | ground truth 3 | con_rgb 3 | dif 1 of row 0 of each item; masks: [B][7][S][S] uint8 grey
// levels (cv2.imread(...) / 255.0, one of the three equal channels); boxes: [B][4] float32
__global__ __launch_bounds__(256) void ucb_resize_kernel(const float* __restrict__ rows10, const unsigned char* __restrict__ masks,
                                                         const float* __restrict__ boxes, int S, void* scratch) {
#pragma clang fp contract(off)
  const int item = blockIdx.y;
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= S * S) return;
  const int oy = p / S, ox = p % S;
  const int size = ucb_box_size(boxes + 4 * item);
  float* w = ucb_scratch(scratch, item, S).w + (size_t)p * kUcbCh;
  if (size <= 0 || size > S || oy >= size || ox >= size) {          // the zero pad of :454-477
#pragma unroll
    for (int c = 0; c < kUcbCh; ++c) w[c] = 0.f;
    return;
  }
  const BilinearTap t(oy, ox, size, S);
  const float* r = rows10 + (size_t)item * S * S * 10;
  const float* tl = r + ((size_t)t.y0 * S + t.x0) * 10; const float* tr = r + ((size_t)t.y0 * S + t.x1) * 10;
  const float* bl = r + ((size_t)t.y1 * S + t.x0) * 10; const float* br = r + ((size_t)t.y1 * S + t.x1) * 10;
  // rows10 channels: im 0-2, gt 3-5, con 6-8, dif 9  ->  w: gt 0-2, pred 3-5, tmp 6-8, mp 9
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    w[c] = t.lerp(tl[3 + c], tr[3 + c], bl[3 + c], br[3 + c]);
    w[3 + c] = t.lerp(tl[6 + c], tr[6 + c], bl[6 + c], br[6 + c]);
    w[6 + c] = t.lerp(tl[c], tr[c], bl[c], br[c]);
  }
  w[9] = t.lerp(tl[9], tr[9], bl[9], br[9]);
  const unsigned char* m = masks + (size_t)item * 7 * S * S;
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    const unsigned char* mk = m + (size_t)k * S * S;
    auto g = [&](int y, int x) { return mask_level(mk[y * S + x]); };
    w[10 + k] = rintf(t.lerp(g(t.y0, t.x0), g(t.y0, t.x1), g(t.y1, t.x0), g(t.y1, t.x1)));         // tf.round: half to even
  }
}

// ---- the stage chain.  Pixel stages: grid (N / 256, B), 256 threads, pixel p = blockIdx.x * 256 + tid.  Item stages: grid (B), 512 threads.

__global__ void ucb_init_kernel(const float* __restrict__ boxes, int S, void* scratch) {       // grid (B), 64 threads
  const int item = blockIdx.x, tid = threadIdx.x;
  UcbItemVars* g = ucb_scratch(scratch, item, S).vars;
  vars_init<UcbVarRule>(g, tid);
  if (tid == 0) {
    const int size = ucb_box_size(boxes + 4 * item);
    g->size = size;
    g->fail = (size <= 0 || size > S) ? UCB_BAD_BOX : UCB_OK;
    g->forehead_rule = g->roi_off = g->left_rule = g->nose_hit = 0;
  }
}

// stage 1: bounding boxes and counts of the rounded masks (:479-489, :533-536, :565-567)
__global__ __launch_bounds__(256) void ucb_s1_kernel(int S, void* scratch) {
  __shared__ int s_v[UCB_NVARS];
  const int item = blockIdx.y, tid = threadIdx.x, p = blockIdx.x * 256 + tid;
  const UcbScratch sc = ucb_scratch(scratch, item, S);
  if (sc.vars->fail) return;
  wg_vars_begin<UcbVarRule>(s_v, tid);
  const float4 w = *reinterpret_cast<const float4*>(sc.w + (size_t)p * kUcbCh + 11 - 3);      // channels 8 .. 11
  const float4 w2 = *reinterpret_cast<const float4*>(sc.w + (size_t)p * kUcbCh + 12);        // channels 12 .. 15
  const int y = p / S, x = p % S;
  ucb_wave_box(s_v, w2.y == 1.f, y, x, NOSE_R0, NOSE_R1, NOSE_C0, NOSE_C1, NOSE_CNT);
  ucb_wave_box(s_v, w2.x == 1.f, y, x, MOUTH_R0, MOUTH_R1, MOUTH_C0, MOUTH_C1, MOUTH_CNT);
  ucb_wave_box(s_v, w2.z == 1.f, y, x, BROW_R0, -1, BROW_C0, -1, -1);
  ucb_wave_box(s_v, w2.z != 0.f, y, x, -1, -1, -1, -1, BROW_CNT);    // np.sum(brow): the rounded mask is 0 / 1, three equal channels
  ucb_wave_box(s_v, w.w == 1.f, y, x, -1, -1, FACE_C0, FACE_C1, FACE_CNT);
  wg_vars_end<UcbVarRule>(s_v, sc.vars, tid);
}

__global__ void ucb_a1_kernel(int S, void* scratch) {            // grid (B), 1 thread: what stage 1 decided
  UcbItemVars* g = ucb_scratch(scratch, blockIdx.x, S).vars;
  if (threadIdx.x != 0 || g->fail) return;
  if (g->v[NOSE_CNT] == 0 || g->v[MOUTH_CNT] == 0) { g->fail = UCB_EMPTY_MASK; return; }
  g->forehead_rule = 3 * g->v[BROW_CNT] > 30 ? 1 : 0;
}

// bbox of the face above the eyebrows (:535-538), only where the forehead rule applies
__global__ __launch_bounds__(256) void ucb_s1b_kernel(int S, void* scratch) {
  __shared__ int s_v[UCB_NVARS];
  const int item = blockIdx.y, tid = threadIdx.x, p = blockIdx.x * 256 + tid;
  const UcbScratch sc = ucb_scratch(scratch, item, S);
  if (sc.vars->fail || !sc.vars->forehead_rule) return;
  wg_vars_begin<UcbVarRule>(s_v, tid);
  const int upper_brow = sc.vars->v[BROW_R0];
  const int y = p / S, x = p % S;
  ucb_wave_box(s_v, y < upper_brow && sc.w[(size_t)p * kUcbCh + 11] == 1.f, y, x, FH_R0, -1, FH_C0, FH_C1, FH_CNT);
  wg_vars_end<UcbVarRule>(s_v, sc.vars, tid);
}

__global__ void ucb_a1b_kernel(int S, void* scratch) {           // grid (B), 1 thread: the slices of stages 2-3
  UcbItemVars* g = ucb_scratch(scratch, blockIdx.x, S).vars;
  if (threadIdx.x != 0 || g->fail) return;
  if (g->forehead_rule && g->v[FH_CNT] == 0) { g->fail = UCB_EMPTY_MASK; return; }
  if (3 * g->v[BROW_CNT] > 0 && g->v[FACE_CNT] == 0) { g->fail = UCB_EMPTY_MASK; return; }
  const double mid_nose_height = (g->v[NOSE_R1] + g->v[NOSE_R0]) / 2.0;
  const int upper_mouth = g->v[MOUTH_R0], lower_mouth = g->v[MOUTH_R1], left_mouth = g->v[MOUTH_C0], right_mouth = g->v[MOUTH_C1];
  py_slice((int)mid_nose_height, upper_mouth, S, g->r1a, g->r1b);
  py_slice(left_mouth, right_mouth, S, g->c1a, g->c1b);
  py_slice(upper_mouth, lower_mouth, S, g->r2a, g->r2b);
  py_slice(upper_mouth, S, S, g->below_lo, g->below_hi);
}

// stage 2: gate the magnitude around mustache and mouth (:473-499); stage 3: counts and the float32 sum for the "mouth and below" rules (:547-564)
__global__ __launch_bounds__(256) void ucb_s23_kernel(int S, void* scratch) {
#pragma clang fp contract(off)
  __shared__ int s_v[UCB_NVARS];
  __shared__ float s_f[256];
  const int item = blockIdx.y, tid = threadIdx.x, p = blockIdx.x * 256 + tid;
  const UcbScratch sc = ucb_scratch(scratch, item, S);
  const UcbItemVars* g = sc.vars;
  if (g->fail) return;
  wg_vars_begin<UcbVarRule>(s_v, tid);
  const float* w = sc.w + (size_t)p * kUcbCh;
  const int y = p / S, x = p % S;
  float mp = w[9] * w[10];
  const bool incol = x >= g->c1a && x < g->c1b;
  if (incol && y >= g->r1a && y < g->r1b && mp < 0.018f) mp = mp * 0.f;
  if (incol && y >= g->r2a && y < g->r2b && mp < 0.02f) mp = mp * 0.f;
  sc.mp[p] = mp;
  const float roi = (y >= g->below_lo && y < g->below_hi) ? w[11] : 0.f;
  const float shadowed = mp > 0.01f ? 1.f : 0.f;
  const unsigned long long m_roi = __ballot(roi != 0.f), m_sr = __ballot(roi != 0.f && shadowed != 0.f);
  if ((tid & 63) == 0) {
    if (m_roi) atomicAdd(&s_v[CNT_ROI], __popcll(m_roi));
    if (m_sr) { atomicAdd(&s_v[CNT_SR], __popcll(m_sr)); atomicAdd(&s_v[CNT_DEN], __popcll(m_sr)); }
  }
  const float a = roi * w[6] * shadowed, b = roi * w[7] * shadowed, c = roi * w[8] * shadowed;
  s_f[tid] = ((a + b) + c) / 3.f;                               // np.mean(roi * tmp * shadowed, 2)
  wg_vars_end<UcbVarRule>(s_v, sc.vars, tid);                            // (its barrier also publishes s_f)
  if (tid < 2) sc.leaf_f[blockIdx.x * 2 + tid] = ucb_leaf_sum<float>(s_f + 128 * tid);
}

__global__ __launch_bounds__(512) void ucb_a23_kernel(int S, void* scratch) {      // grid (B), 512 threads: the tree, then the scalars of stage 4
#pragma clang fp contract(off)
  __shared__ float s_tree[512];
  const int tid = threadIdx.x;
  const UcbScratch sc = ucb_scratch(scratch, blockIdx.x, S);
  UcbItemVars* g = sc.vars;
  if (g->fail) return;
  const float mean_num = ucb_tree_sum<float>(sc.leaf_f, S * S / 128, s_tree, tid, 512);
  if (tid != 0) return;
  const float frac = (float)(3 * g->v[CNT_SR]) / (float)(3 * g->v[CNT_ROI]);
  const float mean_below = mean_num / (float)g->v[CNT_DEN];
  // float32 comparisons, as the host statement's NumPy float32 scalars against Python floats under NumPy >= 2 (NEP 50).  Under NumPy 1.x
  // they would be float64 comparisons, which differ only where frac is exactly float32(0.252), float32(0.3) or float32(0.295) (or
  // mean_below float32(0.358) / float32(0.22)).  Kept as is; tests/ucb_edge_cases.py pins the float32 behaviour at those values.
  g->roi_off = ((0.252f < frac && frac < 0.268f) || (0.3f < frac && frac < 0.31f && mean_below > 0.358f) || (0.295f < frac && frac < 0.3f && mean_below > 0.22f)) ? 1 : 0;
  g->fr0 = g->fr1 = g->fc0 = g->fc1 = 0;
  if (g->forehead_rule) {
    py_slice(g->v[FH_R0] + 20, g->v[BROW_R0] - 40, S, g->fr0, g->fr1);
    py_slice(g->v[FH_C0] + 40, g->v[FH_C1] - 40, S, g->fc0, g->fc1);
  }
  g->left_rule = 0;
  g->left_hi = 0;
  if (3 * g->v[BROW_CNT] > 0) {
    const int left_face = g->v[FACE_C0], right_face = g->v[FACE_C1];
    if (g->v[BROW_C0] - left_face == 0) {
      g->left_rule = 1;
      int lo;
      py_slice(0, (int)(left_face * 0.8 + right_face * 0.2), S, lo, g->left_hi);
    }
  }
}

// stage 4: per-pixel threshold and detection (:501-590), union-find initialisation
__global__ __launch_bounds__(256) void ucb_s4_kernel(int S, void* scratch) {
#pragma clang fp contract(off)
  const int item = blockIdx.y, p = blockIdx.x * 256 + threadIdx.x;
  const UcbScratch sc = ucb_scratch(scratch, item, S);
  const UcbItemVars* g = sc.vars;
  if (g->fail) return;
  const float* w = sc.w + (size_t)p * kUcbCh;
  const int y = p / S, x = p % S;
  const float hair = w[10] - w[11];
  const float intensity = ((w[6] + w[7]) + w[8]) / 3.f;
  float thr = 0.01f;
  if (hair > 0.f) thr = 0.02f;
  if (hair > 0.f && intensity < 0.13f) thr = 0.004f;
  if (g->forehead_rule && y >= g->fr0 && y < g->fr1 && x >= g->fc0 && x < g->fc1 && intensity < 0.4f) thr = -0.001f;
  const float roi = (y >= g->below_lo && y < g->below_hi) ? w[11] : 0.f;
  if (g->roi_off && roi > 0.f) thr = 1.0f;
  if (g->left_rule && x < g->left_hi && w[14] > 0.f && intensity > 0.1f) thr = 1.0f;
  const bool det = sc.mp[p] > thr;
  sc.keep[p] = det ? 1 : 0;
  cc_seed(det, p, x, sc.label, sc.csize, sc.chair);
}

// stage 5: 4-connected components (:594-615): join the runs stage 4 labelled with their left and upper neighbours ...
__global__ __launch_bounds__(256) void ucb_s5a_kernel(int S, void* scratch) {
  const int item = blockIdx.y, p = blockIdx.x * 256 + threadIdx.x;
  const UcbScratch sc = ucb_scratch(scratch, item, S);
  if (sc.vars->fail) return;
  cc_join(sc.label, sc.keep, p, S);
}
// ... then sizes / hair sums at the roots
__global__ __launch_bounds__(256) void ucb_s5b_kernel(int S, void* scratch) {
  const int item = blockIdx.y, p = blockIdx.x * 256 + threadIdx.x;
  const UcbScratch sc = ucb_scratch(scratch, item, S);
  if (sc.vars->fail) return;
  const float* w = sc.w + (size_t)p * kUcbCh;
  cc_root_sums(sc.label, sc.csize, sc.chair, sc.keep[p] != 0, p, [&] { return (int)(w[10] - w[11]); });      // the rounded masks: -1, 0 or 1
}
__global__ __launch_bounds__(256) void ucb_s5c_kernel(int S, void* scratch) {       // the largest component
  __shared__ int s_v[UCB_NVARS];
  const int item = blockIdx.y, tid = threadIdx.x, p = blockIdx.x * 256 + tid;
  const UcbScratch sc = ucb_scratch(scratch, item, S);
  if (sc.vars->fail) return;
  cc_largest<UcbVarRule>(s_v, sc.vars, sc.label, sc.csize, sc.keep, p, tid);
}

// the keep filter (:603-615) and stage 6, part 1: the sums of the nose rule (:650-666)
__global__ __launch_bounds__(256) void ucb_s56_kernel(int S, void* scratch) {
#pragma clang fp contract(off)
  __shared__ int s_v[UCB_NVARS];
  __shared__ double s_d[256];
  const int item = blockIdx.y, tid = threadIdx.x, p = blockIdx.x * 256 + tid;
  const UcbScratch sc = ucb_scratch(scratch, item, S);
  if (sc.vars->fail) return;
  wg_vars_begin<UcbVarRule>(s_v, tid);
  const double min_size = 0.45 * (double)sc.vars->v[MAX_SIZE];
  unsigned char k = 0;
  if (sc.keep[p]) {
    const unsigned root = uf_load(sc.label + p);
    const unsigned sz = uf_load(sc.csize + root);
    if ((double)sz >= min_size && (double)uf_load(sc.chair + root) / (double)sz < 0.8) k = 1;
  }
  sc.keep[p] = k;                                               // only this thread reads keep[p] in this launch
  const float* w = sc.w + (size_t)p * kUcbCh;
  const float mean3 = ((w[6] + w[7]) + w[8]) / 3.f;            // np.mean(tmp, 2): float32
  const double sh = (double)k * (double)mean3;                 // keep is a float64 array in the host statement
  s_d[tid] = sh;
  const unsigned long long m_k = __ballot(k != 0), m_n = __ballot((double)w[13] * sh > 0.0);
  if ((tid & 63) == 0) {
    if (m_k) atomicAdd(&s_v[KEEP_CNT], __popcll(m_k));
    if (m_n) atomicAdd(&s_v[NOSE_SH], __popcll(m_n));
  }
  wg_vars_end<UcbVarRule>(s_v, sc.vars, tid);
  if (tid < 2) sc.leaf_d[blockIdx.x * 2 + tid] = ucb_leaf_sum<double>(s_d + 128 * tid);
}

__global__ __launch_bounds__(512) void ucb_a6_kernel(int S, void* scratch) {        // grid (B), 512 threads: the nose rule's verdict
#pragma clang fp contract(off)
  __shared__ double s_tree[512];
  const int tid = threadIdx.x;
  const UcbScratch sc = ucb_scratch(scratch, blockIdx.x, S);
  UcbItemVars* g = sc.vars;
  if (g->fail) return;
  const double sum_sh = ucb_tree_sum<double>(sc.leaf_d, S * S / 128, s_tree, tid, 512);
  if (tid != 0) return;
  const double mean_intensity = sum_sh / (double)g->v[KEEP_CNT];
  const double frac_nose = (double)g->v[NOSE_SH] / (double)(float)g->v[NOSE_CNT];
  g->nose_hit = 0;
  if ((0.15 < frac_nose && frac_nose < 0.25) || (0.30 < frac_nose && frac_nose < 0.31) || (0.34 < frac_nose && frac_nose < 0.35)) {
    const double mid_nose_height = (g->v[NOSE_R1] + g->v[NOSE_R0]) / 2.0, mid_nose_width = (g->v[NOSE_C1] + g->v[NOSE_C0]) / 2.0;
    const int reach = mean_intensity < 0.15 ? 5 : 65;
    g->nose_hit = 1;
    py_slice((int)mid_nose_height, (int)(double)(g->v[NOSE_R1] + reach), S, g->ra, g->rb);
    py_slice((int)(mid_nose_width - 35), (int)(mid_nose_width + 35), S, g->ca, g->cb);
  }
}

// stage 6, part 2 + stage 7: the nose rule applied, the composite (:711-722) and the seven figures (:744) as one uint8 strip (put_figure).
// losses: [B][2] = ssim, psnr (ssim_finish_kernel); strips: [B][S][7 S][3] uint8; figs: optional
// [B][7][S][S][3] float32; status: [B] (UCB_EMPTY_MASK where the host statement raises on an empty nose / mouth / forehead / face mask)
__global__ __launch_bounds__(256) void ucb_s7_kernel(int S, void* scratch, unsigned char* __restrict__ strips, float* __restrict__ figs, int* __restrict__ status) {
#pragma clang fp contract(off)
  const int item = blockIdx.y, p = blockIdx.x * 256 + threadIdx.x;
  const int N = S * S;
  const UcbScratch sc = ucb_scratch(scratch, item, S);
  const UcbItemVars* g = sc.vars;
  unsigned char* strip = strips + (size_t)item * N * kUcbFigs * 3;
  const int y = p / S, x = p % S;
  if (p == 0) status[item] = g->fail;
  if (g->fail) {                                                // a black strip; NaN losses are left to the finish kernel
    const float zero[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < kUcbFigs; ++k) put_figure<kUcbFigs>(strip, figs, S, item, k, y, x, zero);
    sc.out[(size_t)p * 3] = sc.out[(size_t)p * 3 + 1] = sc.out[(size_t)p * 3 + 2] = 0.f;
    return;
  }
  unsigned char keep = sc.keep[p];
  if (g->nose_hit && y >= g->ra && y < g->rb && x >= g->ca && x < g->cb) keep = 0;
  const float* w = sc.w + (size_t)p * kUcbCh;
  const float d = keep ? 1.f : 0.f;
  const float mp2 = sc.mp[p] * 2.f;
  float f[kUcbFigs][3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float tmp = w[6 + c], pred = w[3 + c];
    const float o = fminf(fmaxf(pred * d + tmp * (1.f - d), 0.f), 1.f);
    sc.out[(size_t)p * 3 + c] = o;
    f[0][c] = tmp; f[1][c] = o; f[2][c] = mp2; f[3][c] = w[c]; f[4][c] = d; f[5][c] = pred; f[6][c] = w[13] * tmp;
  }
#pragma unroll
  for (int k = 0; k < kUcbFigs; ++k) put_figure<kUcbFigs>(strip, figs, S, item, k, y, x, f[k]);
}

struct UcbGscSsimOperands {              // the GSC chain's operands: gt in channels 0-2 of the resized planes, the composite in `out`
  const float* w;
  const float* out;
  __device__ float x(size_t q, int c) const { return w[q * kUcbCh + c]; }
  __device__ float y(size_t q, int c) const { return out[q * 3 + c]; }
};

__global__ __launch_bounds__(256) void ucb_ssim_kernel(int S, void* scratch) {
  const UcbScratch sc = ucb_scratch(scratch, blockIdx.y, S);
  ucb_ssim_tile(UcbGscSsimOperands{sc.w, sc.out}, S, sc.ssim_part);
}

inline hipError_t launch_ucb_post(const float* rows10, const unsigned char* masks, const float* boxes, int B, int S, float* losses,
                                  unsigned char* strips, float* figs, int* status, void* scratch, hipStream_t stream) {
  const int N = S * S;
  hipLaunchKernelGGL(ucb_resize_kernel, dim3((unsigned)((N + 255) / 256), (unsigned)B), dim3(256), 0, stream, rows10, masks, boxes, S, scratch);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const dim3 px((unsigned)(N / 256), (unsigned)B), it((unsigned)B);
  hipLaunchKernelGGL(ucb_init_kernel, it, dim3(64), 0, stream, boxes, S, scratch);
  hipLaunchKernelGGL(ucb_s1_kernel, px, dim3(256), 0, stream, S, scratch);
  hipLaunchKernelGGL(ucb_a1_kernel, it, dim3(64), 0, stream, S, scratch);
  hipLaunchKernelGGL(ucb_s1b_kernel, px, dim3(256), 0, stream, S, scratch);
  hipLaunchKernelGGL(ucb_a1b_kernel, it, dim3(64), 0, stream, S, scratch);
  hipLaunchKernelGGL(ucb_s23_kernel, px, dim3(256), 0, stream, S, scratch);
  hipLaunchKernelGGL(ucb_a23_kernel, it, dim3(512), 0, stream, S, scratch);
  hipLaunchKernelGGL(ucb_s4_kernel, px, dim3(256), 0, stream, S, scratch);
  hipLaunchKernelGGL(ucb_s5a_kernel, px, dim3(256), 0, stream, S, scratch);
  hipLaunchKernelGGL(ucb_s5b_kernel, px, dim3(256), 0, stream, S, scratch);
  hipLaunchKernelGGL(ucb_s5c_kernel, px, dim3(256), 0, stream, S, scratch);
  hipLaunchKernelGGL(ucb_s56_kernel, px, dim3(256), 0, stream, S, scratch);
  hipLaunchKernelGGL(ucb_a6_kernel, it, dim3(512), 0, stream, S, scratch);
  hipLaunchKernelGGL(ucb_s7_kernel, px, dim3(256), 0, stream, S, scratch, strips, figs, status);
  return launch_ssim_tail(
      B, S, [&](dim3 grid, dim3 block) { hipLaunchKernelGGL(ucb_ssim_kernel, grid, block, 0, stream, S, scratch); },
      [&](dim3 grid, dim3 block) { hipLaunchKernelGGL(ssim_finish_kernel<UcbScratch>, grid, block, 0, stream, S, scratch, status, losses); });
}

}  // namespace bsr
