// libbsr_hip.so — host side of the MI355X-native GSC generator forward (C ABI in include/bsr_hip.h).
// Orchestrates Generator.call (/root/reference/model.py:228-290) as a fixed sequence of hand-written
// gfx950 kernels over one pre-planned NHWC workspace; concatenations are channel slices of shared buffers.
#include "../../include/bsr_hip.h"

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <initializer_list>
#include <string>
#include <type_traits>
#include <unordered_map>
#include <vector>

#include "attention.h"
#include "attention256.h"
#include "attention_h16.h"
#include "conv3_f16.h"
#include "conv_n16.h"
#include "gemm_nloop.h"
#include "glue_kernels.h"
#include "igemm_conv.h"
#include "igemm_h16.h"
#include "png_kernels.h"
#include "prep_kernels.h"
#include "prep_group_kernels.h"
#include "rgb_head.h"
#include "stem7.h"
#include "ucb_kernels.h"
#include "ucb_rgb_kernels.h"
#include "ucb_tsm_kernels.h"
#include "sfw_kernels.h"
#include "wino_conv2.h"
#include "wino_convt.h"
#include "wino_clr.h"
#include "wild_crop_kernels.h"
#include "wild_paste_kernels.h"
#include "shadow_synth_kernels.h"
#include "train_losses_kernels.h"
#include "disc_kernels.h"
#include "disc_grad_kernels.h"
#include "disc_wgrad_kernels.h"
#include "clr_tail_grad_kernels.h"
#include "clr_up_grad_kernels.h"
#include "grey_up_grad_kernels.h"
#include "nonlocal_grad_kernels.h"
#include "bottleneck_grad_kernels.h"
#include "colour_trunk_grad_kernels.h"
#include "heads_grad_kernels.h"
#include "vgg_kernels.h"
#include "vgg_grad_kernels.h"

namespace {

thread_local std::string g_last_error;

int fail(int code, const std::string& msg) {
  g_last_error = msg;
  return code;
}

#define HIP_TRY(expr)                                                                              \
  do {                                                                                             \
    hipError_t e__ = (expr);                                                                       \
    if (e__ != hipSuccess)                                                                         \
      return fail(BSR_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e__));                \
  } while (0)

// Every entry point runs on the handle's device and puts the caller's current device back on return.
struct DeviceGuard {
  int prev = -1;
  hipError_t err = hipSuccess;
  explicit DeviceGuard(int device) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != device) err = hipSetDevice(device);
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

// ---- the post-processing entry points (bsr_ucb_post*, bsr_sfw_score): one S check, one set of argument checks ----
bool post_size_ok(int B, int S) { return B > 0 && (S == 32 || S == 64 || S == 128 || S == 256); }

// `name`'s checks of its required pointers, B / S and the scratch alignment, all before the device switch; then `launch` (which returns
// a BSR_* code) on `device`.
template <class Launch>
int run_post(const char* name, std::initializer_list<const void*> required, int B, int S, const void* scratch, int device, Launch launch) {
  for (const void* p : required)
    if (p == nullptr) return fail(BSR_ERR_ARG, std::string(name) + ": null argument");
  if (!post_size_ok(B, S)) return fail(BSR_ERR_ARG, std::string(name) + ": B must be positive and S one of 32, 64, 128, 256 (reference: 256)");
  if (reinterpret_cast<uintptr_t>(scratch) % 256 != 0) return fail(BSR_ERR_ARG, std::string(name) + ": scratch must be 256-byte aligned");
  DeviceGuard guard(device);
  HIP_TRY(guard.err);
  return launch();
}

// ---- the generator backward's stage entry points (bsr_clr_tail_grad, bsr_clr_decoder_grad, bsr_nonlocal_grad): one order of checks ----
struct StageRule {
  bool ok;
  const char* text;
};
struct StageAligned {
  unsigned bytes;
  const char* names;      // as the text lists them: "<names> must be <bytes>-byte aligned"
  std::initializer_list<const void*> ptrs;
};

// `name`'s checks in this order, all before the device switch and none reading through a pointer: the required pointers, `rules` (the
// size rule, the blob's bytes, the pixel strides), the alignment groups, the scratch, `stop_after` against the chain's `launches`; then
// `launch` (which returns a BSR_* code) on `device`.
template <class Launch>
int run_grad_stage(const char* name, std::initializer_list<const void*> required, std::initializer_list<StageRule> rules,
                   std::initializer_list<StageAligned> aligned, const void* scratch, int stop_after, int launches, int device, Launch launch) {
  const std::string n(name);
  for (const void* p : required)
    if (p == nullptr) return fail(BSR_ERR_ARG, n + ": null argument");
  for (const StageRule& r : rules)
    if (!r.ok) return fail(BSR_ERR_ARG, n + ": " + r.text);
  for (const StageAligned& g : aligned)
    for (const void* p : g.ptrs)
      if (reinterpret_cast<uintptr_t>(p) % g.bytes != 0) return fail(BSR_ERR_ARG, n + ": " + g.names + " must be " + std::to_string(g.bytes) + "-byte aligned");
  if (reinterpret_cast<uintptr_t>(scratch) % 256 != 0) return fail(BSR_ERR_ARG, n + ": scratch must be 256-byte aligned");
  if (stop_after < 0 || stop_after > launches) return fail(BSR_ERR_ARG, n + ": stop_after must be 0.." + std::to_string(launches));
  DeviceGuard guard(device);
  HIP_TRY(guard.err);
  return launch();
}

// ---- packed-weight blob (written by blindshadowremoval_amd/pack.py) ----
constexpr uint32_t kBlobMagic = 0x57525342u;  // "BSRW"
constexpr uint32_t kBlobVersion = 1;
struct BlobHeader {
  uint32_t magic, version, n_entries, reserved;
};
struct BlobEntry {
  char name[40];
  uint64_t offset;   // bytes from blob start, 16-byte aligned
  uint64_t nfloats;
  int32_t dims[4];   // conv weights: {nchunk, taps, n_pad, CC+4}; bias: {n_pad,0,0,0}
};

struct LayerW {
  const float* w = nullptr;
  const float* b = nullptr;
  int nchunk = 0, taps = 0, n_pad = 0, ldp = 0;
};

enum KClass { K_CONV3 = 0, K_CONVT = 1, K_CONV1 = 2, K_ATT = 3, K_CONV7 = 4, K_GLUE = 5, K_CONVT_NI2 = 6 };

// Channel plan of a generator.  GSC (/root/reference/model.py:238,259): xa = cat[x 96 | uv 3], blocks 0-2 are 257 wide,
// xh = cat[x_hole 257 | bmask | uv 3].  TSM (/root/reference/model_with_TSM.py:272,293) inserts the ShareLayer output:
// xa = cat[x 96 | x_share 192 | uv 3] = 291, blocks 0-2 keep 291, xh = cat[x_hole 291 | bmask | x_share 582 | uv 3] = 877.
struct Variant {
  bool tsm, rgb;
  int c_a, cs_a, uv_a;        // res0 input: real channels, stride, uv slot
  int c_r, cs_r;              // blocks 0-2 output
  int c_h, cs_h, uv_h;        // blocks 3-5 input/output, uv slot
  // the GSC / TSM values of the rest; the single-stage RGB baseline (model_RGB.py) states its own
  int d = 128, nblk = 6;      // bottleneck width, number of blocks
  int cs_c3 = 128, cs_c2 = 160;   // c3 = [up2 | x2], c2 = [up1 | x3]: the skip concatenations are channel slices
  int cs_y3x = 288;           // y3x = conv3 output + block input, all 9 channel tiles kept (TSM inputs are wider than 257: model_with_TSM.py:105-113)
  int cs_y = 64, cs_qh = 16;  // the last decoder layer's output; the 7x1 head's (kx, co) partial sums
};
constexpr Variant kGSC{false, false, 99, 120, 96, 257, 264, 261, 264, 258};
// 16-bit matrix-core modes (BSR_DTYPE_F16 / BSR_DTYPE_F32X3): K chunks are 32 channels, so the 257 / 261-wide tensors get stride 288
constexpr Variant kGSC16{false, false, 99, 128, 96, 257, 288, 261, 288, 258};
constexpr Variant kTSM{true, false, 291, 312, 288, 291, 312, 877, 888, 874};
constexpr Variant kTSM16{true, false, 291, 320, 288, 291, 320, 877, 896, 874};   // TSM widths at the 16-bit kernels' 32-channel granularity
// RGB baseline (/root/reference/model_RGB.py:198-266): xa = cat[x 96 | uv 3] at stride 128, blocks 0-2 are 513 wide (stride 544); no
// blocks 3-5, no xh (c_h / cs_h / uv_h are 0).  c3 = [up2 128 | x2 64] (:252), c2 = [up1 192 | x3 64] (:251), y3x<i> = [y3 513 | 0] + pad(x)
constexpr Variant kRGB{false, true, 99, 128, 96, 513, 544, 0, 0, 0, 256, 3, 192, 256, 544, 128, 32};
constexpr int CS_Y3X = kGSC.cs_y3x;
constexpr int CS_CF = 64;    // f = clr_up3 output; the gs channel of cat[gs, f] (model.py:267) is read from the gs output
// the names the RGB forward reads its row by
constexpr int RGB_CS_R = kRGB.cs_r, RGB_CS_A = kRGB.cs_a, RGB_D = kRGB.d, RGB_CS_C3 = kRGB.cs_c3, RGB_CS_C2 = kRGB.cs_c2, RGB_CS_QH = kRGB.cs_qh;

struct Region {
  size_t off, floats;
};
// Float offsets into the workspace for a (B,H,W) problem; a slot the variant does not have is zero-sized.  qkv = theta | phi | g, d each
// (fp32 GSC / TSM: q' | t2 | g, with conv2 writing t2 there and the t2 slot unused; with t2 as the values too the rows are q' | t2 at
// stride 2 d in the same slot — forward_impl's res_block).
struct Plan {
  size_t x1, c3, c2, xa, t1, t2, y3[6], qkv, att[6], r[6], xh, ybuf, qh, f1, f2, cf, probe, reg32, share, yh, con, total;
  // A new shape moves every buffer.  All of them are fully rewritten by their producers each forward, pad channels included, except the
  // channel-pad lanes of the buffers listed here, which must read as exact zeros (they are the K pad of the 1x1 layers and feed the
  // residuals).  GSC / TSM: the 1/8-resolution concat buffers xa, xh, r0..r5 (real channels < stride); RGB: xa (channels 99-127).
  Region zero[8];
  int nzero;
};

Plan make_plan(size_t B, size_t H, size_t W, const Variant& v) {
  Plan p{};
  size_t off = 0;
  auto take = [&](size_t floats, bool keep_zero = false) {
    size_t o = off;
    off += (floats + 63) & ~size_t(63);
    if (keep_zero && floats != 0) p.zero[p.nzero++] = {o, floats};
    return o;
  };
  const size_t px = B * H * W, cells = px / 64;
  const size_t px2 = v.rgb ? 0 : px;      // GSC / TSM: the second stage (colour decoder, bmask probe)
  const size_t px1 = px - px2;            // RGB: the head's two 3-channel images (conv2's output, and the copy of con that bsr_probe reads)
  p.x1 = take(px * 32);
  p.c3 = take(px / 4 * v.cs_c3);
  p.c2 = take(px / 16 * v.cs_c2);
  p.xa = take(cells * v.cs_a, true);
  p.t1 = take(cells * v.d);
  p.t2 = take(cells * v.d);
  for (int i = 0; i < v.nblk; ++i) p.y3[i] = take(cells * v.cs_y3x);
  p.qkv = take(cells * 3 * v.d);
  for (int i = 0; i < v.nblk; ++i) p.att[i] = take(cells * v.d);
  for (int i = 0; i < v.nblk; ++i) p.r[i] = take(cells * (i < 3 ? v.cs_r : v.cs_h), !v.rgb);
  p.xh = take(cells * v.cs_h, true);
  p.ybuf = take(px * v.cs_y);
  p.qh = take(px * v.cs_qh);
  p.f1 = take(px2 / 16 * 128);
  p.f2 = take(px2 / 4 * 96);
  p.cf = take(px2 * CS_CF);
  p.probe = take(px2 / 64 * 2);
  p.reg32 = take(v.tsm ? cells * 4 : 0);
  p.share = take(v.tsm ? cells * 2 * v.c_r : 0);
  p.yh = take(px1 * 3);
  p.con = take(px1 * 3);
  p.total = off;
  return p;
}

}  // namespace

struct bsr_handle {
  int device = 0;
  float* d_blob = nullptr;
  float* d_wino = nullptr;       // fp32 GSC / TSM handles: the Winograd weight streams of res0..5.conv2 (wino_conv2.h), derived from the blob's direct images at bsr_create
  float* d_winot = nullptr;      // fp32 GSC handles: the 25-position weight streams of up2, up3 and clr_up3 (wino_convt.h), derived from the blob's direct images at bsr_create
  float* d_wclr = nullptr;       // fp32 GSC / TSM handles: clr_conv1's Winograd image U (wino_clr.h), derived from the blob's direct images ('clr_conv1', 'clr_conv1.gs') at bsr_create
  float* d_keys = nullptr;       // fp32 GSC / TSM handles: the res0..5.c3q images with theta composed onto phi, N = [y3 | q' | g] (keys_compose), derived from the blob's at bsr_create
  float* d_values = nullptr;     // fp32 GSC / TSM handles: per block the `w` image with g composed onto it, the c3q image of N = [y3 | q'] and the g image the att<i> probe
                                 // applies (values_compose), derived from the blob's at bsr_create
  float* att_scratch = nullptr;  // att<i> probes of a forward with conv2's output as the values: att = O Wg + bg is derived into this buffer
  size_t att_scratch_floats = 0;
  std::unordered_map<std::string, LayerW> layers;
  Variant var = kGSC;
  int dtype = BSR_DTYPE_F32;     // BSR_DTYPE_F16 / BSR_DTYPE_F32X3: 16-bit matrix cores on the 3x3 / stride-2 / transposed 3x3 layers (igemm_h16.h), fp32 kernels elsewhere
  float head_bias[2] = {0.f, 0.f};
  const float* tail_w = nullptr;
  const float* clr_gs_w = nullptr;
  float* ws = nullptr;
  size_t ws_floats = 0;
  Plan plan{};                   // of the last forward
  const float* rgb_tail_w = nullptr;   // RGB: conv3 (7x7, 3 -> 3) HWIO weights + bias, 444 floats
  const float* rgb_head_b = nullptr;   // RGB: conv2 bias, 3 floats
  int B = 0, H = 0, W = 0;       // shape of the last forward
  bool ran = false;
  bool att_in_lds = false;       // the last forward ran attention + `w` as ONE launch: the attention output never reached the att<i> workspace slots
  // Range guard of the 16-bit modes (igemm_h16.h): one word of pinned, device-mapped host memory; a kernel that stages an activation
  // outside the fp16 range stores 1 to it (over PCIe, only when it happens).  Sticky until bsr_check_range().
  unsigned* range_flag = nullptr;
  bool fuse_heads = true;        // env BSR_FUSE_HEADS=0: always the two-launch heads (A/B measurements, bit-identity tests)
  bool conv1_gemm = true;        // env BSR_CONV1_GEMM=0: res*.conv1 of the 16-bit modes on the implicit-GEMM kernel at every batch (A/B measurements, bit-identity tests)
  bool att_pv1 = false;          // f16 mode: P.V of the attention with the hi planes only (one matrix instruction per product instead of three).  Measured on
                                 // the f16 parity tests: margins 60 / 75 / 65 % of F16_TOL used against 64 / 69 / 75 % with the split product — the mode's
                                 // error is set by its fp16 activations, not by this — and 1.4 % of the forward (profiles/HISTORY.md round 6); f32x3 keeps the split
  bool conv3_f16 = true;         // env BSR_CONV3_F16=0: the f16 mode's 3x3 / transposed 3x3 layers on igemm_h16_kernel<.., NSPLIT = 1> (the form small test shapes
                                 // and A/B measurements compare against; same operands, another summation order)
  bool fuse_attw = true;         // env BSR_FUSE_ATTW=0: attention and the `w` GEMM as two launches (A/B measurements, bit-identity tests)
  bool wino_conv2 = true;        // env BSR_WINO_CONV2=0: the fp32 res*.conv2 on the direct implicit-GEMM kernel instead of the Winograd F(2x2, 3x3) one (A/B measurements, the two-forms test)
  bool wino_pairs = true;        // env BSR_WINO_PAIRS=0: full grids of the Winograd res*.conv2 on the 4-wave workgroup (one wave per SIMD) instead of the 8-wave one
                                 // (A/B measurements, the bit-identity test of the two shapes in a whole forward)
  bool wino_convt = true;        // env BSR_WINO_CONVT=0: the fp32 GSC up2 / up3 / clr_up3 on the direct implicit-GEMM kernel instead of the 25-product form of wino_convt.h
                                 // (A/B measurements, the two-forms test)
  bool wino_clr = true;          // env BSR_WINO_CLR=0: the fp32 colour tail (clr_conv1 + clr_conv2 + clr_conv3 + dif) on the direct conv_n16_kernel instead of the Winograd
                                 // F(2x2, 3x3) form of wino_clr.h (A/B measurements, the two-forms test)
  bool keys_conv2 = true;        // env BSR_KEYS_CONV2=0: the fp32 attention with phi projected by res*.c3q (N = 672, conv2's output in a buffer of its own) instead of conv2's
                                 // output as the keys (A/B measurements, the two-forms test)
  bool values_conv2 = true;      // env BSR_VALUES_CONV2=0 (read only while keys_conv2 is on): g projected by res*.c3q (N = 544) and the attention on [q' | t2 | g] rows instead
                                 // of conv2's output as the values too (A/B measurements, the two-forms test)
  bool att_is_o = false;         // the last forward ran with conv2's output as the values: the att<i> slots hold O = softmax(f) t2 (probe attv<i>)
  bool timing = false;
  std::vector<hipEvent_t> ev;    // event pool, pairs
  std::vector<int> ev_class;
  std::vector<std::string> ev_name;   // layer name of each event pair ("up3", "res2.conv2", "attention4", ...)
  size_t ev_used = 0;
};

namespace {

const char* const kRangeMsg =
    "an activation exceeded the fp16 range (|x| >= 65520) in a forward of this 16-bit-mode handle: its outputs are not trustworthy "
    "(inf / NaN where the fp32 path stays finite).  Re-run those inputs on a BSR_DTYPE_F32 handle; bsr_check_range() clears the condition";

// Winograd F(2x2, 3x3) filter transform U = G g G^T of a 128 -> 128 3x3 layer (Lavin & Gray 2016), in float64, rounded once:
// the layer's direct image [4 chunks][9 taps (a, b)][128 cout][32 + 4 channels] -> the stream of wino_conv2.h,
// [8 chunks][16 positions 4 xi + nu][128 cout][16 channels].  blindshadowremoval_amd/pack.py: pack_wino states the same in numpy.
constexpr size_t kWinoFloats = 8 * 16 * 128 * 16;
void wino_filter_transform(const float* direct, float* out) {
  static const double G[4][3] = {{1.0, 0.0, 0.0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0.0, 0.0, 1.0}};
  for (int k = 0; k < 128; ++k)
    for (int n = 0; n < 128; ++n) {
      double t[4][3];
      for (int x = 0; x < 4; ++x)
        for (int b = 0; b < 3; ++b) {
          double acc = 0.0;
          for (int a = 0; a < 3; ++a) acc += G[x][a] * (double)direct[((size_t)((k / 32) * 9 + a * 3 + b) * 128 + n) * 36 + k % 32];
          t[x][b] = acc;
        }
      for (int x = 0; x < 4; ++x)
        for (int y = 0; y < 4; ++y) {
          double acc = 0.0;
          for (int b = 0; b < 3; ++b) acc += t[x][b] * G[y][b];
          out[((size_t)((k / 16) * 16 + 4 * x + y) * 128 + n) * 16 + k % 16] = (float)acc;
        }
    }
}

// The 25-position filter transform U = G g G^T of a transposed 3x3 layer Cin -> 64 (wino_convt.h), G = rows (w1, w1, w2, w0 + w2, w0) of the
// taps, in float64, rounded once: the layer's direct image [ceil(cin / 32) chunks][9 taps (a, b)][64 cout][32 + 4 channels] -> the
// stream [cin / 16 chunks][25 positions 5 r + s][2 cout halves][2 K groups][64 lanes 32 h + n][4].
// blindshadowremoval_amd/pack.py: pack_wino_convt states the same in numpy.
constexpr int kWinoTLayers = 3;
const char* const kWinoTNames[kWinoTLayers] = {"up2", "up3", "clr_up3"};
constexpr int kWinoTCin[kWinoTLayers] = {160, 128, 96};
constexpr size_t wino_convt_floats(int cin) { return (size_t)(cin / 16) * 25 * 64 * 16; }
constexpr size_t wino_convt_offset(int layer) { return layer == 0 ? 0 : wino_convt_offset(layer - 1) + wino_convt_floats(kWinoTCin[layer - 1]); }
void wino_convt_filter_transform(const float* direct, float* out, int cin) {
  static const double G[5][3] = {{0.0, 1.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}, {1.0, 0.0, 1.0}, {1.0, 0.0, 0.0}};
  for (int k = 0; k < cin; ++k)
    for (int n = 0; n < 64; ++n) {
      double t[5][3];
      for (int x = 0; x < 5; ++x)
        for (int b = 0; b < 3; ++b) {
          double acc = 0.0;
          for (int a = 0; a < 3; ++a) acc += G[x][a] * (double)direct[((size_t)((k / 32) * 9 + a * 3 + b) * 64 + n) * 36 + k % 32];
          t[x][b] = acc;
        }
      const int kk = k % 16, g = kk / 8, hh = (kk % 8) / 4, j = kk % 4;
      for (int x = 0; x < 5; ++x)
        for (int y = 0; y < 5; ++y) {
          double acc = 0.0;
          for (int b = 0; b < 3; ++b) acc += t[x][b] * G[y][b];
          out[(((((size_t)(k / 16) * 25 + 5 * x + y) * 2 + n / 32) * 2 + g) * 64 + 32 * hh + n % 32) * 4 + j] = (float)acc;
        }
    }
}

// The Winograd F(2x2, 3x3) filter transform U = G g G^T of clr_conv1 (wino_clr.h), in float64, rounded once: the layer's direct image
// [2 chunks][9 taps (a, b)][16 cout][32 + 4 channels] and the gs channel's [16 cout][16 taps, 9 used] -> [16 positions 4 xi + nu][4 K groups g]
// [64 lanes 16 q + r][4 j] = channel 16 g + 4 q + j, cout r, then [16 positions][16 cout] of the gs channel.
// blindshadowremoval_amd/pack.py: pack_wino_clr states the same in numpy.
constexpr size_t kWinoClrFloats = bsr::WinoClrCfg::W_FLOATS;
void wino_clr_filter_transform(const float* direct, const float* w_gs, float* out) {
  static const double G[4][3] = {{1.0, 0.0, 0.0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0.0, 0.0, 1.0}};
  for (int k = 0; k < 65; ++k)      // k = 64: the gs channel
    for (int n = 0; n < 16; ++n) {
      double t[4][3];
      for (int x = 0; x < 4; ++x)
        for (int b = 0; b < 3; ++b) {
          double acc = 0.0;
          for (int a = 0; a < 3; ++a)
            acc += G[x][a] * (double)(k < 64 ? direct[((size_t)((k / 32) * 9 + a * 3 + b) * 16 + n) * 36 + k % 32] : w_gs[n * 16 + a * 3 + b]);
          t[x][b] = acc;
        }
      for (int x = 0; x < 4; ++x)
        for (int y = 0; y < 4; ++y) {
          double acc = 0.0;
          for (int b = 0; b < 3; ++b) acc += t[x][b] * G[y][b];
          const int pos = 4 * x + y;
          if (k < 64) out[((size_t)(pos * 4 + k / 16) * 64 + 16 * ((k % 16) / 4) + n) * 4 + k % 4] = (float)acc;
          else out[bsr::WinoClrCfg::U_FLOATS + pos * 16 + n] = (float)acc;
        }
    }
}

// res<i>.c3q with conv2's output t2 as the attention keys.  The block's logits are f_ij = theta_i . phi_j with theta = t2 Wq + bq and
// phi = t2 Wk + bk (model.py:33-53; Wq, Wk, bq, bk = columns 288..415 / 416..543 of the blob's conv3-composed c3q image), so
//   f_ij = (theta_i Wk^T) . t2_j + theta_i . bk,
// and the softmax over j removes the second term exactly.  With q'_i = t2_i (Wq Wk^T) + bq Wk^T — a 128 -> 128 affine map — the keys are
// t2 itself and the GEMM computes N = [y3 288 | q' 128 | g 128]: 17 channel tiles instead of 21.  Wq Wk^T and bq Wk^T in float64 from
// the image's float32 values, rounded once.  c3q = the blob's [4][1][768][36] image and [768] bias (HOST pointers) -> out_w
// [4][1][kKeysNPad][36] (two zero tiles of slack for the NI = 3 group reads), out_b [kKeysNPad].  blindshadowremoval_amd/pack.py:
// compose_keys_c3q states the same in numpy.
constexpr int kKeysN = 288 + 256, kKeysNPad = kKeysN + 64, kC3qNPad = 768;
constexpr size_t kKeysFloats = (size_t)4 * kKeysNPad * 36 + kKeysNPad;      // image, then bias
void keys_compose(const float* c3q_w, const float* c3q_b, float* out_w, float* out_b) {
  auto src = [&](int k, int n) -> const float& { return c3q_w[((size_t)(k / 32) * kC3qNPad + n) * 36 + k % 32]; };
  memset(out_w, 0, (size_t)4 * kKeysNPad * 36 * sizeof(float));
  memset(out_b, 0, kKeysNPad * sizeof(float));
  for (int ch = 0; ch < 4; ++ch) {
    memcpy(out_w + (size_t)ch * kKeysNPad * 36, c3q_w + (size_t)ch * kC3qNPad * 36, (size_t)288 * 36 * sizeof(float));                                  // y3
    memcpy(out_w + ((size_t)ch * kKeysNPad + 416) * 36, c3q_w + ((size_t)ch * kC3qNPad + 544) * 36, (size_t)128 * 36 * sizeof(float));      // g
  }
  memcpy(out_b, c3q_b, 288 * sizeof(float));
  memcpy(out_b + 416, c3q_b + 544, 128 * sizeof(float));
  for (int m = 0; m < 128; ++m) {                 // column m of Wq Wk^T: sum over the theta / phi channel c, in channel order
    for (int k = 0; k < 128; ++k) {
      double acc = 0.0;
      for (int c = 0; c < 128; ++c) acc += (double)src(k, 288 + c) * (double)src(m, 416 + c);
      out_w[((size_t)(k / 32) * kKeysNPad + 288 + m) * 36 + k % 32] = (float)acc;
    }
    double acc = 0.0;
    for (int c = 0; c < 128; ++c) acc += (double)c3q_b[288 + c] * (double)src(m, 416 + c);
    out_b[288 + m] = (float)acc;
  }
}

// conv2's output t2 as the attention VALUES as well.  g = t2 Wg + bg (Wg, bg = columns 544..671 of the c3q image) feeds the `w` conv with
// no non-linearity in between (model.py:53-56), and softmax rows sum to 1, so
//   softmax(f) g Ww + bw = (softmax(f) t2) (Wg Ww) + (bg Ww + bw):
// the attention runs on [q' | t2] rows with ONE tile as keys and values, c3q computes N = [y3 288 | q' 128] (13 channel tiles instead
// of 17), and the `w` GEMM keeps K = 128 with the composed image.  Sums over the g channel in channel order in float64 from the images'
// float32 values (the products are exact), rounded once.  c3q / w = the blob's [4][1][768][36] and [4][1][384][36] images with their
// biases (HOST pointers) -> out_w [4][1][384][36], out_b [384] in the layout of res<i>.w.  blindshadowremoval_amd/pack.py:
// compose_values_w states the same in numpy.
constexpr int kWNPad = 384;
constexpr int kValuesN = 288 + 128, kValuesNPad = kValuesN + 64;      // the c3q image of this form: the keys image without its g columns
constexpr int kGProbeNPad = 128 + 64;                                 // the g image of the att<i> probe: N = 128 + two zero tiles of slack (NI = 3)
constexpr size_t kValuesWFloats = (size_t)4 * kWNPad * 36 + kWNPad, kValuesC3qFloats = (size_t)4 * kValuesNPad * 36 + kValuesNPad,
                 kGProbeFloats = (size_t)4 * kGProbeNPad * 36 + kGProbeNPad;
constexpr size_t kValuesFloats = kValuesWFloats + kValuesC3qFloats + kGProbeFloats;      // per block: w image, bias | c3q image, bias | g image, bias
void values_compose(const float* c3q_w, const float* c3q_b, const float* w_w, const float* w_b, float* out_w, float* out_b) {
  auto wg = [&](int k, int c) -> double { return (double)c3q_w[((size_t)(k / 32) * kC3qNPad + 544 + c) * 36 + k % 32]; };
  auto ww = [&](int c, int n) -> double { return (double)w_w[((size_t)(c / 32) * kWNPad + n) * 36 + c % 32]; };
  memset(out_w, 0, (size_t)4 * kWNPad * 36 * sizeof(float));
  for (int n = 0; n < kWNPad; ++n) {
    for (int k = 0; k < 128; ++k) {
      double acc = 0.0;
      for (int c = 0; c < 128; ++c) acc += wg(k, c) * ww(c, n);
      out_w[((size_t)(k / 32) * kWNPad + n) * 36 + k % 32] = (float)acc;
    }
    double acc = (double)w_b[n];
    for (int c = 0; c < 128; ++c) acc += (double)c3q_b[544 + c] * ww(c, n);
    out_b[n] = (float)acc;
  }
}
// The two images that are cut, not computed: the keys image (keys_compose) without its g columns, and the blob's g columns alone.
void values_cut(const float* keys_w, const float* keys_b, const float* c3q_w, const float* c3q_b, float* v_w, float* v_b, float* g_w, float* g_b) {
  memset(v_w, 0, (size_t)4 * kValuesNPad * 36 * sizeof(float));
  memset(v_b, 0, kValuesNPad * sizeof(float));
  memset(g_w, 0, (size_t)4 * kGProbeNPad * 36 * sizeof(float));
  memset(g_b, 0, kGProbeNPad * sizeof(float));
  for (int ch = 0; ch < 4; ++ch) {
    memcpy(v_w + (size_t)ch * kValuesNPad * 36, keys_w + (size_t)ch * kKeysNPad * 36, (size_t)kValuesN * 36 * sizeof(float));
    memcpy(g_w + (size_t)ch * kGProbeNPad * 36, c3q_w + ((size_t)ch * kC3qNPad + 544) * 36, (size_t)128 * 36 * sizeof(float));
  }
  memcpy(v_b, keys_b, kValuesN * sizeof(float));
  memcpy(g_b, c3q_b + 544, 128 * sizeof(float));
}

int find_layer(bsr_handle* h, const char* name, int nchunk, int taps, int ldp, int n_min, LayerW* out) {
  auto it = h->layers.find(name);
  if (it == h->layers.end()) return fail(BSR_ERR_BLOB, std::string("blob has no layer '") + name + "'");
  const LayerW& l = it->second;
  if (l.w == nullptr || l.b == nullptr || l.nchunk != nchunk || l.taps != taps || l.ldp != ldp || l.n_pad < n_min) {
    char buf[256];
    snprintf(buf, sizeof buf, "layer '%s': blob has {chunks %d, taps %d, n_pad %d, ldp %d}, kernel needs {%d, %d, >=%d, %d}", name,
             l.nchunk, l.taps, l.n_pad, l.ldp, nchunk, taps, n_min, ldp);
    return fail(BSR_ERR_BLOB, buf);
  }
  *out = l;
  return BSR_OK;
}

// Run-time value -> template argument: f is a generic lambda, called once with the constants of the value.
template <int V>
using int_c = std::integral_constant<int, V>;
// The fp32-input kernels' two precision parameters.  prec: 0 = fp32 matrix instructions, 2 = fp16 ones (split precision in f32x3, and
// wherever the f16 mode does not take plain fp16 operands); half: the f16 mode's fp16 activation tensor on the kernel's other side.
template <class F>
void with_dtype(int dtype, F f) {
  if (dtype == BSR_DTYPE_F32) f(int_c<0>{}, std::false_type{});
  else if (dtype == BSR_DTYPE_F16) f(int_c<2>{}, std::true_type{});
  else f(int_c<2>{}, std::false_type{});
}
// io of the f16 mode's 3x3 layers: bit 0 = `in` is an fp16 tensor, bit 1 = `out` is written as fp16 (the fp16 activation pack of configs[3])
template <class F>
void with_io(int io, F f) {
  if (io == 3) f(int_c<3>{});
  else if (io == 2) f(int_c<2>{});
  else if (io == 1) f(int_c<1>{});
  else f(int_c<0>{});
}

bsr::WinoArgs wino_args(const float* in, float* out, const float* w, const float* bias, int H, int W, int out_cs = 128) {
  bsr::WinoArgs a{};
  a.in = in; a.out = out; a.w = w; a.bias = bias; a.H = H; a.W = W; a.in_cs = 128; a.out_cs = out_cs; a.act = 1;
  return a;
}

struct Launcher {
  bsr_handle* h;
  hipStream_t s;
  int rc = BSR_OK;

  void begin(int cls, const char* name) {
    if (!h->timing) return;
    if (h->ev_used + 2 > h->ev.size()) {
      for (int i = 0; i < 2; ++i) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return;
        h->ev.push_back(e);
      }
      h->ev_class.push_back(cls);
      h->ev_name.emplace_back();
    }
    h->ev_class[h->ev_used / 2] = cls;
    h->ev_name[h->ev_used / 2] = name;
    hipEventRecord(h->ev[h->ev_used], s);
  }
  void end() {
    if (!h->timing || h->ev_used + 2 > h->ev.size()) return;
    hipEventRecord(h->ev[h->ev_used + 1], s);
    h->ev_used += 2;
  }
  void check(hipError_t e, const char* what) {
    if (e != hipSuccess && rc == BSR_OK) rc = fail(BSR_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
  }

  // KH,KW,S,TR,TH,TW,WM,WN,MI,NI,CC,PF_IN
  // io: f16 mode only (with_io)
  template <int KH, int KW, int S, bool TR, int NI, int CC, int INB>
  void conv(int cls, const char* name, const float* in, int in_cs, int in_coff, int k_pad, int H, int W, float* out, int out_cs,
            int out_coff, int n_store, int act, int io = 0) {
    if (rc != BSR_OK) return;
    using C = bsr::ConvCfg<KH, KW, S, TR, 4, 32, 4, 1, 1, NI, CC, INB>;
    constexpr bool k33 = (KH == 3 && KW == 3);
    constexpr bool k11 = (KH == 1 && KW == 1);
    constexpr int CCH = CC == 24 ? 32 : CC;                       // K chunk of the 16-bit kernels (multiple of 16)
    const bool h16 = h->dtype != BSR_DTYPE_F32;
    // 16-bit modes: the 3x3-conv layers take fp16 operands (f16) or hi/lo planes (f32x3); the 1x1 layers are split-precision in both
    const int nsplit = (k33 && h->dtype == BSR_DTYPE_F16) ? 1 : 2;
    LayerW l;
    const int nb = (n_store + C::BN - 1) / C::BN;
    if (h16) {
      if (k_pad % CCH != 0) { rc = fail(BSR_ERR_ARG, std::string("layer '") + name + "': K is not a multiple of the 16-bit kernels' chunk"); return; }
      // words per weight row: padded rows, or the unpadded swizzled 128-byte rows of the DMA-fed f32x3 layers (H16Cfg::LDPW)
      const int ldpw = nsplit == 2 ? bsr::H16Cfg<KH, KW, S, TR, 4, 32, 4, 1, 1, NI, CCH, INB, 2>::LDPW : (CCH + 8) / 2;
      rc = find_layer(h, name, k_pad / CCH, KH * KW, ldpw, nb * C::BN, &l);
    } else {
      rc = find_layer(h, name, k_pad / CC, KH * KW, CC + 4, nb * C::BN, &l);
    }
    if (rc != BSR_OK) return;
    bsr::ConvArgs a{};
    a.in = in; a.in_cs = in_cs; a.in_coff = in_coff; a.H = H; a.W = W;
    a.out = out; a.out_cs = out_cs; a.out_coff = out_coff;
    a.Ho = TR ? 2 * H : (H + S - 1) / S;
    a.Wo = TR ? 2 * W : (W + S - 1) / S;
    a.w = l.w; a.bias = l.b; a.nchunk = l.nchunk; a.n_pad = l.n_pad; a.n_store = n_store;
    // TF SAME pad-before: total = max((out-1)*s + k - in, 0), before = total / 2
    auto pad_before = [](int in, int k, int s) {
      int o = (in + s - 1) / s, tot = (o - 1) * s + k - in;
      return tot > 0 ? tot / 2 : 0;
    };
    a.pad_t = pad_before(H, KH, S);
    a.pad_l = pad_before(W, KW, S);
    a.act = act;
    a.range_flag = h->range_flag;
    const int mh = TR ? H : a.Ho, mw = TR ? W : a.Wo;
    if (mh % 4 != 0 || mw % 32 != 0) {
      rc = fail(BSR_ERR_ARG, std::string("layer '") + name + "': feature map is not a multiple of the 4x32 tile");
      return;
    }
    // f16 mode, stride-1 3x3 and transposed 3x3: the trio-stepped kernel of conv3_f16.h from the layer's `w3` image (pack.py)
    if constexpr (k33 && S == 1) {
      if (h->dtype == BSR_DTYPE_F16 && h->conv3_f16) {
        char nm3[48];
        snprintf(nm3, sizeof nm3, "%s.w3", name);
        LayerW l3;
        const int nblk = (n_store + 63) / 64;
        rc = find_layer(h, nm3, nblk * (k_pad / 32), 9, 16, 64, &l3);
        if (rc != BSR_OK) return;
        a.w = l3.w; a.bias = l3.b; a.nchunk = k_pad / 32; a.n_pad = nblk * 64;
        begin(cls, name);
        with_io(io, [&](auto io_c) { check(bsr::launch_conv3_f16<TR, io_c.value>(a, h->B, s), name); });
        end();
        return;
      }
    }
    begin(cls, name);
    static_assert(k33 || k11, "igemm layers are 3x3 or 1x1");
    // Small batches (round 4): the 1/8-resolution trunk layers have B x 8 pixel tiles of 4x32 — fewer workgroups than CUs below
    // B = 16.  Their 2x32-pixel variant (two waves on the pixel rows x two on the channel halves, the same per-element accumulation
    // order: bit-identical) doubles the grid.
    constexpr bool kTrunk = !TR && S == 1 && NI == 2 && (CC == 32 || (k11 && CC == 24));
    bool half_tile = false;
    if constexpr (kTrunk) half_tile = !h16 && mh % 2 == 0 && (long long)(mh / 4) * (mw / 32) * h->B * nb < bsr::device_cu_count();
    if (half_tile) {
      if constexpr (kTrunk) check(bsr::launch_igemm_conv<KH, KW, S, TR, 2, 32, 2, 2, 1, 1, CC, INB>(a, h->B, s), name);
    } else if (!h16)
      check(bsr::launch_igemm_conv<KH, KW, S, TR, 4, 32, 4, 1, 1, NI, CC, INB>(a, h->B, s), name);
    else if (nsplit == 2)
      check(bsr::launch_igemm_h16<KH, KW, S, TR, 4, 32, 4, 1, 1, NI, CCH, INB, 2>(a, h->B, s), name);
    else if constexpr (k33)
      with_io(io, [&](auto io_c) { check(bsr::launch_igemm_h16<KH, KW, S, TR, 4, 32, 4, 1, 1, NI, CCH, INB, 1, io_c.value>(a, h->B, s), name); });
    end();
  }
  bsr::ConvArgs gemm_args(const LayerW& l, const float* in, int in_cs, float* out, int out_cs, int n_store, int act) const {
    bsr::ConvArgs a{};
    a.in = in; a.in_cs = in_cs; a.out = out; a.out_cs = out_cs;
    a.w = l.w; a.bias = l.b; a.nchunk = l.nchunk; a.n_pad = l.n_pad; a.n_store = n_store; a.act = act;
    a.range_flag = h->range_flag;
    return a;
  }
  // 1x1 conv as a resident-activation GEMM (K = NCH*32) over all N
  // MINW: waves per SIMD the kernel's register budget is sized for (gemm_nloop.h); 1 for the K = 256 GEMMs of the RGB bottleneck
  template <int NI, int NCH, int MINW = 2>
  void gemm(int cls, const char* name, const float* in, int in_cs, size_t pixels, float* out, int out_cs, int n_store, int act,
            const float* res1 = nullptr, int res1_cs = 0, int res1_c = 0,
            float* out2 = nullptr, int out2_cs = 0, int n_split = 0, int n_store1 = 0, const LayerW* image = nullptr, int out2_gap_at = 0,
            int out2_gap = 0) {      // image: a [NCH][1][n_pad][36] image of the handle's own in place of the blob's layer `name`
    if (rc != BSR_OK) return;
    using C = bsr::GemmNLoopCfg<NI, NCH>;
    LayerW l;
    const int tiles = (n_store + 31) / 32;
    // two workgroups per CU share the N range; small batches (fewer than 2 x CUs workgroups that way) split it further, down to one
    // channel group per range — every 32-channel tile is computed the same way whatever range it falls in (bit-identical)
    int kNSplit = 2;
    {
      const long long mblocks = (long long)(pixels / C::BM);
      const int want = (int)((2LL * bsr::device_cu_count() + mblocks - 1) / (mblocks > 0 ? mblocks : 1));
      const int most = (tiles + NI - 1) / NI;
      kNSplit = want < 2 ? 2 : (want > most ? most : want);
#ifdef BSR_NL_NSPLIT
      kNSplit = BSR_NL_NSPLIT > most ? most : BSR_NL_NSPLIT;
#endif
    }
    if (image == nullptr) rc = find_layer(h, name, NCH, 1, 36, (tiles + NI - 1) * 32, &l);   // the last group of a range may read (zero) rows past its tiles
    else if (image->nchunk == NCH && image->ldp == 36 && image->n_pad >= (tiles + NI - 1) * 32) l = *image;
    else rc = fail(BSR_ERR_ARG, std::string("layer '") + name + "': the handle's image does not fit the kernel");
    if (rc != BSR_OK) return;
    if (pixels % C::BM != 0) { rc = fail(BSR_ERR_ARG, std::string("layer '") + name + "': pixel count is not a multiple of 128"); return; }
    bsr::ConvArgs a = gemm_args(l, in, in_cs, out, out_cs, n_store, act);
    a.res1 = res1; a.res1_cs = res1_cs; a.res1_c = res1_c;
    a.out2 = out2; a.out2_cs = out2_cs; a.n_split = n_split; a.n_store1 = n_store1; a.out2_gap_at = out2_gap_at; a.out2_gap = out2_gap;
    a.out2_split = (h->dtype != BSR_DTYPE_F32 && out2 != nullptr) ? 1 : 0;      // conv3 | theta|phi|g of the 16-bit modes: qkv in the split layout of attention_h16.h
    begin(cls, name);
    if (h->dtype == BSR_DTYPE_F32)
      check(bsr::launch_gemm_nloop<NI, NCH, 0, MINW>(a, pixels, kNSplit, s), name);
    else if constexpr (MINW == 2)
      check(bsr::launch_gemm_nloop<NI, NCH, 2>(a, pixels, kNSplit, s), name);      // split-precision in both 16-bit modes
    else
      rc = fail(BSR_ERR_ARG, std::string("layer '") + name + "': the RGB bottleneck GEMMs are fp32 only");
    end();
  }
  // res*.conv1 (K = NCH*32 -> 128, + LeakyReLU) of the 16-bit modes, split precision: ONE workgroup per CU and all of N per workgroup
  // (gemm_nloop.h, MINW = 1, no N split).  forward_impl's conv1_gemm decides when it runs.
  template <int NCH>
  void gemm_all_n(const char* name, const float* in, size_t pixels, float* out) {
    if (rc != BSR_OK) return;
    LayerW l;
    rc = find_layer(h, name, NCH, 1, 36, 128, &l);
    if (rc != BSR_OK) return;
    begin(K_CONV1, name);
    check(bsr::launch_gemm_nloop<4, NCH, 2, 1>(gemm_args(l, in, NCH * 32, out, 128, 128, 1), pixels, 1, s), name);
    end();
  }

  // conv1 = Conv(32, 7x7) + BN + LeakyReLU (model.py:203,230; model_RGB.py:230): dedicated stem kernel (7 row taps x 21 contiguous floats).
  // Split precision in both 16-bit modes; f16 stores x1 as fp16.
  void stem(const float* in, int H, int W, float* out) {
    if (rc != BSR_OK) return;
    LayerW l;
    rc = find_layer(h, "conv1", 1, 7, h->dtype != BSR_DTYPE_F32 ? 36 : 28, 32, &l);
    if (rc != BSR_OK) return;
    bsr::StemArgs a{in, out, l.w, l.b, H, W, 0, 0, 0, h->range_flag};
    begin(K_CONV7, "conv1");
    with_dtype(h->dtype, [&](auto prec, auto half) { check(bsr::launch_stem7<4, prec.value, half.value>(a, h->B, s), "conv1"); });
    end();
  }

  // fp32 res<i>.conv2 (3x3, 128 -> 128, + BN + LeakyReLU) in Winograd F(2x2, 3x3) form (wino_conv2.h).  The blob's layer gives the bias;
  // the weights are the handle's transformed stream.
  void wino(const char* name, int i, const float* in, int H, int W, float* out, int out_cs = 128) {
    if (rc != BSR_OK) return;
    LayerW l;
    rc = find_layer(h, name, 4, 9, 36, 128, &l);
    if (rc != BSR_OK) return;
    if (H % 4 != 0 || W % 32 != 0) { rc = fail(BSR_ERR_ARG, std::string("layer '") + name + "': feature map is not a multiple of the 4x32 tile"); return; }
    begin(K_CONV3, name);
    check(bsr::launch_wino_conv2(wino_args(in, out, h->d_wino + (size_t)i * kWinoFloats, l.b, H, W, out_cs), h->B, s, 0, h->wino_pairs), name);
    end();
  }

  // fp32 GSC up2 / up3 / clr_up3 (ConvT 3x3 stride 2, Cin -> 64, + BN + LeakyReLU) in the 25-product form of wino_convt.h.  The blob's
  // layer gives the bias; the weights are the handle's transformed stream.  Same timing class and name as the direct kernel's launch.
  void winot(const char* name, int layer, const float* in, int in_cs, int H, int W, float* out, int out_cs) {
    if (rc != BSR_OK) return;
    const int cin = kWinoTCin[layer];
    LayerW l;
    rc = find_layer(h, name, cin / 32, 9, 36, 64, &l);
    if (rc != BSR_OK) return;
    if (const char* why = bsr::wino_convt_refusal(h->B, H, W, cin, 64, in_cs, out_cs)) { rc = fail(BSR_ERR_ARG, std::string("layer '") + name + "': " + why); return; }
    bsr::WinoTArgs a{};
    a.in = in; a.out = out; a.w = h->d_winot + wino_convt_offset(layer); a.bias = l.b; a.H = H; a.W = W;
    a.in_cs = in_cs; a.out_cs = out_cs; a.nchunk = cin / 16; a.act = 1;
    begin(K_CONVT_NI2, name);
    check(bsr::launch_wino_convt(a, h->B, s), name);
    end();
  }

  // RGB head conv2 (7x7, 128 -> 3) as a 7x1 implicit GEMM over N = (kx, co): rgb_head.h
  void conv71(const char* name, const float* in, int in_cs, int k_pad, int H, int W, float* out, int out_cs) {
    if (rc != BSR_OK) return;
    LayerW l;
    rc = find_layer(h, name, k_pad / 32, 7, 36, 32, &l);
    if (rc != BSR_OK) return;
    if (H % 4 != 0 || W % 32 != 0) { rc = fail(BSR_ERR_ARG, std::string("layer '") + name + "': image is not a multiple of the 4x32 tile"); return; }
    bsr::ConvArgs a{};
    a.in = in; a.in_cs = in_cs; a.in_coff = 0; a.H = H; a.W = W;
    a.out = out; a.out_cs = out_cs; a.out_coff = 0; a.Ho = H; a.Wo = W;
    a.w = l.w; a.bias = l.b; a.nchunk = l.nchunk; a.n_pad = l.n_pad; a.n_store = 32;
    a.pad_t = 3; a.pad_l = 0; a.act = 0;
    begin(K_CONV7, name);
    check(bsr::launch_igemm_conv<7, 1, 1, false, 4, 32, 4, 1, 1, 1, 32, 1>(a, h->B, s), name);
    end();
  }

  void heads(const float* y, int H, int W, float* qh, const float* inputs, float* gs, float* mask22, size_t npix) {
    if (rc != BSR_OK) return;
    LayerW l;
    rc = find_layer(h, "heads", 2, 7, 36, 16, &l);
    if (rc != BSR_OK) return;
    if (l.n_pad != 16) { rc = fail(BSR_ERR_BLOB, "layer 'heads' must be packed with n_pad 16"); return; }
    if (H % 8 != 0 || W % 32 != 0) { rc = fail(BSR_ERR_ARG, "layer 'heads': image is not a multiple of its tile"); return; }
    bsr::ConvN16Args a{};
    a.in = y; a.in_cs = 64; a.H = H; a.W = W; a.w = l.w; a.bias = l.b; a.out = qh; a.out_cs = 16; a.act = 0;
    a.pad_t = 3; a.pad_l = 0;
    a.inputs = inputs; a.gs_out = gs; a.mask22 = mask22; a.b_mask = h->head_bias[0]; a.b_con = h->head_bias[1];
    a.range_flag = h->range_flag;
    int resident = 0;
    check(bsr::launch_conv_n16<7, 1, false, false, 2, 0, false, true>(a, h->B, s, &resident), "heads");      // query: resident workgroup slots
    const bool fuse = rc == BSR_OK && h->fuse_heads && bsr::conv_n16_fuse_pays(h->B, H, 8, resident);
    begin(K_CONV7, "heads");
    with_dtype(h->dtype, [&](auto prec, auto half) {
      if (fuse) check(bsr::launch_conv_n16<7, 1, false, false, 2, prec.value, half.value, true>(a, h->B, s), "heads");
      else check(bsr::launch_conv_n16<7, 1, false, false, 2, prec.value, half.value>(a, h->B, s), "heads");
    });
    end();
    if (fuse) return;
    begin(K_GLUE, "heads_post");
    hipLaunchKernelGGL(bsr::heads_post_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, s, qh, inputs, h->head_bias[0], h->head_bias[1], gs,
                       mask22, W, npix);
    check(hipGetLastError(), "heads_post");
    end();
  }

  template <int KH, int KW, bool GS, bool TAIL, int RW>
  void conv16(int cls, const char* name, const float* in, int in_cs, int H, int W, float* out, int out_cs, int act, const float* gs,
              const float* inputs, float* con_rgb, float* dif, float* packed = nullptr) {
    if (rc != BSR_OK) return;
    LayerW l;
    rc = find_layer(h, name, 2, KH * KW, 36, 16, &l);
    if (rc != BSR_OK) return;
    if (l.n_pad != 16) { rc = fail(BSR_ERR_BLOB, std::string("layer '") + name + "' must be packed with n_pad 16"); return; }
    bsr::ConvN16Args a{};
    a.in = in; a.in_cs = in_cs; a.H = H; a.W = W; a.w = l.w; a.bias = l.b; a.out = out; a.out_cs = out_cs; a.act = act;
    a.pad_t = (KH - 1) / 2; a.pad_l = (KW - 1) / 2;
    a.gs = gs; a.w_gs = h->clr_gs_w; a.tail_w = h->tail_w; a.inputs = inputs; a.con_rgb = con_rgb; a.dif = dif; a.packed = packed;
    a.range_flag = h->range_flag;
    if (H % (4 * RW) != 0 || W % 32 != 0) { rc = fail(BSR_ERR_ARG, std::string("layer '") + name + "': image is not a multiple of its tile"); return; }
    // the fp32 colour tail in Winograd F(2x2, 3x3) form (wino_clr.h), at every batch and image size; BSR_WINO_CLR=0 keeps the direct kernel.
    // Same timing class and name as the direct kernel's launch.  The 16-bit modes and the heads keep conv_n16_kernel.
    if constexpr (KH == 3 && KW == 3 && GS && TAIL && RW == 2) {
      if (h->dtype == BSR_DTYPE_F32 && h->wino_clr && h->d_wclr != nullptr) {
        if (const char* why = bsr::wino_clr_refusal(h->B, H, W, in_cs)) { rc = fail(BSR_ERR_ARG, std::string("layer '") + name + "': " + why); return; }
        a.w = h->d_wclr;
        begin(cls, name);
        check(bsr::launch_wino_clr(a, h->B, s), name);
        end();
        return;
      }
    }
    begin(cls, name);
    with_dtype(h->dtype, [&](auto prec, auto half) { check(bsr::launch_conv_n16<KH, KW, GS, TAIL, RW, prec.value, half.value>(a, h->B, s), name); });
    end();
  }
};

// Make the workspace hold at least `floats`.  A new allocation holds arbitrary bits (NaN x zero weight = NaN): all of it is cleared once,
// and the handle forgets its last shape.  A forward waits for its own stream and clears on it; bsr_reserve (device_wide) waits for
// the whole device and returns with the clear done.
int grow_workspace(bsr_handle* h, size_t floats, bool device_wide, hipStream_t s) {
  if (floats <= h->ws_floats) return BSR_OK;
  if (device_wide) HIP_TRY(hipDeviceSynchronize());
  else HIP_TRY(hipStreamSynchronize(s));
  if (h->ws) HIP_TRY(hipFree(h->ws));
  h->ws = nullptr;
  h->ws_floats = 0;
  HIP_TRY(hipMalloc(reinterpret_cast<void**>(&h->ws), floats * sizeof(float)));
  h->ws_floats = floats;
  h->B = 0;
  h->ran = false;
  if (device_wide) HIP_TRY(hipMemset(h->ws, 0, floats * sizeof(float)));
  else HIP_TRY(hipMemsetAsync(h->ws, 0, floats * sizeof(float), s));
  return BSR_OK;
}

int ensure_workspace(bsr_handle* h, int B, int H, int W, hipStream_t s) {
  const Plan p = make_plan(B, H, W, h->var);
  const bool fresh = p.total > h->ws_floats;
  const int rc = grow_workspace(h, p.total, false, s);
  if (rc != BSR_OK) return rc;
  if (!fresh && (B != h->B || H != h->H || W != h->W)) {
    // a new shape in the old allocation: only the plan's pad-lane regions (a few MB per image instead of the whole workspace)
    for (int i = 0; i < p.nzero; ++i) HIP_TRY(hipMemsetAsync(h->ws + p.zero[i].off, 0, p.zero[i].floats * sizeof(float), s));
    h->ran = false;
  }
  h->plan = p;
  h->B = B; h->H = H; h->W = W;
  return BSR_OK;
}

// Records of a table that lies in device memory, read back for validation: the copy is ordered behind whatever `stream` still has to do
// to the blob (the upload of the table itself), and the host waits for it.
template <typename T>
int read_records(const unsigned char* blob, size_t off, int n, hipStream_t s, std::vector<T>* out) {
  out->resize((size_t)n);
  HIP_TRY(hipMemcpyAsync(out->data(), blob + off, (size_t)n * sizeof(T), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return BSR_OK;
}

}  // namespace

extern "C" {

int bsr_abi_version(void) { return 8; }

#ifndef BSR_SRC_SHA
#define BSR_SRC_SHA "unhashed"
#endif
// the tag makes the hash findable in the FILE (build.library_sha16 reads it without loading the library into the process)
static const char kSrcShaTag[] = "BSR_SRC_SHA=" BSR_SRC_SHA;
const char* bsr_source_sha(void) { return kSrcShaTag + 12; }

const char* bsr_last_error(void) { return g_last_error.c_str(); }

size_t bsr_workspace_bytes(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0) return 0;
  return make_plan(B, H, W, kGSC).total * sizeof(float);
}

int bsr_create(bsr_handle** out, int device, const void* packed_weights, size_t nbytes, int dtype) {
  if (out == nullptr || packed_weights == nullptr) return fail(BSR_ERR_ARG, "bsr_create: null argument");
  *out = nullptr;
  if (dtype != BSR_DTYPE_F32 && dtype != BSR_DTYPE_F16 && dtype != BSR_DTYPE_F32X3)
    return fail(BSR_ERR_ARG, "bsr_create: dtype must be BSR_DTYPE_F32, BSR_DTYPE_F16 or BSR_DTYPE_F32X3");
  if (nbytes < sizeof(BlobHeader)) return fail(BSR_ERR_BLOB, "bsr_create: blob shorter than its header");
  const uint8_t* blob = static_cast<const uint8_t*>(packed_weights);
  BlobHeader hd;
  memcpy(&hd, blob, sizeof hd);
  if (hd.magic != kBlobMagic || hd.version != kBlobVersion) return fail(BSR_ERR_BLOB, "bsr_create: bad blob magic/version");
  if ((int)hd.reserved != dtype) return fail(BSR_ERR_BLOB, "bsr_create: the blob was packed for another dtype (pack_generator(weights, dtype) must match bsr_create's dtype)");
  const size_t table_end = sizeof(BlobHeader) + (size_t)hd.n_entries * sizeof(BlobEntry);
  if (table_end > nbytes) return fail(BSR_ERR_BLOB, "bsr_create: blob entry table exceeds blob size");
  DeviceGuard guard(device);
  HIP_TRY(guard.err);
  bsr_handle* h = new bsr_handle();
  h->device = device;
  h->dtype = dtype;
  h->att_pv1 = dtype == BSR_DTYPE_F16;
  const struct { const char* env; bool* on; } switches[] = {{"BSR_FUSE_HEADS", &h->fuse_heads}, {"BSR_FUSE_ATTW", &h->fuse_attw}, {"BSR_CONV3_F16", &h->conv3_f16},
                                                            {"BSR_CONV1_GEMM", &h->conv1_gemm}, {"BSR_WINO_CONV2", &h->wino_conv2}, {"BSR_WINO_PAIRS", &h->wino_pairs}, {"BSR_WINO_CONVT", &h->wino_convt}, {"BSR_WINO_CLR", &h->wino_clr},
                                                            {"BSR_KEYS_CONV2", &h->keys_conv2}, {"BSR_VALUES_CONV2", &h->values_conv2}};
  for (const auto& sw : switches)
    if (const char* e_ = getenv(sw.env)) *sw.on = atoi(e_) != 0;
  hipError_t e = hipMalloc(reinterpret_cast<void**>(&h->d_blob), nbytes);
  if (e == hipSuccess) e = hipMemcpy(h->d_blob, blob, nbytes, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    if (h->d_blob) hipFree(h->d_blob);
    delete h;
    return fail(BSR_ERR_HIP, std::string("bsr_create: weight upload: ") + hipGetErrorString(e));
  }
  for (uint32_t i = 0; i < hd.n_entries; ++i) {
    BlobEntry en;
    memcpy(&en, blob + sizeof(BlobHeader) + (size_t)i * sizeof(BlobEntry), sizeof en);
    en.name[sizeof(en.name) - 1] = 0;
    if (en.offset % 16 != 0 || en.offset + en.nfloats * 4 > nbytes) {
      bsr_destroy(h);
      return fail(BSR_ERR_BLOB, std::string("bsr_create: entry '") + en.name + "' is out of bounds or misaligned");
    }
    std::string nm(en.name);
    const float* dptr = reinterpret_cast<const float*>(reinterpret_cast<const uint8_t*>(h->d_blob) + en.offset);
    if (nm == "heads.bias") {
      if (en.nfloats != 2) { bsr_destroy(h); return fail(BSR_ERR_BLOB, "bsr_create: heads.bias must hold 2 floats"); }
      memcpy(h->head_bias, blob + en.offset, 8);
    } else if (nm == "clr_conv1.gs") {
      if (en.nfloats != 256) { bsr_destroy(h); return fail(BSR_ERR_BLOB, "bsr_create: clr_conv1.gs must hold 16x16 floats"); }
      h->clr_gs_w = dptr;
    } else if (nm == "rgb.tail") {
      if (en.nfloats != 7 * 7 * 3 * 3 + 3) { bsr_destroy(h); return fail(BSR_ERR_BLOB, "bsr_create: rgb.tail must hold 7x7x3x3 + 3 floats"); }
      h->rgb_tail_w = dptr;
    } else if (nm == "rgb.head_bias") {
      if (en.nfloats != 3) { bsr_destroy(h); return fail(BSR_ERR_BLOB, "bsr_create: rgb.head_bias must hold 3 floats"); }
      h->rgb_head_b = dptr;
    } else if (nm == "tail.w") {
      if (en.nfloats != 16 * 16 + 16 + 48 + 3) { bsr_destroy(h); return fail(BSR_ERR_BLOB, "bsr_create: tail.w has the wrong size"); }
      h->tail_w = dptr;
    } else if (nm.size() > 2 && nm.compare(nm.size() - 2, 2, ".w") == 0) {
      LayerW& l = h->layers[nm.substr(0, nm.size() - 2)];
      l.w = dptr;
      l.nchunk = en.dims[0]; l.taps = en.dims[1]; l.n_pad = en.dims[2]; l.ldp = en.dims[3];
      if ((uint64_t)l.nchunk * l.taps * l.n_pad * l.ldp != en.nfloats) {
        bsr_destroy(h);
        return fail(BSR_ERR_BLOB, std::string("bsr_create: entry '") + en.name + "' dims do not match its size");
      }
    } else if (nm.size() > 2 && nm.compare(nm.size() - 2, 2, ".b") == 0) {
      h->layers[nm.substr(0, nm.size() - 2)].b = dptr;
    }
  }
  if (h->layers.count("rgb_head") != 0) {      // the RGB baseline (model_RGB.py): its 7x1 head layer exists in no other variant's blob
    if (dtype != BSR_DTYPE_F32) {
      bsr_destroy(h);
      return fail(BSR_ERR_ARG, "bsr_create: these are RGB-baseline weights (model_RGB.py), which run in BSR_DTYPE_F32 only: BSR_DTYPE_F32X3 and BSR_DTYPE_F16 are not provided for them");
    }
    if (h->rgb_tail_w == nullptr || h->rgb_head_b == nullptr) { bsr_destroy(h); return fail(BSR_ERR_BLOB, "bsr_create: RGB blob lacks 'rgb.tail' / 'rgb.head_bias'"); }
    h->var = kRGB;
    *out = h;
    return BSR_OK;
  }
  if (h->tail_w == nullptr || h->clr_gs_w == nullptr) { bsr_destroy(h); return fail(BSR_ERR_BLOB, "bsr_create: blob lacks 'tail.w' / 'clr_conv1.gs'"); }
  if (dtype != BSR_DTYPE_F32) {
    e = hipHostMalloc(reinterpret_cast<void**>(&h->range_flag), 64, hipHostMallocMapped);
    if (e != hipSuccess) { h->range_flag = nullptr; bsr_destroy(h); return fail(BSR_ERR_HIP, std::string("bsr_create: range flag: ") + hipGetErrorString(e)); }
    *h->range_flag = 0u;
  }
  {   // GSC or TSM weights?  (res0.conv1 has K = 120 -> 5 chunks of 24, or K = 312 -> 13)
    auto it = h->layers.find("res0.conv1");
    if (it == h->layers.end()) { bsr_destroy(h); return fail(BSR_ERR_BLOB, "bsr_create: blob has no 'res0.conv1'"); }
    // res0.conv1: GSC K = 120 (5 x 24) | 128 (4 x 32, 16-bit modes); TSM K = 312 (13 x 24) | 320 (10 x 32)
    const int nch = it->second.nchunk;
    if (dtype == BSR_DTYPE_F32) h->var = nch == 13 ? kTSM : kGSC;
    else h->var = nch == 10 ? kTSM16 : kGSC16;
  }
  if (dtype == BSR_DTYPE_F32) {      // the Winograd streams of res0..5.conv2, once per handle (kept whatever BSR_WINO_CONV2 says: 6 MB)
    std::vector<float> u(6 * kWinoFloats);
    for (int i = 0; i < 6; ++i) {
      char nm[32];
      snprintf(nm, sizeof nm, "res%d.conv2", i);
      LayerW l;
      if (find_layer(h, nm, 4, 9, 36, 128, &l) != BSR_OK || l.n_pad != 128) { bsr_destroy(h); return fail(BSR_ERR_BLOB, std::string("bsr_create: layer '") + nm + "' is not a [4][9][128][36] image"); }
      wino_filter_transform(reinterpret_cast<const float*>(blob + (reinterpret_cast<const uint8_t*>(l.w) - reinterpret_cast<const uint8_t*>(h->d_blob))), u.data() + i * kWinoFloats);
    }
    e = hipMalloc(reinterpret_cast<void**>(&h->d_wino), u.size() * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(h->d_wino, u.data(), u.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) { bsr_destroy(h); return fail(BSR_ERR_HIP, std::string("bsr_create: Winograd weights: ") + hipGetErrorString(e)); }
    if (!h->var.tsm) {      // GSC: the 25-position streams of up2, up3 and clr_up3, once per handle (kept whatever BSR_WINO_CONVT says: 2.4 MB)
      std::vector<float> ut(wino_convt_offset(kWinoTLayers));
      for (int i = 0; i < kWinoTLayers; ++i) {
        LayerW l;
        if (find_layer(h, kWinoTNames[i], kWinoTCin[i] / 32, 9, 36, 64, &l) != BSR_OK || l.n_pad != 64) { bsr_destroy(h); return fail(BSR_ERR_BLOB, std::string("bsr_create: layer '") + kWinoTNames[i] + "' is not a [Cin / 32][9][64][36] image"); }
        wino_convt_filter_transform(reinterpret_cast<const float*>(blob + (reinterpret_cast<const uint8_t*>(l.w) - reinterpret_cast<const uint8_t*>(h->d_blob))), ut.data() + wino_convt_offset(i), kWinoTCin[i]);
      }
      e = hipMalloc(reinterpret_cast<void**>(&h->d_winot), ut.size() * sizeof(float));
      if (e == hipSuccess) e = hipMemcpy(h->d_winot, ut.data(), ut.size() * sizeof(float), hipMemcpyHostToDevice);
      if (e != hipSuccess) { bsr_destroy(h); return fail(BSR_ERR_HIP, std::string("bsr_create: transposed-layer Winograd weights: ") + hipGetErrorString(e)); }
    }
    {   // clr_conv1's Winograd image, once per handle (kept whatever BSR_WINO_CLR says: 65 KB)
      LayerW l;
      if (find_layer(h, "clr_conv1", 2, 9, 36, 16, &l) != BSR_OK || l.n_pad != 16) { bsr_destroy(h); return fail(BSR_ERR_BLOB, "bsr_create: layer 'clr_conv1' is not a [2][9][16][36] image"); }
      std::vector<float> uc(kWinoClrFloats);
      auto host_of = [&](const float* dev) { return reinterpret_cast<const float*>(blob + (reinterpret_cast<const uint8_t*>(dev) - reinterpret_cast<const uint8_t*>(h->d_blob))); };
      wino_clr_filter_transform(host_of(l.w), host_of(h->clr_gs_w), uc.data());
      e = hipMalloc(reinterpret_cast<void**>(&h->d_wclr), uc.size() * sizeof(float));
      if (e == hipSuccess) e = hipMemcpy(h->d_wclr, uc.data(), uc.size() * sizeof(float), hipMemcpyHostToDevice);
      if (e != hipSuccess) { bsr_destroy(h); return fail(BSR_ERR_HIP, std::string("bsr_create: colour-tail Winograd weights: ") + hipGetErrorString(e)); }
    }
    // the res0..5.c3q images for conv2's output as the attention keys, once per handle (kept whatever BSR_KEYS_CONV2 says: 2 MB)
    std::vector<float> q(6 * kKeysFloats);
    auto host = [&](const float* dev) { return reinterpret_cast<const float*>(blob + (reinterpret_cast<const uint8_t*>(dev) - reinterpret_cast<const uint8_t*>(h->d_blob))); };
    for (int i = 0; i < 6; ++i) {
      char nm[32];
      snprintf(nm, sizeof nm, "res%d.c3q", i);
      LayerW l;
      if (find_layer(h, nm, 4, 1, 36, kC3qNPad, &l) != BSR_OK || l.n_pad != kC3qNPad) { bsr_destroy(h); return fail(BSR_ERR_BLOB, std::string("bsr_create: layer '") + nm + "' is not a [4][1][768][36] image"); }
      keys_compose(host(l.w), host(l.b), q.data() + i * kKeysFloats, q.data() + i * kKeysFloats + (size_t)4 * kKeysNPad * 36);
    }
    e = hipMalloc(reinterpret_cast<void**>(&h->d_keys), q.size() * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(h->d_keys, q.data(), q.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) { bsr_destroy(h); return fail(BSR_ERR_HIP, std::string("bsr_create: composed c3q weights: ") + hipGetErrorString(e)); }
    // the images for conv2's output as the attention values, once per handle (kept whatever BSR_VALUES_CONV2 says: 2.5 MB)
    std::vector<float> v(6 * kValuesFloats);
    for (int i = 0; i < 6; ++i) {
      char nm[32];
      LayerW l, lw;
      snprintf(nm, sizeof nm, "res%d.c3q", i);
      if (find_layer(h, nm, 4, 1, 36, kC3qNPad, &l) != BSR_OK) { bsr_destroy(h); return BSR_ERR_BLOB; }
      snprintf(nm, sizeof nm, "res%d.w", i);
      if (find_layer(h, nm, 4, 1, 36, kWNPad, &lw) != BSR_OK || lw.n_pad != kWNPad) { bsr_destroy(h); return fail(BSR_ERR_BLOB, std::string("bsr_create: layer '") + nm + "' is not a [4][1][384][36] image"); }
      float* vw = v.data() + i * kValuesFloats;
      float* vc = vw + kValuesWFloats;
      float* vg = vc + kValuesC3qFloats;
      const float* kq = q.data() + i * kKeysFloats;
      values_compose(host(l.w), host(l.b), host(lw.w), host(lw.b), vw, vw + (size_t)4 * kWNPad * 36);
      values_cut(kq, kq + (size_t)4 * kKeysNPad * 36, host(l.w), host(l.b), vc, vc + (size_t)4 * kValuesNPad * 36, vg, vg + (size_t)4 * kGProbeNPad * 36);
    }
    e = hipMalloc(reinterpret_cast<void**>(&h->d_values), v.size() * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(h->d_values, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) { bsr_destroy(h); return fail(BSR_ERR_HIP, std::string("bsr_create: composed w weights: ") + hipGetErrorString(e)); }
  }
  *out = h;
  return BSR_OK;
}

void bsr_destroy(bsr_handle* h) {
  if (h == nullptr) return;
  DeviceGuard guard(h->device);
  for (hipEvent_t e : h->ev) hipEventDestroy(e);
  if (h->ws) hipFree(h->ws);
  if (h->d_blob) hipFree(h->d_blob);
  if (h->d_wino) hipFree(h->d_wino);
  if (h->d_winot) hipFree(h->d_winot);
  if (h->d_wclr) hipFree(h->d_wclr);
  if (h->d_keys) hipFree(h->d_keys);
  if (h->d_values) hipFree(h->d_values);
  if (h->att_scratch) hipFree(h->att_scratch);
  if (h->range_flag) hipHostFree(h->range_flag);
  delete h;
}

int bsr_reserve(bsr_handle* h, int B, int H, int W) {
  if (h == nullptr || B <= 0 || H <= 0 || W <= 0) return fail(BSR_ERR_ARG, "bsr_reserve: bad argument");
  DeviceGuard guard(h->device);
  HIP_TRY(guard.err);
  return grow_workspace(h, make_plan(B, H, W, h->var).total, true, nullptr);
}

int bsr_check_range(bsr_handle* h, void* stream) {
  if (h == nullptr) return fail(BSR_ERR_ARG, "bsr_check_range: null handle");
  if (h->range_flag == nullptr) return BSR_OK;                 // BSR_DTYPE_F32: nothing is ever converted to fp16
  DeviceGuard guard(h->device);
  HIP_TRY(guard.err);
  HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
  // read-and-clear in ONE atomic exchange: a report raised by another stream's forward between a separate read and clear would be
  // lost (one stream per handle remains the rule — bsr_hip.h — but the flag itself no longer depends on it)
  if (__atomic_exchange_n(h->range_flag, 0u, __ATOMIC_SEQ_CST) == 0u) return BSR_OK;
  return fail(BSR_ERR_RANGE, kRangeMsg);
}

int bsr_peek_range(bsr_handle* h) {
  if (h == nullptr) return fail(BSR_ERR_ARG, "bsr_peek_range: null handle");
  if (h->range_flag == nullptr) return BSR_OK;
  // no synchronisation, no clear: the word lives in host memory the kernels write over PCIe; what it says covers every forward that
  // has COMPLETED so far (the caller waited for an event of the one it asks about)
  if (__atomic_load_n(h->range_flag, __ATOMIC_SEQ_CST) == 0u) return BSR_OK;
  return fail(BSR_ERR_RANGE, kRangeMsg);
}

int bsr_set_timing(bsr_handle* h, int enable) {
  if (h == nullptr) return fail(BSR_ERR_ARG, "bsr_set_timing: null handle");
  h->timing = enable != 0;
  h->ev_used = 0;
  return BSR_OK;
}

int bsr_get_timing(bsr_handle* h, float ms[BSR_NUM_CLASSES], int launches[BSR_NUM_CLASSES]) {
  if (h == nullptr || ms == nullptr || launches == nullptr) return fail(BSR_ERR_ARG, "bsr_get_timing: null argument");
  for (int i = 0; i < BSR_NUM_CLASSES; ++i) { ms[i] = 0.f; launches[i] = 0; }
  for (size_t i = 0; i + 1 < h->ev_used; i += 2) {
    HIP_TRY(hipEventSynchronize(h->ev[i + 1]));
    float t = 0.f;
    HIP_TRY(hipEventElapsedTime(&t, h->ev[i], h->ev[i + 1]));
    const int c = h->ev_class[i / 2];
    ms[c] += t;
    launches[c] += 1;
  }
  return BSR_OK;
}

int bsr_timing_launches(bsr_handle* h) { return h == nullptr ? 0 : (int)(h->ev_used / 2); }

int bsr_timing_entry(bsr_handle* h, int i, char* name, size_t name_cap, float* ms, int* cls) {
  if (h == nullptr || name == nullptr || ms == nullptr || cls == nullptr || name_cap == 0) return fail(BSR_ERR_ARG, "bsr_timing_entry: null argument");
  if (i < 0 || (size_t)(2 * i + 1) >= h->ev_used) return fail(BSR_ERR_ARG, "bsr_timing_entry: index out of range");
  HIP_TRY(hipEventSynchronize(h->ev[2 * i + 1]));
  HIP_TRY(hipEventElapsedTime(ms, h->ev[2 * i], h->ev[2 * i + 1]));
  *cls = h->ev_class[i];
  snprintf(name, name_cap, "%s", h->ev_name[i].c_str());
  return BSR_OK;
}

size_t bsr_handle_workspace_bytes(const bsr_handle* h, int B, int H, int W) {
  if (h == nullptr || B <= 0 || H <= 0 || W <= 0) return 0;
  return make_plan(B, H, W, h->var).total * sizeof(float);
}

// The forwards' image-size check, before anything is enqueued.  The entry point's name is part of each literal.  (For these H and W
// multiples the token multiple always holds: (H/8)(W/8) = 128 (H/32)(W/256); it is stated because the attention kernels rely on it.)
static int check_image_size(int H, int W, const char* hw_text, const char* token_text) {
  if (H <= 0 || W <= 0 || H % 32 != 0 || W % 256 != 0) return fail(BSR_ERR_ARG, hw_text);
  if (((H / 8) * (W / 8)) % 128 != 0) return fail(BSR_ERR_ARG, token_text);
  return BSR_OK;
}
#define BSR_CHECK_IMAGE_SIZE(entry, H, W)                                                                                          \
  check_image_size(H, W, entry ": H must be a multiple of 32 and W a multiple of 256 (reference: 256x256)",                         \
                   entry ": (H/8)*(W/8) must be a multiple of 128")

static int forward_impl(bsr_handle* h, const float* inputs, const float* uv, const float* reg, int frame, int share, int B, int H, int W,
                        float* gs, float* con_rgb, float* mask22, float* dif, void* stream, float* packed = nullptr) {
  if (h == nullptr || inputs == nullptr || uv == nullptr || gs == nullptr || mask22 == nullptr || (packed == nullptr && (con_rgb == nullptr || dif == nullptr)))
    return fail(BSR_ERR_ARG, "bsr_forward: null argument");
  if (B <= 0) return fail(BSR_ERR_ARG, "bsr_forward: B must be positive");
  const Variant& V = h->var;
  if (V.rgb)
    return fail(BSR_ERR_ARG, reg != nullptr ? "bsr_forward_tsm: this handle holds RGB-baseline weights: call bsr_forward_rgb"
                                            : "bsr_forward: this handle holds RGB-baseline weights: call bsr_forward_rgb");
  if (V.tsm != (reg != nullptr))
    return fail(BSR_ERR_ARG, V.tsm ? "bsr_forward: this handle holds TSM weights: call bsr_forward_tsm" : "bsr_forward_tsm: this handle holds GSC weights: call bsr_forward");
  if (V.tsm && (frame <= 0 || B % frame != 0 || H != W))
    return fail(BSR_ERR_ARG, "bsr_forward_tsm: B must be a multiple of frame and the image square (warp.py assumes a square map)");
  int rc = BSR_CHECK_IMAGE_SIZE("bsr_forward", H, W);
  if (rc != BSR_OK) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (h->range_flag != nullptr && *reinterpret_cast<volatile unsigned*>(h->range_flag) != 0u)
    return fail(BSR_ERR_RANGE, kRangeMsg);      // an earlier forward overflowed fp16: sticky until bsr_check_range() acknowledges it
  DeviceGuard guard(h->device);
  HIP_TRY(guard.err);
  rc = ensure_workspace(h, B, H, W, s);
  if (rc != BSR_OK) return rc;
  h->ev_used = 0;
  const Plan& p = h->plan;
  float* ws = h->ws;
  const size_t npix = (size_t)B * H * W, ncell = npix / 64;
  const int H2 = H / 2, W2 = W / 2, H4 = H / 4, W4 = W / 4, H8 = H / 8, W8 = W / 8;
  Launcher L{h, s};
  auto glue_begin = [&](const char* what) { L.begin(K_GLUE, what); };
  auto glue_end = [&](const char* what) { L.check(hipGetLastError(), what); L.end(); };

  L.stem(inputs, H, W, ws + p.x1);
  // down1..3 = Conv(stride 2) (model.py:207-209,231-233); x2 / x3 land in their skip-concat slots (model.py:244-245)
  // f16 mode (the fp16 pack of BASELINE configs[3]): the full- / half- / quarter-resolution tensors between the 3x3-conv layers —
  // x1, c3 = [up2 | x2], c2 = [up1 | x3], y, f1, f2, f — live in HBM as fp16 (same workspace slots, first half used); the
  // 1/8-resolution trunk (xa, t1, t2, r*, y3x, qkv, att) and the four outputs stay fp32.  IO16: 1 = fp16 input, 2 = fp16 output.
  const bool p16 = h->dtype == BSR_DTYPE_F16;
  const int io_both = p16 ? 3 : 0, io_in = p16 ? 1 : 0, io_out = p16 ? 2 : 0;
  L.conv<3, 3, 2, false, 2, 16, 1>(K_CONV3, "down1", ws + p.x1, 32, 0, 32, H, W, ws + p.c3, 128, 64, 64, 1, io_both);
  L.conv<3, 3, 2, false, 2, 16, 1>(K_CONV3, "down2", ws + p.c3, 128, 64, 64, H2, W2, ws + p.c2, 160, 96, 64, 1, io_both);
  L.conv<3, 3, 2, false, 3, 16, 1>(K_CONV3, "down3", ws + p.c2, 160, 96, 64, H4, W4, ws + p.xa, V.cs_a, 0, 96, 1, io_in);
  // uv = resize(uv, [h,w]); x = cat[x, uv] (model.py:237-238) and the uv slot of cat[x_hole, bmask, uv] (model.py:259)
  glue_begin("uv_resize8");
  hipLaunchKernelGGL(bsr::uv_resize8_kernel, dim3((unsigned)((ncell * 3 + 255) / 256)), dim3(256), 0, s, uv, H, W, ws + p.xa, V.cs_a, V.uv_a,
                     ws + p.xh, V.cs_h, V.uv_h, ncell);
  glue_end("uv_resize8");

  // TSM: x_share = ShareLayer(x, reg, frame, share) into channels [96, 288) of xa (model_with_TSM.py:271-272)
  auto share_layer = [&](const float* x, int x_cs, int C, float* out, int out_cs, int out_coff) {
    glue_begin("share_layer");
    if (share) hipLaunchKernelGGL(bsr::share_reduce_kernel, dim3((unsigned)(ncell / frame)), dim3(128), 0, s, x, x_cs, C, ws + p.reg32, H8, frame, ws + p.share);
    hipLaunchKernelGGL(bsr::share_unwarp_kernel, dim3((unsigned)ncell), dim3(128), 0, s, ws + p.share, x, x_cs, C, ws + p.reg32, H8, frame, share, out, out_cs, out_coff);
    glue_end("share_layer");
  };
  if (V.tsm) {
    glue_begin("reg_resize8");
    hipLaunchKernelGGL(bsr::reg_resize8_kernel, dim3((unsigned)((ncell * 4 + 255) / 256)), dim3(256), 0, s, reg, H, W, ws + p.reg32, ncell);
    glue_end("reg_resize8");
    share_layer(ws + p.xa, V.cs_a, 96, ws + p.xa, V.cs_a, 96);
  }

  // res*.conv1 (1x1, 99|257|261 -> 128, + BN + LeakyReLU) at full batches: the resident-activation GEMM with ONE workgroup per CU and
  // all of N per workgroup (gemm_nloop.h, MINW = 1) — same operands, same matrix-instruction order per output element as the
  // implicit-GEMM kernels (igemm_h16_kernel<1,1,1,..,NSPLIT = 2> / igemm_conv_kernel<1,1,1,..,CC = 24>): the same bits
  auto conv1_gemm = [&](const char* nm, const float* x, int x_cs) -> bool {
    if (V.tsm || !h->conv1_gemm || L.rc != BSR_OK) return false;
    if (h->dtype == BSR_DTYPE_F32) return false;      // fp32: the implicit-GEMM kernel (the resident form over 24-channel chunks was built and is no faster: profiles/HISTORY.md round 5)
    if (ncell % 128 != 0 || (long long)(ncell / 128) * 2 < bsr::device_cu_count()) return false;
    if (x_cs != 128 && x_cs != 288) return false;
    if (x_cs == 128) L.gemm_all_n<4>(nm, x, ncell, ws + p.t1);
    else L.gemm_all_n<9>(nm, x, ncell, ws + p.t1);
    return true;
  };

  // ResBottleneck + NonLocalBlock (model.py:98-113, 23-61)
  auto res_block = [&](int i, const float* x, int x_cs, int x_c) {
    float* r_out = ws + p.r[i];
    const int o_cs = i < 3 ? V.cs_r : V.cs_h;
    char nm[32];
    float* y3 = ws + p.y3[i];
    snprintf(nm, sizeof nm, "res%d.conv1", i);
    if (!conv1_gemm(nm, x, x_cs)) L.conv<1, 1, 1, false, 2, 24, 3>(K_CONV1, nm, x, x_cs, 0, x_cs, H8, W8, ws + p.t1, 128, 0, 128, 1);
    // conv3+BN (128 -> 257 = y3) and theta|phi|g (257 -> 3x128, no activation in between: model.py:101,33-46) are ONE
    // K = 128 GEMM: the qkv weights are composed offline with conv3's (pack.py), N = [y3 288 | qkv 384].  The y3 output also absorbs
    // the block's skip: y3x = y3 + pad(x), so that the `w` GEMM below reads ONE residual.
    // (The two as ONE launch — the conv2 tile through LDS into a GEMM tail — was built in round 4, bit-identical and no faster: profiles/HISTORY.md;
    // sources at git e99927a.)
    // fp32: conv2 in Winograd F(2x2, 3x3) form (wino_conv2.h: 2.25x fewer matrix instructions), at EVERY batch and image size, so that
    // an image gets the same bits in any batch; BSR_WINO_CONV2=0 keeps the direct kernel.  The 16-bit modes keep theirs.
    // fp32: conv2's output t2 IS the attention's key tensor (keys_compose: theta composed onto phi, exact under the softmax), so conv2
    // writes it into the key slot of the qkv rows, [q' | t2 | g] at stride 384, and c3q — N = [y3 288 | q' 128 | g 128], 17 channel tiles
    // instead of 21 — reads its A operand from there and writes q' and g around it: no workgroup of that launch writes the key
    // columns, so the in-place form has no read-after-write hazard.  The attention kernels see the layout they always had.
    // BSR_KEYS_CONV2=0 keeps phi projected (N = 672, t2 in a buffer of its own); the 16-bit modes have that form only.
    // t2 is the attention's VALUE tensor as well (values_compose: g composed onto `w`): the rows are [q' | t2] at stride 256, c3q computes
    // N = [y3 288 | q' 128] — 13 channel tiles — and writes q' in front of its own A operand (no gap to skip), the attention kernels run
    // their one-tile form (KV1) and the `w` GEMM, fused or not, takes the composed image.  BSR_VALUES_CONV2=0 keeps g projected.
    const bool keys = h->dtype == BSR_DTYPE_F32 && h->keys_conv2;
    const bool values = keys && h->values_conv2;
    h->att_is_o = values;
    float* t2_row = keys ? ws + p.qkv : ws + p.t2;
    const int t2_cs = values ? 256 : keys ? 384 : 128, t2_coff = keys ? 128 : 0;
    const float* vimg = h->d_values + (size_t)i * kValuesFloats;
    const LayerW lvw{vimg, vimg + (size_t)4 * kWNPad * 36, 4, 1, kWNPad, 36};
    float* t2 = t2_row + t2_coff;
    snprintf(nm, sizeof nm, "res%d.conv2", i);
    if (h->dtype == BSR_DTYPE_F32 && h->wino_conv2) L.wino(nm, i, ws + p.t1, H8, W8, t2, t2_cs);
    else L.conv<3, 3, 1, false, 2, 32, 1>(K_CONV3, nm, ws + p.t1, 128, 0, 128, H8, W8, t2_row, t2_cs, t2_coff, 128, 1);
    snprintf(nm, sizeof nm, "res%d.c3q", i);
    if (values) {
      const float* img = vimg + kValuesWFloats;
      const LayerW lv{img, img + (size_t)4 * kValuesNPad * 36, 4, 1, kValuesNPad, 36};
      L.gemm<3, 4>(K_CONV1, nm, t2, t2_cs, ncell, y3, CS_Y3X, kValuesN, 0, x, x_cs, x_cs < 288 ? x_cs : 288, ws + p.qkv, 256, 288, CS_Y3X, &lv);
    } else if (keys) {
      const float* img = h->d_keys + (size_t)i * kKeysFloats;
      const LayerW lk{img, img + (size_t)4 * kKeysNPad * 36, 4, 1, kKeysNPad, 36};
      L.gemm<3, 4>(K_CONV1, nm, t2, t2_cs, ncell, y3, CS_Y3X, kKeysN, 0, x, x_cs, x_cs < 288 ? x_cs : 288, ws + p.qkv, 384, 288, CS_Y3X, &lk, 128, 128);
    } else {
      L.gemm<3, 4>(K_CONV1, nm, t2, t2_cs, ncell, y3, CS_Y3X, 288 + 384, 0, x, x_cs, x_cs < 288 ? x_cs : 288, ws + p.qkv, 384, 288, CS_Y3X);
    }
    // z = y3 + BN(w(att)); out = LeakyReLU(pad(x) + pad(z))  (model.py:56-59, 105-113) = LeakyReLU(y3x + BN(w(att))).
    // ONE launch — the `w` GEMM runs as the tail of the attention kernel on the workgroup's own 128 pixels (attention.h /
    // attention_h16.h, FUSEW; the attention output never goes to HBM).  fp32 small batches (the 4- / 2-wave attention shapes) keep the
    // two launches; on the fp32 path both forms give the same bits (tests/test_gpu_parity.py).
    // 16-bit modes: the one-wave-per-SIMD kernel of attention_h16.h (round 6), whose normalised O^T accumulators are the tail's A operand, at
    // every batch (that kernel has one workgroup shape).  There the two forms sum in different orders and agree to a tolerance, not to the
    // bit, and f16 runs P.V on the hi planes only (att_pv1); tests/test_stage_parity_gpu.py holds both forms to per-stage fp64 budgets.
    const bool h16 = h->dtype != BSR_DTYPE_F32;
    const bool fuse_w = h->fuse_attw && (h16 || bsr::attention_auto_qw(B, H8 * W8) == 4);
    h->att_in_lds = fuse_w;
    if (fuse_w && L.rc == BSR_OK) {
      LayerW l;
      // fp32: the [4][1][n_pad][36] image gemm_tail.h streams through its ring; 16-bit modes (round 6): the `w4` image of
      // attention_h16.h — nine 16-KB tiles in the k order of the O^T accumulators, resident in LDS when the key loop ends
      snprintf(nm, sizeof nm, h16 ? "res%d.w4" : "res%d.w", i);
      L.rc = h16 ? find_layer(h, nm, 9, 1, 128, 32, &l) : find_layer(h, nm, 4, 1, 36, 12 * 32, &l);
      if (values) l = lvw;
      if (L.rc == BSR_OK) {
        bsr::AttWArgs wa{};
        wa.w = l.w; wa.bias = l.b; wa.n_pad = h16 ? 288 : l.n_pad;
        wa.res = y3; wa.res_cs = CS_Y3X; wa.res_c = CS_Y3X;
        wa.out = r_out; wa.out_cs = o_cs; wa.n_store = o_cs < 288 ? o_cs : 288; wa.n_store1 = wa.n_store; wa.act = 1; wa.stagger = 1;
        snprintf(nm, sizeof nm, "res%d.attw", i);
        L.begin(K_ATT, nm);
        if (values)
          L.check(bsr::launch_nonlocal_attention_w<true>(ws + p.qkv, B, H8 * W8, wa, s), "attention+w");
        else if (!h16)
          L.check(bsr::launch_nonlocal_attention_w(ws + p.qkv, B, H8 * W8, wa, s), "attention+w");
        else
          L.check(bsr::launch_nonlocal_attention_h16_w(ws + p.qkv, B, H8 * W8, wa, s, h->att_pv1), "attention_h16+w");
        L.end();
      }
    } else {
      if (L.rc == BSR_OK) {
        snprintf(nm, sizeof nm, "res%d.attention", i);
        L.begin(K_ATT, nm);
        if (values)
          L.check(bsr::launch_nonlocal_attention<true>(ws + p.qkv, ws + p.att[i], B, H8 * W8, s), "attention");
        else if (!h16)
          L.check(bsr::launch_nonlocal_attention(ws + p.qkv, ws + p.att[i], B, H8 * W8, s), "attention");
        else
          L.check(bsr::launch_nonlocal_attention_h16(ws + p.qkv, ws + p.att[i], B, H8 * W8, s, h->att_pv1), "attention_h16");
        L.end();
      }
      snprintf(nm, sizeof nm, "res%d.w", i);
      L.gemm<3, 4>(K_CONV1, nm, ws + p.att[i], 128, ncell, r_out, o_cs, o_cs < 288 ? o_cs : 288, 1, y3, CS_Y3X, CS_Y3X, nullptr, 0, 0, 0, values ? &lvw : nullptr);
    }
    if (x_c > 288 && L.rc == BSR_OK) {      // the block output keeps the wider of x / y (model.py:105-113): channels the GEMM does not cover
      glue_begin("lrelu_copy");
      hipLaunchKernelGGL(bsr::lrelu_copy_kernel, dim3((unsigned)((ncell * (x_c - 288) + 255) / 256)), dim3(256), 0, s, x, x_cs, r_out, o_cs, 288, x_c, ncell);
      glue_end("lrelu_copy");
    }
  };
  res_block(0, ws + p.xa, V.cs_a, V.c_a);
  res_block(1, ws + p.r[0], V.cs_r, V.c_r);
  res_block(2, ws + p.r[1], V.cs_r, V.c_r);

  // greyscale decoder: up1..3 = ConvT (model.py:243-245)
  L.conv<3, 3, 1, true, 1, 24, 1>(K_CONVT, "up1", ws + p.r[2], V.cs_r, 0, V.cs_r, H8, W8, ws + p.c2, 160, 0, 96, 1, io_out);
  // fp32 GSC: up2, up3 and clr_up3 in the 25-product form of wino_convt.h, at EVERY batch and image size (an image gets the same bits in
  // any batch); BSR_WINO_CONVT=0 keeps the direct kernel.  TSM handles and the 16-bit modes keep theirs.
  const bool winot = h->dtype == BSR_DTYPE_F32 && !V.tsm && h->wino_convt && h->d_winot != nullptr;
  if (winot) {
    L.winot("up2", 0, ws + p.c2, 160, H4, W4, ws + p.c3, 128);
    L.winot("up3", 1, ws + p.c3, 128, H2, W2, ws + p.ybuf, 64);
  } else {
    L.conv<3, 3, 1, true, 2, 32, 1>(K_CONVT_NI2, "up2", ws + p.c2, 160, 0, 160, H4, W4, ws + p.c3, 128, 0, 64, 1, io_both);
    L.conv<3, 3, 1, true, 2, 32, 1>(K_CONVT_NI2, "up3", ws + p.c3, 128, 0, 128, H2, W2, ws + p.ybuf, 64, 0, 64, 1, io_both);
  }
  // heads conv2 (mask) / conv3 (con): 7x7, 64 -> 1 each (model.py:246-247) as one 7x1 MFMA conv with N = (kx, head); the 7 horizontal
  // taps + tanh / gs / mask22 (model.py:246-252) either inside the same kernel (row-strip workgroups, when the batch has enough
  // strips to fill the chip) or by heads_post_kernel from the qh scratch tensor — bit-identical results either way
  L.heads(ws + p.ybuf, H, W, ws + p.qh, inputs, gs, mask22, npix);
  // bmask / x_hole (model.py:256-259)
  glue_begin("bmask_xhole");
  hipLaunchKernelGGL(bsr::bmask_xhole_kernel, dim3((unsigned)ncell), dim3(64), 0, s, gs, inputs, H, W, ws + p.r[2], V.cs_r, V.c_r, ws + p.xh,
                     V.cs_h, ws + p.probe);
  glue_end("bmask_xhole");
  if (V.tsm) share_layer(ws + p.xh, V.cs_h, V.c_r, ws + p.xh, V.cs_h, V.c_r + 1);    // model_with_TSM.py:292-293

  res_block(3, ws + p.xh, V.cs_h, V.c_h);
  res_block(4, ws + p.r[3], V.cs_h, V.c_h);
  res_block(5, ws + p.r[4], V.cs_h, V.c_h);

  // colour decoder (model.py:264-269)
  L.conv<3, 3, 1, true, 2, 24, 1>(K_CONVT, "clr_up1", ws + p.r[5], V.cs_h, 0, V.cs_h, H8, W8, ws + p.f1, 128, 0, 128, 1, io_out);
  L.conv<3, 3, 1, true, 1, 32, 1>(K_CONVT, "clr_up2", ws + p.f1, 128, 0, 128, H4, W4, ws + p.f2, 96, 0, 96, 1, io_both);
  if (winot) L.winot("clr_up3", 2, ws + p.f2, 96, H2, W2, ws + p.cf, CS_CF);
  else L.conv<3, 3, 1, true, 2, 32, 1>(K_CONVT_NI2, "clr_up3", ws + p.f2, 96, 0, 96, H2, W2, ws + p.cf, CS_CF, 0, 64, 1, io_both);
  // clr_conv1 (3x3 over cat[gs, f]) + clr_conv2 + clr_conv3 + dif, one kernel (model.py:267-269,288)
  L.conv16<3, 3, true, true, 2>(K_CONV3, "clr_conv1", ws + p.cf, CS_CF, H, W, nullptr, 0, 1, gs, inputs, con_rgb, dif, packed);
  if (L.rc == BSR_OK) h->ran = true;
  return L.rc;
}

// The RGB baseline's Generator.call (/root/reference/model_RGB.py:228-266): stem, down1-3, uv concat, three 513-wide ResBottlenecks,
// up1-3, conv2 (7x7 -> 3), conv3 (7x7 -> 3).  fp32 only (bsr_create refuses other dtypes for these weights).
int bsr_forward_rgb(bsr_handle* h, const float* inputs, const float* uv, int B, int H, int W, float* con, void* stream) {
  if (h == nullptr || inputs == nullptr || uv == nullptr || con == nullptr) return fail(BSR_ERR_ARG, "bsr_forward_rgb: null argument");
  if (!h->var.rgb)
    return fail(BSR_ERR_ARG, h->var.tsm ? "bsr_forward_rgb: this handle holds TSM weights: call bsr_forward_tsm"
                                        : "bsr_forward_rgb: this handle holds GSC weights: call bsr_forward");
  if (B <= 0) return fail(BSR_ERR_ARG, "bsr_forward_rgb: B must be positive");
  int rc = BSR_CHECK_IMAGE_SIZE("bsr_forward_rgb", H, W);
  if (rc != BSR_OK) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  DeviceGuard guard(h->device);
  HIP_TRY(guard.err);
  rc = ensure_workspace(h, B, H, W, s);
  if (rc != BSR_OK) return rc;
  h->ev_used = 0;
  h->att_in_lds = false;
  const Plan& p = h->plan;
  float* ws = h->ws;
  const size_t npix = (size_t)B * H * W, ncell = npix / 64;
  const int H2 = H / 2, W2 = W / 2, H4 = H / 4, W4 = W / 4, H8 = H / 8, W8 = W / 8;
  Launcher L{h, s};
  auto glue_begin = [&](const char* what) { L.begin(K_GLUE, what); };
  auto glue_end = [&](const char* what) { L.check(hipGetLastError(), what); L.end(); };

  L.stem(inputs, H, W, ws + p.x1);      // conv1 (model_RGB.py:230): the GSC stem kernel
  // down1..3 (:231-233); x2 / x3 land in their skip-concat slots (:251-252)
  L.conv<3, 3, 2, false, 2, 16, 1>(K_CONV3, "down1", ws + p.x1, 32, 0, 32, H, W, ws + p.c3, RGB_CS_C3, 128, 64, 1);
  L.conv<3, 3, 2, false, 2, 16, 1>(K_CONV3, "down2", ws + p.c3, RGB_CS_C3, 128, 64, H2, W2, ws + p.c2, RGB_CS_C2, 192, 64, 1);
  L.conv<3, 3, 2, false, 3, 16, 1>(K_CONV3, "down3", ws + p.c2, RGB_CS_C2, 192, 64, H4, W4, ws + p.xa, RGB_CS_A, 0, 96, 1);
  // uv = resize(uv, [h, w]); x = cat[x, uv] (:237-238)
  glue_begin("uv_resize8");
  hipLaunchKernelGGL(bsr::uv_resize8_kernel, dim3((unsigned)((ncell * 3 + 255) / 256)), dim3(256), 0, s, uv, H, W, ws + p.xa, RGB_CS_A, 96,
                     ws + p.xa, RGB_CS_A, 96, ncell);
  glue_end("uv_resize8");

  // ResBottleneck(513) + NonLocalBlock(513) (model.py:81-113, 6-61), blocks 0-2 only (:239-240)
  auto res_block = [&](int i, const float* x, int x_cs) {
    char nm[32];
    float* y3 = ws + p.y3[i];
    snprintf(nm, sizeof nm, "res%d.conv1", i);
    L.conv<1, 1, 1, false, 2, 32, 3>(K_CONV1, nm, x, x_cs, 0, x_cs, H8, W8, ws + p.t1, RGB_D, 0, RGB_D, 1);
    snprintf(nm, sizeof nm, "res%d.conv2", i);
    L.conv<3, 3, 1, false, 2, 32, 1>(K_CONV3, nm, ws + p.t1, RGB_D, 0, RGB_D, H8, W8, ws + p.t2, RGB_D, 0, RGB_D, 1);
    // conv3 + BN (256 -> 513) and theta | phi | g (513 -> 3 x 256) composed offline into ONE K = 256 GEMM (pack.py), N = [y3 544 | qkv 768];
    // y3x = y3 + pad(x) absorbs the block's skip, so that the `w` GEMM reads one residual
    snprintf(nm, sizeof nm, "res%d.c3q", i);
    L.gemm<3, 8, 1>(K_CONV1, nm, ws + p.t2, RGB_D, ncell, y3, RGB_CS_R, RGB_CS_R + 3 * RGB_D, 0, x, x_cs, x_cs, ws + p.qkv, 3 * RGB_D, RGB_CS_R,
                    RGB_CS_R);
    if (L.rc == BSR_OK) {
      snprintf(nm, sizeof nm, "res%d.attention", i);
      L.begin(K_ATT, nm);
      L.check(bsr::launch_nonlocal_attention256(ws + p.qkv, ws + p.att[i], B, H8 * W8, s), "attention256");
      L.end();
    }
    // out = LeakyReLU(y3x + BN(w(att)))  (model.py:56-59, 105-113); pad channels 513-543 come out 0 (zero weights, bias, residual)
    snprintf(nm, sizeof nm, "res%d.w", i);
    L.gemm<3, 8, 1>(K_CONV1, nm, ws + p.att[i], RGB_D, ncell, ws + p.r[i], RGB_CS_R, RGB_CS_R, 1, y3, RGB_CS_R, RGB_CS_R);
  };
  res_block(0, ws + p.xa, RGB_CS_A);
  res_block(1, ws + p.r[0], RGB_CS_R);
  res_block(2, ws + p.r[1], RGB_CS_R);

  // up1..3 = ConvT (:250-252)
  L.conv<3, 3, 1, true, 2, 32, 1>(K_CONVT, "up1", ws + p.r[2], RGB_CS_R, 0, RGB_CS_R, H8, W8, ws + p.c2, RGB_CS_C2, 0, 192, 1);
  L.conv<3, 3, 1, true, 2, 32, 1>(K_CONVT_NI2, "up2", ws + p.c2, RGB_CS_C2, 0, RGB_CS_C2, H4, W4, ws + p.c3, RGB_CS_C3, 0, 128, 1);
  L.conv<3, 3, 1, true, 2, 32, 1>(K_CONVT_NI2, "up3", ws + p.c3, RGB_CS_C3, 0, RGB_CS_C3, H2, W2, ws + p.ybuf, 128, 0, 128, 1);
  // conv2 (:253): 7x1 matrix-core pass, then the seven horizontal taps + bias
  L.conv71("rgb_head", ws + p.ybuf, 128, 128, H, W, ws + p.qh, RGB_CS_QH);
  if (L.rc == BSR_OK) {
    glue_begin("rgb_hsum");
    hipLaunchKernelGGL(bsr::rgb_hsum_kernel, dim3((unsigned)((npix * 3 + 255) / 256)), dim3(256), 0, s, ws + p.qh, RGB_CS_QH, h->rgb_head_b, W,
                       ws + p.yh, npix);
    glue_end("rgb_hsum");
    // conv3 (:254) -> con, and the workspace copy bsr_probe("con") reads
    L.begin(K_CONV7, "rgb_tail");
    L.check(bsr::launch_rgb_conv7(ws + p.yh, h->rgb_tail_w, B, H, W, con, ws + p.con, s), "rgb_tail");
    L.end();
  }
  if (L.rc == BSR_OK) h->ran = true;
  return L.rc;
}

int bsr_forward(bsr_handle* h, const float* inputs, const float* uv, int B, int H, int W, float* gs, float* con_rgb, float* mask22,
                float* dif, void* stream) {
  return forward_impl(h, inputs, uv, nullptr, 1, 0, B, H, W, gs, con_rgb, mask22, dif, stream);
}

int bsr_forward_packed(bsr_handle* h, const float* inputs, const float* uv, int B, int H, int W, float* gs, float* con_rgb_dif, float* mask22,
                       void* stream) {
  if (con_rgb_dif == nullptr) return fail(BSR_ERR_ARG, "bsr_forward_packed: null con_rgb_dif");
  return forward_impl(h, inputs, uv, nullptr, 1, 0, B, H, W, gs, nullptr, mask22, nullptr, stream, con_rgb_dif);
}

int bsr_forward_tsm(bsr_handle* h, const float* inputs, const float* uv, const float* reg, int B, int H, int W, int frame, int share,
                    float* gs, float* con_rgb, float* mask22, float* dif, void* stream) {
  if (reg == nullptr) return fail(BSR_ERR_ARG, "bsr_forward_tsm: null reg");
  return forward_impl(h, inputs, uv, reg, frame, share != 0, B, H, W, gs, con_rgb, mask22, dif, stream);
}

int bsr_prep_rows(int device, const void* d_blob, size_t blob_bytes, size_t rows_off, size_t grid_off, int B, int S, float* out, float* hull_tmp,
                  void* stream) {
  if (d_blob == nullptr || out == nullptr || hull_tmp == nullptr) return fail(BSR_ERR_ARG, "bsr_prep_rows: null argument");
  if (B <= 0 || S <= 0 || (S * S) % 256 != 0) return fail(BSR_ERR_ARG, "bsr_prep_rows: B must be positive and S*S a multiple of 256");
  if (rows_off % 8 != 0 || grid_off % 8 != 0) return fail(BSR_ERR_ARG, "bsr_prep_rows: table offsets must be 8-byte aligned");
  // the two tables the kernels index directly must lie inside the blob (what the row records point to — images, triangle tables — is
  // device memory this library cannot read back cheaply: prep.py validates every record against blob_bytes before the upload)
  if (rows_off > blob_bytes || (size_t)B * sizeof(bsr::PrepRow) > blob_bytes - rows_off || grid_off > blob_bytes ||
      (size_t)S * sizeof(double) > blob_bytes - grid_off)
    return fail(BSR_ERR_ARG, "bsr_prep_rows: the row / grid tables do not fit in blob_bytes");
  DeviceGuard guard(device);
  HIP_TRY(guard.err);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const unsigned char* blob = static_cast<const unsigned char*>(d_blob);
  const dim3 grid((unsigned)(S * S / 256), (unsigned)B);
  hipLaunchKernelGGL(bsr::prep_rows_kernel, grid, dim3(256), 0, s, blob, reinterpret_cast<const bsr::PrepRow*>(blob + rows_off),
                     reinterpret_cast<const double*>(blob + grid_off), S, out, hull_tmp);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(bsr::prep_blur_kernel, grid, dim3(256), 0, s, hull_tmp, S, 16, out);
  HIP_TRY(hipGetLastError());
  return BSR_OK;
}

int bsr_prep_groups(int device, const void* d_blob, size_t blob_bytes, size_t groups_off, size_t grid_off, int B, int S, int planes, float* out,
                    float* hull_tmp, void* stream) {
  if (d_blob == nullptr || out == nullptr || hull_tmp == nullptr) return fail(BSR_ERR_ARG, "bsr_prep_groups: null argument");
  if (B <= 0 || S <= 0 || (S * S) % 256 != 0) return fail(BSR_ERR_ARG, "bsr_prep_groups: B must be positive and S*S a multiple of 256");
  if (planes != 6 && planes != 7) return fail(BSR_ERR_ARG, "bsr_prep_groups: planes must be 6 (img3, gt3) or 7 (img3, cmap3, label1)");
  if (groups_off % 8 != 0 || grid_off % 8 != 0) return fail(BSR_ERR_ARG, "bsr_prep_groups: table offsets must be 8-byte aligned");
  // as in bsr_prep_rows: the two tables the kernels index directly must lie inside the blob; prep.py validates what the records point to
  if (groups_off > blob_bytes || (size_t)B * sizeof(bsr::PrepGroup) > blob_bytes - groups_off || grid_off > blob_bytes ||
      (size_t)S * sizeof(double) > blob_bytes - grid_off)
    return fail(BSR_ERR_ARG, "bsr_prep_groups: the group / grid tables do not fit in blob_bytes");
  DeviceGuard guard(device);
  HIP_TRY(guard.err);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const unsigned char* blob = static_cast<const unsigned char*>(d_blob);
  const bsr::PrepGroup* groups = reinterpret_cast<const bsr::PrepGroup*>(blob + groups_off);
  const double* lin = reinterpret_cast<const double*>(blob + grid_off);
  const dim3 grid((unsigned)(S * S / 256), (unsigned)B);
  if (planes == 6)
    hipLaunchKernelGGL(bsr::prep_groups_kernel<6>, grid, dim3(256), 0, s, blob, groups, lin, S, out, hull_tmp);
  else
    hipLaunchKernelGGL(bsr::prep_groups_kernel<7>, grid, dim3(256), 0, s, blob, groups, lin, S, out, hull_tmp);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(bsr::prep_blur_kernel, dim3((unsigned)(S * S / 256), 2u * (unsigned)B), dim3(256), 0, s, hull_tmp, S, planes + 10, out);
  HIP_TRY(hipGetLastError());
  return BSR_OK;
}

int bsr_png_unfilter(int device, void* d_blob, size_t blob_bytes, size_t items_off, int n, void* stream) {
  if (d_blob == nullptr) return fail(BSR_ERR_ARG, "bsr_png_unfilter: null argument");
  if (n <= 0 || items_off % 8 != 0) return fail(BSR_ERR_ARG, "bsr_png_unfilter: n must be positive and items_off 8-byte aligned");
  // the item table must lie inside the blob; what its records point to is validated by the caller before the upload (prep.py), as for bsr_prep_rows
  if (items_off > blob_bytes || (size_t)n * sizeof(bsr::UnfilterItem) > blob_bytes - items_off)
    return fail(BSR_ERR_ARG, "bsr_png_unfilter: the item table does not fit in blob_bytes");
  DeviceGuard guard(device);
  HIP_TRY(guard.err);
  unsigned char* blob = static_cast<unsigned char*>(d_blob);
  hipLaunchKernelGGL(bsr::png_unfilter_kernel, dim3((unsigned)n), dim3(256), 0, static_cast<hipStream_t>(stream), blob,
                     reinterpret_cast<const bsr::UnfilterItem*>(blob + items_off));
  HIP_TRY(hipGetLastError());
  return BSR_OK;
}

int bsr_png_unfilter_tall(int device, void* d_blob, size_t blob_bytes, size_t items_off, int n, void* stream) {
  if (d_blob == nullptr) return fail(BSR_ERR_ARG, "bsr_png_unfilter_tall: null argument");
  if (n <= 0 || n > 65535 || items_off % 8 != 0) return fail(BSR_ERR_ARG, "bsr_png_unfilter_tall: n must be 1..65535 and items_off 8-byte aligned");
  if (items_off > blob_bytes || (size_t)n * sizeof(bsr::UnfilterTallItem) > blob_bytes - items_off)
    return fail(BSR_ERR_ARG, "bsr_png_unfilter_tall: the item table does not fit in blob_bytes");
  DeviceGuard guard(device);
  HIP_TRY(guard.err);
  unsigned char* blob = static_cast<unsigned char*>(d_blob);
  hipStream_t s = static_cast<hipStream_t>(stream);
  std::vector<bsr::UnfilterTallItem> items;
  if (int rc = read_records(blob, items_off, n, s, &items)) return rc;
  const long long total = (long long)blob_bytes, slack = bsr::kUnfilterSlack;
  for (int i = 0; i < n; ++i) {
    const bsr::UnfilterTallItem& it = items[(size_t)i];
    const bool shape = (it.c == 1 || it.c == 3 || it.c == 4) && it.h >= 1 && it.h <= 65535 && it.w >= 1 && it.w <= 65535 && (long long)it.w * it.c >= 4 &&
                       it.rows_needed >= 0 && (it.grey_out == 0 || it.c == 1);
    if (!shape) return fail(BSR_ERR_ARG, "bsr_png_unfilter_tall: a record needs c in {1,3,4}, 1 <= h, w <= 65535, w c >= 4, rows_needed >= 0, grey_out with c = 1 only");
    const long long raw = (long long)it.h * (1 + (long long)it.w * it.c), outb = (long long)it.h * it.w * (it.grey_out ? 1 : 3);
    // the kernel reads its rows four pixels at a time: kUnfilterSlack readable bytes around the scanlines and behind the output area
    if (it.raw_off < slack || it.raw_off > total || raw + slack > total - it.raw_off || it.out_off < 0 || it.out_off > total || outb + slack > total - it.out_off)
      return fail(BSR_ERR_ARG, "bsr_png_unfilter_tall: a record points outside the blob (16 bytes of the blob must surround the scanlines and follow the output)");
  }
  hipLaunchKernelGGL(bsr::png_unfilter_tall_kernel, dim3((unsigned)n), dim3(256), 0, s, blob, reinterpret_cast<const bsr::UnfilterTallItem*>(blob + items_off));
  HIP_TRY(hipGetLastError());
  return BSR_OK;
}

int bsr_crop_faces(int device, void* d_blob, size_t blob_bytes, size_t items_off, int n, int S, void* stream) {
  if (d_blob == nullptr) return fail(BSR_ERR_ARG, "bsr_crop_faces: null argument");
  if (n <= 0 || n > 65535 || items_off % 8 != 0) return fail(BSR_ERR_ARG, "bsr_crop_faces: n must be 1..65535 and items_off 8-byte aligned");
  if (S != 32 && S != 64 && S != 128 && S != 256) return fail(BSR_ERR_ARG, "bsr_crop_faces: S must be 32, 64, 128 or 256");
  if (items_off > blob_bytes || (size_t)n * sizeof(bsr::CropItem) > blob_bytes - items_off)
    return fail(BSR_ERR_ARG, "bsr_crop_faces: the item table does not fit in blob_bytes");
  DeviceGuard guard(device);
  HIP_TRY(guard.err);
  unsigned char* blob = static_cast<unsigned char*>(d_blob);
  hipStream_t s = static_cast<hipStream_t>(stream);
  std::vector<bsr::CropItem> items;
  if (int rc = read_records(blob, items_off, n, s, &items)) return rc;
  const long long total = (long long)blob_bytes, outb = 3ll * S * S;
  for (int i = 0; i < n; ++i) {
    const bsr::CropItem& it = items[(size_t)i];
    if (it.h < 1 || it.h > 65535 || it.w < 1 || it.w > 65535 || it.preset_x < 0 || it.preset_y < 0 || it.preset_x > (1 << 20) || it.preset_y > (1 << 20))
      return fail(BSR_ERR_ARG, "bsr_crop_faces: a record needs 1 <= h, w <= 65535 and presets in 0..2^20");
    const long long srcb = 3ll * it.h * it.w;
    if (it.src_off < 0 || it.src_off > total || srcb > total - it.src_off || it.out_off < 0 || it.out_off > total || outb > total - it.out_off)
      return fail(BSR_ERR_ARG, "bsr_crop_faces: a record points outside the blob");
    // the box against what it is cut from: the photograph itself (8-bit branch) or the padded canvas around it
    const bool padded = it.preset_x != 0 || it.preset_y != 0;
    const long long cw = padded ? (long long)it.w + 2ll * it.preset_x + 2 : it.w, ch = padded ? (long long)it.h + 2ll * it.preset_y + 2 : it.h;
    if (it.box[0] < 0 || it.box[1] < 0 || it.box[2] <= it.box[0] || it.box[3] <= it.box[1] || it.box[2] > cw || it.box[3] > ch)
      return fail(BSR_ERR_ARG, "bsr_crop_faces: a record's box is empty or leaves its canvas");
  }
  hipLaunchKernelGGL(bsr::crop_faces_kernel, dim3((unsigned)((S / 16) * (S / 16)), (unsigned)n), dim3(256), 0, s, blob,
                     reinterpret_cast<const bsr::CropItem*>(blob + items_off), S);
  HIP_TRY(hipGetLastError());
  return BSR_OK;
}

int bsr_paste_faces(int device, void* d_blob, size_t blob_bytes, size_t items_off, int n, int S, const float* im, int im_stride, const float* con,
                    int con_stride, const float* face, int face_stride, int mode, void* stream) {
  if (d_blob == nullptr || im == nullptr || con == nullptr || face == nullptr) return fail(BSR_ERR_ARG, "bsr_paste_faces: null argument");
  if (n <= 0 || n > 65535 || items_off % 8 != 0) return fail(BSR_ERR_ARG, "bsr_paste_faces: n must be 1..65535 and items_off 8-byte aligned");
  if (S != 32 && S != 64 && S != 128 && S != 256) return fail(BSR_ERR_ARG, "bsr_paste_faces: S must be 32, 64, 128 or 256");
  if (mode != bsr::kPasteResidual && mode != bsr::kPasteReplace) return fail(BSR_ERR_ARG, "bsr_paste_faces: mode must be 0 (residual) or 1 (replace)");
  if (im_stride < 3 || con_stride < 3 || face_stride < 1 || im_stride > 4096 || con_stride > 4096 || face_stride > 4096)
    return fail(BSR_ERR_ARG, "bsr_paste_faces: pixel strides are floats between neighbouring pixels: 3..4096 for im and con, 1..4096 for face");
  if (items_off > blob_bytes || (size_t)n * sizeof(bsr::PasteItem) > blob_bytes - items_off)
    return fail(BSR_ERR_ARG, "bsr_paste_faces: the item table does not fit in blob_bytes");
  DeviceGuard guard(device);
  HIP_TRY(guard.err);
  unsigned char* blob = static_cast<unsigned char*>(d_blob);
  hipStream_t s = static_cast<hipStream_t>(stream);
  std::vector<bsr::PasteItem> items;
  if (int rc = read_records(blob, items_off, n, s, &items)) return rc;
  const long long total = (long long)blob_bytes;
  unsigned tiles = 0;
  for (int i = 0; i < n; ++i) {
    const bsr::PasteItem& it = items[(size_t)i];
    if (it.h < 1 || it.h > 65535 || it.w < 1 || it.w > 65535 || it.preset_x < 0 || it.preset_y < 0 || it.preset_x > (1 << 20) || it.preset_y > (1 << 20))
      return fail(BSR_ERR_ARG, "bsr_paste_faces: a record needs 1 <= h, w <= 65535 and presets in 0..2^20");
    if (it.photo_off < 0 || it.photo_off > total || 3ll * it.h * it.w > total - it.photo_off)
      return fail(BSR_ERR_ARG, "bsr_paste_faces: a record points outside the blob");
    // the photograph must not cover the record table the kernel is reading
    if (it.photo_off < (long long)(items_off + (size_t)n * sizeof(bsr::PasteItem)) && it.photo_off + 3ll * it.h * it.w > (long long)items_off)
      return fail(BSR_ERR_ARG, "bsr_paste_faces: a record's photograph overlaps the item table");
    // the box against its canvas, as bsr_crop_faces; a side of at least 2 pixels
    const bool padded = it.preset_x != 0 || it.preset_y != 0;
    const long long cw = padded ? (long long)it.w + 2ll * it.preset_x + 2 : it.w, ch = padded ? (long long)it.h + 2ll * it.preset_y + 2 : it.h;
    if (it.box[0] < 0 || it.box[1] < 0 || it.box[2] > cw || it.box[3] > ch || (long long)it.box[2] - it.box[0] < 2 || (long long)it.box[3] - it.box[1] < 2)
      return fail(BSR_ERR_ARG, "bsr_paste_faces: a record's box has a side under 2 pixels or leaves its canvas");
    if (it.row < 0 || it.row >= n) return fail(BSR_ERR_ARG, "bsr_paste_faces: a record's row is not one of the n rows of im / con / face");
    const unsigned t = bsr::paste_tiles(it);
    if (t > tiles) tiles = t;
  }
  if (tiles == 0) return BSR_OK;                    // no box meets its photograph: every photograph stays as it is
  bsr::PastePlanes pl{im, con, face, im_stride, con_stride, face_stride};
  hipLaunchKernelGGL(bsr::paste_faces_kernel, dim3(tiles, (unsigned)n), dim3(256), 0, s, blob, reinterpret_cast<const bsr::PasteItem*>(blob + items_off), S, pl,
                     mode);
  HIP_TRY(hipGetLastError());
  return BSR_OK;
}

size_t bsr_shadow_synth_scratch_bytes(int B, int S) { return post_size_ok(B, S) && B <= 65535 ? (size_t)B * bsr::shadow_item_scratch_bytes(S) : 0; }

int bsr_shadow_synth(int device, const float* mask, const float* gt, const float* img_dark, const float* face, const void* draws, size_t draws_bytes,
                     int B, int S, float* img, float* mask_sv, float* mask_edge, int* status, float* aux, void* scratch, void* stream) {
  if (B > 65535) return fail(BSR_ERR_ARG, "bsr_shadow_synth: B must be 1..65535");
  if (B > 0 && draws_bytes != (size_t)B * bsr::kShadowWords * sizeof(uint32_t))
    return fail(BSR_ERR_ARG, "bsr_shadow_synth: draws_bytes must be B records of 16384 bytes (shadow_synth.pack_draws)");
  if (reinterpret_cast<uintptr_t>(draws) % 4 != 0) return fail(BSR_ERR_ARG, "bsr_shadow_synth: draws must be 4-byte aligned");
  return run_post("bsr_shadow_synth", {mask, gt, img_dark, face, draws, img, mask_sv, mask_edge, status, scratch}, B, S, scratch, device, [&] {
    HIP_TRY(bsr::launch_shadow_synth(mask, gt, img_dark, face, static_cast<const uint32_t*>(draws), B, S, img, mask_sv, mask_edge, status, aux, scratch,
                                     static_cast<hipStream_t>(stream)));
    return BSR_OK;
  });
}

size_t bsr_train_losses_scratch_bytes(int B, int S) { return post_size_ok(B, S) && B <= 65535 ? (size_t)B * bsr::loss_item_scratch_bytes(S) : 0; }

int bsr_train_losses(int device, const float* img, const float* gt, const float* mask_sv, const float* gs, const float* con_rgb, int B, int S, double* sums,
                     float* losses3, float* mask_edge, float* bmaskgt, float* dif_grad, void* scratch, void* stream) {
  if (B > 65535) return fail(BSR_ERR_ARG, "bsr_train_losses: B must be 1..65535");
  if (reinterpret_cast<uintptr_t>(sums) % 8 != 0) return fail(BSR_ERR_ARG, "bsr_train_losses: sums must be 8-byte aligned");
  return run_post("bsr_train_losses", {img, gt, mask_sv, gs, con_rgb, sums, losses3, scratch}, B, S, scratch, device, [&] {
    HIP_TRY(bsr::launch_train_losses(img, gt, mask_sv, gs, con_rgb, B, S, sums, losses3, mask_edge, bmaskgt, dif_grad, scratch,
                                     static_cast<hipStream_t>(stream)));
    return BSR_OK;
  });
}

size_t bsr_train_losses_grad_scratch_bytes(int B, int S) { return post_size_ok(B, S) && B <= 65535 ? bsr::loss_grad_scratch_bytes(B, S) : 0; }

size_t bsr_train_losses_grad_offset(int B, int S, int level) {
  if (!post_size_ok(B, S) || B > 65535 || level < 0 || level >= bsr::kLossLevels) return SIZE_MAX;
  return bsr::loss_grad_map_offset(B, S, level);
}

int bsr_train_losses_grad(int device, const float* img, const float* gt, const float* mask_sv, const float* gs, const float* con_rgb, const float* upstream,
                          int B, int S, double* sums, float* losses3, float* grad_gs, float* grad_con, float* d_recon_c, float* d_grad, void* scratch,
                          void* stream) {
  if (B > 65535) return fail(BSR_ERR_ARG, "bsr_train_losses_grad: B must be 1..65535");
  if (reinterpret_cast<uintptr_t>(sums) % 8 != 0) return fail(BSR_ERR_ARG, "bsr_train_losses_grad: sums must be 8-byte aligned");
  return run_post("bsr_train_losses_grad", {img, gt, mask_sv, gs, con_rgb, sums, losses3, grad_gs, grad_con, scratch}, B, S, scratch, device, [&] {
    HIP_TRY(bsr::launch_train_losses_grad(img, gt, mask_sv, gs, con_rgb, upstream, B, S, sums, losses3, grad_gs, grad_con, d_recon_c, d_grad, scratch,
                                          static_cast<hipStream_t>(stream)));
    return BSR_OK;
  });
}

size_t bsr_disc_blob_bytes(void) { return 3 * bsr::disc_record_floats() * sizeof(float); }

size_t bsr_disc_losses_scratch_bytes(int B, int S) { return post_size_ok(B, S) && B <= bsr::kDiscMaxB ? bsr::disc_map_offset(B, S, 3, 0) : 0; }

size_t bsr_disc_act_offset(int B, int S, int k, int layer) {
  if (!post_size_ok(B, S) || B > bsr::kDiscMaxB || k < 1 || k > 3 || layer < 0 || layer > bsr::kDiscLayers + 1) return SIZE_MAX;
  return bsr::disc_map_offset(B, S, k - 1, layer);
}

int bsr_disc_losses(int device, const void* d_blob, size_t blob_bytes, const float* gt, const float* con_rgb, const float* mask_sv, int B, int S, double* sums,
                    float* losses3, float* logits, void* scratch, void* stream) {
  if (B > bsr::kDiscMaxB) return fail(BSR_ERR_ARG, "bsr_disc_losses: B must be 1..32767");
  if (blob_bytes != bsr_disc_blob_bytes()) return fail(BSR_ERR_ARG, "bsr_disc_losses: blob_bytes must be bsr_disc_blob_bytes() (pack.pack_discriminators)");
  if (reinterpret_cast<uintptr_t>(d_blob) % 16 != 0) return fail(BSR_ERR_ARG, "bsr_disc_losses: d_blob must be 16-byte aligned");
  if (reinterpret_cast<uintptr_t>(sums) % 8 != 0) return fail(BSR_ERR_ARG, "bsr_disc_losses: sums must be 8-byte aligned");
  return run_post("bsr_disc_losses", {d_blob, gt, con_rgb, mask_sv, sums, losses3, scratch}, B, S, scratch, device, [&] {
    HIP_TRY(bsr::launch_disc_losses(static_cast<const float*>(d_blob), gt, con_rgb, mask_sv, B, S, sums, losses3, logits, scratch,
                                    static_cast<hipStream_t>(stream)));
    return BSR_OK;
  });
}

size_t bsr_disc_dgrad_blob_bytes(void) { return 3 * bsr::disc_dgrad_w_off(bsr::kDiscLayers) * sizeof(float); }

size_t bsr_disc_grad_scratch_bytes(int B, int S) { return post_size_ok(B, S) && B <= bsr::kDiscMaxB ? bsr::disc_grad_offset(B, S, 3, 0) : 0; }

size_t bsr_disc_grad_offset(int B, int S, int k, int layer) {
  if (!post_size_ok(B, S) || B > bsr::kDiscMaxB || k < 1 || k > 3 || layer < 0 || layer > bsr::kDiscLayers) return SIZE_MAX;
  return bsr::disc_grad_offset(B, S, k - 1, layer);
}

namespace {

int disc_gen_grad(const char* name, int device, const void* d_blob, size_t blob_bytes, const void* d_dgrad_blob, size_t dgrad_bytes, const float* gt,
                  const float* con_rgb, const float* mask_sv, const float* upstream, int B, int S, double* sums, float* losses3, float* logits, float* grad,
                  void* scratch, int stop_after, void* stream) {
  const std::string n(name);
  if (B > bsr::kDiscMaxB) return fail(BSR_ERR_ARG, n + ": B must be 1..32767");
  if (blob_bytes != bsr_disc_blob_bytes()) return fail(BSR_ERR_ARG, n + ": blob_bytes must be bsr_disc_blob_bytes() (pack.pack_discriminators)");
  if (dgrad_bytes != bsr_disc_dgrad_blob_bytes())
    return fail(BSR_ERR_ARG, n + ": dgrad_bytes must be bsr_disc_dgrad_blob_bytes() (pack.pack_discriminators_dgrad)");
  if (reinterpret_cast<uintptr_t>(d_blob) % 16 != 0 || reinterpret_cast<uintptr_t>(d_dgrad_blob) % 16 != 0)
    return fail(BSR_ERR_ARG, n + ": d_blob and d_dgrad_blob must be 16-byte aligned");
  if (reinterpret_cast<uintptr_t>(sums) % 8 != 0) return fail(BSR_ERR_ARG, n + ": sums must be 8-byte aligned");
  if (stop_after < 0 || stop_after > bsr::kDiscGradLaunches) return fail(BSR_ERR_ARG, n + ": stop_after must be 0..6");
  return run_post(name, {d_blob, d_dgrad_blob, gt, con_rgb, mask_sv, sums, losses3, grad, scratch}, B, S, scratch, device, [&] {
    HIP_TRY(bsr::launch_disc_gen_grad(static_cast<const float*>(d_blob), static_cast<const float*>(d_dgrad_blob), gt, con_rgb, mask_sv, upstream, B, S, sums,
                                      losses3, logits, grad, scratch, stop_after, static_cast<hipStream_t>(stream)));
    return BSR_OK;
  });
}

}  // namespace

int bsr_disc_gen_grad(int device, const void* d_blob, size_t blob_bytes, const void* d_dgrad_blob, size_t dgrad_bytes, const float* gt, const float* con_rgb,
                      const float* mask_sv, const float* upstream, int B, int S, double* sums, float* losses3, float* logits, float* grad, void* scratch,
                      void* stream) {
  return disc_gen_grad("bsr_disc_gen_grad", device, d_blob, blob_bytes, d_dgrad_blob, dgrad_bytes, gt, con_rgb, mask_sv, upstream, B, S, sums, losses3, logits,
                       grad, scratch, bsr::kDiscGradLaunches, stream);
}

int bsr_debug_disc_gen_grad(int device, const void* d_blob, size_t blob_bytes, const void* d_dgrad_blob, size_t dgrad_bytes, const float* gt,
                            const float* con_rgb, const float* mask_sv, const float* upstream, int B, int S, double* sums, float* losses3, float* logits,
                            float* grad, void* scratch, int stop_after, void* stream) {
  return disc_gen_grad("bsr_debug_disc_gen_grad", device, d_blob, blob_bytes, d_dgrad_blob, dgrad_bytes, gt, con_rgb, mask_sv, upstream, B, S, sums, losses3,
                       logits, grad, scratch, stop_after, stream);
}

size_t bsr_disc_wgrad_blob_bytes(void) { return 3 * bsr::disc_wgrad_w_off(bsr::kDiscLayers) * sizeof(float); }

size_t bsr_disc_wgrad_scratch_bytes(int B, int S) { return post_size_ok(B, S) && B <= bsr::kDiscMaxB ? bsr::disc_wgrad_plan(B, S).total : 0; }

size_t bsr_disc_wgrad_floats(void) { return bsr::disc_wgrad_var_offset(bsr::kDiscVars); }

size_t bsr_disc_wgrad_var_offset(int index) { return index < 0 || index >= bsr::kDiscVars ? SIZE_MAX : bsr::disc_wgrad_var_offset(index); }

size_t bsr_disc_wgrad_offset(int B, int S, int k, int layer) {
  if (!post_size_ok(B, S) || B > bsr::kDiscMaxB || k < 1 || k > 3 || layer < 1 || layer > bsr::kDiscLayers + 1) return SIZE_MAX;
  return bsr::disc_wgrad_map_offset(B, S, k - 1, layer);
}

namespace {

int disc_wgrad(const char* name, int device, const void* d_blob, size_t blob_bytes, const void* d_dgrad_blob, size_t dgrad_bytes, const void* d_wgrad_blob,
               size_t wgrad_bytes, const float* gt, const float* con_rgb, const float* mask_sv, int B, int S, double* sums, float* losses3, float* logits,
               float* grads, void* scratch, int stop_after, void* stream) {
  const std::string n(name);
  if (B > bsr::kDiscMaxB) return fail(BSR_ERR_ARG, n + ": B must be 1..32767");
  if (blob_bytes != bsr_disc_blob_bytes()) return fail(BSR_ERR_ARG, n + ": blob_bytes must be bsr_disc_blob_bytes() (pack.pack_discriminators)");
  if (dgrad_bytes != bsr_disc_dgrad_blob_bytes())
    return fail(BSR_ERR_ARG, n + ": dgrad_bytes must be bsr_disc_dgrad_blob_bytes() (pack.pack_discriminators_dgrad)");
  if (wgrad_bytes != bsr_disc_wgrad_blob_bytes())
    return fail(BSR_ERR_ARG, n + ": wgrad_bytes must be bsr_disc_wgrad_blob_bytes() (pack.pack_discriminators_wgrad)");
  if (reinterpret_cast<uintptr_t>(d_blob) % 16 != 0 || reinterpret_cast<uintptr_t>(d_dgrad_blob) % 16 != 0 || reinterpret_cast<uintptr_t>(d_wgrad_blob) % 16 != 0)
    return fail(BSR_ERR_ARG, n + ": d_blob, d_dgrad_blob and d_wgrad_blob must be 16-byte aligned");
  if (reinterpret_cast<uintptr_t>(sums) % 8 != 0) return fail(BSR_ERR_ARG, n + ": sums must be 8-byte aligned");
  if (reinterpret_cast<uintptr_t>(grads) % 4 != 0) return fail(BSR_ERR_ARG, n + ": grads must be 4-byte aligned");
  if (stop_after < 0 || stop_after > bsr::kDiscWgradLaunches) return fail(BSR_ERR_ARG, n + ": stop_after must be 0..11");
  return run_post(name, {d_blob, d_dgrad_blob, d_wgrad_blob, gt, con_rgb, mask_sv, sums, losses3, grads, scratch}, B, S, scratch, device, [&] {
    HIP_TRY(bsr::launch_disc_wgrad(static_cast<const float*>(d_blob), static_cast<const float*>(d_dgrad_blob), static_cast<const float*>(d_wgrad_blob), gt,
                                   con_rgb, mask_sv, B, S, sums, losses3, logits, grads, scratch, stop_after, static_cast<hipStream_t>(stream)));
    return BSR_OK;
  });
}

}  // namespace

int bsr_disc_wgrad(int device, const void* d_blob, size_t blob_bytes, const void* d_dgrad_blob, size_t dgrad_bytes, const void* d_wgrad_blob, size_t wgrad_bytes,
                   const float* gt, const float* con_rgb, const float* mask_sv, int B, int S, double* sums, float* losses3, float* logits, float* grads,
                   void* scratch, void* stream) {
  return disc_wgrad("bsr_disc_wgrad", device, d_blob, blob_bytes, d_dgrad_blob, dgrad_bytes, d_wgrad_blob, wgrad_bytes, gt, con_rgb, mask_sv, B, S, sums, losses3,
                    logits, grads, scratch, bsr::kDiscWgradLaunches, stream);
}

int bsr_debug_disc_wgrad(int device, const void* d_blob, size_t blob_bytes, const void* d_dgrad_blob, size_t dgrad_bytes, const void* d_wgrad_blob,
                         size_t wgrad_bytes, const float* gt, const float* con_rgb, const float* mask_sv, int B, int S, double* sums, float* losses3,
                         float* logits, float* grads, void* scratch, int stop_after, void* stream) {
  return disc_wgrad("bsr_debug_disc_wgrad", device, d_blob, blob_bytes, d_dgrad_blob, dgrad_bytes, d_wgrad_blob, wgrad_bytes, gt, con_rgb, mask_sv, B, S, sums,
                    losses3, logits, grads, scratch, stop_after, stream);
}

size_t bsr_clr_tail_grad_blob_bytes(void) { return bsr::kClrBlobFloats * sizeof(float); }

size_t bsr_clr_tail_grad_scratch_bytes(int B, int H, int W) { return bsr::clr_tail_size_ok(B, H, W) ? bsr::clr_tail_plan(B, H, W).total : 0; }

size_t bsr_clr_tail_grad_floats(void) { return bsr::clr_tail_var_offset(bsr::kClrVars); }

size_t bsr_clr_tail_grad_var_offset(int index) { return index < 0 || index >= bsr::kClrVars ? SIZE_MAX : bsr::clr_tail_var_offset(index); }

size_t bsr_clr_tail_grad_offset(int B, int H, int W, int map) {
  if (!bsr::clr_tail_size_ok(B, H, W) || map < 0 || map > 6) return SIZE_MAX;
  return bsr::clr_tail_plan(B, H, W).map[map];
}

int bsr_clr_tail_grad_partials(int B, int H, int W) { return bsr::clr_tail_size_ok(B, H, W) ? bsr::clr_tail_plan(B, H, W).P : 0; }

namespace {

int clr_tail_grad(const char* name, int device, const void* d_blob, size_t blob_bytes, const float* gs, const float* f, int f_cs, const float* g_con,
                  const float* g_gs, int B, int H, int W, float* d_f, float* d_gs, float* grads, int keep, void* scratch, int stop_after, void* stream) {
  return run_grad_stage(
      name, {d_blob, gs, f, g_con, d_f, d_gs, grads, scratch},
      {{bsr::clr_tail_size_ok(B, H, W), "B must be positive, H a multiple of 8 and W a multiple of 32 (conv_n16_kernel's tile), at most 2^26 pixels in all"},
       {blob_bytes == bsr_clr_tail_grad_blob_bytes(), "blob_bytes must be bsr_clr_tail_grad_blob_bytes() (pack.pack_clr_tail_grad)"},
       {f_cs >= 64 && f_cs % 4 == 0, "f_cs must be a multiple of 4 and at least 64"}},
      {{16, "d_blob, f and d_f", {d_blob, f, d_f}}, {4, "gs, g_con, g_gs, d_gs and grads", {gs, g_con, g_gs, d_gs, grads}}}, scratch, stop_after,
      bsr::kClrTailLaunches, device, [&] {
        HIP_TRY(bsr::launch_clr_tail_grad(static_cast<const float*>(d_blob), gs, f, f_cs, g_con, g_gs, B, H, W, d_f, d_gs, grads, keep != 0, scratch,
                                          stop_after, static_cast<hipStream_t>(stream)));
        return BSR_OK;
      });
}

}  // namespace

int bsr_clr_tail_grad(int device, const void* d_blob, size_t blob_bytes, const float* gs, const float* f, int f_cs, const float* g_con, const float* g_gs,
                      int B, int H, int W, float* d_f, float* d_gs, float* grads, int keep, void* scratch, void* stream) {
  return clr_tail_grad("bsr_clr_tail_grad", device, d_blob, blob_bytes, gs, f, f_cs, g_con, g_gs, B, H, W, d_f, d_gs, grads, keep, scratch,
                       bsr::kClrTailLaunches, stream);
}

int bsr_debug_clr_tail_grad(int device, const void* d_blob, size_t blob_bytes, const float* gs, const float* f, int f_cs, const float* g_con,
                            const float* g_gs, int B, int H, int W, float* d_f, float* d_gs, float* grads, int keep, void* scratch, int stop_after,
                            void* stream) {
  return clr_tail_grad("bsr_debug_clr_tail_grad", device, d_blob, blob_bytes, gs, f, f_cs, g_con, g_gs, B, H, W, d_f, d_gs, grads, keep, scratch, stop_after,
                       stream);
}

size_t bsr_clr_decoder_grad_blob_bytes(void) { return bsr::up_blob_off(3, 0) * sizeof(float); }

size_t bsr_clr_decoder_grad_scratch_bytes(int B, int H, int W, int keep) { return bsr::up_size_ok(B, H, W) ? bsr::up_plan(B, H, W, keep != 0).total : 0; }

size_t bsr_clr_decoder_grad_floats(void) { return bsr::up_var_offset(bsr::kUpVars); }

size_t bsr_clr_decoder_grad_var_offset(int index) { return index < 0 || index >= bsr::kUpVars ? SIZE_MAX : bsr::up_var_offset(index); }

size_t bsr_clr_decoder_grad_offset(int B, int H, int W, int map) {
  if (!bsr::up_size_ok(B, H, W) || map < 0 || map > 8) return SIZE_MAX;
  return bsr::up_plan(B, H, W, true).map[map];
}

int bsr_clr_decoder_grad_partials(int B, int H, int W, int layer) {
  return bsr::up_size_ok(B, H, W) && layer >= 1 && layer <= 3 ? bsr::up_plan(B, H, W, false).P[layer - 1] : 0;
}

namespace {

int clr_decoder_grad(const char* name, int device, const void* d_blob, size_t blob_bytes, const float* x, int x_cs, const float* f1, int f1_cs, const float* f2,
                     int f2_cs, const float* f, int f_cs, const float* d_f, int B, int H, int W, float* d_x, float* grads, int keep, void* scratch, int stop_after,
                     void* stream) {
  return run_grad_stage(
      name, {d_blob, x, f1, f2, f, d_f, d_x, grads, scratch},
      {{bsr::up_size_ok(B, H, W), "B must be positive, H a multiple of 32 and W a multiple of 256 (the generator's rule), at most 2^26 pixels in all"},
       {blob_bytes == bsr_clr_decoder_grad_blob_bytes(),
        "blob_bytes must be bsr_clr_decoder_grad_blob_bytes() (pack.pack_clr_decoder_grad; the GSC width 261 only, not TSM's 877)"},
       {x_cs >= 261, "x_cs must be at least 261"},
       {f1_cs >= 128 && f1_cs % 4 == 0 && f2_cs >= 96 && f2_cs % 4 == 0 && f_cs >= 64 && f_cs % 4 == 0,
        "f1_cs, f2_cs, f_cs must be multiples of 4 and at least 128, 96, 64"}},
      {{16, "d_blob, f1, f2, f and d_f", {d_blob, f1, f2, f, d_f}}, {4, "x, d_x and grads", {x, d_x, grads}}}, scratch, stop_after, bsr::kUpLaunches, device,
      [&] {
        HIP_TRY(bsr::launch_clr_decoder_grad(static_cast<const float*>(d_blob), x, x_cs, f1, f1_cs, f2, f2_cs, f, f_cs, d_f, B, H, W, d_x, grads, keep != 0,
                                             scratch, stop_after, static_cast<hipStream_t>(stream)));
        return BSR_OK;
      });
}

}  // namespace

int bsr_clr_decoder_grad(int device, const void* d_blob, size_t blob_bytes, const float* x, int x_cs, const float* f1, int f1_cs, const float* f2, int f2_cs,
                         const float* f, int f_cs, const float* d_f, int B, int H, int W, float* d_x, float* grads, int keep, void* scratch, void* stream) {
  return clr_decoder_grad("bsr_clr_decoder_grad", device, d_blob, blob_bytes, x, x_cs, f1, f1_cs, f2, f2_cs, f, f_cs, d_f, B, H, W, d_x, grads, keep, scratch,
                          bsr::kUpLaunches, stream);
}

int bsr_debug_clr_decoder_grad(int device, const void* d_blob, size_t blob_bytes, const float* x, int x_cs, const float* f1, int f1_cs, const float* f2,
                               int f2_cs, const float* f, int f_cs, const float* d_f, int B, int H, int W, float* d_x, float* grads, int keep, void* scratch,
                               int stop_after, void* stream) {
  return clr_decoder_grad("bsr_debug_clr_decoder_grad", device, d_blob, blob_bytes, x, x_cs, f1, f1_cs, f2, f2_cs, f, f_cs, d_f, B, H, W, d_x, grads, keep,
                          scratch, stop_after, stream);
}

size_t bsr_nonlocal_grad_blob_bytes(void) { return bsr::nl_blob_off(6) * sizeof(float); }

size_t bsr_nonlocal_grad_scratch_bytes(int B, int h, int w) { return bsr::nl_size_ok(B, h, w) ? bsr::nl_plan(B, h, w).total : 0; }

size_t bsr_nonlocal_grad_floats(void) { return bsr::nl_var_offset(bsr::kNlVars); }

size_t bsr_nonlocal_grad_var_offset(int index) { return index < 0 || index >= bsr::kNlVars ? SIZE_MAX : bsr::nl_var_offset(index); }

size_t bsr_nonlocal_grad_offset(int B, int h, int w, int map) {
  if (!bsr::nl_size_ok(B, h, w) || map < 0 || map >= bsr::kNlMaps) return SIZE_MAX;
  return bsr::nl_plan(B, h, w).map[map];
}

int bsr_nonlocal_grad_partials(int B, int h, int w) { return bsr::nl_size_ok(B, h, w) ? bsr::nl_plan(B, h, w).P : 0; }

namespace {

int nonlocal_grad(const char* name, int device, const void* d_blob, size_t blob_bytes, const float* y3x, int y3x_cs, const float* xin, int xin_cs,
                  const float* out, int out_cs, const float* d_out, int B, int h, int w, float* d_y3, float* d_skip, float* grads, void* scratch,
                  int stop_after, void* stream) {
  return run_grad_stage(
      name, {d_blob, y3x, xin, out, d_out, d_y3, d_skip, grads, scratch},
      {{bsr::nl_size_ok(B, h, w),
        "B must be positive, h a multiple of 4 and w a multiple of 32 (the generator's rule at 1/8 resolution), at most 2^21 tokens in all"},
       {blob_bytes == bsr_nonlocal_grad_blob_bytes(),
        "blob_bytes must be bsr_nonlocal_grad_blob_bytes() (pack.pack_nonlocal_grad; the GSC width 261 only, not TSM's 877)"},
       {y3x_cs >= 257 && xin_cs >= 261 && out_cs >= 261, "y3x_cs must be at least 257, xin_cs and out_cs at least 261"}},
      {{16, "d_blob", {d_blob}}, {4, "y3x, xin, out, d_out, d_y3, d_skip and grads", {y3x, xin, out, d_out, d_y3, d_skip, grads}}}, scratch, stop_after,
      bsr::kNlLaunches, device, [&] {
        HIP_TRY(bsr::launch_nonlocal_grad(static_cast<const float*>(d_blob), y3x, y3x_cs, xin, xin_cs, out, out_cs, d_out, B, h, w, d_y3, d_skip, grads,
                                          scratch, stop_after, static_cast<hipStream_t>(stream)));
        return BSR_OK;
      });
}

}  // namespace

int bsr_nonlocal_grad(int device, const void* d_blob, size_t blob_bytes, const float* y3x, int y3x_cs, const float* xin, int xin_cs, const float* out,
                      int out_cs, const float* d_out, int B, int h, int w, float* d_y3, float* d_skip, float* grads, void* scratch, void* stream) {
  return nonlocal_grad("bsr_nonlocal_grad", device, d_blob, blob_bytes, y3x, y3x_cs, xin, xin_cs, out, out_cs, d_out, B, h, w, d_y3, d_skip, grads, scratch,
                       bsr::kNlLaunches, stream);
}

int bsr_debug_nonlocal_grad(int device, const void* d_blob, size_t blob_bytes, const float* y3x, int y3x_cs, const float* xin, int xin_cs, const float* out,
                            int out_cs, const float* d_out, int B, int h, int w, float* d_y3, float* d_skip, float* grads, void* scratch, int stop_after,
                            void* stream) {
  return nonlocal_grad("bsr_debug_nonlocal_grad", device, d_blob, blob_bytes, y3x, y3x_cs, xin, xin_cs, out, out_cs, d_out, B, h, w, d_y3, d_skip, grads,
                       scratch, stop_after, stream);
}

size_t bsr_bottleneck_grad_blob_bytes(void) { return bsr::bn_blob_off(13) * sizeof(float); }

size_t bsr_bottleneck_grad_scratch_bytes(int B, int h, int w) { return bsr::nl_size_ok(B, h, w) ? bsr::bn_plan(B, h, w).total : 0; }

size_t bsr_bottleneck_grad_floats(void) { return bsr::bn_var_offset(bsr::kBnVars); }

size_t bsr_bottleneck_grad_var_offset(int index) { return index < 0 || index >= bsr::kBnVars ? SIZE_MAX : bsr::bn_var_offset(index); }

size_t bsr_bottleneck_grad_offset(int B, int h, int w, int map) {
  if (!bsr::nl_size_ok(B, h, w) || map < 0 || map >= bsr::kBnMaps) return SIZE_MAX;
  return bsr::bn_plan(B, h, w).map[map];
}

int bsr_bottleneck_grad_partials(int B, int h, int w) { return bsr::nl_size_ok(B, h, w) ? bsr::bn_plan(B, h, w).P : 0; }

namespace {

int bottleneck_grad(const char* name, int device, const void* d_blob, size_t blob_bytes, const float* xin, int xin_cs, const float* d_y3,
                    const float* d_skip, int B, int h, int w, float* d_xin, float* grads, void* scratch, int stop_after, void* stream) {
  return run_grad_stage(
      name, {d_blob, xin, d_y3, d_xin, grads, scratch},
      {{bsr::nl_size_ok(B, h, w),
        "B must be positive, h a multiple of 4 and w a multiple of 32 (the generator's rule at 1/8 resolution), at most 2^21 pixels in all"},
       {blob_bytes == bsr_bottleneck_grad_blob_bytes(),
        "blob_bytes must be bsr_bottleneck_grad_blob_bytes() (pack.pack_bottleneck_grad; the GSC width 261 only, not TSM's 877)"},
       {xin_cs >= 261, "xin_cs must be at least 261"}},
      {{16, "d_blob", {d_blob}}, {4, "xin, d_y3, d_skip, d_xin and grads", {xin, d_y3, d_skip, d_xin, grads}}}, scratch, stop_after,
      bsr::kBnLaunches, device, [&] {
        HIP_TRY(bsr::launch_bottleneck_grad(static_cast<const float*>(d_blob), xin, xin_cs, d_y3, d_skip, B, h, w, d_xin, grads, scratch, stop_after,
                                            static_cast<hipStream_t>(stream)));
        return BSR_OK;
      });
}

}  // namespace

int bsr_bottleneck_grad(int device, const void* d_blob, size_t blob_bytes, const float* xin, int xin_cs, const float* d_y3, const float* d_skip, int B,
                        int h, int w, float* d_xin, float* grads, void* scratch, void* stream) {
  return bottleneck_grad("bsr_bottleneck_grad", device, d_blob, blob_bytes, xin, xin_cs, d_y3, d_skip, B, h, w, d_xin, grads, scratch, bsr::kBnLaunches,
                         stream);
}

int bsr_debug_bottleneck_grad(int device, const void* d_blob, size_t blob_bytes, const float* xin, int xin_cs, const float* d_y3, const float* d_skip,
                              int B, int h, int w, float* d_xin, float* grads, void* scratch, int stop_after, void* stream) {
  return bottleneck_grad("bsr_debug_bottleneck_grad", device, d_blob, blob_bytes, xin, xin_cs, d_y3, d_skip, B, h, w, d_xin, grads, scratch, stop_after,
                         stream);
}

namespace {

// the size queries of a chain of blocks (block_chain_grad.h), as the bsr_<stage>_grad_* queries below answer them
size_t chain_blob_bytes(const bsr::BlockChain& c) { return bsr::chain_blob_off(c, 2 * c.n) * sizeof(float); }

size_t chain_scratch_bytes(const bsr::BlockChain& c, int B, int h, int w) { return bsr::nl_size_ok(B, h, w) ? bsr::chain_plan(c, B, h, w).total : 0; }

size_t chain_var_offset_checked(const bsr::BlockChain& c, int index) { return index < 0 || index >= c.vars() ? SIZE_MAX : bsr::chain_var_offset(c, index); }

size_t chain_offset_checked(const bsr::BlockChain& c, int B, int h, int w, int map) {
  if (!bsr::nl_size_ok(B, h, w) || map < 0 || map >= c.maps()) return SIZE_MAX;
  return bsr::chain_plan(c, B, h, w).map[map];
}

}  // namespace

size_t bsr_colour_trunk_grad_blob_bytes(void) { return chain_blob_bytes(bsr::kColourChain); }

size_t bsr_colour_trunk_grad_scratch_bytes(int B, int h, int w) { return chain_scratch_bytes(bsr::kColourChain, B, h, w); }

size_t bsr_colour_trunk_grad_floats(void) { return bsr::chain_var_offset(bsr::kColourChain, bsr::kColourChain.vars()); }

size_t bsr_colour_trunk_grad_var_offset(int index) { return chain_var_offset_checked(bsr::kColourChain, index); }

size_t bsr_colour_trunk_grad_offset(int B, int h, int w, int map) { return chain_offset_checked(bsr::kColourChain, B, h, w, map); }

namespace {

int colour_trunk_grad(const char* name, int device, const void* d_blob, size_t blob_bytes, const float* y3x4, int y3x4_cs, const float* out4, int out4_cs,
                      const float* y3x3, int y3x3_cs, const float* out3, int out3_cs, const float* xh, int xh_cs, const float* d_xin, const float* d_x, int B,
                      int h, int w, float* d_res2, float* grads, void* scratch, int stop_after, void* stream) {
  return run_grad_stage(
      name, {d_blob, y3x4, out4, y3x3, out3, xh, d_xin, d_res2, grads, scratch},
      {{bsr::nl_size_ok(B, h, w),
        "B must be positive, h a multiple of 4 and w a multiple of 32 (the generator's rule at 1/8 resolution), at most 2^21 pixels in all"},
       {blob_bytes == bsr_colour_trunk_grad_blob_bytes(),
        "blob_bytes must be bsr_colour_trunk_grad_blob_bytes() (pack.pack_colour_trunk_grad; the GSC width 261 only, not TSM's 877)"},
       {y3x4_cs >= 257 && y3x3_cs >= 257 && out4_cs >= 261 && out3_cs >= 261 && xh_cs >= 261,
        "y3x4_cs and y3x3_cs must be at least 257, out4_cs, out3_cs and xh_cs at least 261"}},
      {{16, "d_blob, d_x and d_res2", {d_blob, d_x, d_res2}},
       {4, "y3x4, out4, y3x3, out3, xh, d_xin and grads", {y3x4, out4, y3x3, out3, xh, d_xin, grads}}},
      scratch, stop_after, bsr::kColourChain.launches(), device, [&] {
        HIP_TRY(bsr::launch_colour_trunk_grad(static_cast<const float*>(d_blob), y3x4, y3x4_cs, out4, out4_cs, y3x3, y3x3_cs, out3, out3_cs, xh, xh_cs, d_xin,
                                              d_x, B, h, w, d_res2, grads, scratch, stop_after, static_cast<hipStream_t>(stream)));
        return BSR_OK;
      });
}

}  // namespace

int bsr_colour_trunk_grad(int device, const void* d_blob, size_t blob_bytes, const float* y3x4, int y3x4_cs, const float* out4, int out4_cs,
                          const float* y3x3, int y3x3_cs, const float* out3, int out3_cs, const float* xh, int xh_cs, const float* d_xin, const float* d_x,
                          int B, int h, int w, float* d_res2, float* grads, void* scratch, void* stream) {
  return colour_trunk_grad("bsr_colour_trunk_grad", device, d_blob, blob_bytes, y3x4, y3x4_cs, out4, out4_cs, y3x3, y3x3_cs, out3, out3_cs, xh, xh_cs, d_xin,
                           d_x, B, h, w, d_res2, grads, scratch, bsr::kColourChain.launches(), stream);
}

int bsr_debug_colour_trunk_grad(int device, const void* d_blob, size_t blob_bytes, const float* y3x4, int y3x4_cs, const float* out4, int out4_cs,
                                const float* y3x3, int y3x3_cs, const float* out3, int out3_cs, const float* xh, int xh_cs, const float* d_xin,
                                const float* d_x, int B, int h, int w, float* d_res2, float* grads, void* scratch, int stop_after, void* stream) {
  return colour_trunk_grad("bsr_debug_colour_trunk_grad", device, d_blob, blob_bytes, y3x4, y3x4_cs, out4, out4_cs, y3x3, y3x3_cs, out3, out3_cs, xh, xh_cs,
                           d_xin, d_x, B, h, w, d_res2, grads, scratch, stop_after, stream);
}

int bsr_debug_hole_grad(int device, const float* xh, int xh_cs, const float* d_xin3, const float* d_x, int B, int h, int w, float* d_res2, void* stream) {
  return run_grad_stage(
      "bsr_debug_hole_grad", {xh, d_xin3, d_res2},
      {{bsr::nl_size_ok(B, h, w),
        "B must be positive, h a multiple of 4 and w a multiple of 32 (the generator's rule at 1/8 resolution), at most 2^21 pixels in all"},
       {xh_cs >= 258, "xh_cs must be at least 258"}},
      {{16, "d_xin3, d_x and d_res2", {d_xin3, d_x, d_res2}}, {4, "xh", {xh}}}, nullptr, 0, 0, device, [&] {
        HIP_TRY(bsr::launch_hole_grad(d_xin3, xh, xh_cs, d_x, B * h * w, d_res2, static_cast<hipStream_t>(stream)));
        return BSR_OK;
      });
}

size_t bsr_lower_trunk_grad_blob_bytes(void) { return chain_blob_bytes(bsr::kLowerChain); }

size_t bsr_lower_trunk_grad_scratch_bytes(int B, int h, int w) { return chain_scratch_bytes(bsr::kLowerChain, B, h, w); }

size_t bsr_lower_trunk_grad_floats(void) { return bsr::chain_var_offset(bsr::kLowerChain, bsr::kLowerChain.vars()); }

size_t bsr_lower_trunk_grad_var_offset(int index) { return chain_var_offset_checked(bsr::kLowerChain, index); }

size_t bsr_lower_trunk_grad_offset(int B, int h, int w, int map) { return chain_offset_checked(bsr::kLowerChain, B, h, w, map); }

namespace {

int lower_trunk_grad(const char* name, int device, const void* d_blob, size_t blob_bytes, const float* y3x2, int y3x2_cs, const float* out2, int out2_cs,
                     const float* y3x1, int y3x1_cs, const float* out1, int out1_cs, const float* y3x0, int y3x0_cs, const float* out0, int out0_cs,
                     const float* x0, int x0_cs, const float* d_res2, int B, int h, int w, float* d_x0, float* grads, void* scratch, int stop_after,
                     void* stream) {
  return run_grad_stage(
      name, {d_blob, y3x2, out2, y3x1, out1, y3x0, out0, x0, d_res2, d_x0, grads, scratch},
      {{bsr::nl_size_ok(B, h, w),
        "B must be positive, h a multiple of 4 and w a multiple of 32 (the generator's rule at 1/8 resolution), at most 2^21 pixels in all"},
       {blob_bytes == bsr_lower_trunk_grad_blob_bytes(),
        "blob_bytes must be bsr_lower_trunk_grad_blob_bytes() (pack.pack_lower_trunk_grad; the GSC widths 99 and 257 only, not TSM's 291 or RGB's 513)"},
       {y3x2_cs >= 257 && y3x1_cs >= 257 && y3x0_cs >= 257 && out2_cs >= 257 && out1_cs >= 257 && out0_cs >= 257 && x0_cs >= 99,
        "y3x2_cs, y3x1_cs, y3x0_cs, out2_cs, out1_cs and out0_cs must be at least 257, x0_cs at least 99"}},
      {{16, "d_blob", {d_blob}},
       {4, "y3x2, out2, y3x1, out1, y3x0, out0, x0, d_res2, d_x0 and grads", {y3x2, out2, y3x1, out1, y3x0, out0, x0, d_res2, d_x0, grads}}},
      scratch, stop_after, bsr::kLowerChain.launches(), device, [&] {
        // block 2's input is out1, block 1's is out0, block 0's is x0
        const bsr::ChainBlockIn in[3] = {{y3x2, out1, out2, y3x2_cs, out1_cs, out2_cs}, {y3x1, out0, out1, y3x1_cs, out0_cs, out1_cs},
                                         {y3x0, x0, out0, y3x0_cs, x0_cs, out0_cs}};
        float* d_last = d_x0;
        int left = stop_after;
        HIP_TRY(bsr::launch_block_chain(bsr::kLowerChain, static_cast<const float*>(d_blob), in, d_res2, B, h, w, &d_last, grads, scratch, left,
                                        static_cast<hipStream_t>(stream)));
        return BSR_OK;
      });
}

}  // namespace

int bsr_lower_trunk_grad(int device, const void* d_blob, size_t blob_bytes, const float* y3x2, int y3x2_cs, const float* out2, int out2_cs,
                         const float* y3x1, int y3x1_cs, const float* out1, int out1_cs, const float* y3x0, int y3x0_cs, const float* out0, int out0_cs,
                         const float* x0, int x0_cs, const float* d_res2, int B, int h, int w, float* d_x0, float* grads, void* scratch, void* stream) {
  return lower_trunk_grad("bsr_lower_trunk_grad", device, d_blob, blob_bytes, y3x2, y3x2_cs, out2, out2_cs, y3x1, y3x1_cs, out1, out1_cs, y3x0, y3x0_cs,
                          out0, out0_cs, x0, x0_cs, d_res2, B, h, w, d_x0, grads, scratch, bsr::kLowerChain.launches(), stream);
}

int bsr_debug_lower_trunk_grad(int device, const void* d_blob, size_t blob_bytes, const float* y3x2, int y3x2_cs, const float* out2, int out2_cs,
                               const float* y3x1, int y3x1_cs, const float* out1, int out1_cs, const float* y3x0, int y3x0_cs, const float* out0,
                               int out0_cs, const float* x0, int x0_cs, const float* d_res2, int B, int h, int w, float* d_x0, float* grads,
                               void* scratch, int stop_after, void* stream) {
  return lower_trunk_grad("bsr_debug_lower_trunk_grad", device, d_blob, blob_bytes, y3x2, y3x2_cs, out2, out2_cs, y3x1, y3x1_cs, out1, out1_cs, y3x0,
                          y3x0_cs, out0, out0_cs, x0, x0_cs, d_res2, B, h, w, d_x0, grads, scratch, stop_after, stream);
}

size_t bsr_heads_grad_blob_bytes(void) { return (size_t)bsr::kHgBlobFloats * sizeof(float); }

size_t bsr_heads_grad_scratch_bytes(int B, int H, int W) { return bsr::hg_size_ok(B, H, W) ? bsr::hg_plan(B, H, W).total : 0; }

size_t bsr_heads_grad_floats(void) { return bsr::hg_var_offset(bsr::kHgVars); }

size_t bsr_heads_grad_var_offset(int index) { return index < 0 || index >= bsr::kHgVars ? SIZE_MAX : bsr::hg_var_offset(index); }

size_t bsr_heads_grad_offset(int B, int H, int W, int map) {
  if (!bsr::hg_size_ok(B, H, W) || map < 0 || map >= bsr::kHgMaps) return SIZE_MAX;
  return bsr::hg_plan(B, H, W).map[map];
}

int bsr_heads_grad_partials(int B, int H, int W) { return bsr::hg_size_ok(B, H, W) ? bsr::hg_plan(B, H, W).P : 0; }

namespace {

int heads_grad(const char* name, int device, const void* d_blob, size_t blob_bytes, const float* inputs, const float* mask22, const float* y, int y_cs,
               const float* d_gs, int B, int H, int W, float* d_y, float* grads, void* scratch, int stop_after, void* stream) {
  return run_grad_stage(
      name, {d_blob, inputs, mask22, y, d_gs, d_y, grads, scratch},
      {{bsr::hg_size_ok(B, H, W), "B must be positive, H a multiple of 8 and W a multiple of 32 (the forward heads' tile), at most 2^26 pixels in all"},
       {blob_bytes == bsr_heads_grad_blob_bytes(), "blob_bytes must be bsr_heads_grad_blob_bytes() (pack.pack_heads_grad)"},
       {y_cs >= 64 && y_cs % 4 == 0, "y_cs must be a multiple of 4 and at least 64"}},
      {{16, "d_blob, y and d_y", {d_blob, y, d_y}}, {4, "inputs, mask22, d_gs and grads", {inputs, mask22, d_gs, grads}}}, scratch, stop_after,
      bsr::kHgLaunches, device, [&] {
        HIP_TRY(bsr::launch_heads_grad(static_cast<const float*>(d_blob), inputs, mask22, y, y_cs, d_gs, B, H, W, d_y, grads, scratch, stop_after,
                                       static_cast<hipStream_t>(stream)));
        return BSR_OK;
      });
}

}  // namespace

int bsr_heads_grad(int device, const void* d_blob, size_t blob_bytes, const float* inputs, const float* mask22, const float* y, int y_cs,
                   const float* d_gs, int B, int H, int W, float* d_y, float* grads, void* scratch, void* stream) {
  return heads_grad("bsr_heads_grad", device, d_blob, blob_bytes, inputs, mask22, y, y_cs, d_gs, B, H, W, d_y, grads, scratch, bsr::kHgLaunches, stream);
}

int bsr_debug_heads_grad(int device, const void* d_blob, size_t blob_bytes, const float* inputs, const float* mask22, const float* y, int y_cs,
                         const float* d_gs, int B, int H, int W, float* d_y, float* grads, void* scratch, int stop_after, void* stream) {
  return heads_grad("bsr_debug_heads_grad", device, d_blob, blob_bytes, inputs, mask22, y, y_cs, d_gs, B, H, W, d_y, grads, scratch, stop_after, stream);
}

size_t bsr_grey_decoder_grad_blob_bytes(void) { return bsr::up_blob_off(bsr::kGreyUp, 3, 0) * sizeof(float); }

size_t bsr_grey_decoder_grad_scratch_bytes(int B, int H, int W, int keep) {
  return bsr::up_size_ok(B, H, W) ? bsr::up_plan(bsr::kGreyUp, B, H, W, keep != 0).total : 0;
}

size_t bsr_grey_decoder_grad_floats(void) { return bsr::up_var_offset(bsr::kGreyUp, bsr::kUpVars); }

size_t bsr_grey_decoder_grad_var_offset(int index) { return index < 0 || index >= bsr::kUpVars ? SIZE_MAX : bsr::up_var_offset(bsr::kGreyUp, index); }

size_t bsr_grey_decoder_grad_offset(int B, int H, int W, int map) {
  if (!bsr::up_size_ok(B, H, W) || map < 0 || map > 8) return SIZE_MAX;
  return bsr::up_plan(bsr::kGreyUp, B, H, W, true).map[map];
}

int bsr_grey_decoder_grad_partials(int B, int H, int W, int layer) {
  return bsr::up_size_ok(B, H, W) && layer >= 1 && layer <= 3 ? bsr::up_plan(bsr::kGreyUp, B, H, W, false).P[layer - 1] : 0;
}

namespace {

int grey_decoder_grad(const char* name, int device, const void* d_blob, size_t blob_bytes, const float* x, int x_cs, const float* c2, int c2_cs,
                      const float* c3, int c3_cs, const float* y, int y_cs, const float* d_y, int B, int H, int W, float* d_x, float* d_x3, float* d_x2,
                      float* grads, int keep, void* scratch, int stop_after, void* stream) {
  return run_grad_stage(
      name, {d_blob, x, c2, c3, y, d_y, d_x, d_x3, d_x2, grads, scratch},
      {{bsr::up_size_ok(B, H, W), "B must be positive, H a multiple of 32 and W a multiple of 256 (the generator's rule), at most 2^26 pixels in all"},
       {blob_bytes == bsr_grey_decoder_grad_blob_bytes(),
        "blob_bytes must be bsr_grey_decoder_grad_blob_bytes() (pack.pack_grey_decoder_grad; the GSC width 257 only, not TSM's 291)"},
       {x_cs >= 257, "x_cs must be at least 257"},
       {c2_cs >= 160 && c2_cs % 4 == 0 && c3_cs >= 128 && c3_cs % 4 == 0 && y_cs >= 64 && y_cs % 4 == 0,
        "c2_cs, c3_cs, y_cs must be multiples of 4 and at least 160, 128, 64"}},
      {{16, "d_blob, c2, c3, y, d_y, d_x3 and d_x2", {d_blob, c2, c3, y, d_y, d_x3, d_x2}}, {4, "x, d_x and grads", {x, d_x, grads}}}, scratch, stop_after,
      bsr::kUpLaunches, device, [&] {
        HIP_TRY(bsr::launch_grey_decoder_grad(static_cast<const float*>(d_blob), x, x_cs, c2, c2_cs, c3, c3_cs, y, y_cs, d_y, B, H, W, d_x, d_x3, d_x2, grads,
                                              keep != 0, scratch, stop_after, static_cast<hipStream_t>(stream)));
        return BSR_OK;
      });
}

}  // namespace

int bsr_grey_decoder_grad(int device, const void* d_blob, size_t blob_bytes, const float* x, int x_cs, const float* c2, int c2_cs, const float* c3, int c3_cs,
                          const float* y, int y_cs, const float* d_y, int B, int H, int W, float* d_x, float* d_x3, float* d_x2, float* grads, int keep,
                          void* scratch, void* stream) {
  return grey_decoder_grad("bsr_grey_decoder_grad", device, d_blob, blob_bytes, x, x_cs, c2, c2_cs, c3, c3_cs, y, y_cs, d_y, B, H, W, d_x, d_x3, d_x2, grads,
                           keep, scratch, bsr::kUpLaunches, stream);
}

int bsr_debug_grey_decoder_grad(int device, const void* d_blob, size_t blob_bytes, const float* x, int x_cs, const float* c2, int c2_cs, const float* c3,
                                int c3_cs, const float* y, int y_cs, const float* d_y, int B, int H, int W, float* d_x, float* d_x3, float* d_x2,
                                float* grads, int keep, void* scratch, int stop_after, void* stream) {
  return grey_decoder_grad("bsr_debug_grey_decoder_grad", device, d_blob, blob_bytes, x, x_cs, c2, c2_cs, c3, c3_cs, y, y_cs, d_y, B, H, W, d_x, d_x3, d_x2,
                           grads, keep, scratch, stop_after, stream);
}

size_t bsr_vgg_blob_bytes(void) { return bsr::vgg_w_off(bsr::kVggLayers) * sizeof(float); }

size_t bsr_vgg_scratch_bytes(int B, int S) { return post_size_ok(B, S) && B <= bsr::kVggMaxB ? bsr::vgg_act_offset(B, S, bsr::kVggMaps + 1) : 0; }

size_t bsr_vgg_act_offset(int B, int S, int layer) {
  if (!post_size_ok(B, S) || B > bsr::kVggMaxB || layer < 0 || layer >= bsr::kVggMaps) return SIZE_MAX;
  return bsr::vgg_act_offset(B, S, layer);
}

int bsr_vgg_per_loss(int device, const void* d_blob, size_t blob_bytes, const float* gt, const float* con_rgb, int B, int S, double* sums, float* loss1,
                     void* scratch, void* stream) {
  if (B > bsr::kVggMaxB) return fail(BSR_ERR_ARG, "bsr_vgg_per_loss: B must be 1..4096");
  if (blob_bytes != bsr_vgg_blob_bytes()) return fail(BSR_ERR_ARG, "bsr_vgg_per_loss: blob_bytes must be bsr_vgg_blob_bytes() (pack.pack_vgg)");
  if (reinterpret_cast<uintptr_t>(d_blob) % 16 != 0) return fail(BSR_ERR_ARG, "bsr_vgg_per_loss: d_blob must be 16-byte aligned");
  if (reinterpret_cast<uintptr_t>(sums) % 8 != 0) return fail(BSR_ERR_ARG, "bsr_vgg_per_loss: sums must be 8-byte aligned");
  return run_post("bsr_vgg_per_loss", {d_blob, gt, con_rgb, sums, loss1, scratch}, B, S, scratch, device, [&] {
    HIP_TRY(bsr::launch_vgg_per_loss(static_cast<const float*>(d_blob), gt, con_rgb, B, S, sums, loss1, scratch, static_cast<hipStream_t>(stream)));
    return BSR_OK;
  });
}

size_t bsr_vgg_dgrad_blob_bytes(void) { return bsr::vgg_dgrad_w_off(bsr::kVggLayers) * sizeof(float); }

size_t bsr_vgg_grad_scratch_bytes(int B, int S) { return post_size_ok(B, S) && B <= bsr::kVggMaxB ? bsr::vgg_grad_offset(B, S, 2) : 0; }

size_t bsr_vgg_grad_offset(int B, int S, int which) {
  if (!post_size_ok(B, S) || B > bsr::kVggMaxB || which < 0 || which > 1) return SIZE_MAX;
  return bsr::vgg_grad_offset(B, S, which);
}

namespace {

int vgg_per_loss_grad(const char* name, int device, const void* d_blob, size_t blob_bytes, const void* d_dgrad_blob, size_t dgrad_bytes, const float* gt,
                      const float* con_rgb, const float* upstream, int B, int S, double* sums, float* loss1, float* grad, void* scratch, int stop_after,
                      void* stream) {
  const std::string n(name);
  if (B > bsr::kVggMaxB) return fail(BSR_ERR_ARG, n + ": B must be 1..4096");
  if (blob_bytes != bsr_vgg_blob_bytes()) return fail(BSR_ERR_ARG, n + ": blob_bytes must be bsr_vgg_blob_bytes() (pack.pack_vgg)");
  if (dgrad_bytes != bsr_vgg_dgrad_blob_bytes()) return fail(BSR_ERR_ARG, n + ": dgrad_bytes must be bsr_vgg_dgrad_blob_bytes() (pack.pack_vgg_dgrad)");
  if (reinterpret_cast<uintptr_t>(d_blob) % 16 != 0 || reinterpret_cast<uintptr_t>(d_dgrad_blob) % 16 != 0)
    return fail(BSR_ERR_ARG, n + ": d_blob and d_dgrad_blob must be 16-byte aligned");
  if (reinterpret_cast<uintptr_t>(sums) % 8 != 0) return fail(BSR_ERR_ARG, n + ": sums must be 8-byte aligned");
  if (stop_after < 0 || stop_after > bsr::kVggGradLaunches) return fail(BSR_ERR_ARG, n + ": stop_after must be 0..18");
  return run_post(name, {d_blob, d_dgrad_blob, gt, con_rgb, sums, loss1, grad, scratch}, B, S, scratch, device, [&] {
    HIP_TRY(bsr::launch_vgg_per_loss_grad(static_cast<const float*>(d_blob), static_cast<const float*>(d_dgrad_blob), gt, con_rgb, upstream, B, S, sums, loss1,
                                          grad, scratch, stop_after, static_cast<hipStream_t>(stream)));
    return BSR_OK;
  });
}

}  // namespace

int bsr_vgg_per_loss_grad(int device, const void* d_blob, size_t blob_bytes, const void* d_dgrad_blob, size_t dgrad_bytes, const float* gt, const float* con_rgb,
                          const float* upstream, int B, int S, double* sums, float* loss1, float* grad, void* scratch, void* stream) {
  return vgg_per_loss_grad("bsr_vgg_per_loss_grad", device, d_blob, blob_bytes, d_dgrad_blob, dgrad_bytes, gt, con_rgb, upstream, B, S, sums, loss1, grad, scratch,
                           bsr::kVggGradLaunches, stream);
}

int bsr_debug_vgg_per_loss_grad(int device, const void* d_blob, size_t blob_bytes, const void* d_dgrad_blob, size_t dgrad_bytes, const float* gt,
                                const float* con_rgb, const float* upstream, int B, int S, double* sums, float* loss1, float* grad, void* scratch, int stop_after,
                                void* stream) {
  return vgg_per_loss_grad("bsr_debug_vgg_per_loss_grad", device, d_blob, blob_bytes, d_dgrad_blob, dgrad_bytes, gt, con_rgb, upstream, B, S, sums, loss1, grad,
                           scratch, stop_after, stream);
}

size_t bsr_png_file_bytes(int H, int W) {
  bsr::PngGeom g;
  return bsr::png_geometry(H, W, &g) ? (size_t)g.file_bytes : 0;
}

size_t bsr_png_scratch_bytes(int B) { return B > 0 ? (size_t)B * bsr::kPngSub * 4 * sizeof(unsigned long long) : 0; }

int bsr_png_encode(int device, const unsigned char* pixels, int B, int H, int W, unsigned char* out, size_t out_stride, void* scratch, void* stream) {
  if (pixels == nullptr || out == nullptr || scratch == nullptr) return fail(BSR_ERR_ARG, "bsr_png_encode: null argument");
  bsr::PngGeom g;
  if (B <= 0 || !bsr::png_geometry(H, W, &g)) return fail(BSR_ERR_ARG, "bsr_png_encode: B, H, W must be positive, W <= 5461 and H <= 65535");
  if (out_stride < g.file_bytes) return fail(BSR_ERR_ARG, "bsr_png_encode: out_stride is smaller than bsr_png_file_bytes(H, W)");
  if (reinterpret_cast<uintptr_t>(scratch) % 8 != 0) return fail(BSR_ERR_ARG, "bsr_png_encode: scratch must be 8-byte aligned");
  DeviceGuard guard(device);
  HIP_TRY(guard.err);
  bsr::PngFigs none{};
  HIP_TRY(bsr::launch_png_encode(pixels, none, B, g, out, out_stride, static_cast<unsigned long long*>(scratch), static_cast<hipStream_t>(stream)));
  return BSR_OK;
}

int bsr_png_encode_figs(int device, int n_figs, const float* const* figs, const float* const* muls, const float* scales, const int* channels,
                        const int* pixel_strides, const int* mul_strides, int B, int H, int Wf, unsigned char* out, size_t out_stride, void* scratch,
                        void* stream) {
  if (figs == nullptr || channels == nullptr || pixel_strides == nullptr || out == nullptr || scratch == nullptr)
    return fail(BSR_ERR_ARG, "bsr_png_encode_figs: null argument");
  if (n_figs < 1 || n_figs > bsr::kPngMaxFigs) return fail(BSR_ERR_ARG, "bsr_png_encode_figs: 1 to 8 figures per strip");
  bsr::PngGeom g;
  if (B <= 0 || Wf <= 0 || !bsr::png_geometry(H, n_figs * Wf, &g))
    return fail(BSR_ERR_ARG, "bsr_png_encode_figs: B, H, Wf must be positive, the strip's width n_figs * Wf <= 5461 and H <= 65535");
  if (out_stride < g.file_bytes) return fail(BSR_ERR_ARG, "bsr_png_encode_figs: out_stride is smaller than bsr_png_file_bytes(H, n_figs * Wf)");
  if (reinterpret_cast<uintptr_t>(scratch) % 8 != 0) return fail(BSR_ERR_ARG, "bsr_png_encode_figs: scratch must be 8-byte aligned");
  bsr::PngFigs f{};
  f.n = n_figs;
  f.Wf = Wf;
  for (int k = 0; k < n_figs; ++k) {
    if (figs[k] == nullptr || (channels[k] != 1 && channels[k] != 3) || pixel_strides[k] < channels[k])
      return fail(BSR_ERR_ARG, "bsr_png_encode_figs: every figure needs a pointer, 1 or 3 channels and a pixel stride of at least its channels");
    f.ptr[k] = figs[k];
    f.mul[k] = muls != nullptr ? muls[k] : nullptr;
    f.scale[k] = scales != nullptr ? scales[k] : 1.f;
    f.ch[k] = channels[k];
    f.ps[k] = pixel_strides[k];
    f.mps[k] = (mul_strides != nullptr && f.mul[k] != nullptr) ? mul_strides[k] : 1;
    if (f.mul[k] != nullptr && f.mps[k] < 1) return fail(BSR_ERR_ARG, "bsr_png_encode_figs: a multiplier needs a positive pixel stride");
  }
  DeviceGuard guard(device);
  HIP_TRY(guard.err);
  HIP_TRY(bsr::launch_png_encode(nullptr, f, B, g, out, out_stride, static_cast<unsigned long long*>(scratch), static_cast<hipStream_t>(stream)));
  return BSR_OK;
}

size_t bsr_ucb_post_scratch_bytes(int B, int S) { return post_size_ok(B, S) ? (size_t)B * bsr::ucb_item_scratch_bytes(S) : 0; }

int bsr_ucb_post(int device, const float* rows10, const unsigned char* masks, const float* boxes, int B, int S, float* losses,
                 unsigned char* strips, float* figs, int* status, void* scratch, void* stream) {
  return run_post("bsr_ucb_post", {rows10, masks, boxes, losses, strips, status, scratch}, B, S, scratch, device, [&] {
    HIP_TRY(bsr::launch_ucb_post(rows10, masks, boxes, B, S, losses, strips, figs, status, scratch, static_cast<hipStream_t>(stream)));
    return BSR_OK;
  });
}

size_t bsr_ucb_post_rgb_scratch_bytes(int B, int S) { return post_size_ok(B, S) ? (size_t)B * bsr::ucb_rgb_item_scratch_bytes(S) : 0; }

int bsr_ucb_post_rgb(int device, const float* rows9, const unsigned char* masks, const float* boxes, int B, int S, float* losses,
                     unsigned char* strips, float* figs, int* status, void* scratch, void* stream) {
  return run_post("bsr_ucb_post_rgb", {rows9, masks, boxes, losses, strips, status, scratch}, B, S, scratch, device, [&] {
    HIP_TRY(bsr::launch_ucb_post_rgb(rows9, masks, boxes, B, S, losses, strips, figs, status, scratch, static_cast<hipStream_t>(stream)));
    return BSR_OK;
  });
}

size_t bsr_ucb_post_tsm_scratch_bytes(int B, int S) { return post_size_ok(B, S) ? (size_t)B * bsr::ucb_tsm_item_scratch_bytes(S) : 0; }

int bsr_ucb_post_tsm(int device, const float* rows, const unsigned char* masks, const float* boxes, int B, int S, float* losses,
                     double* nose_stats, unsigned char* strips, float* figs, int* status, void* scratch, void* stream) {
  return run_post("bsr_ucb_post_tsm", {rows, masks, boxes, losses, nose_stats, strips, status, scratch}, B, S, scratch, device, [&] {
    HIP_TRY(bsr::launch_ucb_post_tsm(rows, masks, boxes, B, S, losses, nose_stats, strips, figs, status, scratch, static_cast<hipStream_t>(stream)));
    return BSR_OK;
  });
}

size_t bsr_sfw_score_scratch_bytes(int B, int S) { return post_size_ok(B, S) ? (size_t)B * bsr::sfw_item_scratch_bytes(S) : 0; }

int bsr_sfw_score(int device, const float* rows3, int B, int S, float* losses, double* auc, float* pred, float* label, int* status,
                  void* scratch, void* stream) {
  return run_post("bsr_sfw_score", {rows3, losses, auc, pred, label, status, scratch}, B, S, scratch, device, [&] {
    HIP_TRY(bsr::launch_sfw_score(rows3, B, S, losses, auc, pred, label, status, scratch, static_cast<hipStream_t>(stream)));
    return BSR_OK;
  });
}

int bsr_clock_trace(int device, unsigned long long* out, int samples, int spin, const int* stop, int* taken, void* stream) {
  if (out == nullptr || stop == nullptr || taken == nullptr || samples <= 0 || spin < 0) return fail(BSR_ERR_ARG, "bsr_clock_trace: bad argument");
  DeviceGuard guard(device);
  HIP_TRY(guard.err);
  hipLaunchKernelGGL(bsr::clock_trace_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), out, samples, spin, stop, taken);
  HIP_TRY(hipGetLastError());
  return BSR_OK;
}

int bsr_debug_split_qkv(const float* qkv, void* qkv_split, int B, int tokens, void* stream) {
  if (qkv == nullptr || qkv_split == nullptr) return fail(BSR_ERR_ARG, "bsr_debug_split_qkv: null argument");
  if (B <= 0 || tokens <= 0 || tokens % 128 != 0) return fail(BSR_ERR_ARG, "bsr_debug_split_qkv: tokens must be a positive multiple of 128");
  const size_t pairs = (size_t)B * tokens * 192;
  hipLaunchKernelGGL(bsr::a4_split_qkv_kernel, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), qkv,
                     static_cast<char*>(qkv_split), pairs);
  HIP_TRY(hipGetLastError());
  return BSR_OK;
}

int bsr_debug_attention_split(const void* qkv_split, float* y, int B, int tokens, int pv1, void* stream) {
  if (qkv_split == nullptr || y == nullptr) return fail(BSR_ERR_ARG, "bsr_debug_attention_split: null argument");
  if (B <= 0 || tokens <= 0 || tokens % 128 != 0) return fail(BSR_ERR_ARG, "bsr_debug_attention_split: tokens must be a positive multiple of 128");
  HIP_TRY(bsr::launch_nonlocal_attention_h16(static_cast<const float*>(qkv_split), y, B, tokens, static_cast<hipStream_t>(stream), pv1 != 0));
  return BSR_OK;
}

int bsr_debug_attention_dtype(const float* qkv, float* y, int B, int tokens, int dtype, void* stream) {
  if (qkv == nullptr || y == nullptr) return fail(BSR_ERR_ARG, "bsr_debug_attention: null argument");
  if (B <= 0 || tokens <= 0 || tokens % 128 != 0) return fail(BSR_ERR_ARG, "bsr_debug_attention: tokens must be a positive multiple of 128");
  if (dtype == BSR_DTYPE_F32) {
    HIP_TRY(bsr::launch_nonlocal_attention(qkv, y, B, tokens, static_cast<hipStream_t>(stream)));
  } else if (dtype == BSR_DTYPE_F32X3 || dtype == BSR_DTYPE_F16) {
    // the kernel of the 16-bit modes reads theta|phi|g as their producer leaves them (split into fp16 planes: attention_h16.h); this
    // hook splits a scratch copy first (allocated and freed here: a test hook, not a hot path)
    void* tmp = nullptr;
    HIP_TRY(hipMalloc(&tmp, (size_t)B * tokens * bsr::kA4TokBytes));
    int rc = bsr_debug_split_qkv(qkv, tmp, B, tokens, stream);
    if (rc == BSR_OK) rc = bsr_debug_attention_split(tmp, y, B, tokens, 0, stream);
    hipError_t e = hipStreamSynchronize(static_cast<hipStream_t>(stream));
    hipFree(tmp);
    if (rc != BSR_OK) return rc;
    HIP_TRY(e);
  } else {
    return fail(BSR_ERR_ARG, "bsr_debug_attention: unknown dtype");
  }
  return BSR_OK;
}

int bsr_debug_attention_qw(const float* qkv, float* y, int B, int tokens, int qw, void* stream) {
  if (qkv == nullptr || y == nullptr) return fail(BSR_ERR_ARG, "bsr_debug_attention_qw: null argument");
  if (B <= 0 || tokens <= 0 || tokens % 128 != 0) return fail(BSR_ERR_ARG, "bsr_debug_attention_qw: tokens must be a positive multiple of 128");
  if (qw != 0 && qw != 1 && qw != 2 && qw != 4) return fail(BSR_ERR_ARG, "bsr_debug_attention_qw: qw must be 0 (automatic), 1, 2 or 4 query waves per workgroup");
  HIP_TRY(bsr::launch_nonlocal_attention(qkv, y, B, tokens, static_cast<hipStream_t>(stream), qw));
  return BSR_OK;
}

int bsr_debug_attention_kv1(const float* qkv2, float* y, int B, int tokens, int qw, void* stream) {
  if (qkv2 == nullptr || y == nullptr) return fail(BSR_ERR_ARG, "bsr_debug_attention_kv1: null argument");
  if (B <= 0 || tokens <= 0 || tokens % 128 != 0) return fail(BSR_ERR_ARG, "bsr_debug_attention_kv1: tokens must be a positive multiple of 128");
  if (qw != 0 && qw != 1 && qw != 2 && qw != 4) return fail(BSR_ERR_ARG, "bsr_debug_attention_kv1: qw must be 0 (automatic), 1, 2 or 4 query waves per workgroup");
  HIP_TRY(bsr::launch_nonlocal_attention<true>(qkv2, y, B, tokens, static_cast<hipStream_t>(stream), qw));
  return BSR_OK;
}

int bsr_debug_attention_rgb(const float* qkv, float* y, int B, int tokens, void* stream) {
  if (qkv == nullptr || y == nullptr) return fail(BSR_ERR_ARG, "bsr_debug_attention_rgb: null argument");
  if (B <= 0 || tokens <= 0 || tokens % 32 != 0) return fail(BSR_ERR_ARG, "bsr_debug_attention_rgb: tokens must be a positive multiple of 32");
  HIP_TRY(bsr::launch_nonlocal_attention256(qkv, y, B, tokens, static_cast<hipStream_t>(stream)));
  return BSR_OK;
}

int bsr_debug_wino_conv(const float* x, const float* w, const float* bias, float* y, int B, int H, int W, int nw, void* stream) {
  if (x == nullptr || w == nullptr || bias == nullptr || y == nullptr) return fail(BSR_ERR_ARG, "bsr_debug_wino_conv: null argument");
  if (B <= 0 || H <= 0 || W <= 0 || H % 4 != 0 || W % 32 != 0) return fail(BSR_ERR_ARG, "bsr_debug_wino_conv: H must be a positive multiple of 4 and W of 32");
  if ((long long)B * H * W * 128 * 4 >= (1LL << 31)) return fail(BSR_ERR_ARG, "bsr_debug_wino_conv: tensor too large");
  if (nw != 0 && nw != 2 && nw != 4 && nw != 8) return fail(BSR_ERR_ARG, "bsr_debug_wino_conv: nw must be 0 (automatic), 2, 4 or 8 waves per workgroup");
  HIP_TRY(bsr::launch_wino_conv2(wino_args(x, y, w, bias, H, W), B, static_cast<hipStream_t>(stream), nw));
  return BSR_OK;
}

int bsr_debug_wino_convt(const float* x, const float* w_direct, const float* bias, float* y, int B, int H, int W, int cin, int cout, int in_cs,
                         int out_cs, int act, void* stream) {
  if (x == nullptr || w_direct == nullptr || bias == nullptr || y == nullptr) return fail(BSR_ERR_ARG, "bsr_debug_wino_convt: null argument");
  if (const char* why = bsr::wino_convt_refusal(B, H, W, cin, cout, in_cs, out_cs)) return fail(BSR_ERR_ARG, std::string("bsr_debug_wino_convt: ") + why);
  if ((long long)B * H * W * in_cs * 4 >= (1LL << 40)) return fail(BSR_ERR_ARG, "bsr_debug_wino_convt: tensor too large");
  hipStream_t s = static_cast<hipStream_t>(stream);
  std::vector<float> u(wino_convt_floats(cin));
  wino_convt_filter_transform(w_direct, u.data(), cin);
  float* d_u = nullptr;
  HIP_TRY(hipMalloc(reinterpret_cast<void**>(&d_u), u.size() * sizeof(float)));
  hipError_t e = hipMemcpy(d_u, u.data(), u.size() * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    bsr::WinoTArgs a{};
    a.in = x; a.out = y; a.w = d_u; a.bias = bias; a.H = H; a.W = W; a.in_cs = in_cs; a.out_cs = out_cs; a.nchunk = cin / 16; a.act = act ? 1 : 0;
    e = bsr::launch_wino_convt(a, B, s);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  hipFree(d_u);
  HIP_TRY(e);
  return BSR_OK;
}

int bsr_debug_wino_convt_filter(const float* direct, float* out, int cin) {
  if (direct == nullptr || out == nullptr) return fail(BSR_ERR_ARG, "bsr_debug_wino_convt_filter: null argument");
  if (cin <= 0 || cin % 16 != 0) return fail(BSR_ERR_ARG, "bsr_debug_wino_convt_filter: Cin must be a positive multiple of 16");
  wino_convt_filter_transform(direct, out, cin);
  return BSR_OK;
}

int bsr_debug_wino_clr_filter(const float* direct, const float* w_gs, float* out) {
  if (direct == nullptr || w_gs == nullptr || out == nullptr) return fail(BSR_ERR_ARG, "bsr_debug_wino_clr_filter: null argument");
  wino_clr_filter_transform(direct, w_gs, out);
  return BSR_OK;
}

int bsr_debug_wino_clr(const float* gs, const float* f, int in_cs, const float* inputs, const float* w_direct, const float* w_gs, const float* bias,
                       const float* tail_w, float* con_rgb, float* dif, float* packed, int B, int H, int W, int wino, void* stream) {
  if (gs == nullptr || f == nullptr || inputs == nullptr || w_direct == nullptr || w_gs == nullptr || bias == nullptr || tail_w == nullptr)
    return fail(BSR_ERR_ARG, "bsr_debug_wino_clr: null argument");
  if (packed == nullptr && (con_rgb == nullptr || dif == nullptr)) return fail(BSR_ERR_ARG, "bsr_debug_wino_clr: neither packed nor con_rgb | dif given");
  if (const char* why = bsr::wino_clr_refusal(B, H, W, in_cs)) return fail(BSR_ERR_ARG, std::string("bsr_debug_wino_clr: ") + why);
  hipStream_t s = static_cast<hipStream_t>(stream);
  // one device image of the weights (HOST pointers): direct [2][9][16][36] | gs [16][16] | bias [16] | tail [337 -> 340] | U
  constexpr size_t kDirect = 2 * 9 * 16 * 36, kGs = kDirect, kBias = kGs + 256, kTail = kBias + 16, kU = kTail + 340;
  std::vector<float> img(kU + kWinoClrFloats, 0.f);
  memcpy(img.data(), w_direct, kDirect * sizeof(float));
  memcpy(img.data() + kGs, w_gs, 256 * sizeof(float));
  memcpy(img.data() + kBias, bias, 16 * sizeof(float));
  memcpy(img.data() + kTail, tail_w, 337 * sizeof(float));
  wino_clr_filter_transform(w_direct, w_gs, img.data() + kU);
  float* d = nullptr;
  HIP_TRY(hipMalloc(reinterpret_cast<void**>(&d), img.size() * sizeof(float)));
  hipError_t e = hipMemcpy(d, img.data(), img.size() * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    bsr::ConvN16Args a{};
    a.in = f; a.in_cs = in_cs; a.H = H; a.W = W; a.w = wino ? d + kU : d; a.bias = d + kBias; a.act = 1; a.pad_t = 1; a.pad_l = 1;
    a.gs = gs; a.w_gs = d + kGs; a.tail_w = d + kTail; a.inputs = inputs; a.con_rgb = con_rgb; a.dif = dif; a.packed = packed;
    e = wino ? bsr::launch_wino_clr(a, B, s) : bsr::launch_conv_n16<3, 3, true, true, 2>(a, B, s);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  hipFree(d);
  HIP_TRY(e);
  return BSR_OK;
}

int bsr_debug_wino_filter(const float* direct, float* out) {
  if (direct == nullptr || out == nullptr) return fail(BSR_ERR_ARG, "bsr_debug_wino_filter: null argument");
  wino_filter_transform(direct, out);
  return BSR_OK;
}

int bsr_debug_keys_compose(const float* c3q_w, const float* c3q_b, float* out_w, float* out_b) {
  if (c3q_w == nullptr || c3q_b == nullptr || out_w == nullptr || out_b == nullptr) return fail(BSR_ERR_ARG, "bsr_debug_keys_compose: null argument");
  keys_compose(c3q_w, c3q_b, out_w, out_b);
  return BSR_OK;
}

int bsr_debug_values_compose(const float* c3q_w, const float* c3q_b, const float* w_w, const float* w_b, float* out_w, float* out_b) {
  if (c3q_w == nullptr || c3q_b == nullptr || w_w == nullptr || w_b == nullptr || out_w == nullptr || out_b == nullptr)
    return fail(BSR_ERR_ARG, "bsr_debug_values_compose: null argument");
  values_compose(c3q_w, c3q_b, w_w, w_b, out_w, out_b);
  return BSR_OK;
}

int bsr_debug_attention(const float* qkv, float* y, int B, int tokens, void* stream) {
  return bsr_debug_attention_dtype(qkv, y, B, tokens, BSR_DTYPE_F32, stream);
}

// bsr_probe's name tables: where a named intermediate of the last forward lies in the workspace.  half: an fp16 tensor (f16 mode).
// derive: an att<i> probe of a forward that kept O = softmax(f) t2 in the slot: bsr_probe computes att = O Wg + bg of block `derive` - 1 first.
struct ProbeSrc { size_t off; int hh, ww, cs, coff, c; bool half; int derive; };

// `prefix` followed by one digit below n: the digit, else -1
static int probe_index(const std::string& nm, const char* prefix, int n) {
  const size_t len = strlen(prefix);
  if (nm.size() == len + 1 && nm.compare(0, len, prefix) == 0 && nm[len] >= '0' && nm[len] < '0' + n) return nm[len] - '0';
  return -1;
}

static int probe_src_rgb(const bsr_handle* h, const std::string& nm, ProbeSrc* src) {
  const Plan& p = h->plan;
  const int H = h->H, W = h->W;
  int i;
  if (nm == "x1") *src = {p.x1, H, W, 32, 0, 32};
  else if (nm == "x2") *src = {p.c3, H / 2, W / 2, RGB_CS_C3, 128, 64};
  else if (nm == "x3") *src = {p.c2, H / 4, W / 4, RGB_CS_C2, 192, 64};
  else if (nm == "x0") *src = {p.xa, H / 8, W / 8, RGB_CS_A, 0, 99};
  else if ((i = probe_index(nm, "res", 3)) >= 0) *src = {p.r[i], H / 8, W / 8, RGB_CS_R, 0, 513};
  else if ((i = probe_index(nm, "att", 3)) >= 0) *src = {p.att[i], H / 8, W / 8, RGB_D, 0, RGB_D};
  else if ((i = probe_index(nm, "y3x", 3)) >= 0) *src = {p.y3[i], H / 8, W / 8, RGB_CS_R, 0, 513};
  else if (nm == "up1") *src = {p.c2, H / 4, W / 4, RGB_CS_C2, 0, 192};
  else if (nm == "up2") *src = {p.c3, H / 2, W / 2, RGB_CS_C3, 0, 128};
  else if (nm == "up3") *src = {p.ybuf, H, W, 128, 0, 128};
  else if (nm == "y") *src = {p.yh, H, W, 3, 0, 3};
  else if (nm == "con") *src = {p.con, H, W, 3, 0, 3};
  else return fail(BSR_ERR_STATE, "bsr_probe: unknown probe '" + nm + "' for an RGB handle");
  return BSR_OK;
}

static int probe_src_gsc(const bsr_handle* h, const std::string& nm, ProbeSrc* src) {
  const Plan& p = h->plan;
  const Variant& v = h->var;
  const int H = h->H, W = h->W;
  const bool p16 = h->dtype == BSR_DTYPE_F16;          // the tensors the f16 mode keeps as fp16 (forward_impl)
  int i;
  if (nm == "x1") *src = {p.x1, H, W, 32, 0, 32, p16};
  else if (nm == "x2") *src = {p.c3, H / 2, W / 2, 128, 64, 64, p16};
  else if (nm == "x3") *src = {p.c2, H / 4, W / 4, 160, 96, 64, p16};
  else if (nm == "x0") *src = {p.xa, H / 8, W / 8, v.cs_a, 0, v.c_a};
  else if ((i = probe_index(nm, "res", 6)) >= 0) *src = {p.r[i], H / 8, W / 8, i < 3 ? v.cs_r : v.cs_h, 0, i < 3 ? v.c_r : v.c_h};
  else if ((i = probe_index(nm, "att", 6)) >= 0) {
    // fused attention + w (fp32, full batches): the attention output stays in LDS, the att<i> slots hold whatever an earlier
    // forward left there — refuse rather than hand out stale data
    if (h->att_in_lds)
      return fail(BSR_ERR_STATE, "bsr_probe: att<i> does not exist for the last forward — attention and the `w` GEMM ran as one launch and the "
                                 "attention output never left LDS (create the handle with BSR_FUSE_ATTW=0 in the environment to probe it)");
    *src = {p.att[i], H / 8, W / 8, 128, 0, 128, false, h->att_is_o ? i + 1 : 0};
  }
  else if ((i = probe_index(nm, "attv", 6)) >= 0) {      // the attention over conv2's output as the values, O = softmax(f) t2, as the kernel stored it
    if (!h->att_is_o) return fail(BSR_ERR_STATE, "bsr_probe: attv<i> exists only for a forward with conv2's output as the attention values (fp32, BSR_KEYS_CONV2 and BSR_VALUES_CONV2 on)");
    if (h->att_in_lds)
      return fail(BSR_ERR_STATE, "bsr_probe: attv<i> does not exist for the last forward — attention and the `w` GEMM ran as one launch and the "
                                 "attention output never left LDS (create the handle with BSR_FUSE_ATTW=0 in the environment to probe it)");
    *src = {p.att[i], H / 8, W / 8, 128, 0, 128};
  }
  else if (nm == "qkv") {      // the rows the LAST block's attention read (one buffer serves all six blocks): fp32 handles only
    if (h->dtype != BSR_DTYPE_F32) return fail(BSR_ERR_STATE, "bsr_probe: qkv is an fp32 tensor of BSR_DTYPE_F32 handles only");
    const int c = h->att_is_o ? 256 : 384;
    *src = {p.qkv, H / 8, W / 8, c, 0, c};
  }
  else if ((i = probe_index(nm, "y3x", 6)) >= 0) *src = {p.y3[i], H / 8, W / 8, CS_Y3X, 0, CS_Y3X};
  else if (nm == "up1") *src = {p.c2, H / 4, W / 4, 160, 0, 96, p16};
  else if (nm == "up2") *src = {p.c3, H / 2, W / 2, 128, 0, 64, p16};
  else if (nm == "y") *src = {p.ybuf, H, W, 64, 0, 64, p16};
  else if (nm == "d32") *src = {p.probe, H / 8, W / 8, 2, 0, 1};
  else if (nm == "bmask") *src = {p.probe, H / 8, W / 8, 2, 1, 1};
  else if (nm == "xh") *src = {p.xh, H / 8, W / 8, v.cs_h, 0, v.c_h};
  else if (nm == "f1") *src = {p.f1, H / 4, W / 4, 128, 0, 128, p16};
  else if (nm == "f2") *src = {p.f2, H / 2, W / 2, 96, 0, 96, p16};
  else if (nm == "f") *src = {p.cf, H, W, CS_CF, 0, 64, p16};
  else return fail(BSR_ERR_STATE, "bsr_probe: unknown probe '" + nm + "'");
  return BSR_OK;
}

int bsr_probe(bsr_handle* h, const char* name, float* dst, size_t cap_floats, int shape4[4], void* stream) {
  if (h == nullptr || name == nullptr || dst == nullptr || shape4 == nullptr) return fail(BSR_ERR_ARG, "bsr_probe: null argument");
  if (!h->ran) return fail(BSR_ERR_STATE, "bsr_probe: no forward has run on this handle");
  DeviceGuard guard(h->device);
  HIP_TRY(guard.err);
  ProbeSrc src{};
  const int rc = h->var.rgb ? probe_src_rgb(h, name, &src) : probe_src_gsc(h, name, &src);
  if (rc != BSR_OK) return rc;
  const size_t npix = (size_t)h->B * src.hh * src.ww;
  shape4[0] = h->B; shape4[1] = src.hh; shape4[2] = src.ww; shape4[3] = src.c;
  if (npix * src.c > cap_floats) return fail(BSR_ERR_ARG, "bsr_probe: destination too small");
  const float* from = h->ws + src.off;
  if (src.derive) {
    // att = O Wg + bg, the reference's softmax(f) g: one K = 128, N = 128 GEMM with the block's own g columns into a scratch of the handle's
    if (h->att_scratch_floats < npix * 128) {
      if (h->att_scratch) hipFree(h->att_scratch);
      h->att_scratch = nullptr;
      h->att_scratch_floats = 0;
      HIP_TRY(hipMalloc(reinterpret_cast<void**>(&h->att_scratch), npix * 128 * sizeof(float)));
      h->att_scratch_floats = npix * 128;
    }
    const float* img = h->d_values + (size_t)(src.derive - 1) * kValuesFloats + kValuesWFloats + kValuesC3qFloats;
    bsr::ConvArgs a{};
    a.in = from; a.in_cs = 128; a.out = h->att_scratch; a.out_cs = 128;
    a.w = img; a.bias = img + (size_t)4 * kGProbeNPad * 36; a.nchunk = 4; a.n_pad = kGProbeNPad; a.n_store = 128; a.act = 0;
    HIP_TRY((bsr::launch_gemm_nloop<3, 4, 0, 2>(a, npix, 2, static_cast<hipStream_t>(stream))));
    from = h->att_scratch;
  }
  hipLaunchKernelGGL(bsr::slice_copy_kernel, dim3((unsigned)((npix * src.c + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     from, src.cs, src.coff, src.c, dst, npix, src.half ? 1 : 0);
  HIP_TRY(hipGetLastError());
  return BSR_OK;
}

int bsr_last_f(bsr_handle* h, const float** f, int* f_cs, int shape4[4]) {
  if (h == nullptr || f == nullptr || f_cs == nullptr || shape4 == nullptr) return fail(BSR_ERR_ARG, "bsr_last_f: null argument");
  if (h->var.rgb) return fail(BSR_ERR_STATE, "bsr_last_f: an RGB handle has no colour tail");
  if (h->dtype != BSR_DTYPE_F32) return fail(BSR_ERR_STATE, "bsr_last_f: f is an fp32 tensor of BSR_DTYPE_F32 handles only (the 16-bit modes keep it as fp16)");
  if (!h->ran) return fail(BSR_ERR_STATE, "bsr_last_f: no forward has run on this handle");
  *f = h->ws + h->plan.cf;
  *f_cs = CS_CF;
  shape4[0] = h->B; shape4[1] = h->H; shape4[2] = h->W; shape4[3] = 64;
  return BSR_OK;
}

int bsr_last_y(bsr_handle* h, const float** y, int* y_cs, int shape4[4]) {
  if (h == nullptr || y == nullptr || y_cs == nullptr || shape4 == nullptr) return fail(BSR_ERR_ARG, "bsr_last_y: null argument");
  if (h->var.rgb) return fail(BSR_ERR_STATE, "bsr_last_y: an RGB handle has no grey heads");
  if (h->dtype != BSR_DTYPE_F32) return fail(BSR_ERR_STATE, "bsr_last_y: y is an fp32 tensor of BSR_DTYPE_F32 handles only (the 16-bit modes keep it as fp16)");
  if (!h->ran) return fail(BSR_ERR_STATE, "bsr_last_y: no forward has run on this handle");
  *y = h->ws + h->plan.ybuf;
  *y_cs = h->var.cs_y;
  shape4[0] = h->B; shape4[1] = h->H; shape4[2] = h->W; shape4[3] = 64;
  return BSR_OK;
}

int bsr_last_decoder(bsr_handle* h, const float** x, int* x_cs, const float** f1, const float** f2, const float** f, int shape4[4]) {
  if (h == nullptr || x == nullptr || x_cs == nullptr || f1 == nullptr || f2 == nullptr || f == nullptr || shape4 == nullptr)
    return fail(BSR_ERR_ARG, "bsr_last_decoder: null argument");
  if (h->var.rgb) return fail(BSR_ERR_STATE, "bsr_last_decoder: an RGB handle has no colour decoder");
  if (h->var.tsm) return fail(BSR_ERR_STATE, "bsr_last_decoder: the colour decoder's backward takes the GSC width 261 only, not a TSM handle's 877");
  if (h->dtype != BSR_DTYPE_F32)
    return fail(BSR_ERR_STATE, "bsr_last_decoder: the decoder's tensors are fp32 in BSR_DTYPE_F32 handles only (the 16-bit modes keep them as fp16)");
  if (!h->ran) return fail(BSR_ERR_STATE, "bsr_last_decoder: no forward has run on this handle");
  *x = h->ws + h->plan.r[5];
  *x_cs = h->var.cs_h;
  *f1 = h->ws + h->plan.f1;
  *f2 = h->ws + h->plan.f2;
  *f = h->ws + h->plan.cf;
  shape4[0] = h->B; shape4[1] = h->H; shape4[2] = h->W; shape4[3] = 64;
  return BSR_OK;
}

int bsr_last_grey_decoder(bsr_handle* h, const float** x, int* x_cs, const float** c2, int* c2_cs, const float** c3, int* c3_cs, const float** y, int* y_cs,
                          int shape4[4]) {
  if (h == nullptr || x == nullptr || x_cs == nullptr || c2 == nullptr || c2_cs == nullptr || c3 == nullptr || c3_cs == nullptr || y == nullptr ||
      y_cs == nullptr || shape4 == nullptr)
    return fail(BSR_ERR_ARG, "bsr_last_grey_decoder: null argument");
  if (h->var.rgb) return fail(BSR_ERR_STATE, "bsr_last_grey_decoder: the grey decoder's backward takes the GSC widths only, not an RGB handle's 513");
  if (h->var.tsm) return fail(BSR_ERR_STATE, "bsr_last_grey_decoder: the grey decoder's backward takes the GSC width 257 only, not a TSM handle's 291");
  if (h->dtype != BSR_DTYPE_F32)
    return fail(BSR_ERR_STATE, "bsr_last_grey_decoder: the decoder's tensors are fp32 in BSR_DTYPE_F32 handles only (the 16-bit modes keep them as fp16)");
  if (!h->ran) return fail(BSR_ERR_STATE, "bsr_last_grey_decoder: no forward has run on this handle");
  *x = h->ws + h->plan.r[2];
  *x_cs = h->var.cs_r;
  *c2 = h->ws + h->plan.c2;
  *c2_cs = h->var.cs_c2;
  *c3 = h->ws + h->plan.c3;
  *c3_cs = h->var.cs_c3;
  *y = h->ws + h->plan.ybuf;
  *y_cs = h->var.cs_y;
  shape4[0] = h->B; shape4[1] = h->H; shape4[2] = h->W; shape4[3] = 64;
  return BSR_OK;
}

// bsr_last_block and bsr_last_block5 under the caller's own name
static int last_block(const char* name, bsr_handle* h, int block, const float** y3x, int* y3x_cs, const float** xin, const float** out, int* x_cs,
                      int shape4[4]) {
  const std::string n(name);
  if (h == nullptr || y3x == nullptr || y3x_cs == nullptr || xin == nullptr || out == nullptr || x_cs == nullptr || shape4 == nullptr)
    return fail(BSR_ERR_ARG, n + ": null argument");
  if (block < 3 || block > 5) return fail(BSR_ERR_ARG, n + ": block must be 3, 4 or 5 (the 261-wide blocks)");
  if (h->var.rgb) return fail(BSR_ERR_STATE, n + ": an RGB handle has no res_stack/" + std::to_string(block));
  if (h->var.tsm) return fail(BSR_ERR_STATE, n + ": the non-local block's backward takes the GSC width 261 only, not a TSM handle's 877");
  if (h->dtype != BSR_DTYPE_F32)
    return fail(BSR_ERR_STATE, n + ": the block's tensors are kept for the backward in BSR_DTYPE_F32 handles only, not in the 16-bit modes");
  if (!h->ran) return fail(BSR_ERR_STATE, n + ": no forward has run on this handle");
  // forward_impl's res_block(i) alone writes y3[i] (c3q) and r[i] (the `w` GEMM, fused into the attention launch or on its own), and
  // bmask_xhole alone writes xh: on both routes nothing after block 3 or 4 touches their slots
  *y3x = h->ws + h->plan.y3[block];
  *y3x_cs = h->var.cs_y3x;
  *xin = h->ws + (block == 3 ? h->plan.xh : h->plan.r[block - 1]);
  *out = h->ws + h->plan.r[block];
  *x_cs = h->var.cs_h;
  shape4[0] = h->B; shape4[1] = h->H / 8; shape4[2] = h->W / 8; shape4[3] = 261;
  return BSR_OK;
}

int bsr_last_block(bsr_handle* h, int block, const float** y3x, int* y3x_cs, const float** xin, const float** out, int* x_cs, int shape4[4]) {
  return last_block("bsr_last_block", h, block, y3x, y3x_cs, xin, out, x_cs, shape4);
}

int bsr_last_block5(bsr_handle* h, const float** y3x, int* y3x_cs, const float** xin, const float** out, int* x_cs, int shape4[4]) {
  return last_block("bsr_last_block5", h, 5, y3x, y3x_cs, xin, out, x_cs, shape4);
}

int bsr_last_lower_trunk(bsr_handle* h, const float* tensors7[7], int strides7[7], int shape4[4]) {
  if (h == nullptr || tensors7 == nullptr || strides7 == nullptr || shape4 == nullptr) return fail(BSR_ERR_ARG, "bsr_last_lower_trunk: null argument");
  if (h->var.rgb) return fail(BSR_ERR_STATE, "bsr_last_lower_trunk: the lower trunk's backward takes the GSC width 257 only, not an RGB handle's 513");
  if (h->var.tsm) return fail(BSR_ERR_STATE, "bsr_last_lower_trunk: the lower trunk's backward takes the GSC width 257 only, not a TSM handle's 291");
  if (h->dtype != BSR_DTYPE_F32)
    return fail(BSR_ERR_STATE, "bsr_last_lower_trunk: the blocks' tensors are kept for the backward in BSR_DTYPE_F32 handles only, not in the 16-bit modes");
  if (!h->ran) return fail(BSR_ERR_STATE, "bsr_last_lower_trunk: no forward has run on this handle");
  // make_plan gives xa, every y3[i] and every r[i] a slot of its own.  forward_impl's down3 and uv_resize8 alone write xa, both ahead of
  // res_block(0); res_block(i) alone writes y3[i] and r[i]; up1 and bmask_xhole only read r[2]: nothing after block 0 touches xa, and
  // nothing after block i its y3[i] and r[i]
  for (int k = 0; k < 3; ++k) {
    tensors7[2 * k] = h->ws + h->plan.y3[2 - k];
    strides7[2 * k] = h->var.cs_y3x;
    tensors7[2 * k + 1] = h->ws + h->plan.r[2 - k];
    strides7[2 * k + 1] = h->var.cs_r;
  }
  tensors7[6] = h->ws + h->plan.xa;
  strides7[6] = h->var.cs_a;
  shape4[0] = h->B; shape4[1] = h->H / 8; shape4[2] = h->W / 8; shape4[3] = 257;
  return BSR_OK;
}

}  // extern "C"
