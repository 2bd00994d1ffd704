/* libbsr_hip — C ABI of the MI355X-native GSC generator forward pass.
 *
 * The reference has no FFI / plugin boundary: the hot path is entered through a Python call on a
 * tf.keras.Model,
 *     deshadow_img_gs, deshadow_img_c, _, mask_pred = self.gen(img, uv, reg, chuck=1, training=False)
 * (/root/reference/train_test_GSC.py:422, :871; Generator.call at /root/reference/model.py:228-290).
 * This header is what a binding for that call site binds instead (INTEGRATION.md shows the ctypes stub):
 * plain pointers and sizes, no framework types.  All tensor pointers are DEVICE pointers owned by the
 * caller (NHWC float32, dense); the library owns only its packed weights and its activation workspace.
 *
 * Threading: a handle is bound to one device and is not re-entrant; bsr_forward is asynchronous on the
 * given hipStream_t and the caller synchronises.  Multi-GPU = one handle per device (deployment: one process per GPU;
 * one process may also hold handles on several devices — per-device launch state is kept per device ordinal).  Every
 * entry point switches to the handle's device and restores the caller's current device before returning.
 * Every function returns 0 on success or a non-zero code; bsr_last_error() describes the last failure
 * of the calling thread.
 */
#ifndef BSR_HIP_H_
#define BSR_HIP_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bsr_handle bsr_handle;

#define BSR_OK 0
#define BSR_ERR_ARG 1      /* bad argument / shape */
#define BSR_ERR_BLOB 2     /* malformed or mismatching packed-weight blob */
#define BSR_ERR_HIP 3      /* a HIP runtime call failed */
#define BSR_ERR_STATE 4    /* probe requested before any forward, unknown probe name, ... */
#define BSR_ERR_RANGE 5    /* 16-bit modes: an activation did not fit fp16 (|x| >= 65520) — see bsr_check_range */

#define BSR_DTYPE_F32 0
#define BSR_DTYPE_F16 1     /* BASELINE configs[3]: fp16 operands (fp32 accumulate) on the 3x3-conv path via v_mfma_f32_32x32x16_f16, with the tensors between
                               those layers kept as fp16 in the library's workspace; trunk, 1x1 / attention kernels (split precision) and all
                               inputs / outputs of the ABI stay fp32.  ~1.3e-3 absolute accuracy */
#define BSR_DTYPE_F32X3 2   /* split-precision fp32: every operand of the matrix kernels is split into hi + lo fp16 halves at staging time and contracted
                               with three fp16 matrix instructions (hi.hi + hi.lo + lo.hi, fp32 accumulate) at 16/3 of the fp32 matrix rate.
                               Accuracy: x = hi + lo to 2^-22 |x| while |x| >= 2^-3; smaller operands carry an absolute error of up to 2^-25
                               (lo is an unscaled fp16 subnormal), i.e. 2^-17..2^-20 relative for typical folded weights — the 1e-3 end-to-end
                               parity bar holds with the fp32 path's margin (measured 4.5e-6), it is NOT 2^-22 per product.  Activations / outputs
                               stay fp32.  Range: |activation| must stay below 65504 (fp16 max); a violation is DETECTED on the device and
                               reported as BSR_ERR_RANGE (bsr_check_range), never silently turned into inf / NaN outputs. */

/* Replaces Generator() construction + tf.train.Checkpoint(generator=...).restore(...)
 * (/root/reference/train_test_GSC.py:120, :143-148, :365, :845).
 * packed_weights: HOST pointer to the blob written by blindshadowremoval_amd.pack.pack_generator()
 * (BatchNorm folded, MFMA-friendly layout); it is copied to the device, the caller may free it.
 * dtype: BSR_DTYPE_F32 (the arithmetic type of the measured path), BSR_DTYPE_F16 or BSR_DTYPE_F32X3; the blob must have been packed
 * for the same dtype (pack_generator(weights, dtype): the 16-bit modes carry fp16 weight planes for the 3x3-conv layers). */
int bsr_create(bsr_handle** out, int device, const void* packed_weights, size_t nbytes, int dtype);

/* Replaces Generator.call(inputs, uv, reg, chuck, training=False) (/root/reference/model.py:228-290).
 * inputs, uv : [B,H,W,3] float32 device pointers (reg / chuck are unused by the reference's GSC forward).
 * gs [B,H,W,1], con_rgb [B,H,W,3], mask22 [B,H,W,3], dif [B,H,W,1] : caller-allocated outputs, in the order
 * of the reference's return statement (model.py:290).  H % 32 == 0 and W % 256 == 0 (reference: 256 x 256).
 * stream: a hipStream_t (NULL = default stream). */
int bsr_forward(bsr_handle* h, const float* inputs, const float* uv, int B, int H, int W,
                float* gs, float* con_rgb, float* mask22, float* dif, void* stream);

/* bsr_forward with the two outputs the reference's callers consume (train_test_GSC.py:871-873: deshadow_img_c, mask_pred) written as
 * ONE tensor con_rgb_dif [B,H,W,4] = con_rgb(3) | dif(1): the payload of the multi-GPU output all-gather (one 16-byte store per pixel,
 * no separate packing pass).  Values are bit-identical to bsr_forward's con_rgb / dif. */
int bsr_forward_packed(bsr_handle* h, const float* inputs, const float* uv, int B, int H, int W,
                       float* gs, float* con_rgb_dif, float* mask22, void* stream);

/* TSM variant (BASELINE config 5): replaces Generator.call(inputs, uv, reg, frame, share, chuck, training=False) of
 * /root/reference/model_with_TSM.py:261-325 (call site /root/reference/train_with_TSM.py:676).  The handle must have been
 * created from TSM weights (res_stack/0/conv1 with 291 input channels).  reg: [B,H,W,6] = reg_in(3) | reg_out(3) offset
 * fields (image-fraction units); consecutive groups of `frame` images share features through the UV/offset warp
 * (ShareLayer, model_with_TSM.py:199-229; warp.py:134-165).  share = 0 reproduces the tf.cond(share, ...) false branch. */
int bsr_forward_tsm(bsr_handle* h, const float* inputs, const float* uv, const float* reg, int B, int H, int W, int frame, int share,
                    float* gs, float* con_rgb, float* mask22, float* dif, void* stream);

/* The single-stage RGB baseline (added in ABI 8: additive, no existing signature changed): replaces Generator.call(inputs, uv, reg, chuck, training=False) of /root/reference/model_RGB.py:228-266
 * (call site /root/reference/train_RGB_test.py:414).  The handle must have been created from RGB weights (pack_generator of the
 * model_RGB.py variable set; bsr_create recognises them and accepts BSR_DTYPE_F32 only).  con [B,H,W,3]: caller-allocated output, the
 * reference's only return value.  Same shape rules as bsr_forward; asynchronous and allocation-free after bsr_reserve.  bsr_forward /
 * bsr_forward_tsm refuse an RGB handle and this entry refuses a GSC or TSM one (BSR_ERR_ARG).  Probes: x1 x2 x3 x0 y3x<i> att<i> res<i>
 * (i < 3) up1 up2 up3 y (conv2's output) con.  bsr_workspace_bytes(B,H,W) describes GSC handles; use bsr_handle_workspace_bytes. */
int bsr_forward_rgb(bsr_handle* h, const float* inputs, const float* uv, int B, int H, int W, float* con, void* stream);

/* Range guard of BSR_DTYPE_F32X3 / BSR_DTYPE_F16.  Those modes convert fp32 activations to fp16 operands inside the kernels; a value of
 * magnitude >= 65520 would become inf (and its lo half NaN) where the fp32 path stays finite.  Every converting kernel checks what
 * it converts and sets a sticky, host-visible flag on the handle.  bsr_check_range synchronises `stream` (the stream the forwards
 * ran on), returns BSR_ERR_RANGE if any forward since the last call overflowed — the outputs of those forwards must be discarded
 * and the inputs re-run on a BSR_DTYPE_F32 handle — and clears the flag.  Without a call the condition is still not silent:
 * bsr_forward / bsr_forward_tsm refuse with BSR_ERR_RANGE once a completed forward has raised the flag.  Always BSR_OK on a
 * BSR_DTYPE_F32 handle.  (NaN inputs are not a range error; they propagate to the outputs.) */
int bsr_check_range(bsr_handle* h, void* stream);
/* The same condition WITHOUT synchronising and WITHOUT clearing it: BSR_ERR_RANGE if any forward that has completed so far raised the
 * flag.  For pipelined callers that keep several forwards in flight and wait on their own events (FSRNet's loops): after the event of
 * forward k, a set flag means forward k — or one submitted after it that has already finished — overflowed.  ABI 5. */
int bsr_peek_range(bsr_handle* h);

/* Bytes of activation workspace the library holds for a batch of B HxW images (grown lazily by
 * bsr_forward; growth synchronises the stream — call bsr_reserve first to keep forwards allocation-free). */
size_t bsr_workspace_bytes(int B, int H, int W);                              /* GSC channel plan */
size_t bsr_handle_workspace_bytes(const bsr_handle* h, int B, int H, int W);  /* the plan of THIS handle's variant (GSC or the wider TSM one) */
int bsr_reserve(bsr_handle* h, int B, int H, int W);

/* Test hook: copy a named intermediate of the LAST forward (dense NHWC, real channel count) into dst
 * (device pointer, capacity cap_floats).  shape4 receives [B,H,W,C].  Names: x1 x2 x3 x0 res0..res5 up1 up2
 * y d32 bmask xh f1 f2 f y3x<i> att<i> — att<i> (the attention output of block i) only exists when the last forward ran attention and the
 * `w` GEMM as separate launches (small batches, the 16-bit modes, BSR_FUSE_ATTW=0); after a fused forward it never left LDS and the
 * probe returns BSR_ERR_STATE.  shape4 is filled even when cap_floats is too small (BSR_ERR_ARG), so a caller can
 * size its buffer with a first call of capacity 0. */
int bsr_probe(bsr_handle* h, const char* name, float* dst, size_t cap_floats, int shape4[4], void* stream);
/* Where the last forward's f (clr_up3's output, the colour tail's input) lies in the handle's workspace: *f the device pointer, *f_cs the
 * floats between pixels, shape4 = [B,H,W,64].  No copy, no launch: the pointer is valid until the next forward, reserve or destroy on
 * the handle, for work ordered after that forward on its stream (bsr_clr_tail_grad reads it in place).  BSR_DTYPE_F32 GSC / TSM handles
 * only: BSR_ERR_STATE before any forward, for the 16-bit modes (f is fp16 there) and for RGB handles.  Added under ABI 8. */
int bsr_last_f(bsr_handle* h, const float** f, int* f_cs, int shape4[4]);
/* Where the last forward's y (up3's output, the grey heads' input) lies in the handle's workspace: *y the device pointer, *y_cs the
 * floats between pixels, shape4 = [B,H,W,64].  up3 alone writes the slot and the heads alone read it, so it holds until the next
 * forward; bsr_heads_grad reads it in place.  The same rules and error codes as bsr_last_f.  Added under ABI 8. */
int bsr_last_y(bsr_handle* h, const float** y, int* y_cs, int shape4[4]);
/* The colour decoder's tensors of the last forward in the handle's workspace: *x res_stack/5's output (261 channels, *x_cs floats between
 * pixels) at [B,H/8,W/8], *f1 [B,H/4,W/4,128], *f2 [B,H/2,W/2,96], *f [B,H,W,64], all dense but x; shape4 = [B,H,W,64], the image's.  The
 * same rules and error codes as bsr_last_f, GSC handles only (BSR_ERR_STATE for TSM handles too).  Added under ABI 8. */
int bsr_last_decoder(bsr_handle* h, const float** x, int* x_cs, const float** f1, const float** f2, const float** f, int shape4[4]);
/* What the last forward kept of res_stack/5 in the handle's workspace, at [B,H/8,W/8]: *y3x = y3 + pad(xin) (bnorm3's output plus the
 * block's input; *y3x_cs floats between pixels, the first 257 channels are read), *xin the block's input (res_stack/4's output) and *out
 * the block's output, 261 channels each with *x_cs floats between pixels; shape4 = [B,H/8,W/8,261].  Each lies in a slot of its own that
 * nothing after the block overwrites.  The same rules and error codes as bsr_last_decoder.  Added under ABI 8. */
int bsr_last_block5(bsr_handle* h, const float** y3x, int* y3x_cs, const float** xin, const float** out, int* x_cs, int shape4[4]);
/* The same of res_stack/`block`, block 3, 4 or 5 (bsr_last_block5 is block 5 of it, under its own name in the error texts): *y3x and *out are the block's own; *xin is xh =
 * cat[x_hole 257 | bmask | uv 3] for block 3 (bmask at channel 257) and the block below's output for blocks 4 and 5.  The forward gives
 * every block's y3x and output, and xh, a slot of its own, on the fused-attention route and on the separate-launch route, so nothing
 * after the block overwrites them.  The rules and error codes of bsr_last_block5; any other block gives BSR_ERR_ARG.  Added under ABI 8. */
int bsr_last_block(bsr_handle* h, int block, const float** y3x, int* y3x_cs, const float** xin, const float** out, int* x_cs, int shape4[4]);
/* What the last forward kept of res_stack/2, /1 and /0, the blocks below the hole, in place: tensors7 = y3x and the output of block 2,
 * of block 1, of block 0, then xa = cat[down3's output 96 | the resized uv 3], block 0's input; strides7 their floats between pixels
 * (288, 264, 288, 264, 288, 264, 120 on a GSC handle); shape4 = [B,H/8,W/8,257].  Block 2's input is block 1's output and block 1's is
 * block 0's.  Every one lies in a slot of its own that nothing after its block overwrites; xa's lanes past channel 98 and the outputs'
 * past 256 are the forward's padding.  The rules and error codes of bsr_last_block5.  bsr_last_block keeps refusing blocks other than
 * 3, 4 and 5: their tensors are 261 wide, these 257.  Added under ABI 8. */
int bsr_last_lower_trunk(bsr_handle* h, const float* tensors7[7], int strides7[7], int shape4[4]);

/* Per-kernel-class device time (ms) of the last forward run with timing enabled; classes are indexed
 * 0: conv3x3 (+stride-2), 1: transposed 3x3 (all but class 6), 2: conv1x1, 3: attention, 4: conv7 (stem + heads), 5: glue,
 * 6: the dominant kernel instantiation igemm_conv_kernel<3,3,1,true,4,32,4,1,1,2,32,1> (up2, up3, clr_up3).
 * bsr_set_timing(h, 1) makes every following forward record HIP events around each launch on the
 * forward's stream (adds host overhead; off by default). */
#define BSR_NUM_CLASSES 7
int bsr_set_timing(bsr_handle* h, int enable);
int bsr_get_timing(bsr_handle* h, float ms_per_class[BSR_NUM_CLASSES], int launches_per_class[BSR_NUM_CLASSES]);
/* The same events, launch by launch in issue order: bsr_timing_launches() entries; entry i = the layer name the launch computes
 * ("conv1", "down1", "res3.conv2", "res3.c3q" (conv3 + theta|phi|g; fp32 GSC / TSM: conv3 + q', the keys and values of the attention being conv2's output), "res3.attention", "res3.w", "up2", "heads", "clr_conv1", glue
 * kernel names), its device time and its class.  bench.py derives the per-kernel roofline from these. */
int bsr_timing_launches(bsr_handle* h);
int bsr_timing_entry(bsr_handle* h, int i, char* name, size_t name_cap, float* ms, int* cls);

/* Input preparation for a batch of rows on the device: the per-sample work of the reference's test loaders
 * (/root/reference/dataset.py:619-638, 148-170; utils.py:356-433 face_crop_and_resize, :255-276 generate_face_region;
 * warp.py:194-232 generate_offset_map / generate_uv_map) after PNG decoding and Delaunay triangulation, which stay on the host.
 * d_blob: ONE device buffer holding, at 8-byte aligned offsets, B row records (csrc/prep_kernels.h PrepRow: image / ground-truth
 * RGB8 offsets and size, crop box, four triangle tables), `S` float64 grid coordinates (numpy.linspace(0, 1, S)) and the data
 * they point to — blindshadowremoval_amd/prep.py builds it.  out: [B,S,S,16] float32 = img3 | gt3 | uvm3 | reg_in3 | reg_out3 |
 * face1 (the packed layout FSRNet.test_step / test_step_FFHQ split, train_test_GSC.py:419,870); hull_tmp: [B,S,S] float32 scratch.
 * device: the GPU d_blob / out / hull_tmp live on (the call runs there whatever the caller's current device is); blob_bytes: size of
 * d_blob — the row and grid tables are checked against it (BSR_ERR_ARG), and the builder of the blob must keep every offset a row
 * record holds (img_off / gt_off + h*w*3, tri_off[k] + ntri[k]*144) inside it: prep.py does, before the upload.  ABI 4. */
int bsr_prep_rows(int device, const void* d_blob, size_t blob_bytes, size_t rows_off, size_t grid_off, int B, int S, float* out, float* hull_tmp,
                  void* stream);

/* Input preparation of B groups of two rows — an item and its mirror image, the elements of the TSM loaders (dataset_with_TSM.py
 * parse_fn_test, parse_fn_test_sfw) — in one launch chain.  d_blob as for bsr_prep_rows, with B group records at groups_off
 * (csrc/prep_group_kernels.h PrepGroup, 144 bytes: { int64 img_off, gt_off, aux_off; int32 h, w, box[4]; int64 tri_off[8]; int32 ntri[8] }
 * — two RGB8 images, one grey8 plane, the crop box, the four meshes of bsr_prep_rows for the item's landmarks and the four for the
 * mirror landmarks).  planes = 6: out [B,2,S,S,16] = img3 | gt3 | uvm3 | reg_in3 | reg_out3 | face1 (aux_off unread); planes = 7: out
 * [B,2,S,S,17] = img3 | cmap3 | label1 | ... with the label plane's grey levels undivided.  Row 0 of a group has the bits bsr_prep_rows
 * gives the same item; row 1 holds row 0's crop planes mirrored in x and the mirror meshes' channels.  hull_tmp: [2B,S,S] float32
 * scratch.  BSR_ERR_ARG for a null pointer, B <= 0, S*S not a multiple of 256, planes other than 6 / 7, unaligned offsets or tables that
 * leave blob_bytes; the builder of the blob keeps what the records point to inside it (prep.py).  Added under ABI 8. */
int bsr_prep_groups(int device, const void* d_blob, size_t blob_bytes, size_t groups_off, size_t grid_off, int B, int S, int planes, float* out,
                    float* hull_tmp, void* stream);

/* PNG scanline reconstruction (RFC 2083 section 6) of n images on the device — what cv2.imread / PIL do after inflating a file
 * (/root/reference/dataset.py:151,622: the images parse_fn_test / parse_fn_test_FFHQ read), moved behind the copy to the device so that a
 * loader's worker stops at the inflated stream.  d_blob (device, blob_bytes): at items_off (8-byte aligned) n records
 * { int64 raw_off, out_off; int32 h, w, c, grey_out } — raw_off: h x (1 + w c) bytes of FILTERED scanlines (filter-type byte first; c = 1
 * grey, 3 RGB, 4 RGBA of an 8-bit non-interlaced file), out_off: where the RGB8 image [h][w][3] is written (grey replicated, alpha
 * dropped — PIL's convert("RGB"); grey_out != 0 with c = 1: one byte per pixel, [h][w] — the UCB masks); both inside the blob, validated by the caller like bsr_prep_rows' records: h <= 256 (one workgroup
 * per image, one thread per row, pixels on the anti-diagonal), w c >= 4, and 16 readable bytes of the blob in front of and behind every
 * filtered image (a thread reads its row four pixels at a time).  ABI 8. */
int bsr_png_unfilter(int device, void* d_blob, size_t blob_bytes, size_t items_off, int n, void* stream);

/* bsr_png_unfilter for files of any height (an uncropped photograph of the reference's "Preprocessing New Images" procedure,
 * /root/reference/dataprocess.py:25, is 1024 rows).  Same blob conventions; n records of 40 bytes at items_off:
 * { int64 raw_off, out_off; int32 h, w, c, grey_out, rows_needed, pad } — 1 <= h <= 65535, w c >= 4; one workgroup per image walks it in
 * bands of 256 rows, the last reconstructed row of a band being the row above the next.  rows_needed > 0 stops the walk after that many
 * rows (the rows below a crop box are never read); 0 = all.  The output equals the host reconstruction bit for bit.  This entry reads the
 * records back (it synchronises `stream`) and checks every one against blob_bytes BEFORE it launches: offsets, sizes, 16 bytes of the
 * blob in front of and behind the scanlines and behind the [h][w][3 | 1] output area; BSR_ERR_ARG and nothing launched otherwise.
 * Added under ABI 8. */
int bsr_png_unfilter_tall(int device, void* d_blob, size_t blob_bytes, size_t items_off, int n, void* stream);

/* The crop of /root/reference/dataprocess.py:39-62,72 on the device: n records of 48 bytes at items_off (8-byte aligned)
 * { int64 src_off, out_off; int32 h, w, box[4], preset_x, preset_y } — src_off: an RGB8 photograph [h][w][3] in the blob, out_off: where
 * the RGB8 crop [S][S][3] is written, box = x0, y0, x1, y1.  preset_x == preset_y == 0: the box lies in the photograph and the resize
 * is OpenCV's 8-bit INTER_LINEAR (fixed point); otherwise the box is in the coordinates of the reference's float64 zero canvas of
 * (h + 2 preset_y + 2) x (w + 2 preset_x + 2) pixels with the photograph at (preset_y, preset_x) — implied, never materialised — and the
 * resize is the floating INTER_LINEAR on doubles, rounded half-even and saturated to a byte.  Every byte equals
 * blindshadowremoval_amd/wild_crop.py's host statement.  S = 32, 64, 128 or 256.  The entry reads the records back (it synchronises
 * `stream`) and validates each against blob_bytes before launching — offsets, h w 3, S S 3, the box against its canvas — so that no
 * record can make the kernel read or write outside the blob: BSR_ERR_ARG and nothing launched otherwise.  Added under ABI 8. */
int bsr_crop_faces(int device, void* d_blob, size_t blob_bytes, size_t items_off, int n, int S, void* stream);

/* The way back for in-the-wild photographs: the network's change, resized to the crop box, written into the photograph the crop was cut
 * from, IN PLACE in the blob.  The reference has no counterpart; every byte equals blindshadowremoval_amd/wild_paste.py's host statement
 * (paste_face), which also writes the arithmetic out.  n records of 48 bytes at items_off (8-byte aligned)
 * { int64 photo_off; int32 h, w, box[4], preset_x, preset_y, row, pad } — photo_off: the RGB8 photograph [h][w][3] in the blob; box and
 * presets as bsr_crop_faces' record (canvas coordinates, the canvas never materialised: only pixels of the photograph are produced,
 * pixels outside the box are not touched); row: the item's row of im / con / face, 0 <= row < n.  im, con [n][S][S][3] and face
 * [n][S][S][1] are float32 device tensors addressed through their pixel strides (floats between neighbouring pixels; rows and items
 * dense in that stride — a channel slice of the packed NHWC row is fine).  mode 0 = residual: out = sat_u8(rint(photo + interp((clip(con)
 * - im) face) 255)); mode 1 = replace: out = sat_u8(rint((interp(clip(con)) a + photo / 255 (1 - a)) 255)), a = interp(face).  S = 32, 64,
 * 128 or 256.  Like bsr_crop_faces the entry reads the records back (it synchronises `stream`) and validates each against blob_bytes
 * before launching — offset and h w 3, the box against its canvas and a side of at least 2, the row, the photograph clear of the
 * record table — and the mode and strides: BSR_ERR_ARG with a message and nothing launched otherwise.  An ADDITION under ABI 8: no
 * existing signature changes, bsr_abi_version() stays 8. */
int bsr_paste_faces(int device, void* d_blob, size_t blob_bytes, size_t items_off, int n, int S, const float* im, int im_stride, const float* con,
                    int con_stride, const float* face, int face_stride, int mode, void* stream);

/* The reference's training-shadow synthesis, process_mask (train_test_GSC.py:81-105) with the utils.py functions it calls, for B items
 * on the device; blindshadowremoval_amd/shadow_synth.py is the host statement and writes the arithmetic and the two rules of our own
 * out.  mask, face [B][S][S][1] and gt, img_dark [B][S][S][3] are dense float32 NHWC device tensors.  Every random draw of the
 * reference is an argument: draws holds B records of 16384 bytes (shadow_synth.pack_draws: branch uniforms, blur sizes, persistences,
 * red gains, the Perlin gradients as (cos, sin) pairs and the Gaussian taps — the device evaluates no sin, cos or exp), draws_bytes
 * their total.  Outputs: img, mask_sv, mask_edge [B][S][S][3] float32 and status [B] int32 — 0 ok; 1 the thresholded Perlin map blurs
 * to a maximum of 0 (the reference divides 0 by 0): img = clip(gt, 0, 1), mask_sv = mask_edge = 0; 2 a record's integers are out of
 * range (disc size 1..11, blur size 1..2, Gaussian radii 0..min(82, S - 1)): outputs as for 1, nothing indexed with them.  aux is
 * optional (may be NULL): [B][3][S][S] float32 = the Perlin map, the brightness mask, the mask that is composited.  The Perlin map,
 * its threshold, the blend guidance, the brightness mask and the disc blurs are bit-identical to the host statement; the Gaussians
 * differ from it by float32 summation order at most.  scratch: bsr_shadow_synth_scratch_bytes(B, S) bytes, 256-byte aligned; its
 * reduction words are reset by the chain itself on every call.  S = 32, 64, 128 or 256, B = 1..65535 (0 from the size query
 * otherwise).  Four launches on `stream`, no host synchronisation.  ADDITIONS under ABI 8: bsr_abi_version() stays 8. */
size_t bsr_shadow_synth_scratch_bytes(int B, int S);
int bsr_shadow_synth(int device, const float* mask, const float* gt, const float* img_dark, const float* face, const void* draws, size_t draws_bytes,
                     int B, int S, float* img, float* mask_sv, float* mask_edge, int* status, float* aux, void* scratch, void* stream);

/* The reconstruction and gradient losses of the reference's train_step (train_test_GSC.py:253-258, 287-301, 307-328; utils.py:22-52,
 * 116-125) for a batch on the device: recon_gs, recon_c and grad; blindshadowremoval_amd/train_losses.py is the host statement and
 * writes the arithmetic out.  img, gt, mask_sv, con_rgb [B][S][S][3] and gs [B][S][S][1] are dense float32 NHWC device tensors.
 * Outputs: sums [B][18] float64, the per-item partial sums in train_losses.SUM_NAMES' order; losses3 [3] float32 = recon_gs, recon_c,
 * grad over the whole batch; and, each optional (may be NULL), the figures mask_edge [B][S][S], bmaskgt [B][S][S] and dif_grad
 * [B][S][S][3] (the sum of the five dif_grad planes / 1.2).  The three planes are bit-identical to the host statement; the sums are
 * float64 sums in a fixed order (no floating-point atomics: a call repeats its bits).  scratch:
 * bsr_train_losses_scratch_bytes(B, S) bytes, 256-byte aligned; every word a launch reads is written earlier in the same call.
 * S = 32, 64, 128 or 256, B = 1..65535 (0 from the size query otherwise).  Three launches on `stream`, no host synchronisation.  A bad
 * argument gives BSR_ERR_ARG with a message and nothing launched.  ADDITIONS under ABI 8: bsr_abi_version() stays 8. */
size_t bsr_train_losses_scratch_bytes(int B, int S);
int bsr_train_losses(int device, const float* img, const float* gt, const float* mask_sv, const float* gs, const float* con_rgb, int B, int S,
                     double* sums, float* losses3, float* mask_edge, float* bmaskgt, float* dif_grad, void* scratch, void* stream);

/* The same three losses and the gradient of upstream[0] recon_gs + upstream[1] recon_c + upstream[2] grad with respect to gs and
 * con_rgb; train_losses.step_losses_grad is the host statement and writes the arithmetic out.  Inputs as bsr_train_losses; upstream: three
 * float32 on the device, or NULL for ones.  sums and losses3 are bsr_train_losses' bytes.  Outputs: grad_gs [B][S][S][1], grad_con
 * [B][S][S][3] = d_recon_c + d_grad (added in float64, rounded once) and, each optional (may be NULL), the two parts d_recon_c and d_grad
 * [B][S][S][3].  grad_gs and d_recon_c are formed in float64 in the statement's order and are bit-identical to it; d_grad goes through
 * the five maps g_l (the transposed resize back to S of the signed weights, level l = 0..4, [B][S >> l][S >> l][3] float32), which stay
 * in the scratch: scratch is bsr_train_losses_grad_scratch_bytes(B, S) bytes, 256-byte aligned = the forward's scratch, unchanged,
 * followed by the gradient's; bsr_train_losses_grad_offset(B, S, level) is the byte offset of g_level, SIZE_MAX for arguments out of
 * range.  The forward's three launches and three more on `stream`: no host synchronisation, no second stream, no floating-point
 * atomics, every sum in a fixed order: a call repeats its bits.  Every word read is written earlier in the same call.  Sizes and errors
 * as bsr_train_losses.  ADDITIONS under ABI 8: bsr_abi_version() stays 8. */
size_t bsr_train_losses_grad_scratch_bytes(int B, int S);
size_t bsr_train_losses_grad_offset(int B, int S, int level);
int bsr_train_losses_grad(int device, const float* img, const float* gt, const float* mask_sv, const float* gs, const float* con_rgb,
                          const float* upstream, int B, int S, double* sums, float* losses3, float* grad_gs, float* grad_con, float* d_recon_c,
                          float* d_grad, void* scratch, void* stream);

/* The three multi-scale patch discriminators of the reference's train_step and its three GAN losses (train_test_GSC.py:264-268, 302,
 * 334-336; model.py:115-147, 292-312; utils.py:100-102; training=False) for a batch on the device: gen, disc_real and disc_fake;
 * blindshadowremoval_amd/discriminator.py is the host statement and writes the arithmetic out.  d_blob: the device copy of
 * pack.pack_discriminators' blob, blob_bytes = bsr_disc_blob_bytes(), 16-byte aligned.  gt, con_rgb, mask_sv [B][S][S][3] are dense
 * float32 NHWC device tensors; the discriminators see rows [0, B) = [gt | mask_sv] (real) and [B, 2B) = [con_rgb | mask_sv] (fake).
 * Outputs: sums [B][9] float64, the per-item partial sums in discriminator.DISC_SUM_NAMES' order; losses3 [3] float32 = gen, disc_real,
 * disc_fake over the whole batch; and, optional (may be NULL), logits = the three maps [2B][h_k][h_k] one after the other, h_k = max(S /
 * (16 downsize), 1).  The sums are float64 sums in a fixed order (no floating-point atomics: a call repeats its bits).  scratch:
 * bsr_disc_losses_scratch_bytes(B, S) bytes, 256-byte aligned; every word a launch reads is written earlier in the same call.  It
 * holds every activation afterwards: bsr_disc_act_offset(B, S, k, layer) is the byte offset of discriminator k's (1..3) map `layer` —
 * 0 its input [2B][s][s][8] (channels 6, 7 zero), 1..4 the stride-2 layers' outputs [2B][.][.][32, 32, 64, 64], 5 the logits — and
 * SIZE_MAX for arguments out of range.  S = 32, 64, 128 or 256, B = 1..32767 (0 from the size query otherwise).  Seven launches on
 * `stream`, one after the other, no host synchronisation.  A bad argument gives BSR_ERR_ARG with a message and nothing launched.
 * ADDITIONS under ABI 8: bsr_abi_version() stays 8. */
size_t bsr_disc_blob_bytes(void);
size_t bsr_disc_losses_scratch_bytes(int B, int S);
size_t bsr_disc_act_offset(int B, int S, int k, int layer);
int bsr_disc_losses(int device, const void* d_blob, size_t blob_bytes, const float* gt, const float* con_rgb, const float* mask_sv, int B, int S,
                    double* sums, float* losses3, float* logits, void* scratch, void* stream);

/* bsr_disc_losses and the data gradient d gen / d con_rgb in one call (blindshadowremoval_amd/discriminator.py: gen_grad is the host
 * statement).  For the generator's update the discriminators are constants and gt and mask_sv are data, so this is the whole backward
 * of the term: no weight gradient, no state.  d_dgrad_blob: the device copy of pack.pack_discriminators_dgrad's blob, dgrad_bytes =
 * bsr_disc_dgrad_blob_bytes() (the folded kernels with the channel roles swapped, no bias), 16-byte aligned.  upstream: a device
 * float32[1] the gradient is multiplied by, or NULL for 1.  Outputs: sums, losses3 and logits exactly as bsr_disc_losses writes them
 * (the same launches), and grad [B][S][S][3] float32.  The forward's seven launches, then six more on `stream`, one after the other:
 * the head's gradient with conv3's slope, the gradient convolutions of conv3, conv2, conv1 (matrix instructions, sub-pixel form) and
 * conv0 (narrow), and the gather through the three resizes; each covers all three discriminators and works on the B fake rows only.
 * No host synchronisation, no second stream, no floating-point atomics: a call repeats its bits.  scratch:
 * bsr_disc_grad_scratch_bytes(B, S) bytes, 256-byte aligned = the forward's scratch, unchanged (bsr_disc_act_offset keeps its values),
 * followed by the gradient maps: bsr_disc_grad_offset(B, S, k, layer) is the byte offset of discriminator k's (1..3) gradient at its
 * image channels [B][s][s][4] (channel 3 zero) for layer 0 and at conv0..conv3's pre-activation [B][.][.][32, 32, 64, 64] for layer
 * 1..4; SIZE_MAX for arguments out of range.  Every word read is written earlier in the same call.  Sizes and errors as
 * bsr_disc_losses.  bsr_debug_disc_gen_grad stops after `stop_after` (0..6) of the backward launches, for the tests' stage-by-stage
 * comparison.  ADDITIONS under ABI 8: bsr_abi_version() stays 8. */
size_t bsr_disc_dgrad_blob_bytes(void);
size_t bsr_disc_grad_scratch_bytes(int B, int S);
size_t bsr_disc_grad_offset(int B, int S, int k, int layer);
int bsr_disc_gen_grad(int device, const void* d_blob, size_t blob_bytes, const void* d_dgrad_blob, size_t dgrad_bytes, const float* gt,
                      const float* con_rgb, const float* mask_sv, const float* upstream, int B, int S, double* sums, float* losses3, float* logits,
                      float* grad, void* scratch, void* stream);
int bsr_debug_disc_gen_grad(int device, const void* d_blob, size_t blob_bytes, const void* d_dgrad_blob, size_t dgrad_bytes, const float* gt,
                            const float* con_rgb, const float* mask_sv, const float* upstream, int B, int S, double* sums, float* losses3,
                            float* logits, float* grad, void* scratch, int stop_after, void* stream);

/* bsr_disc_losses and d d_total_loss / d the discriminators' 54 trainable variables in one call, d_total_loss = disc_real + disc_fake,
 * training=False (blindshadowremoval_amd/discriminator.py: disc_grad is the host statement).  d_wgrad_blob: the device copy of
 * pack.pack_discriminators_wgrad's blob, wgrad_bytes = bsr_disc_wgrad_blob_bytes() (the unfolded kernels and the per-channel vectors
 * bias, inv, moving_mean, rstd), 16-byte aligned; d_blob and d_dgrad_blob as bsr_disc_gen_grad takes them.  Outputs: sums, losses3 and
 * logits exactly as bsr_disc_losses writes them (the same launches), and grads, bsr_disc_wgrad_floats() float32: the variables of
 * weights.discriminator_trainable_names() in that order, each dense in its own shape (HWIO kernels), variable `index` (0..53) at float
 * offset bsr_disc_wgrad_var_offset(index); SIZE_MAX for an index out of range.  The forward's seven launches, then eleven more on
 * `stream`, one after the other (csrc/disc_wgrad_kernels.h): the per-pixel hinge seed and the head's input gradient, the head's kernel
 * gradient, per stride-2 layer the kernel gradient (matrix instructions, the reduction over the output pixels split over workgroups
 * into partials) and, down to conv1, the data gradient over all 2B rows, then the fold of the partials in a fixed order in float64 and
 * the per-channel gradients.  No host synchronisation, no second stream, no floating-point atomics: a call repeats its bits.  scratch:
 * bsr_disc_wgrad_scratch_bytes(B, S) bytes, 256-byte aligned = the forward's scratch, unchanged, followed by the gradient maps and the
 * partials: bsr_disc_wgrad_offset(B, S, k, layer) is the byte offset of discriminator k's (1..3) gradient at conv0..conv3's
 * BatchNormalization output [2B][.][.][32, 32, 64, 64] for layer 1..4 and of its seed [2B][h][h] for layer 5; SIZE_MAX for arguments out
 * of range.  Every word read is written earlier in the same call.  Sizes and errors as bsr_disc_losses.  bsr_debug_disc_wgrad stops
 * after `stop_after` (0..11) of the backward launches, for the tests' stage-by-stage comparison.  ADDITIONS under ABI 8:
 * bsr_abi_version() stays 8. */
size_t bsr_disc_wgrad_blob_bytes(void);
size_t bsr_disc_wgrad_scratch_bytes(int B, int S);
size_t bsr_disc_wgrad_floats(void);
size_t bsr_disc_wgrad_var_offset(int index);
size_t bsr_disc_wgrad_offset(int B, int S, int k, int layer);
int bsr_disc_wgrad(int device, const void* d_blob, size_t blob_bytes, const void* d_dgrad_blob, size_t dgrad_bytes, const void* d_wgrad_blob,
                   size_t wgrad_bytes, const float* gt, const float* con_rgb, const float* mask_sv, int B, int S, double* sums, float* losses3,
                   float* logits, float* grads, void* scratch, void* stream);
int bsr_debug_disc_wgrad(int device, const void* d_blob, size_t blob_bytes, const void* d_dgrad_blob, size_t dgrad_bytes, const void* d_wgrad_blob,
                         size_t wgrad_bytes, const float* gt, const float* con_rgb, const float* mask_sv, int B, int S, double* sums, float* losses3,
                         float* logits, float* grads, void* scratch, int stop_after, void* stream);

/* The start of gen_tape.gradient(g_total_loss, gen_trainable_vars) (train_test_GSC.py:344), training=False: the generator's colour tail
 * backward — clr_conv1 (3x3, cat[gs, f] 65 -> 16, BN, LeakyReLU), clr_conv2 (1x1, BN, LeakyReLU), clr_conv3 (1x1, 16 -> 3), model.py:217-219,
 * 267-269.  Stateless; all pointers are caller-owned device pointers.  Inputs: d_blob, bsr_clr_tail_grad_blob_bytes() bytes of
 * pack.pack_clr_tail_grad, 16-byte aligned; gs [B,H,W,1]; f, the 64 channels of clr_up3's output with f_cs floats between pixels (a
 * multiple of 4, at least 64; 16-byte aligned); g_con [B,H,W,3] = d loss / d con_rgb; g_gs [B,H,W,1] = what reaches gs directly, or null.
 * Outputs: d_f [B,H,W,64] (16-byte aligned), d_gs [B,H,W,1] = the path through clr_conv1's channel 0 plus g_gs, and grads,
 * bsr_clr_tail_grad_floats() float32: the ten variables of weights.generator_tail_trainable_names() in that order, each dense in its own
 * shape, variable `index` (0..9) at float offset bsr_clr_tail_grad_var_offset(index); SIZE_MAX for an index out of range.  Six launches
 * on `stream`, one after the other (csrc/clr_tail_grad_kernels.h), no host synchronisation, no floating-point atomics: a call repeats
 * its bits.  scratch: bsr_clr_tail_grad_scratch_bytes(B, H, W) bytes, 256-byte aligned; every word read is written earlier in the same
 * call.  bsr_clr_tail_grad_offset(B, H, W, map) is the byte offset of map 0 a1, 1 a2 (written only with keep != 0), 2 gz1 — each
 * [B,H,W,16] float32 — 3 the per-pixel launch's float64 partials [.][344], 4 the kernel gradient's float32 partials [P][4][160][16] with
 * P = bsr_clr_tail_grad_partials(B, H, W), 5 W1 [9][65][16] float64, 6 the sums [344] float64; SIZE_MAX out of range.  H must be a
 * multiple of 8 and W of 32 (0 from the size queries otherwise); a bad argument gives BSR_ERR_ARG with a message and nothing launched.
 * bsr_debug_clr_tail_grad stops after `stop_after` (0..6) launches.  ADDITIONS under ABI 8: bsr_abi_version() stays 8. */
size_t bsr_clr_tail_grad_blob_bytes(void);
size_t bsr_clr_tail_grad_scratch_bytes(int B, int H, int W);
size_t bsr_clr_tail_grad_floats(void);
size_t bsr_clr_tail_grad_var_offset(int index);
size_t bsr_clr_tail_grad_offset(int B, int H, int W, int map);
int bsr_clr_tail_grad_partials(int B, int H, int W);
int bsr_clr_tail_grad(int device, const void* d_blob, size_t blob_bytes, const float* gs, const float* f, int f_cs, const float* g_con, const float* g_gs,
                      int B, int H, int W, float* d_f, float* d_gs, float* grads, int keep, void* scratch, void* stream);
int bsr_debug_clr_tail_grad(int device, const void* d_blob, size_t blob_bytes, const float* gs, const float* f, int f_cs, const float* g_con,
                            const float* g_gs, int B, int H, int W, float* d_f, float* d_gs, float* grads, int keep, void* scratch, int stop_after,
                            void* stream);

/* The next layer group of the generator's backward, training=False: the colour decoder clr_up1 (261 -> 128), clr_up2 (128 -> 96), clr_up3
 * (96 -> 64), each Conv2DTranspose(3, stride 2, SAME) + BN + LeakyReLU (model.py:214-216, 264-266).  Stateless; all pointers are
 * caller-owned device pointers.  H, W are the IMAGE's (H a multiple of 32, W of 256, the generator's own rule).  Inputs: d_blob,
 * bsr_clr_decoder_grad_blob_bytes() bytes of pack.pack_clr_decoder_grad (GSC width only), 16-byte aligned; x [B,H/8,W/8,261], clr_up1's
 * input, with x_cs >= 261 floats between pixels; f1 [B,H/4,W/4,128], f2 [B,H/2,W/2,96], f [B,H,W,64], the three layers' outputs as the
 * forward kept them, with f1_cs, f2_cs, f_cs floats between pixels (multiples of 4, 16-byte aligned); d_f [B,H,W,64] dense = d loss / d f,
 * never written.  Outputs: d_x [B,H/8,W/8,261] dense, and grads, bsr_clr_decoder_grad_floats() float32: the twelve variables of
 * weights.generator_decoder_trainable_names() in that order, each dense in its own shape, variable `index` (0..11) at float offset
 * bsr_clr_decoder_grad_var_offset(index); SIZE_MAX out of range.  Nine launches on `stream`, one after the other
 * (csrc/clr_up_grad_kernels.h), no host synchronisation, no floating-point atomics: a call repeats its bits.  scratch:
 * bsr_clr_decoder_grad_scratch_bytes(B, H, W, keep) bytes, 256-byte aligned; every word read is written earlier in the same call.
 * bsr_clr_decoder_grad_offset(B, H, W, map) is the byte offset of map 0 gz1 [B,H/4,W/4,128], 1 gz2 [B,H/2,W/2,96], 2 gz3 [B,H,W,64]
 * (float32; gz3 is the scratch's last part, there and written only with keep != 0), 3..5 Wg of clr_up1..3 [9][O][C] float64, 6..8 the sums
 * S of clr_up1..3 [O] float64; SIZE_MAX out of range.  bsr_clr_decoder_grad_partials(B, H, W, layer) is the number of partials P of layer
 * 1..3's kernel gradient (0 for bad arguments).  A bad argument gives BSR_ERR_ARG with a message and nothing launched.
 * bsr_debug_clr_decoder_grad stops after `stop_after` (0..9) launches.  ADDITIONS under ABI 8: bsr_abi_version() stays 8. */
size_t bsr_clr_decoder_grad_blob_bytes(void);
size_t bsr_clr_decoder_grad_scratch_bytes(int B, int H, int W, int keep);
size_t bsr_clr_decoder_grad_floats(void);
size_t bsr_clr_decoder_grad_var_offset(int index);
size_t bsr_clr_decoder_grad_offset(int B, int H, int W, int map);
int bsr_clr_decoder_grad_partials(int B, int H, int W, int layer);
int bsr_clr_decoder_grad(int device, const void* d_blob, size_t blob_bytes, const float* x, int x_cs, const float* f1, int f1_cs, const float* f2, int f2_cs,
                         const float* f, int f_cs, const float* d_f, int B, int H, int W, float* d_x, float* grads, int keep, void* scratch, void* stream);
int bsr_debug_clr_decoder_grad(int device, const void* d_blob, size_t blob_bytes, const float* x, int x_cs, const float* f1, int f1_cs, const float* f2,
                               int f2_cs, const float* f, int f_cs, const float* d_f, int B, int H, int W, float* d_x, float* grads, int keep, void* scratch,
                               int stop_after, void* stream);

/* The next layer group of the generator's backward, training=False: the upper half of res_stack/5 — relu3, the block's zero-padded skip
 * and the NonLocalBlock (model.py:6-61, 102-113).  Stateless; all pointers are caller-owned device pointers.  h, w are the 1/8-resolution
 * GRID's (h a multiple of 4, w of 32: the generator's rule there; T = h w tokens per image).  Inputs: d_blob,
 * bsr_nonlocal_grad_blob_bytes() bytes of pack.pack_nonlocal_grad (GSC width only), 16-byte aligned; y3x = y3 + pad(xin), xin, out as
 * bsr_last_block5 hands them out (or dense tensors), with y3x_cs >= 257, xin_cs, out_cs >= 261 floats between pixels; d_out [B,h,w,261]
 * dense = d loss / d out, never written.  Outputs: d_y3 [B,h,w,257] dense (at bnorm3's output), d_skip [B,h,w,261] dense (what the skip
 * carries to the block's input), and grads, bsr_nonlocal_grad_floats() float32: the ten variables of
 * weights.generator_nonlocal_trainable_names() in that order, each dense in its own shape, variable `index` (0..9) at float offset
 * bsr_nonlocal_grad_var_offset(index); SIZE_MAX out of range.  Twelve launches on `stream`, one after the other
 * (csrc/nonlocal_grad_kernels.h), no host synchronisation, no floating-point atomics: a call repeats its bits.  scratch:
 * bsr_nonlocal_grad_scratch_bytes(B, h, w) bytes, 256-byte aligned; every word read is written earlier in the same call.
 * bsr_nonlocal_grad_offset(B, h, w, map) is the byte offset of map 0 y3 [N][272], 1 dz [N][272], 2 theta | phi | g [N][384], 3 A [N][128],
 * 4 L [N][2] (the row maximum m and r = 1 / sum exp(S - m)), 5 dA [N][128], 6 D [N], 7 d_theta | d_phi | d_g [N][384] (float32, N = B T), 8 Wgd [128][257] float64, 9 Sz [257] float64;
 * SIZE_MAX out of range.  bsr_nonlocal_grad_partials(B, h, w) is the number of row slices of the two kernel gradients (0 for bad
 * arguments).  A bad argument gives BSR_ERR_ARG with a message and nothing launched.  bsr_debug_nonlocal_grad stops after `stop_after`
 * (0..12) launches.  ADDITIONS under ABI 8: bsr_abi_version() stays 8. */
size_t bsr_nonlocal_grad_blob_bytes(void);
size_t bsr_nonlocal_grad_scratch_bytes(int B, int h, int w);
size_t bsr_nonlocal_grad_floats(void);
size_t bsr_nonlocal_grad_var_offset(int index);
size_t bsr_nonlocal_grad_offset(int B, int h, int w, int map);
int bsr_nonlocal_grad_partials(int B, int h, int w);
int bsr_nonlocal_grad(int device, const void* d_blob, size_t blob_bytes, const float* y3x, int y3x_cs, const float* xin, int xin_cs, const float* out,
                      int out_cs, const float* d_out, int B, int h, int w, float* d_y3, float* d_skip, float* grads, void* scratch, void* stream);
int bsr_debug_nonlocal_grad(int device, const void* d_blob, size_t blob_bytes, const float* y3x, int y3x_cs, const float* xin, int xin_cs, const float* out,
                            int out_cs, const float* d_out, int B, int h, int w, float* d_y3, float* d_skip, float* grads, void* scratch, int stop_after,
                            void* stream);

/* The backward of the lower half of the generator's res_stack/5 (training=False, fp32, GSC width): conv1/bnorm1/relu1 (1x1, 261 -> 128),
 * conv2/bnorm2/relu2 (3x3, 128 -> 128), conv3/bnorm3 (1x1, 128 -> 257) and the sum with what the skip carries.  d_blob:
 * bsr_bottleneck_grad_blob_bytes() bytes of pack.pack_bottleneck_grad (GSC width only; block 3, 4 or 5: their shapes are the same), 16-byte
 * aligned; xin [B,h,w,261 of xin_cs] the block's input, d_y3 dense [B,h,w,257] the gradient at bnorm3's output, d_skip dense [B,h,w,261]
 * or null for none.  Outputs: d_xin dense [B,h,w,261] and grads, bsr_bottleneck_grad_floats() float32: the twelve variables of
 * weights.generator_bottleneck_trainable_names() in that order, each dense in its own shape, variable `index` (0..11) at float offset
 * bsr_bottleneck_grad_var_offset(index); SIZE_MAX out of range.  The chain forms a1 and a2 again from xin and reads nothing else of the
 * forward.  Twelve launches on `stream`, one after the other (csrc/bottleneck_grad_kernels.h), no host synchronisation, no floating-point
 * atomics: a call repeats its bits.  scratch: bsr_bottleneck_grad_scratch_bytes(B, h, w) bytes, 256-byte aligned; every word read is
 * written earlier in the same call.  bsr_bottleneck_grad_offset(B, h, w, map) is the byte offset of map 0 xin [N][272], 1 d_y3 [N][272],
 * 2 a1, 3 a2, 4 gz2, 5 gz1 [N][128], 6 the three kernel gradients before the BN factor (float64 [261 x 128 | 9 x 128 x 128 | 128 x 257]),
 * 7 the column sums of gz1, gz2, d_y3 (float64 [128 | 128 | 257]); SIZE_MAX out of range.  bsr_bottleneck_grad_partials(B, h, w) is the
 * number of row slices of the three kernel gradients (0 for bad arguments).  A bad argument gives BSR_ERR_ARG with a message and nothing
 * launched.  bsr_debug_bottleneck_grad stops after `stop_after` (0..12) of the launches. */
size_t bsr_bottleneck_grad_blob_bytes(void);
size_t bsr_bottleneck_grad_scratch_bytes(int B, int h, int w);
size_t bsr_bottleneck_grad_floats(void);
size_t bsr_bottleneck_grad_var_offset(int index);
size_t bsr_bottleneck_grad_offset(int B, int h, int w, int map);
int bsr_bottleneck_grad_partials(int B, int h, int w);
int bsr_bottleneck_grad(int device, const void* d_blob, size_t blob_bytes, const float* xin, int xin_cs, const float* d_y3, const float* d_skip, int B,
                        int h, int w, float* d_xin, float* grads, void* scratch, void* stream);
int bsr_debug_bottleneck_grad(int device, const void* d_blob, size_t blob_bytes, const float* xin, int xin_cs, const float* d_y3, const float* d_skip,
                              int B, int h, int w, float* d_xin, float* grads, void* scratch, int stop_after, void* stream);

/* The backward of the generator between res_stack/5's input and res_stack/2's output (training=False, fp32, GSC width; the reference's
 * model.py:256-262): res_stack/4, res_stack/3 and the hole x_hole = x (1 - bmask), xh = cat[x_hole | bmask | uv] with bmask under
 * stop_gradient.  d_blob: bsr_colour_trunk_grad_blob_bytes() bytes of pack.pack_colour_trunk_grad, the four existing blobs end to end
 * (block 4's non-local and bottleneck blobs, then block 3's), 16-byte aligned.  Inputs as bsr_last_block hands them out (or dense
 * tensors): y3x4, out4 of block 4, y3x3, out3 of block 3 and xh, with y3x*_cs >= 257 and out*_cs, xh_cs >= 261 floats between pixels;
 * block 4's input is out3 and block 3's is xh.  d_xin dense [B,h,w,261] = d loss / d (res_stack/5's input) (bsr_bottleneck_grad's d_xin);
 * d_x dense [B,h,w,257], the grey branch's gradient at res_stack/2's output (bsr_grey_decoder_grad's d_x), 16-byte aligned, or null for
 * none.  Neither is written.  Outputs: d_res2 dense [B,h,w,257], 16-byte aligned, = d_xin3[..., :257] (1 - bmask) + d_x with d_xin3 the
 * gradient at block 3's input and bmask = xh[..., 257] in {0, 1}: the complete gradient at res_stack/2's output (channel 257 of d_xin3,
 * bmask, and channels 258..260, uv, reach nothing); and grads, bsr_colour_trunk_grad_floats() = 696076 float32: the 44 variables of
 * weights.generator_colour_trunk_trainable_names() in that order (block 3's twelve bottleneck variables, its ten non-local ones, then
 * block 4's), variable `index` (0..43) at float offset bsr_colour_trunk_grad_var_offset(index); SIZE_MAX out of range.  49 launches on
 * `stream`, one after the other (csrc/colour_trunk_grad_kernels.h): bsr_nonlocal_grad's twelve and bsr_bottleneck_grad's twelve for block
 * 4, the same for block 3, and the hole's one; no host synchronisation, no floating-point atomics: a call repeats its bits.  scratch:
 * bsr_colour_trunk_grad_scratch_bytes(B, h, w) bytes, 256-byte aligned; every word read is written earlier in the same call; each of
 * the four sub-chains has a region of its own.  bsr_colour_trunk_grad_offset(B, h, w, map) is the byte offset of map 0..9
 * bsr_nonlocal_grad_offset's maps of block 4, 10..17 bsr_bottleneck_grad_offset's of block 4, 18..27 and 28..35 the same of block 3,
 * 36 d_y3 [N][257], 37 d_skip [N][261] and 38 d_xin [N][261] of block 4, 39..41 the same of block 3; SIZE_MAX out of range.  A bad
 * argument gives BSR_ERR_ARG with a message and nothing launched.  bsr_debug_colour_trunk_grad stops after `stop_after` (0..49) of the
 * launches, one running count across the sub-chains.  ADDITIONS under ABI 8: bsr_abi_version() stays 8. */
size_t bsr_colour_trunk_grad_blob_bytes(void);
size_t bsr_colour_trunk_grad_scratch_bytes(int B, int h, int w);
size_t bsr_colour_trunk_grad_floats(void);
size_t bsr_colour_trunk_grad_var_offset(int index);
size_t bsr_colour_trunk_grad_offset(int B, int h, int w, int map);
int bsr_colour_trunk_grad(int device, const void* d_blob, size_t blob_bytes, const float* y3x4, int y3x4_cs, const float* out4, int out4_cs,
                          const float* y3x3, int y3x3_cs, const float* out3, int out3_cs, const float* xh, int xh_cs, const float* d_xin, const float* d_x,
                          int B, int h, int w, float* d_res2, float* grads, void* scratch, void* stream);
int bsr_debug_colour_trunk_grad(int device, const void* d_blob, size_t blob_bytes, const float* y3x4, int y3x4_cs, const float* out4, int out4_cs,
                                const float* y3x3, int y3x3_cs, const float* out3, int out3_cs, const float* xh, int xh_cs, const float* d_xin,
                                const float* d_x, int B, int h, int w, float* d_res2, float* grads, void* scratch, int stop_after, void* stream);
/* Test hook (additive in ABI 8): the chain's last launch alone (csrc/colour_trunk_grad_kernels.h, hole_grad_kernel), d_res2 =
 * d_xin3[..., :257] (1 - xh[..., 257]) + d_x with d_xin3 dense [B,h,w,261], d_x dense [B,h,w,257] or null, d_res2 dense [B,h,w,257], the
 * three 16-byte aligned, and xh_cs >= 258 floats between xh's pixels.  The size rule and error codes of bsr_colour_trunk_grad. */
int bsr_debug_hole_grad(int device, const float* xh, int xh_cs, const float* d_xin3, const float* d_x, int B, int h, int w, float* d_res2, void* stream);

/* The backward of the generator between res_stack/2's output and the trunk's input (training=False, fp32, GSC width; the reference's
 * model.py Generator.call: x = cat[down3 96 | uv 3], then res_stack/0, /1, /2): the three blocks both branches share.  d_blob:
 * bsr_lower_trunk_grad_blob_bytes() bytes of pack.pack_lower_trunk_grad, six blobs end to end in the order of the launches (block 2's
 * non-local and bottleneck blobs, block 1's, block 0's; the bottleneck blobs at the widths 257, 257 and 99 of the blocks' inputs), each a
 * multiple of 16 bytes, 16-byte aligned.  Inputs as bsr_last_lower_trunk hands them out (or dense tensors): y3x<b>, out<b> of blocks 2,
 * 1, 0 with at least 257 floats between pixels and x0 = cat[down3's output | uv] with x0_cs >= 99; channels of x0 past 98 are never
 * read.  d_res2 dense [B,h,w,257] = d loss / d (res_stack/2's output) (bsr_colour_trunk_grad's d_res2), never written.  Outputs: d_x0
 * dense [B,h,w,99], the gradient at x0 (channels 0..95 at down3's output; 96..98 belong to uv, an input); and grads,
 * bsr_lower_trunk_grad_floats() = 1022354 float32: the 66 variables of weights.generator_lower_trunk_trainable_names() in that order
 * (block 0's twelve bottleneck variables, its ten non-local ones, then block 1's, then block 2's), variable `index` (0..65) at float
 * offset bsr_lower_trunk_grad_var_offset(index); SIZE_MAX out of range.  72 launches on `stream`, one after the other
 * (csrc/block_chain_grad.h): bsr_nonlocal_grad's twelve and bsr_bottleneck_grad's twelve per block at the block's input width
 * (block 0: K = 112 for conv1, two row tiles for its kernel gradient, one column tile for its data gradient); no host synchronisation,
 * no floating-point atomics: a call repeats its bits.  scratch: bsr_lower_trunk_grad_scratch_bytes(B, h, w) bytes, 256-byte aligned;
 * every word read is written earlier in the same call; each of the six sub-chains has a region of its own.
 * bsr_lower_trunk_grad_offset(B, h, w, map) is the byte offset of map 0..9 bsr_nonlocal_grad_offset's maps of block 2, 10..17
 * bsr_bottleneck_grad_offset's of block 2, 18..35 the same of block 1, 36..53 of block 0 (its xp [N][112], its Wg [99 x 128 | ..]),
 * 54 d_y3 [N][257], 55 d_skip [N][257], 56 d_xin [N][257] of block 2, 57..59 of block 1, 60 d_y3 [N][257] and 61 d_skip [N][99] of
 * block 0; SIZE_MAX out of range.  A bad argument gives BSR_ERR_ARG with a message and nothing launched.  bsr_debug_lower_trunk_grad
 * stops after `stop_after` (0..72) of the launches, one running count across the sub-chains.  ADDITIONS under ABI 8:
 * bsr_abi_version() stays 8. */
size_t bsr_lower_trunk_grad_blob_bytes(void);
size_t bsr_lower_trunk_grad_scratch_bytes(int B, int h, int w);
size_t bsr_lower_trunk_grad_floats(void);
size_t bsr_lower_trunk_grad_var_offset(int index);
size_t bsr_lower_trunk_grad_offset(int B, int h, int w, int map);
int bsr_lower_trunk_grad(int device, const void* d_blob, size_t blob_bytes, const float* y3x2, int y3x2_cs, const float* out2, int out2_cs,
                         const float* y3x1, int y3x1_cs, const float* out1, int out1_cs, const float* y3x0, int y3x0_cs, const float* out0, int out0_cs,
                         const float* x0, int x0_cs, const float* d_res2, int B, int h, int w, float* d_x0, float* grads, void* scratch, void* stream);
int bsr_debug_lower_trunk_grad(int device, const void* d_blob, size_t blob_bytes, const float* y3x2, int y3x2_cs, const float* out2, int out2_cs,
                               const float* y3x1, int y3x1_cs, const float* out1, int out1_cs, const float* y3x0, int y3x0_cs, const float* out0,
                               int out0_cs, const float* x0, int x0_cs, const float* d_res2, int B, int h, int w, float* d_x0, float* grads,
                               void* scratch, int stop_after, void* stream);

/* The backward of the generator's grey heads (training=False, fp32; the reference's model.py:246-250): conv2 (7x7, 64 -> 1, tanh) gives
 * mask, conv3 (7x7, 64 -> 1) gives con, gs = gray(inputs) (1 + mask) + con.  d_blob: bsr_heads_grad_blob_bytes() bytes of
 * pack.pack_heads_grad (GSC or TSM weights), 16-byte aligned; inputs and mask22 dense [B,H,W,3], the forward's input and output (mask is
 * read as mask22[.., 0] - mask22[.., 2], exactly the forward's tanh); y [B,H,W,64 of y_cs] the heads' input as bsr_last_y hands it out
 * (or a dense tensor), y_cs a multiple of 4; d_gs dense [B,H,W,1] the complete gradient at gs (bsr_clr_tail_grad's).  H a multiple of 8,
 * W of 32.  Outputs: d_y dense [B,H,W,64] and grads, bsr_heads_grad_floats() = 6274 float32: the four variables of
 * weights.generator_heads_trainable_names() in that order (conv2's kernel and bias, conv3's kernel and bias), variable `index` (0..3) at
 * float offset bsr_heads_grad_var_offset(index); SIZE_MAX out of range.  Five launches on `stream`, one after the other
 * (csrc/heads_grad_kernels.h), no host synchronisation, no floating-point atomics: a call repeats its bits.  scratch:
 * bsr_heads_grad_scratch_bytes(B, H, W) bytes, 256-byte aligned; every word read is written earlier in the same call.
 * bsr_heads_grad_offset(B, H, W, map) is the byte offset of map 0 g2 = (g_m, g_con) [N][2], 1 mask [N], 2 the two kernel gradients in
 * float64 [2][7][7][64] (head 0 mask, 1 con), 3 the sums of g_m and g_con (float64 [2]); SIZE_MAX out of range.
 * bsr_heads_grad_partials(B, H, W) is the number of tile slices of the kernel gradient, each of which writes four partials, one per wave
 * (0 for bad arguments).  A bad argument gives BSR_ERR_ARG with a message and nothing launched.  bsr_debug_heads_grad stops after
 * `stop_after` (0..5) of the launches.  ADDITIONS under ABI 8: bsr_abi_version() stays 8. */
size_t bsr_heads_grad_blob_bytes(void);
size_t bsr_heads_grad_scratch_bytes(int B, int H, int W);
size_t bsr_heads_grad_floats(void);
size_t bsr_heads_grad_var_offset(int index);
size_t bsr_heads_grad_offset(int B, int H, int W, int map);
int bsr_heads_grad_partials(int B, int H, int W);
int bsr_heads_grad(int device, const void* d_blob, size_t blob_bytes, const float* inputs, const float* mask22, const float* y, int y_cs,
                   const float* d_gs, int B, int H, int W, float* d_y, float* grads, void* scratch, void* stream);
int bsr_debug_heads_grad(int device, const void* d_blob, size_t blob_bytes, const float* inputs, const float* mask22, const float* y, int y_cs,
                         const float* d_gs, int B, int H, int W, float* d_y, float* grads, void* scratch, int stop_after, void* stream);

/* The backward of the generator's grey decoder (training=False, fp32; the reference's model.py:243-245): up1 (257 -> 96, H/8 -> H/4), up2
 * (cat[up1, x3] 160 -> 64, -> H/2), up3 (cat[up2, x2] 128 -> 64, -> H), each Conv2DTranspose(3, stride 2, SAME) + BN + LeakyReLU.
 * Stateless; all pointers are caller-owned device pointers.  H, W are the IMAGE's (H a multiple of 32, W of 256).  Inputs: d_blob,
 * bsr_grey_decoder_grad_blob_bytes() bytes of pack.pack_grey_decoder_grad (GSC width only), 16-byte aligned; x [B,H/8,W/8,257],
 * res_stack/2's output, with x_cs >= 257 floats between pixels (any value: lanes past channel 256 are never read); c2 [B,H/4,W/4,160] =
 * [up1 96 | x3 64], c3 [B,H/2,W/2,128] = [up2 64 | x2 64], y [B,H,W,64] = up3's output, the concatenations whole as the forward laid them
 * out, with c2_cs, c3_cs, y_cs floats between pixels (multiples of 4, 16-byte aligned); d_y [B,H,W,64] dense = d loss / d y
 * (bsr_heads_grad's), never written.  Outputs, all dense: d_x [B,H/8,W/8,257]; d_x3 [B,H/4,W/4,64] and d_x2 [B,H/2,W/2,64], the gradients
 * at the skip halves of c2 and c3, without the encoder's LeakyReLU mask; and grads, bsr_grey_decoder_grad_floats() = 388608 float32: the
 * twelve variables of weights.generator_grey_decoder_trainable_names() in that order, variable `index` (0..11) at float offset
 * bsr_grey_decoder_grad_var_offset(index); SIZE_MAX out of range.  Nine launches on `stream`, one after the other
 * (csrc/grey_up_grad_kernels.h), no host synchronisation, no floating-point atomics: a call repeats its bits.  scratch:
 * bsr_grey_decoder_grad_scratch_bytes(B, H, W, keep) bytes, 256-byte aligned; every word read is written earlier in the same call.
 * bsr_grey_decoder_grad_offset(B, H, W, map) is the byte offset of map 0 gz1 [B,H/4,W/4,96], 1 gz2 [B,H/2,W/2,64], 2 gz3 [B,H,W,64]
 * (float32; gz3 is the scratch's last part, there and written only with keep != 0), 3..5 Wg of up1..3 [9][O][C] float64, 6..8 the sums S of
 * up1..3 [O] float64; SIZE_MAX out of range.  bsr_grey_decoder_grad_partials(B, H, W, layer) is the number of partials P of layer 1..3's
 * kernel gradient, min(cap, ceil(tiles / 3)) with caps 85, 51, 128 (0 for bad arguments).  A bad argument gives BSR_ERR_ARG with a
 * message and nothing launched.  bsr_debug_grey_decoder_grad stops after `stop_after` (0..9) launches.
 * bsr_last_grey_decoder: where the last forward's x, c2, c3, y lie in the handle's workspace, with their floats between pixels; shape4 =
 * [B,H,W,64], the image's.  The rules and error codes of bsr_last_decoder.  ADDITIONS under ABI 8: bsr_abi_version() stays 8. */
size_t bsr_grey_decoder_grad_blob_bytes(void);
size_t bsr_grey_decoder_grad_scratch_bytes(int B, int H, int W, int keep);
size_t bsr_grey_decoder_grad_floats(void);
size_t bsr_grey_decoder_grad_var_offset(int index);
size_t bsr_grey_decoder_grad_offset(int B, int H, int W, int map);
int bsr_grey_decoder_grad_partials(int B, int H, int W, int layer);
int bsr_grey_decoder_grad(int device, const void* d_blob, size_t blob_bytes, const float* x, int x_cs, const float* c2, int c2_cs, const float* c3, int c3_cs,
                          const float* y, int y_cs, const float* d_y, int B, int H, int W, float* d_x, float* d_x3, float* d_x2, float* grads, int keep,
                          void* scratch, void* stream);
int bsr_debug_grey_decoder_grad(int device, const void* d_blob, size_t blob_bytes, const float* x, int x_cs, const float* c2, int c2_cs, const float* c3,
                                int c3_cs, const float* y, int y_cs, const float* d_y, int B, int H, int W, float* d_x, float* d_x3, float* d_x2,
                                float* grads, int keep, void* scratch, int stop_after, void* stream);
int bsr_last_grey_decoder(bsr_handle* h, const float** x, int* x_cs, const float** c2, int* c2_cs, const float** c3, int* c3_cs, const float** y, int* y_cs,
                          int shape4[4]);

/* The VGG19 perceptual term of the reference's train_step (train_test_GSC.py:128-139, 153-160, 303; utils.py:104-114) for a batch on
 * the device: per_loss = style_content_loss(feat_extractor, concat([gt, con_rgb])); blindshadowremoval_amd/perceptual.py is the host
 * statement and writes the arithmetic out.  d_blob: the device copy of pack.pack_vgg's blob, blob_bytes = bsr_vgg_blob_bytes() (about
 * 52 MB), 16-byte aligned.  gt, con_rgb [B][S][S][3] are dense float32 NHWC device tensors; the network sees rows [0, B) = gt (real) and
 * [B, 2B) = con_rgb (fake).  Outputs: sums [B][5] float64, per item the float64 sums of the float32 terms |real - fake| over the
 * post-ReLU outputs of block{1..5}_conv1 (perceptual.PER_SUM_NAMES); loss1 [1] float32 = the five means added in order over the whole
 * batch.  The sums are taken in a fixed order (no floating-point atomics: a call repeats its bits).  scratch: bsr_vgg_scratch_bytes(B,
 * S) bytes, 256-byte aligned; every word a launch reads is written earlier in the same call.  It holds every activation afterwards
 * (5.5 GB at 32 items of 256 x 256): bsr_vgg_act_offset(B, S, layer) is the byte offset of map `layer` — 0 the preprocessed input
 * [2B][S][S][8] (BGR, channels 3..7 zero), 1..13 the conv layers' post-ReLU outputs in the network's order, 14..17 the four pooled maps
 * — and SIZE_MAX for arguments out of range.  S = 32, 64, 128 or 256, B = 1..4096 (0 from the size query otherwise).  Twenty launches on
 * `stream`, one after the other, no host synchronisation.  A bad argument gives BSR_ERR_ARG with a message and nothing launched.
 * ADDITIONS under ABI 8: bsr_abi_version() stays 8. */
size_t bsr_vgg_blob_bytes(void);
size_t bsr_vgg_scratch_bytes(int B, int S);
size_t bsr_vgg_act_offset(int B, int S, int layer);
int bsr_vgg_per_loss(int device, const void* d_blob, size_t blob_bytes, const float* gt, const float* con_rgb, int B, int S, double* sums,
                     float* loss1, void* scratch, void* stream);

/* bsr_vgg_per_loss and its data gradient d per_loss / d con_rgb in one call (blindshadowremoval_amd/perceptual.py: per_loss_grad is the
 * host statement).  VGG19 is frozen and gt is a constant, so this is the whole backward of the term: no weight gradient, no state.
 * d_dgrad_blob: the device copy of pack.pack_vgg_dgrad's blob, dgrad_bytes = bsr_vgg_dgrad_blob_bytes() (per layer the taps turned by
 * 180 degrees and the channel roles swapped, no bias), 16-byte aligned.  upstream: a device float32[1] the gradient is multiplied by, or
 * NULL for 1.  Outputs: sums and loss1 exactly as bsr_vgg_per_loss writes them (the same launches), and grad [B][S][S][3] float32 =
 * (255 * d per / d bgr[2 - c]) * upstream.  The forward's 20 launches, then 18 more on `stream`, one after the other: the seed at
 * block5_conv1, thirteen data-gradient convolutions (the forward kernel's main loop on B rows) and four un-pools; no host
 * synchronisation, no second stream, no floating-point atomics: a call repeats its bits.  scratch: bsr_vgg_grad_scratch_bytes(B, S)
 * bytes, 256-byte aligned = the forward's scratch, unchanged (bsr_vgg_act_offset keeps its values), followed by two gradient buffers
 * at bsr_vgg_grad_offset(B, S, 0 / 1) of B * S * S * 64 floats each (SIZE_MAX for arguments out of range); every word read is written
 * earlier in the same call.  Sizes and errors as bsr_vgg_per_loss.  bsr_debug_vgg_per_loss_grad stops after `stop_after` (0..18) of
 * the backward launches, whose order is: seed, then for layer 13 down to 1 its gradient convolution, followed by the un-pool where the
 * layer is the first of its block; launch j = 1..17 writes buffer (j - 1) & 1, launch 18 writes grad.  For the tests' stage-by-stage
 * comparison.  ADDITIONS under ABI 8: bsr_abi_version() stays 8. */
size_t bsr_vgg_dgrad_blob_bytes(void);
size_t bsr_vgg_grad_scratch_bytes(int B, int S);
size_t bsr_vgg_grad_offset(int B, int S, int which);
int bsr_vgg_per_loss_grad(int device, const void* d_blob, size_t blob_bytes, const void* d_dgrad_blob, size_t dgrad_bytes, const float* gt,
                          const float* con_rgb, const float* upstream, int B, int S, double* sums, float* loss1, float* grad, void* scratch,
                          void* stream);
int bsr_debug_vgg_per_loss_grad(int device, const void* d_blob, size_t blob_bytes, const void* d_dgrad_blob, size_t dgrad_bytes,
                                const float* gt, const float* con_rgb, const float* upstream, int B, int S, double* sums, float* loss1,
                                float* grad, void* scratch, int stop_after, void* stream);

/* The output sink of the reference's loops on the device: replaces `cv2.imwrite(fname, strip)` of Logging.save_img
 * (/root/reference/utils.py:196-204; called per item from train_test_GSC.py:744-746 and :889-890) up to the write() itself.
 * pixels: [B,H,W,3] uint8 RGB strips (device).  out: B complete PNG FILE images, out_stride bytes apart (device or device-mapped
 * pinned memory), each exactly bsr_png_file_bytes(H, W) long: 8-bit truecolour, filter type 0, the zlib stream as stored deflate
 * blocks (lossless: any decoder returns `pixels`; size = raw size + 0.3 %), Adler-32 and chunk CRC-32s computed on the device.
 * scratch: bsr_png_scratch_bytes(B) bytes of device memory, 8-byte aligned (the per-file checksum accumulators and arrival tickets).
 * ABI 7: the scratch must be ZERO when it is first used (one hipMemset when it is allocated) and every call leaves it zero again — the
 * encoder is ONE launch whose last workgroup per file finishes the file and clears its accumulators (ABI 5-6 cleared them with a memset per
 * call and finished with a third launch).  A scratch that is not zero gives files with wrong checksums.  One call at a time per scratch.
 * W <= 5461; the Adler-32 sums are reduced per workgroup, so every admitted size (up to 65535 x 5461 pixels) checksums correctly.
 * Asynchronous on `stream`. */
size_t bsr_png_file_bytes(int H, int W);
size_t bsr_png_scratch_bytes(int B);
int bsr_png_encode(int device, const unsigned char* pixels, int B, int H, int W, unsigned char* out, size_t out_stride, void* scratch,
                   void* stream);

/* The same files straight from the FIGURES: replaces Logging.get_imgs + cv2.imwrite (/root/reference/utils.py:180-204: clip to [0,1],
 * x 255, to uint8, figures side by side) for a batch.  The strip is n_figs figures of H x Wf pixels side by side (W = n_figs * Wf);
 * figure k is float32 [B,H,Wf] with channels[k] = 1 (grey, replicated) or 3 channels, its pixels pixel_strides[k] floats apart (a
 * channel slice of a wider NHWC tensor is fine), optionally multiplied by the one-channel float32 image muls[k] (pixels mul_strides[k]
 * floats apart; muls / its entries may be NULL) and by scales[k] (scales may be NULL = 1): test_step_FFHQ's third figure is
 * mask_pred * face * 2 (/root/reference/train_test_GSC.py:872-873).  byte = round-half-even(clamp(v, 0, 1) * 255), each product rounded
 * to float32 as the reference's elementwise operations are.  The pointer arrays are HOST arrays of DEVICE pointers.  out, out_stride,
 * scratch, stream: as bsr_png_encode with W = n_figs * Wf.  ABI 6. */
int bsr_png_encode_figs(int device, int n_figs, const float* const* figs, const float* const* muls, const float* scales, const int* channels,
                        const int* pixel_strides, const int* mul_strides, int B, int H, int Wf, unsigned char* out, size_t out_stride, void* scratch,
                        void* stream);

/* The per-item post-processing of FSRNet.test_step on the device: replaces /root/reference/train_test_GSC.py:424-748 (resize to the crop
 * box + zero pad :437-477, region thresholds :479-590, 4-connected components :594-615, nose rule :650-666, composite :711-722, SSIM /
 * PSNR :724-725, the seven figures of :744 as one strip) for a batch of B items.
 * rows10: [B,S,S,10] float32 = input 3 | ground truth 3 | con_rgb 3 | dif 1 (row 0 of each item's generator call, :419-422);
 * masks: [B,7,S,S] uint8 grey levels of the seven segmentation masks in the order of :386-392 (face+hair, face, mouth, nose, eyebrow,
 * eye, glasses — what cv2.imread returns, before the / 255.0); boxes: [B,4] float32 crop boxes.  All device pointers.
 * losses: [B,2] float32 = ssim, psnr; strips: [B,S,7*S,3] uint8 RGB (the figure strip Logging.save_img writes — feed it to
 * bsr_png_encode); figs: optional [B,7,S,S,3] float32 (the figures themselves; may be NULL); status: [B] int32 — 0 = done,
 * 1 = a mask the reference takes a bounding box of is empty (the reference raises there), 2 = the crop box does not fit S.
 * scratch: bsr_ucb_post_scratch_bytes(B, S) bytes, 256-byte aligned.  S in {32, 64, 128, 256} (reference: 256).  Every decision
 * (rounded masks, thresholds, components, rules) is bit-identical to blindshadowremoval_amd/ucb_post.py, the host statement.  ABI 5. */
size_t bsr_ucb_post_scratch_bytes(int B, int S);
int bsr_ucb_post(int device, const float* rows10, const unsigned char* masks, const float* boxes, int B, int S, float* losses,
                 unsigned char* strips, float* figs, int* status, void* scratch, void* stream);

/* The per-item post-processing of the RGB baseline's FSRNet.test_step on the device (added in ABI 8: additive, no existing signature
 * changed): replaces /root/reference/train_RGB_test.py:427-502 (resize to the crop box + zero pad, the rounded with-hair face mask,
 * composite + clip, SSIM / PSNR, the three figures input | composite | ground truth as one strip) for a batch of B items.
 * rows9: [B,S,S,9] float32 = input 3 | ground truth 3 | con 3 (row 0 of each item's generator call); masks: [B,S,S] uint8 grey levels
 * of the with-hair face mask (the only one of the seven the reference reads after resizing them); boxes: [B,4] float32.  All device
 * pointers.  losses: [B,2] float32 = ssim, psnr; strips: [B,S,3*S,3] uint8 RGB; figs: optional [B,3,S,S,3] float32 (may be NULL);
 * status: [B] int32 — 0 = done, 2 = the crop box is empty or does not fit S (black strip, NaN losses).
 * scratch: bsr_ucb_post_rgb_scratch_bytes(B, S) bytes, 256-byte aligned (0 = unsupported S).  S in {32, 64, 128, 256}.  Every figure
 * is bit-identical to blindshadowremoval_amd/ucb_post_rgb.py, the host statement. */
size_t bsr_ucb_post_rgb_scratch_bytes(int B, int S);
int bsr_ucb_post_rgb(int device, const float* rows9, const unsigned char* masks, const float* boxes, int B, int S, float* losses,
                     unsigned char* strips, float* figs, int* status, void* scratch, void* stream);

/* The scoring of the GSC model's FSRNet.test_step_sfw on the device (added in ABI 8: additive, no existing signature changed): replaces
 * /root/reference/train_test_GSC.py:808-832 after the generator call for a batch of B items.
 * rows3: [B,S,S,3] float32 = mask (the label plane's grey level after the crop resize, 0..255) | dif | face of row 0 of each item.
 * All device pointers.  losses: [B,2] float32 = ssim, psnr of the mask against mask_pred = dif * face (one channel, max_val 1);
 * auc: [B] float64 = sklearn.metrics.roc_auc_score over [1, 0] ++ (mask == 2) against [1, 0] ++ mask_pred, exact (bit-identical to
 * the Mann-Whitney form with average ranks); pred: [B,S,S] float32 mask_pred; label: [B,S,S] float32 (mask == 2);
 * status: [B] int32 — 0 = done, 3 = a mask_pred value is NaN or infinite (auc NaN; the reference's roc_auc_score raises).
 * scratch: bsr_sfw_score_scratch_bytes(B, S) bytes, 256-byte aligned (0 = unsupported S).  S in {32, 64, 128, 256}. */
size_t bsr_sfw_score_scratch_bytes(int B, int S);
int bsr_sfw_score(int device, const float* rows3, int B, int S, float* losses, double* auc, float* pred, float* label, int* status,
                  void* scratch, void* stream);

/* The per-item post-processing of the temporal-sharing model's FSRNet.test_step on the device (added in ABI 8: additive, no existing
 * signature changed): replaces /root/reference/train_with_TSM.py:441-614 after the generator call for a batch of B items — the flat
 * threshold on dif * face_hair, the 4-connected components and their size / hair filter, the nose rule, the composites of the image and
 * of its mirror, clip -> resize -> pad of the output, SSIM / PSNR, the eight figures as one strip.
 * rows: [B,S,S,13] float32 = input 3 | ground truth 3 | con 3 of the image | con 3 of the mirror | dif 1 of the image; masks: [B,3,S,S]
 * uint8 grey levels of the with-hair face, face and nose masks; boxes: [B,4] float32.  All device pointers.  losses: [B,2] float32 =
 * ssim, psnr; nose_stats: [B,2] float64 = frac_nose_in_shadow, mean_intensity (NaN when the kept set is empty, NaN both for a failed
 * item); strips: [B,S,8*S,3] uint8 RGB; figs: optional [B,8,S,S,3] float32 (may be NULL); status: [B] int32 — 0 = done, 1 = the nose
 * mask has no pixel of level 255, 2 = the crop box is empty or does not fit S (black strip, NaN losses).
 * scratch: bsr_ucb_post_tsm_scratch_bytes(B, S) bytes, 256-byte aligned (0 = unsupported S).  S in {32, 64, 128, 256}.  Every decision
 * and figure is bit-identical to blindshadowremoval_amd/ucb_post_tsm.py, the host statement. */
size_t bsr_ucb_post_tsm_scratch_bytes(int B, int S);
int bsr_ucb_post_tsm(int device, const float* rows, const unsigned char* masks, const float* boxes, int B, int S, float* losses,
                     double* nose_stats, unsigned char* strips, float* figs, int* status, void* scratch, void* stream);

/* Test hook: the fused NonLocalBlock attention kernel alone (/root/reference/model.py:51-53).
 * qkv [B,tokens,384] (theta | phi | g, 128 channels each) -> y [B,tokens,128]; tokens % 128 == 0. */
int bsr_debug_attention(const float* qkv, float* y, int B, int tokens, void* stream);
/* Test hook (added in ABI 8: additive, no existing signature changed): the d = 256 attention of the RGB baseline's 513-channel NonLocalBlock alone (csrc/attention256.h).
 * qkv [B,tokens,768] (theta | phi | g, 256 channels each) -> y [B,tokens,256]; tokens % 32 == 0. */
int bsr_debug_attention_rgb(const float* qkv, float* y, int B, int tokens, void* stream);
/* The same with the kernel of a given BSR_DTYPE_*: F32 = fp32 matrix cores; F32X3 / F16 = the split-precision kernel (attention is
 * split-precision in both 16-bit modes). */
int bsr_debug_attention_dtype(const float* qkv, float* y, int B, int tokens, int dtype, void* stream);
/* The two steps of the F32X3 / F16 case above, separately (ABI 7): the kernel of the 16-bit modes (csrc/attention_h16.h) reads theta | phi | g
 * as the conv3|theta|phi|g GEMM leaves them in those modes — per token 3 x [128 fp16 hi | 128 fp16 lo] (1536 bytes, hi = fp16(x),
 * lo = fp16(x - hi), theta pre-scaled by log2 e).  bsr_debug_split_qkv converts an fp32 [B,tokens,384] tensor to that layout (same size
 * in bytes), bsr_debug_attention_split runs the attention kernel on it; pv1 != 0 = the P.V product with the hi planes only.
 * Both refuse B <= 0 and tokens that are not a positive multiple of 128 before anything is launched. */
int bsr_debug_split_qkv(const float* qkv, void* qkv_split, int B, int tokens, void* stream);
int bsr_debug_attention_split(const void* qkv_split, float* y, int B, int tokens, int pv1, void* stream);
/* The fp32 kernel with a given workgroup shape: qw = query waves per workgroup (4 = 128 queries, 2 = 64, 1 = 32; 0 = what the
 * forward picks for this batch: the largest block that still gives every CU a workgroup).  All shapes give bit-identical outputs. */
int bsr_debug_attention_qw(const float* qkv, float* y, int B, int tokens, int qw, void* stream);
/* Test hook (additive in ABI 8, no existing signature changed): the Winograd F(2x2, 3x3) kernel of the fp32 res*.conv2 alone
 * (csrc/wino_conv2.h).  x [B,H,W,128] -> y [B,H,W,128] = LeakyReLU_0.3(conv3x3_SAME(x) + bias); w = the [8][16][128][16] transformed
 * weights of blindshadowremoval_amd.pack.pack_wino (what bsr_create derives from the blob), bias [128]; H % 4 == 0, W % 32 == 0 (device pointers).  nw = waves per workgroup:
 * 8 (128 output channels, two waves per SIMD), 4 (128, one wave per SIMD), 2 (64), 0 = what the forward picks for this grid.  All shapes give
 * bit-identical outputs. */
int bsr_debug_wino_conv(const float* x, const float* w, const float* bias, float* y, int B, int H, int W, int nw, void* stream);
/* Test hook (additive, host only, no GPU call): the filter transform bsr_create applies to the direct image of each res<i>.conv2 of an
 * fp32 blob.  direct = the layer's [4][9][128][36] image (HOST pointer), out = [8][16][128][16] floats (HOST pointer). */
int bsr_debug_wino_filter(const float* direct, float* out);
/* Test hook (additive): the 25-product transposed-conv kernel of the fp32 GSC up2 / up3 / clr_up3 alone (csrc/wino_convt.h).
 * x [B,H,W,in_cs] (cin channels read) -> y [B,2H,2W,out_cs] (channels 0..63 written, the rest untouched) =
 * act(ConvT3x3_stride2_SAME(x) + bias), act != 0: LeakyReLU_0.3.  x, bias [64], y are device pointers; w_direct is the layer's direct
 * image [ceil(cin / 32)][9][cout][36] as in the blob (HOST pointer): the entry transforms it as bsr_create does, launches and waits.
 * H and W even, cin a multiple of 16, cout = 64, in_cs >= cin, out_cs >= 64; anything else is refused before any launch. */
int bsr_debug_wino_convt(const float* x, const float* w_direct, const float* bias, float* y, int B, int H, int W, int cin, int cout, int in_cs,
                         int out_cs, int act, void* stream);
/* Test hook (additive, host only, no GPU call): the filter transform bsr_create applies to the direct images of up2, up3 and clr_up3 of
 * an fp32 GSC blob.  direct = the layer's [ceil(cin / 32)][9][64][36] image, out = [cin / 16][25][2][2][64][4] floats (HOST pointers). */
int bsr_debug_wino_convt_filter(const float* direct, float* out, int cin);
/* Test hook (additive): the fp32 colour tail alone — clr_conv1 (3x3 over cat[gs, f], 65 -> 16, + LeakyReLU_0.3) with clr_conv2, clr_conv3 and
 * the grayscale difference fused behind it — in Winograd F(2x2, 3x3) form (wino != 0: csrc/wino_clr.h) or in direct form (wino == 0:
 * conv_n16_kernel<3, 3, true, true, 2>).  gs [B,H,W,1], f [B,H,W,in_cs] (channels 0..63 read), inputs [B,H,W,3] and the outputs are device
 * pointers.  packed == NULL: con_rgb [B,H,W,3] and dif [B,H,W,1] are written; else packed [B,H,W,4] = con_rgb | dif and they are not.
 * The weights are HOST pointers as in the blob: w_direct = 'clr_conv1' [2][9][16][36], w_gs = 'clr_conv1.gs' [16][16], bias [16],
 * tail_w = 'tail.w' [337]; the entry transforms them as bsr_create does, launches and waits.  H % 8 == 0, W % 32 == 0, in_cs >= 64 and
 * a multiple of 4; anything else is refused before any launch. */
int bsr_debug_wino_clr(const float* gs, const float* f, int in_cs, const float* inputs, const float* w_direct, const float* w_gs, const float* bias,
                       const float* tail_w, float* con_rgb, float* dif, float* packed, int B, int H, int W, int wino, void* stream);
/* Test hook (additive, host only, no GPU call): the filter transform bsr_create applies to clr_conv1 of an fp32 GSC / TSM blob.
 * direct = 'clr_conv1' [2][9][16][36], w_gs = 'clr_conv1.gs' [16][16], out = [16][4][64][4] + [16][16] floats (HOST pointers;
 * blindshadowremoval_amd.pack.pack_wino_clr). */
int bsr_debug_wino_clr_filter(const float* direct, const float* w_gs, float* out);
/* Test hook (additive, host only, no GPU call): the image bsr_create derives from each res<i>.c3q of an fp32 GSC / TSM blob for the
 * attention that takes conv2's output as its keys (env BSR_KEYS_CONV2, default on): N = [y3 288 | q' 128 | g 128 | 64 zero] with
 * q' = theta composed onto phi's weights in float64 (blindshadowremoval_amd.pack.compose_keys_c3q).  c3q_w = the layer's [4][1][768][36]
 * image, c3q_b = its [768] bias, out_w = [4][1][608][36] floats, out_b = [608] floats (all HOST pointers). */
int bsr_debug_keys_compose(const float* c3q_w, const float* c3q_b, float* out_w, float* out_b);
/* Test hook (additive, host only, no GPU call): the `w` image bsr_create derives per block of an fp32 GSC / TSM blob for the attention
 * that takes conv2's output as its VALUES as well (env BSR_VALUES_CONV2, default on, read while BSR_KEYS_CONV2 is on): W' = Wg Ww,
 * b' = bw + bg Ww in float64, rounded once (blindshadowremoval_amd.pack.compose_values_w).  With it res<i>.c3q computes
 * N = [y3 288 | q' 128] (13 channel tiles; the qkv rows are [q' | t2] at stride 256) and the `w` GEMM keeps K = 128.  c3q_w / c3q_b = the
 * layer's [4][1][768][36] image and [768] bias, w_w / w_b = res<i>.w's [4][1][384][36] image and [384] bias, out_w / out_b in the layout
 * of the latter (all HOST pointers). */
int bsr_debug_values_compose(const float* c3q_w, const float* c3q_b, const float* w_w, const float* w_b, float* out_w, float* out_b);
/* Test hook (additive): the fp32 attention kernel in its shared-tile form alone — qkv2 [B,tokens,256] rows [q | kv], ONE tensor as keys
 * and values -> y [B,tokens,128]; qw as bsr_debug_attention_qw.  Bit-identical to bsr_debug_attention_qw on [q | kv | kv] rows.
 * bsr_probe on such a forward: "att<i>" stays the reference's softmax(f) g (derived from the stored O = softmax(f) t2 by one small
 * GEMM with the block's g columns), "attv<i>" is O itself, "qkv" the rows the last block's attention read. */
int bsr_debug_attention_kv1(const float* qkv2, float* y, int B, int tokens, int qw, void* stream);

/* Measurement hook (ABI 7): one wave on `stream` writes (shader cycle counter, 100-MHz real-time counter) pairs to out[2 * samples] every
 * spin x ~3.4 us until *stop (device memory, written from another stream) is non-zero or `samples` pairs are taken; *taken receives the
 * count.  GHz over an interval = d(cycles) / d(ticks) x 0.1.  bench.py runs it beside its `sustained` region: the clock the chip holds
 * under the forward's load, from inside the chip. */
int bsr_clock_trace(int device, unsigned long long* out, int samples, int spin, const int* stop, int* taken, void* stream);

void bsr_destroy(bsr_handle* h);

const char* bsr_last_error(void);

/* ABI version of this header (bumped on any signature change). */
int bsr_abi_version(void);

/* The hash (first 16 hex digits of SHA-256) of the sources this binary was compiled from: every file under csrc/ plus this header,
 * as blindshadowremoval_amd.build.source_sha16() computes it.  The Python binding refuses to load a library whose hash differs from
 * the tree's (a stale built artefact), and bench.py prints it; "unhashed" when compiled outside build.py.  ABI 5. */
const char* bsr_source_sha(void);

#ifdef __cplusplus
}
#endif
#endif /* BSR_HIP_H_ */
