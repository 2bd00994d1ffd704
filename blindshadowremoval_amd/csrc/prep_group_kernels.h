// Input preparation of the TSM loaders' groups of two rows on the device: an item and its mirror image, the elements of
// dataset.build_ucb_tsm_pair ([2,S,S,16] = img3, gt3 | uvm3, reg_in3, reg_out3, face1) and dataset.build_sfw_pair ([2,S,S,17] = img3,
// cmap3, label1 | ...).  Row 0 is what prep_rows_kernel computes for the item; row 1 carries the SAME crop planes mirrored in x
// (crop[:, ::-1, :]) and the interpolated channels of the MIRROR landmarks' meshes (lm_m of face_crop_and_resize(with_mirror=True)).
//
// One workgroup is a 16x16-pixel block of row 0 and the mirrored block of row 1: a thread evaluates the bilinear crop-resize of its
// pixel (oy, ox) ONCE and writes it to row 0 at (oy, ox) and to row 1 at (oy, S-1-ox), then walks the item's four meshes at (oy, ox) and
// the mirror's four at (oy, S-1-ox) — the second row adds no second pass over the source images.  Arithmetic, cull and winner rule are
// prep_meshes' (csrc/prep_kernels.h): float64, the host statement's operation order, contraction off.  No atomics; every output element
// has one writer.  The blur is prep_blur_kernel over the 2B hull planes.
#pragma once
#include "prep_kernels.h"

#pragma clang fp contract(off)

namespace bsr {

struct PrepGroup {              // one group of the batch; offsets are bytes from the blob start
  int64_t img_off, gt_off;      // RGB8 [h][w][3]: planes 0-2 and 3-5 (UCB: input and ground truth; SFW: frame and colour map), both / 255
  int64_t aux_off;              // grey8 [h][w]: plane 6 of the 17-channel layout (the SFW label, grey levels 0 / 1 / 2 as they are); unread with 6 planes
  int32_t h, w;
  int32_t box[4];               // crop box of row 0 (x0, y0, x1, y1); may leave the image
  int64_t tri_off[8];           // the four meshes of PrepRow for the item's landmarks (0-3) and for the mirror landmarks (4-7)
  int32_t ntri[8];
};

// grid (S*S / 256, B); block 256.  out: [B][2][S][S][PLANES + 10]; hull: [2B][S][S] raw hull masks (0 / 1) for prep_blur_kernel.
template <int PLANES>
__global__ __launch_bounds__(256) void prep_groups_kernel(const unsigned char* __restrict__ blob, const PrepGroup* __restrict__ groups,
                                                          const double* __restrict__ grid, int S, float* __restrict__ out, float* __restrict__ hull) {
  static_assert(PLANES == 6 || PLANES == 7, "img3 + gt3, or img3 + cmap3 + label1");
  constexpr int C = PLANES + 10;
  __shared__ double s_tri[kPrepMaxTri * kPrepTriDoubles];
  __shared__ int s_cnt[4];
  const PrepGroup& g = groups[blockIdx.y];                      // read in place, as prep_rows_kernel reads its row
  const int bpr = S / 16;
  const int by = blockIdx.x / bpr, bx = blockIdx.x % bpr;
  const int oy = by * 16 + (threadIdx.x >> 4), ox = bx * 16 + (threadIdx.x & 15);
  const int mx = S - 1 - ox;                                    // this thread's column in row 1: block bpr - 1 - bx
  const size_t plane = (size_t)S * S;
  const size_t pix0 = (size_t)oy * S + ox, pix1 = (size_t)oy * S + mx;
  float* o0 = out + ((size_t)blockIdx.y * 2 * plane + pix0) * C;
  float* o1 = out + (((size_t)blockIdx.y * 2 + 1) * plane + pix1) * C;

  // ---- crop + INTER_LINEAR resize, as prep_rows_kernel; one evaluation, two stores ----
  {
    const int n = g.box[2] - g.box[0];
    const double scale = (double)n / (double)S;
    auto axis = [&](int oidx, int& i0, int& i1, double& wgt) {
      double src = ((double)oidx + 0.5) * scale - 0.5;
      src = src > 0.0 ? src : 0.0;
      int f = (int)floor(src);
      i0 = f < n - 1 ? f : n - 1;
      i1 = i0 + 1 < n - 1 ? i0 + 1 : n - 1;
      wgt = src - (double)i0;
    };
    int y0, y1, x0, x1;
    double wy, wx;
    axis(oy, y0, y1, wy);
    axis(ox, x0, x1, wx);
#pragma unroll
    for (int p = 0; p < PLANES; ++p) {
      const unsigned char* im = blob + (p < 3 ? g.img_off : (p < 6 ? g.gt_off : g.aux_off));
      auto tap = [&](int cy, int cx) -> double {                  // crop pixel (cy, cx): image pixel or 0 outside
        const int iy = cy + g.box[1], ix = cx + g.box[0];
        if (iy < 0 || iy >= g.h || ix < 0 || ix >= g.w) return 0.0;
        if (p < 6) return (double)im[((size_t)iy * g.w + ix) * 3 + (p % 3)] / 255.0;
        return (double)im[(size_t)iy * g.w + ix];                 // the label plane keeps its grey levels (cv2.imread(path, 0), not / 255)
      };
      double v = 0.0;
      if (n > 0) {
        const double top = tap(y0, x0) * (1.0 - wx) + tap(y0, x1) * wx;
        const double bot = tap(y1, x0) * (1.0 - wx) + tap(y1, x1) * wx;
        v = top * (1.0 - wy) + bot * wy;
      }
      o0[p] = (float)v;
      o1[p] = (float)v;
    }
  }

  // ---- the item's meshes at (oy, ox), the mirror's at (oy, mx) ----
  const double py = grid[oy];
  prep_meshes(blob, g.tri_off, g.ntri, grid, bx, by, grid[ox], py, s_tri, s_cnt, o0 + PLANES, hull + (size_t)blockIdx.y * 2 * plane + pix0);
  prep_meshes(blob, g.tri_off + 4, g.ntri + 4, grid, bpr - 1 - bx, by, grid[mx], py, s_tri, s_cnt, o1 + PLANES,
              hull + ((size_t)blockIdx.y * 2 + 1) * plane + pix1);
}

}  // namespace bsr
