// The bilinear cell of one sample, shared by every kernel that samples a map (corr.hip, uvfused.hip):
// mmcv's ms_deform_attn_im2col_bilinear. A sample at (xim, yim) of an H x W map (pixel units,
// loc * size - 0.5) is taken only for -1 < yim < H and -1 < xim < W; its cell is the 2 x 2 pixels at
// (floor(yim), floor(xim)), corners outside the map read as zero, and the corner weights are products
// of the two fractions. corr_geo.h says where a sample lies, this header what it reads there.
// Plain C++ apart from the function qualifiers, so a host compiler can build it too
// (tests/corr_cell_check.cc).
#pragma once

#include <math.h>

#if defined(__HIPCC__)
#define TSPLAT_CC_HD __host__ __device__ __forceinline__
#else
#define TSPLAT_CC_HD inline
#endif

namespace tsplat {
namespace corr {

// corner k = 0..3 of a cell is pixel (y0 + (k >> 1), x0 + (k & 1)): top-left, top-right, bottom-left,
// bottom-right, mmcv's v1..v4
struct Cell {
    int y0, x0;    // top-left corner; >= -1 in a taken sample, (-1, -1) otherwise
    float ly, lx;  // fractions below / right of the corner, in [0, 1) in a taken sample
    unsigned in;   // bit k: corner k lies in the map; 0 if the sample is not taken
};

// Fills the cell of the sample at (xim, yim) and says whether the sample is taken. The window test is
// written so that a NaN falls outside. Branch-free: a caller that tests the result gets the early
// exit, one that does not (point_corners) walks an empty mask.
TSPLAT_CC_HD bool cell_at(float xim, float yim, int H, int W, Cell& c) {
    const bool taken = yim > -1.0f && xim > -1.0f && yim < (float)H && xim < (float)W;
    const float fy = floorf(yim), fx = floorf(xim);
    c.y0 = taken ? (int)fy : -1;
    c.x0 = taken ? (int)fx : -1;
    c.ly = yim - fy;
    c.lx = xim - fx;
    // (-1, -1) has no row inside but for `taken`: its bottom row is row 0
    const bool top = taken && c.y0 >= 0, bottom = taken && c.y0 + 1 <= H - 1, left = c.x0 >= 0, right = c.x0 + 1 <= W - 1;
    c.in = (unsigned)(top && left) | (unsigned)(top && right) << 1 | (unsigned)(bottom && left) << 2 |
           (unsigned)(bottom && right) << 3;
    return taken;
}

// weight w[k] of corner k from the fractions: (1 - ly)(1 - lx), (1 - ly) lx, ly (1 - lx), ly lx
TSPLAT_CC_HD void cell_weights(float ly, float lx, float w[4]) {
    const float hy = 1.0f - ly, hx = 1.0f - lx;
    w[0] = hy * hx;
    w[1] = hy * lx;
    w[2] = ly * hx;
    w[3] = ly * lx;
}

}  // namespace corr
}  // namespace tsplat
