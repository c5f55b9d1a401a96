// The two device steps that the exact-fp32 and the split-bf16 Winograd kernels (winoconv.hip,
// winoconv3.hip) share as written: the workgroup order of every convolution kernel and the filter
// transform of both weight kernels.
#pragma once

#include "common.h"

namespace tsplat {
namespace wino_steps {

// XCD-aware (tile block, output block) order: the dispatcher deals workgroup ids (x fastest)
// round-robin over the 8 XCDs; remapped bijectively, each XCD runs a contiguous range of
// (tile block, output block) pairs with the output blocks of one tile block adjacent, so the tile
// block's input comes from that XCD's L2 for all of them (x-fastest order re-read the whole input map
// from HBM / MALL once per output block: 673 -> 211 MB fetched for the 85 MB input of 2 x 163 -> 168 at
// 256^2, profiles/r4/traffic_wino3_163x168_b1.json)
__device__ __forceinline__ void xcd_tile_order(int& tb, int& cb) {
    const int nwg = gridDim.x * gridDim.y, id = blockIdx.x + blockIdx.y * gridDim.x;
    const int q = nwg / 8, r = nwg % 8, xcd = id % 8;
    const int logical = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + id / 8;
    tb = logical / gridDim.y;
    cb = logical - tb * gridDim.y;
}

// U = G g G^T of filter (o, c) of g [co][ci][3][3] (zero when !ok: a padded entry), u[4 r + s];
// G = [[1, 0, 0], [1/2, 1/2, 1/2], [1/2, -1/2, 1/2], [0, 0, 1]]
__device__ __forceinline__ void filter_transform(const float* __restrict__ g, int o, int c, int ci, bool ok,
                                                 float (&u)[16]) {
    float k[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) k[i][j] = ok ? g[((size_t)o * ci + c) * 9 + 3 * i + j] : 0.0f;
    float t[4][3];  // G g
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        t[0][j] = k[0][j];
        t[1][j] = 0.5f * (k[0][j] + k[1][j] + k[2][j]);
        t[2][j] = 0.5f * (k[0][j] - k[1][j] + k[2][j]);
        t[3][j] = k[2][j];
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        u[4 * r + 0] = t[r][0];
        u[4 * r + 1] = 0.5f * (t[r][0] + t[r][1] + t[r][2]);
        u[4 * r + 2] = 0.5f * (t[r][0] - t[r][1] + t[r][2]);
        u[4 * r + 3] = t[r][2];
    }
}

}  // namespace wino_steps
}  // namespace tsplat
