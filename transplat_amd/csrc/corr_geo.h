// Camera geometry shared by the correlation kernels (corr.hip, uvfused.hip): every kernel that
// places depth samples does it through these helpers, with fma contraction off, so they all place
// them identically. What a placed sample reads is corr_cell.h's; the softmax over a (pixel, depth)
// pair's points is here too, for the three kernels that weight their samples by it.
#pragma once

#include "common.h"
#include "corr_cell.h"

namespace tsplat {
namespace corr {

constexpr int kC = 128;        // feature channels (= embed_dims)
constexpr int kMaxPoints = 8;

struct Cam {
    float kinv[9], k[9], r[9], t[3];
};

struct Geo {
    int B, H, W, D;
};

// (b v)-ordered query n = 2b + v uses camera (v b) index v*B + b
__device__ __forceinline__ const float* cam_ptr(const float* cams, const Geo& g, int n) {
    const int b = n >> 1, v = n & 1;
    return cams + (size_t)(v * g.B + b) * 30;
}

// ray of integer pixel (x, y) in the own camera, rotated into the other: R K^-1 [x, y, 1]
__device__ __forceinline__ void pixel_ray(const float* c, float x, float y, float ray[3]) {
#pragma clang fp contract(off)
    const float* ki = c;
    const float* R = c + 18;
    const float p0 = ki[0] * x + ki[1] * y + ki[2];
    const float p1 = ki[3] * x + ki[4] * y + ki[5];
    const float p2 = ki[6] * x + ki[7] * y + ki[8];
    ray[0] = R[0] * p0 + R[1] * p1 + R[2] * p2;
    ray[1] = R[3] * p0 + R[4] * p1 + R[5] * p2;
    ray[2] = R[6] * p0 + R[7] * p1 + R[8] * p2;
}

// ref_3d of the ray at depth 1/disp: normalised grid coordinate / 2 + 0.5, in [0, 1] on-image
__device__ __forceinline__ void sample_ref(const float* c, const Geo& g, const float ray[3],
                                           float disp, float& rx, float& ry) {
#pragma clang fp contract(off)
    const float* K = c + 9;
    const float* t = c + 27;
    const float depth = 1.0f / disp;
    const float P0 = ray[0] * depth + t[0];
    const float P1 = ray[1] * depth + t[1];
    const float P2 = ray[2] * depth + t[2];
    const float u = K[0] * P0 + K[1] * P1 + K[2] * P2;
    const float v = K[3] * P0 + K[4] * P1 + K[5] * P2;
    const float w = fmaxf(K[6] * P0 + K[7] * P1 + K[8] * P2, 1e-3f);
    const float gx = 2.0f * (u / w) / (float)(g.W - 1) - 1.0f;
    const float gy = 2.0f * (v / w) / (float)(g.H - 1) - 1.0f;
    rx = gx / 2.0f + 0.5f;
    ry = gy / 2.0f + 0.5f;
}

// torch softmax over the P <= PMAX points of a (pixel, depth) pair, fast exponential: lv holds the
// logits, -INFINITY from P on (or all PMAX of them when P == PMAX); w[pt >= P] = 0
template <int PMAX>
__device__ __forceinline__ void point_softmax(int P, const float (&lv)[PMAX], float (&w)[PMAX]) {
    float mx = -INFINITY;
#pragma unroll
    for (int pt = 0; pt < PMAX; ++pt) mx = fmaxf(mx, lv[pt]);
    float ssum = 0.f;
#pragma unroll
    for (int pt = 0; pt < PMAX; ++pt) {
        w[pt] = pt < P ? __expf(lv[pt] - mx) : 0.f;
        ssum += w[pt];
    }
#pragma unroll
    for (int pt = 0; pt < PMAX; ++pt) w[pt] = w[pt] / ssum;
}

}  // namespace corr
}  // namespace tsplat
