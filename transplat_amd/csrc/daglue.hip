// The PyTorch glue around Depth-Anything-V2 as HIP kernels (reference src/model/encoder/
// encoder_trans.py:215-240: normalise, channel reorder, resize to 252^2 in front of the model; resize,
// per-view min / max and (d - min) / (max - min) behind it). Each kernel computes, per element, the
// same fp32 operations in the same order as the launches it replaces, so its values are theirs bit
// for bit. Built with -ffp-contract=off (transplat_amd/build.py) like upsample.hip, whose
// interpolation formula this file repeats: a contracted `hr - h0` would take the weights from the
// unrounded source coordinate.
#include "common.h"

namespace tsplat {
namespace daglue {

constexpr int kThreads = 256;

// images [nimg, 3, h, w] -> the DINOv2 patch matrix [nimg * (1 + gh gw), 3 p p]: row 0 of an image
// (the class-token slot) zeros, row 1 + py gw + px the patch (py, px) of
//   interpolate_bilinear_ac(cat((n[2], n[0], n[1])), (gh p, gw p)),  n = (image - mean[c]) / std[c]
// unfolded as [channel][i][j] (the patch projection's weight layout). One thread per element,
// consecutive threads along a row.
__global__ void __launch_bounds__(kThreads) patches_kernel(const float* __restrict__ img, const float* __restrict__ mean,
                                                           const float* __restrict__ stdv, float* __restrict__ out,
                                                           int h, int w, int gh, int gw, int p, float rh, float rw,
                                                           int total) {
    const int idx = blockIdx.x * kThreads + threadIdx.x;
    if (idx >= total) return;
    const int kk = 3 * p * p;
    const int row = idx / kk, col = idx - row * kk;
    const int rpi = 1 + gh * gw;
    const int im = row / rpi, r = row - im * rpi;
    if (r == 0) {
        out[idx] = 0.f;
        return;
    }
    const int py = (r - 1) / gw, px = (r - 1) - py * gw;
    const int c = col / (p * p), ij = col - c * p * p;
    const int i = ij / p, j = ij - i * p;
    const int sc = c == 0 ? 2 : c - 1;  // channel order (2, 0, 1)
    const int oy = py * p + i, ox = px * p + j;
    const float hr = rh * (float)oy, wr = rw * (float)ox;
    const int h0 = (int)hr, w0 = (int)wr;
    const int h1 = h0 + (h0 < h - 1 ? 1 : 0), w1 = w0 + (w0 < w - 1 ? 1 : 0);
    const float l1 = hr - (float)h0, l0 = 1.f - l1, m1 = wr - (float)w0, m0 = 1.f - m1;
    const float* src = img + ((size_t)im * 3 + sc) * h * w;
    const float mu = mean[sc], sd = stdv[sc];
    const float a = (src[(size_t)h0 * w + w0] - mu) / sd, b = (src[(size_t)h0 * w + w1] - mu) / sd;
    const float cq = (src[(size_t)h1 * w + w0] - mu) / sd, d = (src[(size_t)h1 * w + w1] - mu) / sd;
    out[idx] = l0 * (m0 * a + m1 * b) + l1 * (m0 * cq + m1 * d);
}

// min / max that keep a NaN once seen, as torch's aminmax / amin / amax do
__device__ __forceinline__ float nan_min(float a, float b) { return (b < a || b != b) ? b : a; }
__device__ __forceinline__ float nan_max(float a, float b) { return (b > a || b != b) ? b : a; }

// (min, max) over the workgroup, valid in every thread; `red` holds 2 * kThreads / 64 floats
__device__ __forceinline__ void block_minmax(float& lo, float& hi, float* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = nan_min(lo, __shfl_xor(lo, o));
        hi = nan_max(hi, __shfl_xor(hi, o));
    }
    constexpr int nw = kThreads / 64;
    if ((threadIdx.x & 63) == 0) {
        red[threadIdx.x >> 6] = lo;
        red[nw + (threadIdx.x >> 6)] = hi;
    }
    __syncthreads();
    lo = red[0];
    hi = red[nw];
#pragma unroll
    for (int k = 1; k < nw; ++k) {
        lo = nan_min(lo, red[k]);
        hi = nan_max(hi, red[nw + k]);
    }
}

// x [nimg, h, w] (the DPT's last 1x1 output) -> y [nimg, ho, wo] = interpolate_bilinear_ac(relu(x))
// and one (min, max) pair of y per workgroup: partials [nimg][gridDim.x][2], plain stores (no atomics:
// the replayed step is bit-identical). blockIdx.y = image.
__global__ void __launch_bounds__(kThreads) resize_minmax_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                                 float* __restrict__ partials, int h, int w, int ho,
                                                                 int wo, float rh, float rw) {
    __shared__ float red[2 * kThreads / 64];
    const int im = blockIdx.y;
    const int npx = ho * wo;
    const float* src = x + (size_t)im * h * w;
    // every thread of a workgroup holds a valid pixel: the tail block's spare threads repeat the last
    const int i = min((int)(blockIdx.x * kThreads + threadIdx.x), npx - 1);
    const int oy = i / wo, ox = i - oy * wo;
    const float hr = rh * (float)oy, wr = rw * (float)ox;
    const int h0 = (int)hr, w0 = (int)wr;
    const int h1 = h0 + (h0 < h - 1 ? 1 : 0), w1 = w0 + (w0 < w - 1 ? 1 : 0);
    const float l1 = hr - (float)h0, l0 = 1.f - l1, m1 = wr - (float)w0, m0 = 1.f - m1;
    auto relu = [](float v) { return v < 0.f ? 0.f : v; };  // a NaN stays, as in torch
    const float a = relu(src[(size_t)h0 * w + w0]), b = relu(src[(size_t)h0 * w + w1]);
    const float cq = relu(src[(size_t)h1 * w + w0]), d = relu(src[(size_t)h1 * w + w1]);
    const float v = l0 * (m0 * a + m1 * b) + l1 * (m0 * cq + m1 * d);
    y[(size_t)im * npx + i] = v;
    float lo = v, hi = v;
    block_minmax(lo, hi, red);
    if (threadIdx.x == 0) {
        float* pp = partials + ((size_t)im * gridDim.x + blockIdx.x) * 2;
        pp[0] = lo;
        pp[1] = hi;
    }
}

// out [nimg, npx] = (y - min) / (max - min) with the image's min / max folded from its nblk partial
// pairs (every workgroup folds them again: a few hundred L2-resident floats). max == min gives
// 0 / 0 = NaN as the elementwise sequence this replaces does.
__global__ void __launch_bounds__(kThreads) normalize_kernel(const float* __restrict__ y,
                                                             const float* __restrict__ partials,
                                                             float* __restrict__ out, int npx, int nblk) {
    __shared__ float red[2 * kThreads / 64];
    const int im = blockIdx.y;
    const float* pp = partials + (size_t)im * nblk * 2;
    float lo = pp[0], hi = pp[1];
    for (int k = threadIdx.x; k < nblk; k += kThreads) {
        lo = nan_min(lo, pp[2 * k]);
        hi = nan_max(hi, pp[2 * k + 1]);
    }
    block_minmax(lo, hi, red);
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= npx) return;
    const size_t e = (size_t)im * npx + i;
    out[e] = (y[e] - lo) / (hi - lo);
}

}  // namespace daglue
}  // namespace tsplat

extern "C" int tsplat_da_patches_fwd(const float* image, const float* mean, const float* stdv, float* out,
                                     int32_t nimg, int32_t height, int32_t width, int32_t grid_h, int32_t grid_w,
                                     int32_t patch, void* stream_) {
    using namespace tsplat::daglue;
    if (!image || !mean || !stdv || !out || nimg <= 0 || height <= 0 || width <= 0 || grid_h <= 0 || grid_w <= 0 ||
        patch <= 0)
        return TSPLAT_EINVAL;
    const int64_t total = (int64_t)nimg * (1 + (int64_t)grid_h * grid_w) * 3 * patch * patch;
    if (total >= (1ll << 31) || (int64_t)nimg * 3 * height * width >= (1ll << 31)) return TSPLAT_EINVAL;
    const int ho = grid_h * patch, wo = grid_w * patch;
    const float rh = ho > 1 ? (float)(height - 1) / (float)(ho - 1) : 0.f;
    const float rw = wo > 1 ? (float)(width - 1) / (float)(wo - 1) : 0.f;
    hipLaunchKernelGGL(patches_kernel, dim3((unsigned)((total + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                       (hipStream_t)stream_, image, mean, stdv, out, height, width, grid_h, grid_w, patch, rh, rw,
                       (int)total);
    TSPLAT_CHECK_LAUNCH();
    return TSPLAT_OK;
}

extern "C" int32_t tsplat_depth_norm_blocks(int32_t out_height, int32_t out_width) {
    if (out_height <= 0 || out_width <= 0) return 0;
    const int64_t npx = (int64_t)out_height * out_width;
    if (npx >= (1ll << 31)) return 0;
    return (int32_t)((npx + tsplat::daglue::kThreads - 1) / tsplat::daglue::kThreads);
}

extern "C" int tsplat_depth_norm_fwd(const float* x, float* resized, float* partials, float* out, int32_t nimg,
                                     int32_t height, int32_t width, int32_t out_height, int32_t out_width,
                                     void* stream_) {
    using namespace tsplat::daglue;
    if (!x || !resized || !partials || !out || nimg <= 0 || nimg > 65535 || height <= 0 || width <= 0) return TSPLAT_EINVAL;
    const int nblk = tsplat_depth_norm_blocks(out_height, out_width);
    if (nblk <= 0 || (int64_t)height * width >= (1ll << 31)) return TSPLAT_EINVAL;
    const float rh = out_height > 1 ? (float)(height - 1) / (float)(out_height - 1) : 0.f;
    const float rw = out_width > 1 ? (float)(width - 1) / (float)(out_width - 1) : 0.f;
    hipStream_t stream = (hipStream_t)stream_;
    hipLaunchKernelGGL(resize_minmax_kernel, dim3((unsigned)nblk, (unsigned)nimg), dim3(kThreads), 0, stream, x, resized,
                       partials, height, width, out_height, out_width, rh, rw);
    TSPLAT_CHECK_LAUNCH();
    hipLaunchKernelGGL(normalize_kernel, dim3((unsigned)nblk, (unsigned)nimg), dim3(kThreads), 0, stream, resized,
                       partials, out, out_height * out_width, nblk);
    TSPLAT_CHECK_LAUNCH();
    return TSPLAT_OK;
}
