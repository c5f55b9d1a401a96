// LPIPS of the evaluation (reference compute_lpips, src/evaluation/metrics.py:22-33: LPIPS(net="vgg"),
// version 0.1, linear layers on, forward(gt, pred, normalize=True)) -- the parts around the thirteen
// VGG16 convolutions, which run on the exact-fp32 Winograd kernel (winoconv.hip) with bias and ReLU fused.
//
//   lpips_scale_kernel   x <- ((2 x - 1) - shift_c) / scale_c of gt and pred into one [2n, 3, H, W] batch
//   lpips_tap_kernel     one tap: per pixel the channel unit-normalisation of both images, the squared
//                        difference under the tap's 1x1 weights, the sum over the workgroup's pixels;
//                        the same pass writes the 2x2 max-pooled map the next VGG block reads
//   lpips_reduce_kernel  per pair: each tap's partial sums in a fixed order / (H_k W_k), the taps summed
//
// Per tap and pixel, with f0, f1 the two images' features, a = sqrt(sum f0^2), b = sqrt(sum f1^2):
//   d = sum_c w_c (f0_c / (a + 1e-10) - f1_c / (b + 1e-10))^2
//     = S00 / (a + e)^2 + S11 / (b + e)^2 - 2 S01 / ((a + e) (b + e)),   Sij = sum_c w_c fi_c fj_c
// the one-pass five-sum form (sum f0^2, sum f1^2, S00, S11, S01): every feature is read once. All five
// sums, d and the spatial sums are float64 on the fp32 features (the products of two floats are exact in
// double), so the cancellation in d costs ~1e-16 / d of it, far below the fp32 rounding of the result.
// An all-zero pixel gives S = 0 and 0 / 1e-20 = 0. For an identical pair the five sums of the two images
// are the same numbers and d = t + t - 2 t = 0 exactly.
//
// Tap kernel layout. A lane owns one 2x2 pixel quad (lanes run along W: two 8-byte loads per channel and
// image on even widths, 512 contiguous bytes per wave and row) and one of kSplit channel slices
// (channels slice, slice + kSplit, ...); it writes the pooled value of its quad for its channels. The
// slices' 4 x 5 sums meet in LDS, the lanes of slice 0 add them in slice order and form d, and the
// workgroup's sum of d is reduced by wave shuffles and across the four waves through LDS: one ordinary
// store per workgroup, no atomics. kSplit = 4 (64 quads per workgroup) where a pair has >= 16384 quads
// (relu1_2 at 256^2: 256 workgroups per pair, 16 channels per lane), else 16 (16 quads per workgroup:
// relu5_3 at 16^2 is 4 workgroups per pair and 32 channels per lane instead of one 512-long chain). The
// choice depends on the map alone, never on n, so a pair's value does not depend on its batch.
// Pixels of an odd last row / column belong to a quad whose other pixels read as zero (d = 0 there) and
// which writes no pooled value (floor mode).
//
// Compiled with -ffp-contract=off (build.py FILE_FLAGS): the scale kernel is torch's separate fp32
// multiply, subtract, subtract and IEEE divide, bit for bit.
#include <cmath>

#include "common.h"

namespace tsplat {
namespace lpips {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kSums = 5;
constexpr int kMaxTaps = 8;
constexpr int kBigQuads = 16384;  // quads per pair from which kSplit = 4

__device__ inline double wave_sum(double v) {
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_down(v, off, kWave);
    return v;  // lane 0 holds the sum
}

__global__ void __launch_bounds__(kThreads) lpips_scale_kernel(const float* __restrict__ gt, const float* __restrict__ pred,
                                                               float* __restrict__ out, int n, int plane) {
    const int p = blockIdx.y;  // image * 3 + channel of the output batch, gt images first
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= plane) return;
    const int c = p % 3;
    const float shift = c == 0 ? -0.030f : (c == 1 ? -0.088f : -0.188f);
    const float scale = c == 0 ? 0.458f : (c == 1 ? 0.448f : 0.450f);
    const float* src = p < 3 * n ? gt + (size_t)p * plane : pred + (size_t)(p - 3 * n) * plane;
    float v = src[i];
    v = v * 2.0f;
    v = v - 1.0f;
    v = v - shift;
    out[(size_t)p * plane + i] = v / scale;
}

struct Quad {
    float v[4];  // (y0, x0), (y0, x0 + 1), (y0 + 1, x0), (y0 + 1, x0 + 1); 0 outside the map
};

// p: the quad's top-left pixel in one channel plane. vec: width even and the base 8-byte aligned, so
// both pixels of a row are one 8-byte load; a quad of an even-width map always has its second column.
__device__ inline Quad load_quad(const float* __restrict__ p, int width, bool vec, bool has_x1, bool has_y1) {
    Quad q;
    if (vec) {
        const float2 t = *reinterpret_cast<const float2*>(p);
        q.v[0] = t.x;
        q.v[1] = t.y;
        if (has_y1) {
            const float2 u = *reinterpret_cast<const float2*>(p + width);
            q.v[2] = u.x;
            q.v[3] = u.y;
        } else {
            q.v[2] = q.v[3] = 0.0f;
        }
    } else {
        q.v[0] = p[0];
        q.v[1] = has_x1 ? p[1] : 0.0f;
        q.v[2] = has_y1 ? p[width] : 0.0f;
        q.v[3] = has_x1 && has_y1 ? p[width + 1] : 0.0f;
    }
    return q;
}

template <int kSplit>
__global__ void __launch_bounds__(kThreads) lpips_tap_kernel(const float* __restrict__ feat, const float* __restrict__ lin,
                                                             double* __restrict__ partials, float* __restrict__ pooled,
                                                             int n, int channels, int height, int width, int quads_x,
                                                             int quads, int blocks_per_pair, int vec) {
    constexpr int kQuads = kThreads / kSplit;  // quads of one workgroup
    __shared__ double ssum[4 * kSums][kThreads];
    __shared__ double swave[kWaves];

    const int tid = threadIdx.x;
    const int slot = tid % kQuads, slice = tid / kQuads;
    const int pair = blockIdx.x / blocks_per_pair;
    const int q = (blockIdx.x - pair * blocks_per_pair) * kQuads + slot;
    const bool valid = q < quads;

    double acc[4][kSums];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int s = 0; s < kSums; ++s) acc[k][s] = 0.0;

    if (valid) {
        const int qy = q / quads_x, qx = q - qy * quads_x;
        const int y0 = 2 * qy, x0 = 2 * qx;
        const bool has_x1 = x0 + 1 < width, has_y1 = y0 + 1 < height;
        const size_t plane = (size_t)height * width;
        const int pool_h = height / 2, pool_w = width / 2;
        const size_t pool_plane = (size_t)pool_h * pool_w;
        const bool pool = pooled != nullptr && has_x1 && has_y1;  // qy < pool_h and qx < pool_w
        const size_t at = (size_t)y0 * width + x0;
        const float* p0 = feat + (size_t)pair * channels * plane + at;
        const float* p1 = feat + (size_t)(n + pair) * channels * plane + at;
        const size_t o0 = (size_t)pair * channels * pool_plane + (size_t)qy * pool_w + qx;
        const size_t o1 = (size_t)(n + pair) * channels * pool_plane + (size_t)qy * pool_w + qx;
        for (int c = slice; c < channels; c += kSplit) {
            const double w = (double)lin[c];
            const Quad a = load_quad(p0 + (size_t)c * plane, width, vec != 0, has_x1, has_y1);
            const Quad b = load_quad(p1 + (size_t)c * plane, width, vec != 0, has_x1, has_y1);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const double x = (double)a.v[k], y = (double)b.v[k];
                const double wx = w * x, wy = w * y;
                acc[k][0] += x * x;
                acc[k][1] += y * y;
                acc[k][2] += wx * x;
                acc[k][3] += wy * y;
                acc[k][4] += wx * y;
            }
            if (pool) {
                pooled[o0 + (size_t)c * pool_plane] = fmaxf(fmaxf(a.v[0], a.v[1]), fmaxf(a.v[2], a.v[3]));
                pooled[o1 + (size_t)c * pool_plane] = fmaxf(fmaxf(b.v[0], b.v[1]), fmaxf(b.v[2], b.v[3]));
            }
        }
    }

    // the slices' sums meet in LDS ([sum][thread]: a wave writes 64 consecutive doubles per sum)
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int s = 0; s < kSums; ++s) ssum[k * kSums + s][tid] = acc[k][s];
    __syncthreads();

    double d = 0.0;
    if (slice == 0) {  // tid = slot
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            double t[kSums];
#pragma unroll
            for (int s = 0; s < kSums; ++s) {
                t[s] = acc[k][s];
                for (int j = 1; j < kSplit; ++j) t[s] += ssum[k * kSums + s][j * kQuads + slot];
            }
            const double ia = sqrt(t[0]) + 1e-10, ib = sqrt(t[1]) + 1e-10;
            d += t[2] / (ia * ia) + t[3] / (ib * ib) - 2.0 * (t[4] / (ia * ib));
        }
    }

    d = wave_sum(d);
    if ((tid & (kWave - 1)) == 0) swave[tid / kWave] = d;
    __syncthreads();
    if (tid == 0) {
        double t = swave[0];
#pragma unroll
        for (int wv = 1; wv < kWaves; ++wv) t += swave[wv];
        partials[blockIdx.x] = t;  // [pair][block]
    }
}

struct ReduceArgs {
    int ntaps;
    int blocks[kMaxTaps];     // partials per pair of tap k
    double pixels[kMaxTaps];  // H_k W_k
};

// one wave per pair; workspace [tap][pair][block]
__global__ void __launch_bounds__(kWave) lpips_reduce_kernel(const double* __restrict__ workspace, float* __restrict__ out,
                                                             float* __restrict__ out_layers, int n, ReduceArgs a) {
    const int pair = blockIdx.x, lane = threadIdx.x;
    const double* p = workspace;
    double total = 0.0;
    for (int k = 0; k < a.ntaps; ++k) {
        const int nb = a.blocks[k];
        const double* mine = p + (size_t)pair * nb;
        double s = 0.0;
        for (int i = lane; i < nb; i += kWave) s += mine[i];
        s = wave_sum(s);
        const double layer = s / a.pixels[k];
        total += layer;
        if (lane == 0 && out_layers) out_layers[(size_t)pair * a.ntaps + k] = (float)layer;
        p += (size_t)n * nb;
    }
    if (lane == 0) out[pair] = (float)total;
}

inline int split_of(int64_t quads) { return quads >= kBigQuads ? 4 : 16; }

// workgroups per pair of one tap, or 0 when the arguments are invalid or n * blocks exceeds a 1-D grid
inline int64_t tap_blocks(int32_t n, int32_t channels, int32_t height, int32_t width) {
    if (n <= 0 || channels <= 0 || height <= 0 || width <= 0) return 0;
    const int64_t quads = (int64_t)((height + 1) / 2) * ((width + 1) / 2);
    const int per = kThreads / split_of(quads);
    const int64_t blocks = (quads + per - 1) / per;
    return blocks * n <= INT32_MAX ? blocks : 0;
}

}  // namespace lpips
}  // namespace tsplat

extern "C" int tsplat_lpips_scale_fwd(const float* gt, const float* pred, float* out, int32_t n, int32_t height,
                                      int32_t width, void* stream_) {
    using namespace tsplat::lpips;
    if (!gt || !pred || !out || n <= 0 || height <= 0 || width <= 0) return TSPLAT_EINVAL;
    const int64_t plane = (int64_t)height * width;
    if (6 * (int64_t)n > 65535 || plane > INT32_MAX - kThreads) return TSPLAT_EINVAL;  // grid.y, 32-bit pixel index
    hipLaunchKernelGGL(lpips_scale_kernel, dim3((unsigned)((plane + kThreads - 1) / kThreads), (unsigned)(6 * n)),
                       dim3(kThreads), 0, (hipStream_t)stream_, gt, pred, out, n, (int)plane);
    TSPLAT_CHECK_LAUNCH();
    return TSPLAT_OK;
}

extern "C" int32_t tsplat_lpips_tap_blocks(int32_t channels, int32_t height, int32_t width) {
    return (int32_t)tsplat::lpips::tap_blocks(1, channels, height, width);
}

extern "C" size_t tsplat_lpips_workspace_bytes(int32_t n, int32_t channels, int32_t height, int32_t width) {
    return (size_t)tsplat::lpips::tap_blocks(n, channels, height, width) * (size_t)(n > 0 ? n : 0) * sizeof(double);
}

extern "C" int tsplat_lpips_tap_fwd(const float* feat, const float* lin, void* partials, float* pooled, int32_t n,
                                    int32_t channels, int32_t height, int32_t width, void* stream_) {
    using namespace tsplat::lpips;
    if (!feat || !lin || !partials) return TSPLAT_EINVAL;
    const int64_t blocks = tap_blocks(n, channels, height, width);
    if (blocks == 0) return TSPLAT_EINVAL;
    const int quads_x = (width + 1) / 2;
    const int64_t quads = (int64_t)((height + 1) / 2) * quads_x;
    if (quads > INT32_MAX - kThreads) return TSPLAT_EINVAL;  // 32-bit quad index
    const int vec = width % 2 == 0 && (uintptr_t)feat % 8 == 0;
    const dim3 grid((unsigned)(blocks * n));
    hipStream_t stream = (hipStream_t)stream_;
    if (split_of(quads) == 4)
        hipLaunchKernelGGL(lpips_tap_kernel<4>, grid, dim3(kThreads), 0, stream, feat, lin, (double*)partials, pooled, n,
                           channels, height, width, quads_x, (int)quads, (int)blocks, vec);
    else
        hipLaunchKernelGGL(lpips_tap_kernel<16>, grid, dim3(kThreads), 0, stream, feat, lin, (double*)partials, pooled,
                           n, channels, height, width, quads_x, (int)quads, (int)blocks, vec);
    TSPLAT_CHECK_LAUNCH();
    return TSPLAT_OK;
}

extern "C" int tsplat_lpips_reduce_fwd(const void* workspace, const int32_t* blocks, const int64_t* pixels,
                                       int32_t ntaps, float* out, float* out_layers, int32_t n, void* stream_) {
    using namespace tsplat::lpips;
    if (!workspace || !blocks || !pixels || !out || n <= 0 || ntaps <= 0 || ntaps > kMaxTaps) return TSPLAT_EINVAL;
    ReduceArgs a;
    a.ntaps = ntaps;
    for (int k = 0; k < kMaxTaps; ++k) {
        a.blocks[k] = k < ntaps ? blocks[k] : 0;
        a.pixels[k] = k < ntaps ? (double)pixels[k] : 1.0;
        if (k < ntaps && (blocks[k] <= 0 || pixels[k] <= 0)) return TSPLAT_EINVAL;
    }
    hipLaunchKernelGGL(lpips_reduce_kernel, dim3((unsigned)n), dim3(tsplat::kWave), 0, (hipStream_t)stream_,
                       (const double*)workspace, out, out_layers, n, a);
    TSPLAT_CHECK_LAUNCH();
    return TSPLAT_OK;
}
