// Evaluation metrics on the device: SSIM as the reference's compute_ssim computes it
// (src/evaluation/metrics.py:36-52: skimage.metrics.structural_similarity(gt, hat, win_size=11,
// gaussian_weights=True, channel_axis=0, data_range=1.0) per [3, H, W] image), so the evaluation loop
// keeps its one synchronisation per shard instead of one host round trip per target view.
//
// Per channel, with F the separable 11-tap Gaussian of scipy.ndimage.gaussian_filter(sigma = 1.5,
// truncate = 3.5) (w_i = exp(-i^2 / (2 1.5^2)), i = -5..5, normalised in float64):
//   ux = F(x), uy = F(y), uxx = F(x x), uyy = F(y y), uxy = F(x y)
//   vx = c (uxx - ux^2), vy = c (uyy - uy^2), vxy = c (uxy - ux uy), c = 121 / 120
//   S = (2 ux uy + C1) (2 vxy + C2) / ((ux^2 + uy^2 + C1) (vx + vy + C2)), C1 = 1e-4, C2 = 9e-4
// and the image's value is the mean of S over rows 5..H-6, columns 5..W-6 and the channels. skimage
// crops the filter's 5-pixel border, so no boundary value of the `reflect` mode reaches the result and
// the kernel has no boundary code: an output pixel reads only pixels inside the image.
//
// Everything between the fp32 inputs and the fp32 result is float64: the products x x, x y of two
// floats are exact in double, the five filtered planes, the SSIM map and both reductions are double.
// (uxx - ux^2 against C2 = 9e-4 loses ~1e-4 of S in flat regions when formed in fp32.)
//
// ssim_tile_kernel: one workgroup per (image, channel, 32 x 32 tile of the cropped map). The 42 x 42
// windows of x and y are staged in LDS as floats (row loads, lanes along the row), the horizontal pass
// writes five [42][32] double planes to LDS (a 32-lane half reads / writes 32 consecutive columns of
// one row: conflict-free for the 4-byte reads, and one 256-B bank row for the 8-byte accesses), the
// vertical pass runs per thread down a column for 4 consecutive rows, and the tile's sum of S is
// reduced by wave shuffles, then across the four waves through LDS, and stored by one lane -- no
// atomics. ssim_finish_kernel: one workgroup per image adds that image's tile sums in a fixed order
// and divides by 3 (H - 10) (W - 10). An image's value therefore depends on neither the batch size nor
// its place in the batch, and repeats bit for bit.
#include <cmath>

#include "common.h"

namespace tsplat {
namespace metrics {

constexpr int kRadius = 5;
constexpr int kTaps = 2 * kRadius + 1;    // 11
constexpr int kTile = 32;                 // output tile edge (cropped coordinates)
constexpr int kWin = kTile + 2 * kRadius; // 42: input window edge
constexpr int kThreads = 256;
constexpr int kRowsPerThread = kTile * kTile / kThreads;  // 4 output rows per thread, one column

struct Weights {
    double w[kTaps];
};

// scipy.ndimage._filters._gaussian_kernel1d(sigma = 1.5, order = 0, radius = 5)
inline Weights gaussian_weights() {
    Weights g;
    const double sigma = 1.5;
    double sum = 0.0;
    for (int i = 0; i < kTaps; ++i) {
        const double x = (double)(i - kRadius);
        g.w[i] = std::exp(-0.5 / (sigma * sigma) * x * x);
        sum += g.w[i];
    }
    for (int i = 0; i < kTaps; ++i) g.w[i] /= sum;
    return g;
}

__device__ inline double wave_sum(double v) {
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_down(v, off, kWave);
    return v;  // lane 0 holds the sum
}

__global__ void __launch_bounds__(kThreads) ssim_tile_kernel(const float* __restrict__ gt, const float* __restrict__ pred,
                                                             double* __restrict__ partials, int height, int width,
                                                             int tiles_x, int tiles_y, Weights g) {
    __shared__ float sx[kWin][kWin];
    __shared__ float sy[kWin][kWin];
    __shared__ double sh[5][kWin][kTile];  // horizontally filtered x, y, xx, yy, xy
    __shared__ double swave[kThreads / kWave];

    const int tid = threadIdx.x;
    const int tiles = tiles_x * tiles_y;
    const int plane = blockIdx.x / tiles;  // image * 3 + channel
    const int tile = blockIdx.x - plane * tiles;
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int oy = ty * kTile, ox = tx * kTile;  // tile origin: cropped row r is image row r + 5, window row r
    const size_t base = (size_t)plane * height * width;

    // window rows oy .. oy + 41, columns ox .. ox + 41 of the image; zero past its bottom / right edge
    // (only masked outputs of a partial tile read those)
    for (int i = tid; i < kWin * kWin; i += kThreads) {
        const int r = i / kWin, c = i - r * kWin;
        const int iy = oy + r, ix = ox + c;
        float a = 0.0f, b = 0.0f;
        if (iy < height && ix < width) {
            const size_t at = base + (size_t)iy * width + ix;
            a = gt[at];
            b = pred[at];
        }
        sx[r][c] = a;
        sy[r][c] = b;
    }
    __syncthreads();

    // horizontal pass: 42 rows x 32 columns
    for (int i = tid; i < kWin * kTile; i += kThreads) {
        const int r = i / kTile, c = i - r * kTile;
        double ax = 0.0, ay = 0.0, axx = 0.0, ayy = 0.0, axy = 0.0;
#pragma unroll
        for (int k = 0; k < kTaps; ++k) {
            const double x = (double)sx[r][c + k], y = (double)sy[r][c + k];
            const double w = g.w[k];
            ax += w * x;
            ay += w * y;
            axx += w * (x * x);
            ayy += w * (y * y);
            axy += w * (x * y);
        }
        sh[0][r][c] = ax;
        sh[1][r][c] = ay;
        sh[2][r][c] = axx;
        sh[3][r][c] = ayy;
        sh[4][r][c] = axy;
    }
    __syncthreads();

    // vertical pass + SSIM map: column c, output rows r0 .. r0 + 3 (window rows r0 .. r0 + 13)
    const int c = tid & (kTile - 1);
    const int r0 = (tid / kTile) * kRowsPerThread;
    double acc[5][kRowsPerThread];
#pragma unroll
    for (int q = 0; q < 5; ++q)
#pragma unroll
        for (int j = 0; j < kRowsPerThread; ++j) acc[q][j] = 0.0;
#pragma unroll
    for (int k = 0; k < kTaps + kRowsPerThread - 1; ++k) {
        double v[5];
#pragma unroll
        for (int q = 0; q < 5; ++q) v[q] = sh[q][r0 + k][c];
#pragma unroll
        for (int j = 0; j < kRowsPerThread; ++j) {
            if (k - j >= 0 && k - j < kTaps) {  // resolved at compile time
                const double w = g.w[k - j];
#pragma unroll
                for (int q = 0; q < 5; ++q) acc[q][j] += w * v[q];
            }
        }
    }
    const double cov_norm = 121.0 / 120.0, c1 = 0.01 * 0.01, c2 = 0.03 * 0.03;
    const int out_h = height - 2 * kRadius, out_w = width - 2 * kRadius;
    double sum = 0.0;
#pragma unroll
    for (int j = 0; j < kRowsPerThread; ++j) {
        const double ux = acc[0][j], uy = acc[1][j];
        const double vx = cov_norm * (acc[2][j] - ux * ux);
        const double vy = cov_norm * (acc[3][j] - uy * uy);
        const double vxy = cov_norm * (acc[4][j] - ux * uy);
        const double s = ((2.0 * ux * uy + c1) * (2.0 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2));
        if (oy + r0 + j < out_h && ox + c < out_w) sum += s;
    }

    sum = wave_sum(sum);
    if ((tid & (kWave - 1)) == 0) swave[tid / kWave] = sum;
    __syncthreads();
    if (tid == 0) {
        double t = swave[0];
#pragma unroll
        for (int wv = 1; wv < kThreads / kWave; ++wv) t += swave[wv];
        partials[blockIdx.x] = t;  // [image][channel][tile]
    }
}

__global__ void __launch_bounds__(kThreads) ssim_finish_kernel(const double* __restrict__ partials, float* __restrict__ ssim,
                                                               int per_image, double count) {
    __shared__ double ssum[kThreads];
    const int tid = threadIdx.x;
    const double* p = partials + (size_t)blockIdx.x * per_image;
    double s = 0.0;
    for (int i = tid; i < per_image; i += kThreads) s += p[i];
    ssum[tid] = s;
    __syncthreads();
    for (int half = kThreads / 2; half > 0; half >>= 1) {
        if (tid < half) ssum[tid] += ssum[tid + half];
        __syncthreads();
    }
    if (tid == 0) ssim[blockIdx.x] = (float)(ssum[0] / count);
}

// tiles per image plane, or 0 when n * 3 * tiles does not fit a 1-D grid
inline int64_t total_tiles(int32_t n, int32_t height, int32_t width, int* tiles_x, int* tiles_y) {
    *tiles_x = ceil_div(width - 2 * kRadius, kTile);
    *tiles_y = ceil_div(height - 2 * kRadius, kTile);
    const int64_t per_plane = (int64_t)*tiles_x * *tiles_y;
    if (per_plane > INT32_MAX / 3) return 0;
    const int64_t total = per_plane * 3 * n;
    return total <= INT32_MAX ? total : 0;
}

}  // namespace metrics
}  // namespace tsplat

extern "C" size_t tsplat_ssim_workspace_bytes(int32_t n, int32_t height, int32_t width) {
    using namespace tsplat::metrics;
    if (n <= 0 || height < kTaps || width < kTaps) return 0;
    int tiles_x, tiles_y;
    return (size_t)total_tiles(n, height, width, &tiles_x, &tiles_y) * sizeof(double);
}

extern "C" int tsplat_ssim_fwd(const float* gt, const float* pred, float* ssim, void* workspace, int32_t n,
                               int32_t height, int32_t width, void* stream_) {
    using namespace tsplat::metrics;
    if (!gt || !pred || !ssim || !workspace || n <= 0 || height < kTaps || width < kTaps) return TSPLAT_EINVAL;
    int tiles_x, tiles_y;
    const int64_t total = total_tiles(n, height, width, &tiles_x, &tiles_y);
    if (total == 0) return TSPLAT_EINVAL;
    hipStream_t stream = (hipStream_t)stream_;
    double* partials = (double*)workspace;
    hipLaunchKernelGGL(ssim_tile_kernel, dim3((unsigned)total), dim3(kThreads), 0, stream, gt, pred, partials, height,
                       width, tiles_x, tiles_y, gaussian_weights());
    TSPLAT_CHECK_LAUNCH();
    const double count = 3.0 * (double)(height - 2 * kRadius) * (double)(width - 2 * kRadius);
    hipLaunchKernelGGL(ssim_finish_kernel, dim3(n), dim3(kThreads), 0, stream, (const double*)partials, ssim,
                       3 * tiles_x * tiles_y, count);
    TSPLAT_CHECK_LAUNCH();
    return TSPLAT_OK;
}
