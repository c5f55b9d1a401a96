// Video frames in one launch: tone map of the colour render, the white gap, the turbo-mapped log
// depth below it, HWC layout and the uint8 conversion. Replaces, per video, the reference's
// depth_map closure (src/model/model_wrapper.py:736-741, a numpy + matplotlib round trip), vcat
// (src/visualization/layout.py:171-189) and the clip * 255 -> uint8 of model_wrapper.py:771 /
// prep_image (src/misc/image_io.py:53). Without a depth input it is prep_image on the device.
#include "common.h"
#include "turbo_lut.h"

namespace tsplat {
namespace frames {

constexpr int kGap = 8;      // vcat's default gap, white
constexpr int kPix = 4;      // consecutive pixels of one row per thread: 12 bytes = 3 dwords
constexpr int kThreads = 256;

__device__ inline uint8_t tone(float c) {  // uint8(clip(c, 0, 1) * 255): fp32 multiply, truncation
    // the reference's clip keeps NaN, whose uint8 conversion is undefined; here NaN gives 0
    c = c >= 0.f ? (c <= 1.f ? c : 1.f) : 0.f;
    return (uint8_t)(c * 255.0f);
}

// VEC: W % 4 == 0 and 16-byte aligned inputs, 4-byte aligned output: float4 loads, dword stores
template <bool VEC>
__global__ void __launch_bounds__(kThreads)
frames_kernel(const float* __restrict__ color, const float* __restrict__ depth, const double* __restrict__ quant,
              int T, int H, int W, uint8_t* __restrict__ out) {
    __shared__ uint8_t lut[256 * 3];
    const bool with_depth = depth != nullptr;
    if (with_depth) {
        for (int i = threadIdx.x; i < 256 * 3; i += kThreads) lut[i] = (uint8_t)(kTurbo[i / 3][i % 3] * 255.0f);
        __syncthreads();
    }
    const int h_out = with_depth ? 2 * H + kGap : H;
    const int groups = (W + kPix - 1) / kPix;
    const int64_t total = (int64_t)T * h_out * groups;
    const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= total) return;
    const int gx = (int)(idx % groups);
    const int y = (int)((idx / groups) % h_out);
    const int t = (int)(idx / ((int64_t)groups * h_out));
    const int x0 = gx * kPix;
    const int npix = min(kPix, W - x0);

    uint8_t px[kPix * 3];
    if (y < H) {
        const float* src = color + ((size_t)t * 3 * H + y) * W + x0;
        for (int c = 0; c < 3; ++c) {
            float v[kPix];
            if (VEC) {
                const float4 f = *reinterpret_cast<const float4*>(src + (size_t)c * H * W);
                v[0] = f.x, v[1] = f.y, v[2] = f.z, v[3] = f.w;
            } else {
                for (int i = 0; i < kPix; ++i) v[i] = i < npix ? src[(size_t)c * H * W + i] : 0.f;
            }
            for (int i = 0; i < kPix; ++i) px[3 * i + c] = tone(v[i]);
        }
    } else if (y < H + kGap) {
        for (int i = 0; i < kPix * 3; ++i) px[i] = 255;
    } else {
        const float* src = depth + ((size_t)t * H + (y - H - kGap)) * W + x0;
        float v[kPix];
        if (VEC) {
            const float4 f = *reinterpret_cast<const float4*>(src);
            v[0] = f.x, v[1] = f.y, v[2] = f.z, v[3] = f.w;
        } else {
            for (int i = 0; i < kPix; ++i) v[i] = i < npix ? src[i] : 1.f;
        }
        const double near = log(quant[0]), far = log(quant[1]);
        const double inv = far - near;
        for (int i = 0; i < kPix; ++i) {
            const double r = 1.0 - (log((double)v[i]) - near) / inv;
            int e = -1;  // NaN (far == near, an empty positive population): black
            if (r == r) {
                const double c = r < 0.0 ? 0.0 : (r > 1.0 ? 1.0 : r);
                e = min((int)(c * 256.0), 255);
            }
            for (int c = 0; c < 3; ++c) px[3 * i + c] = e < 0 ? 0 : lut[3 * e + c];
        }
    }

    uint8_t* dst = out + (((size_t)t * h_out + y) * W + x0) * 3;
    if (VEC) {
        uint32_t w[3];
        for (int j = 0; j < 3; ++j)
            w[j] = (uint32_t)px[4 * j] | ((uint32_t)px[4 * j + 1] << 8) | ((uint32_t)px[4 * j + 2] << 16) |
                   ((uint32_t)px[4 * j + 3] << 24);
        uint32_t* d32 = reinterpret_cast<uint32_t*>(dst);
        d32[0] = w[0], d32[1] = w[1], d32[2] = w[2];
    } else {  // tail path: widths that are no multiple of 4, unaligned buffers
        for (int i = 0; i < npix * 3; ++i) dst[i] = px[i];
    }
}

}  // namespace frames
}  // namespace tsplat

extern "C" int tsplat_video_frames_fwd(const float* color, const float* depth, const double* quantiles,
                                       int32_t frames, int32_t height, int32_t width, uint8_t* out, void* stream_) {
    using namespace tsplat::frames;
    if (!color || !out || (depth && !quantiles) || frames <= 0 || height <= 0 || width <= 0) return TSPLAT_EINVAL;
    const int64_t h_out = depth ? 2 * (int64_t)height + kGap : height;
    const int64_t groups = (width + kPix - 1) / kPix;
    const int64_t total = (int64_t)frames * h_out * groups;
    const int64_t blocks = (total + kThreads - 1) / kThreads;
    if (blocks > 0x7fffffff) return TSPLAT_EINVAL;
    const bool vec = width % kPix == 0 && ((uintptr_t)color & 15) == 0 && ((uintptr_t)depth & 15) == 0 &&
                     ((uintptr_t)out & 3) == 0;
    hipStream_t stream = (hipStream_t)stream_;
    if (vec)
        hipLaunchKernelGGL(frames_kernel<true>, dim3((unsigned)blocks), dim3(kThreads), 0, stream, color, depth,
                           quantiles, frames, height, width, out);
    else
        hipLaunchKernelGGL(frames_kernel<false>, dim3((unsigned)blocks), dim3(kThreads), 0, stream, color, depth,
                           quantiles, frames, height, width, out);
    TSPLAT_CHECK_LAUNCH();
    return TSPLAT_OK;
}
