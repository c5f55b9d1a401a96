// The squeeze-excite gate of the camera-parameter encoder (reference src/model/utils/cam_param_encoder.py:
// 45-93): gate = sigmoid(W4 relu(W3 (W2 relu(W1 x + b1) + b2) + b3) + b4) on the 16 img2world entries
// of a view, with W1 / b1 = context_mlp.fc1 with the BatchNorm1d folded in, W2 = context_mlp.fc2,
// W3 / W4 = context_se.conv_reduce / conv_expand (1x1 on a 1x1 map). It depends on the cameras only,
// so it runs once in the camera prep instead of as seven launches in the matching stage.
// One workgroup per view, one thread per output channel, the activations of a layer handed to the
// next through LDS; plain fp32 FMAs (four partial sums per row, added pairwise).
#include "common.h"

namespace tsplat {
namespace camgate {

constexpr int kC = 128;   // width of every hidden layer and of the gate
constexpr int kIn = 16;   // img2world entries

// y = w[row] . x + b[row] over K inputs (K % 4 == 0; w rows and x 16-byte aligned)
template <int K>
__device__ __forceinline__ float row_dot(const float* __restrict__ w, const float* x, float b) {
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
    for (int i = 0; i < K / 4; ++i) {
        const float4 wv = reinterpret_cast<const float4*>(w)[i];
        const float4 xv = reinterpret_cast<const float4*>(x)[i];
        a0 = fmaf(wv.x, xv.x, a0);
        a1 = fmaf(wv.y, xv.y, a1);
        a2 = fmaf(wv.z, xv.z, a2);
        a3 = fmaf(wv.w, xv.w, a3);
    }
    return ((a0 + a1) + (a2 + a3)) + b;
}

__global__ void __launch_bounds__(kC)
cam_gate_kernel(const float* __restrict__ cam, const float* __restrict__ w1, const float* __restrict__ b1,
                const float* __restrict__ w2, const float* __restrict__ b2, const float* __restrict__ w3,
                const float* __restrict__ b3, const float* __restrict__ w4, const float* __restrict__ b4,
                float* __restrict__ gate) {
    __shared__ __attribute__((aligned(16))) float sx[kIn];
    __shared__ __attribute__((aligned(16))) float sa[kC];
    __shared__ __attribute__((aligned(16))) float sb[kC];
    const int j = threadIdx.x, n = blockIdx.x;
    if (j < kIn) sx[j] = cam[(size_t)n * kIn + j];
    __syncthreads();
    sa[j] = fmaxf(row_dot<kIn>(w1 + (size_t)j * kIn, sx, b1[j]), 0.f);
    __syncthreads();
    sb[j] = row_dot<kC>(w2 + (size_t)j * kC, sa, b2[j]);
    __syncthreads();
    sa[j] = fmaxf(row_dot<kC>(w3 + (size_t)j * kC, sb, b3[j]), 0.f);
    __syncthreads();
    const float z = row_dot<kC>(w4 + (size_t)j * kC, sa, b4[j]);
    gate[(size_t)n * kC + j] = 1.0f / (1.0f + expf(-z));
}

}  // namespace camgate
}  // namespace tsplat

extern "C" int tsplat_cam_gate_fwd(const float* cam, const float* w1, const float* b1, const float* w2,
                                   const float* b2, const float* w3, const float* b3, const float* w4,
                                   const float* b4, float* gate, int32_t views, int32_t in_features,
                                   int32_t channels, void* stream_) {
    using namespace tsplat::camgate;
    if (!cam || !w1 || !b1 || !w2 || !b2 || !w3 || !b3 || !w4 || !b4 || !gate || views < 0 || in_features != kIn ||
        channels != kC || (uintptr_t)w1 % 16 || (uintptr_t)w2 % 16 || (uintptr_t)w3 % 16 || (uintptr_t)w4 % 16)
        return TSPLAT_EINVAL;
    if (views == 0) return TSPLAT_OK;
    hipLaunchKernelGGL(cam_gate_kernel, dim3(views), dim3(kC), 0, (hipStream_t)stream_, cam, w1, b1, w2, b2, w3, b3,
                       w4, b4, gate);
    TSPLAT_CHECK_LAUNCH();
    return TSPLAT_OK;
}
