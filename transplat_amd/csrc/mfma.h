// Device helpers shared by the MFMA kernels: the vector types of the MFMA builtins, the split-bf16
// ("bf16x3") operand split, and the activations of the C ABI's two `act` numberings.
#pragma once

#include "common.h"

namespace tsplat {

typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef float floatx8 __attribute__((ext_vector_type(8)));
typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef float floatx2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef short shortx8 __attribute__((ext_vector_type(8)));
typedef short shortx4 __attribute__((ext_vector_type(4)));

// The split every bf16x3 kernel's precision statement rests on: x = hi + lo with hi = bf16(x),
// lo = bf16(x - hi) (both round-to-nearest-even; x - hi is exact in fp32), packed low-half-first (the
// first value of a pair in bits 0..15). |x - hi - lo| <= 2^-18 |x|, so a product taken as
// hi*hi' + hi*lo' + lo*hi' (the dropped lo*lo' is another 2^-18) is within 3 * 2^-18 relative of x x'.
// Kernels that split the same way with other instructions keep their form next to their use
// (winattn.hip, uvfused.hip, linear.hip, split.hip), and each kernel orders its three MFMAs
// itself: the order fixes the bits.

// (a, b) rounded to bf16 and packed (a in the low half): one v_cvt_pk_bf16_f32
__device__ __forceinline__ uint32_t pack_bf16(float a, float b) {
    return __builtin_bit_cast(uint32_t, __builtin_convertvector((floatx2){a, b}, bf16x2));
}

// hi / lo halves of the pair (a, b) as two packed dwords: cvt_pk, shift, and, two subtractions, cvt_pk
__device__ __forceinline__ void split_pair(float a, float b, uint32_t& hi, uint32_t& lo) {
    hi = pack_bf16(a, b);
    const float ah = __builtin_bit_cast(float, hi << 16), bh = __builtin_bit_cast(float, hi & 0xffff0000u);
    lo = pack_bf16(a - ah, b - bh);
}

// the same rule on a whole vector (floatxN -> bf16xN hi, lo) written as vector converts (mha.hip)
template <typename BV, typename FV>
__device__ __forceinline__ void split_vec(FV f, BV& hi, BV& lo) {
    hi = __builtin_convertvector(f, BV);
    lo = __builtin_convertvector(f - __builtin_convertvector(hi, FV), BV);
}

// exact GELU (the device library's erff)
__device__ __forceinline__ float gelu_erf(float v) { return 0.5f * v * (1.0f + erff(v * 0.70710678118654752f)); }

// `act` of the convolution entry points (kernels.py _WINO_ACT): 0 none, 1 ReLU, 2 GELU
__device__ __forceinline__ float conv_act(float v, int act) {
    if (act == 1) return fmaxf(v, 0.0f);
    if (act == 2) return gelu_erf(v);
    return v;
}

// `act` of the norm / upsample / bias entry points (kernels.py _ACTS): 0 none, 1 SiLU, 2 GELU, 3 ReLU
__device__ __forceinline__ float activate(float v, int act) {
    if (act == 1) return v / (1.0f + expf(-v));
    if (act == 2) return gelu_erf(v);
    if (act == 3) return fmaxf(v, 0.0f);
    return v;
}

}  // namespace tsplat
