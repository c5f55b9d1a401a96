// Two-lane reductions inside a wave as VALU swaps, shared by the attention and linear kernels
// (winattn.hip, linear.hip, mha.hip).
#pragma once

#include "common.h"

namespace tsplat {

// max / sum of lanes l and l ^ 32 (the two half-waves), in VALU via v_permlane32_swap instead of
// an LDS-routed ds_bpermute: swap(x, x) returns (x[row 0], x[row 1]) in every lane
__device__ __forceinline__ float halves_max(float x) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ __forceinline__ float halves_sum(float x) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

// lanes l and l ^ 16 (v_permlane16_swap exchanges 16-lane rows 0 <-> 1 and 2 <-> 3, VALU only)
__device__ __forceinline__ float rows_max(float x) {
    const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ __forceinline__ float rows_sum(float x) {
    const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

}  // namespace tsplat
