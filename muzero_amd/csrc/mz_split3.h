// mz_split3.h -- the float32 -> three-bf16 split of the split-bf16 convs, defined ONCE for both libraries: the planner's inference conv
// (mz_conv_split.h) and the learner's forward / data-gradient conv (mz_learn_conv_split.h) split their operands with these two functions.
//     x = h + m + l,   h = bf16(x), m = bf16(x - h), l = bf16(x - h - m)      (round to nearest even; both subtractions are exact)
#pragma once
#include <hip/hip_runtime.h>

namespace mz {

__host__ __device__ __forceinline__ unsigned conv_bf16_rne(unsigned u) { return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16; }

// x = h + m + l exactly (finite x): bf16 bit patterns of the three terms
__device__ __forceinline__ void conv_split3(float x, unsigned& h, unsigned& m, unsigned& l) {
    h = conv_bf16_rne(__float_as_uint(x));
    const float r1 = x - __uint_as_float(h << 16);
    m = conv_bf16_rne(__float_as_uint(r1));
    const float r2 = r1 - __uint_as_float(m << 16);
    l = conv_bf16_rne(__float_as_uint(r2));
}

}  // namespace mz
