// wave.hpp -- the sum, and the minimum of a 64-bit key, over the 64 lanes of a wave as an xor butterfly: every lane ends with the
// same result in the same bits.
#pragma once
#include <hip/hip_runtime.h>

namespace qsp {

__device__ inline double wave_sum(double a) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
    return a;
}

__device__ inline unsigned long long wave_min(unsigned long long key) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(key, o, 64);
        key = other < key ? other : key;
    }
    return key;
}

}  // namespace qsp
