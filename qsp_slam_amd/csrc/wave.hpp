// wave.hpp -- the sum over the 64 lanes of a wave as an xor butterfly: every lane ends with the same total in the same bits.
#pragma once
#include <hip/hip_runtime.h>

namespace qsp {

__device__ inline double wave_sum(double a) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
    return a;
}

}  // namespace qsp
