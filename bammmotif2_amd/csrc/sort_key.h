// The order-preserving unsigned key of a float: what the radix sort (occ.hip) orders by and the merge of sorted runs
// (fdr.hip: k_fdr_merge) compares, so that the two cannot disagree about an order or about the bits they write back.
// Device code only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace bamm {

// float bits -> unsigned key in the order of the values; -0 counts as +0 (std::less<float> compares values).  The scorer
// cannot produce -0 (its sums start from +0, and +0 + -0 = +0): the mapping is for arrays that come from elsewhere.
__device__ __forceinline__ uint32_t key_of(float x) {
    uint32_t u = __float_as_uint(x);
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
// the float a key came from (-0 comes back as +0): equal keys are equal bits
__device__ __forceinline__ float float_of(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

}  // namespace bamm
