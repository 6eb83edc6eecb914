// ba_enum_common.hpp -- what the two exhaustive kernels share, k_enum (ba_enum.hip,
// docs/SEMANTICS.md §8) and k_kenum (ba_kenum.hip, §11): one lane holds one
// 64-strategy word w = S / 64, and a free bit of the strategy index is a plane of it.
#pragma once
#include "ba_wave_proto.hpp"

namespace ba {

// plane of free bit i (uniform) in word w
__device__ __forceinline__ uint64_t enum_plane(uint32_t i, uint32_t wlo, uint32_t whi) {
    if (i < 6u) {
        return i == 0u   ? 0xAAAAAAAAAAAAAAAAull
               : i == 1u ? 0xCCCCCCCCCCCCCCCCull
               : i == 2u ? 0xF0F0F0F0F0F0F0F0ull
               : i == 3u ? 0xFF00FF00FF00FF00ull
               : i == 4u ? 0xFFFF0000FFFF0000ull
                         : 0xFFFFFFFF00000000ull;
    }
    const uint32_t sh = i - 6u;
    const uint32_t h = sh < 32u ? wlo : whi;
    const int32_t s = (int32_t)(h << (31u - (sh & 31u))) >> 31;  // -(bit sh of w)
    return (uint64_t)(int64_t)s;
}

__device__ __forceinline__ uint64_t enum_wave_sum(uint64_t x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
    return x;
}

}  // namespace ba
