// segments_common.hpp -- what the two segments kernels share (k_segments.hip over a timeline's winners, k_occurrence_segments.hip
// over all cells of an occurrences row): the LDS budget of a workgroup and the mask helpers of the one-wave walk.
#pragma once
#include "internal.hpp"

namespace lbad {

constexpr size_t kSgLdsBudget = 160 * 1024 - 64;

// the bits of mask word w that [o, e) covers; the caller passes only words the span reaches (o / 64 <= w <= (e - 1) / 64)
__device__ __forceinline__ unsigned long long sg_span_bits(uint32_t w, uint32_t o, uint32_t e) {
    const uint32_t lo = w == (o >> 6) ? (o & 63u) : 0u;
    const uint32_t hi = w == ((e - 1u) >> 6) ? ((e - 1u) & 63u) : 63u;
    return (~0ull << lo) & (~0ull >> (63u - hi));
}

__device__ __forceinline__ void sg_wave_sync() {
    // LDS operations of one wave execute in order; this only stops the compiler from moving them
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

}  // namespace lbad
