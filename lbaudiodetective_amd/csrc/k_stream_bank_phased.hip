// k_stream_bank_phased.hip -- the device side the phased stream bank adds to k_stream_bank.hip (api_stream_bank.cpp, DESIGN.md
// 4.4aa): per real channel a RING of the last 128 frame rows in HBM, row number t of the channel at slot t mod 128.
//
// A push transforms a channel's new windows once (whatever the number of phases) into the push's block of new rows; stage 2 at
// a row hop (k_haar_select32_hop.hip, k_haar_select_hop.hip) then reads every frame the push completes -- at any phase -- from
// the ring (the rows of earlier pushes) and from that block.  Behind it the kernel here moves the channel's last
// min(n_new, 128) new rows to their ring slots, for the frames later pushes complete.  A copy: one workgroup per channel of the
// push, 16-byte words where the row width allows them; a slot has one writer (the rows are at most 128, consecutive), and
// nothing is read that this launch writes.
#include "internal.hpp"

namespace lbad {
namespace {

constexpr uint32_t kRingThreads = 256;
constexpr uint32_t kRingMaxGrid = 1u << 16;

template <typename T>
__device__ __forceinline__ void ring_rows(T* __restrict__ ring, const T* __restrict__ fresh, uint32_t row_t, const PhasedRow& row) {
    const uint32_t start = row.n_new > kRowsPerFrame ? row.n_new - kRowsPerFrame : 0u;
    const uint32_t n = (row.n_new - start) * row_t;                   // <= 128 rows
    T* __restrict__ dst = ring + (uint64_t)row.channel * kRowsPerFrame * row_t;
    const T* __restrict__ src = fresh + (row.new_row0 + start) * row_t;
    for (uint32_t i = threadIdx.x; i < n; i += kRingThreads) {
        const uint32_t r = i / row_t, c = i - r * row_t;
        dst[((row.ring_at + start + r) & (kRowsPerFrame - 1u)) * row_t + c] = src[i];
    }
}

__global__ __launch_bounds__(kRingThreads) void bank_row_ring_kernel(float* __restrict__ ring, uint32_t row_dw,
                                                                     const PhasedRow* __restrict__ rows, uint32_t n_rows,
                                                                     const float* __restrict__ fresh) {
    for (uint32_t r = blockIdx.x; r < n_rows; r += gridDim.x) {
        const PhasedRow row = rows[r];
        if ((row_dw & 3u) == 0)        // (the ring and the block of new rows are 16-byte aligned, so every row is)
            ring_rows(reinterpret_cast<float4*>(ring), reinterpret_cast<const float4*>(fresh), row_dw / 4, row);
        else
            ring_rows(ring, fresh, row_dw, row);
    }
}

}  // namespace

hipError_t launch_bank_row_ring(float* d_row_ring, uint32_t row_dw, const PhasedRow* d_rows, uint32_t n_rows, const float* d_new_rows,
                                hipStream_t stream) {
    if (n_rows == 0 || row_dw == 0) return hipSuccess;
    hipLaunchKernelGGL(bank_row_ring_kernel, dim3(strided_grid(n_rows, kRingMaxGrid)), dim3(kRingThreads), 0, stream, d_row_ring, row_dw,
                       d_rows, n_rows, d_new_rows);
    return hipGetLastError();
}

}  // namespace lbad
