// k_stream_bank.hip -- the device side of the stream bank (api_stream_bank.cpp): N live channels whose carried
// partial frames and most recent sub-fingerprints stay in HBM between pushes.
//
// A push hands over one ragged block of new samples.  The host knows every count, so it plans the push alone and uploads one
// BankRow per channel that received samples; nothing here is read back.  For a channel, cat = carried[0, p) ++ fresh[0, n) is the
// signal it still owes frames for; frame f of the push reads cat[f * hop, f * hop + W + hop).
//
//   stage     one workgroup per complete frame of the pass: its W + hop samples out of cat into a batch of one-frame clips (rows
//             of W + hop floats: 16-byte aligned, even) for fingerprint_clips_device.  A frame may lie in the carried samples, in
//             the fresh ones or across the seam.
//   rows      behind the last pass, one lane per 16 bytes of the push's packed sub-fingerprints: into the caller's block (channel
//             order, then time) and into the channel's history ring at (total + f) mod H -- only the last H frames of a channel,
//             so no ring slot has two writers.
//   carry     behind the last pass, one workgroup per row: the samples the channel carries on.  A channel without a complete
//             frame appends its fresh samples behind the p it has.  Otherwise cat[ready * hop, p + n) moves to the front, and since
//             that would move the carried samples left over themselves the channel has TWO carried buffers: the launch reads side
//             s and writes side s ^ 1, and the host flips its record of the side.  No launch reads what another workgroup of it
//             may write.
//   window    one lane per 16 bytes of the output: the Q most recent ring rows of every listed channel, oldest first; the host
//             supplies each listed channel's first slot, so a channel may be listed twice and in any order.
//
// These are copies: 16-byte loads and stores where the addresses allow (the carried buffers, the clips, the rings and the packed
// blocks are 16-byte aligned by construction, and hop is a multiple of 128 samples), and 4-byte loads for a fresh run that starts
// off a 16-byte boundary -- a channel's run begins wherever the runs before it end.
#include "internal.hpp"

namespace lbad {
namespace {

constexpr uint32_t kBankThreads = 256;
constexpr uint32_t kBankMaxGrid = 1u << 16;      // most workgroups of a launch (its workgroups stride over the rest)

// the row whose frames hold frame g of the push: the last r with rows[r].first <= g.  A row without a complete frame shares its
// `first` with the row behind it, and the last row's is the push's total when it has none, so the answer always has the frame.
__device__ __forceinline__ uint32_t bank_row_of(const BankRow* __restrict__ rows, uint32_t n_rows, uint32_t g) {
    uint32_t lo = 0, hi = n_rows;                // rows[lo].first <= g < rows[hi].first (hi == n_rows: none)
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (rows[mid].first <= g) lo = mid; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ bool bank_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// n4 x 16 bytes from src (any 4-byte boundary) to dst (a 16-byte boundary) by the whole workgroup: 16-byte loads where src allows
// them, four 4-byte loads a lane otherwise; four independent steps in flight per lane
__device__ __forceinline__ void bank_copy_words(float4* __restrict__ dst, const float* __restrict__ src, uint32_t n4) {
    if (bank_aligned16(src)) {
        const float4* __restrict__ src4 = reinterpret_cast<const float4*>(src);
#pragma unroll 4
        for (uint32_t i = threadIdx.x; i < n4; i += kBankThreads) dst[i] = src4[i];
    } else {
#pragma unroll 4
        for (uint32_t i = threadIdx.x; i < n4; i += kBankThreads) {
            const float* __restrict__ s = src + 4ull * i;
            dst[i] = make_float4(s[0], s[1], s[2], s[3]);
        }
    }
}

// dst[0, len) = cat[s0, s0 + len), cat = carried[0, p) ++ fresh[0, ...), by the whole workgroup.  The caller guarantees that the
// range lies inside cat.  With dst on a 16-byte boundary the range goes as 16-byte words: those wholly in the carried part, those
// wholly in the fresh part, and sample by sample the one word that holds the seam and the up to three samples behind the last word.
__device__ __forceinline__ void bank_copy(float* __restrict__ dst, uint32_t len, const float* __restrict__ carried, uint32_t p,
                                          const float* __restrict__ fresh, uint64_t s0) {
    auto at = [&](uint64_t s) { return s < p ? carried[s] : fresh[s - p]; };
    if (!bank_aligned16(dst)) {
        for (uint32_t i = threadIdx.x; i < len; i += kBankThreads) dst[i] = at(s0 + i);
        return;
    }
    const uint32_t whole = len & ~3u;
    const uint32_t n_carried = s0 < p ? (uint32_t)(p - s0 < len ? p - s0 : len) : 0u;   // samples of the range that are carried
    const uint32_t a = (n_carried & ~3u) < whole ? (n_carried & ~3u) : whole;           // [0, a): words of carried samples
    const uint32_t b = ((n_carried + 3u) & ~3u) < whole ? ((n_carried + 3u) & ~3u) : whole;   // [b, whole): words of fresh samples
    float4* __restrict__ dst4 = reinterpret_cast<float4*>(dst);
    if (a) bank_copy_words(dst4, carried + s0, a / 4);
    if (whole > b) bank_copy_words(dst4 + b / 4, fresh + (s0 + b - p), (whole - b) / 4);      // (s0 + b >= p here)
    if (threadIdx.x < b - a) dst[a + threadIdx.x] = at(s0 + a + threadIdx.x);
    if (threadIdx.x < len - whole) dst[whole + threadIdx.x] = at(s0 + whole + threadIdx.x);
}

__device__ __forceinline__ float* bank_carry(const BankDev& b, uint32_t side, uint32_t channel) {
    return b.carry + ((uint64_t)side * b.n_channels + channel) * b.carry_stride;
}

// frames [g0, g0 + nf) of the push -> clips[nf][W + hop]
__global__ __launch_bounds__(kBankThreads) void bank_stage_kernel(BankDev b, const BankRow* __restrict__ rows, uint32_t n_rows,
                                                                  const float* __restrict__ fresh, uint32_t g0, uint32_t nf,
                                                                  float* __restrict__ clips) {
    const uint32_t len = b.window + b.hop;
    for (uint32_t i = blockIdx.x; i < nf; i += gridDim.x) {
        const uint32_t g = g0 + i;
        const BankRow row = rows[bank_row_of(rows, n_rows, g)];
        const uint64_t f = g - row.first;
        bank_copy(clips + (uint64_t)i * len, len, bank_carry(b, row.side, row.channel), row.p, fresh + row.fresh_at, f * b.hop);
    }
}

// the push's packed sub-fingerprints (total x 32 bytes at packed) -> out (optional) and the rings
__global__ __launch_bounds__(kBankThreads) void bank_commit_rows_kernel(BankDev b, const BankRow* __restrict__ rows, uint32_t n_rows,
                                                                        const uint4* __restrict__ packed, uint32_t total,
                                                                        uint4* __restrict__ out) {
    const uint64_t halves = 2ull * total;
    uint4* __restrict__ ring = reinterpret_cast<uint4*>(b.ring);
    for (uint64_t t = (uint64_t)blockIdx.x * kBankThreads + threadIdx.x; t < halves; t += (uint64_t)gridDim.x * kBankThreads) {
        const uint32_t g = (uint32_t)(t >> 1);
        const BankRow row = rows[bank_row_of(rows, n_rows, g)];
        const uint32_t f = g - row.first;
        const uint4 v = packed[t];
        if (out) out[t] = v;
        if (row.ready - f <= b.history) {        // a later frame of this push takes the slot of an earlier one otherwise
            const uint64_t slot = ((uint64_t)row.ring_at + f) % b.history;
            ring[((uint64_t)row.channel * b.history + slot) * 2 + (t & 1u)] = v;
        }
    }
}

// what every row's channel carries on
__global__ __launch_bounds__(kBankThreads) void bank_commit_carry_kernel(BankDev b, const BankRow* __restrict__ rows, uint32_t n_rows,
                                                                         const float* __restrict__ fresh) {
    for (uint32_t r = blockIdx.x; r < n_rows; r += gridDim.x) {
        const BankRow row = rows[r];
        float* cur = bank_carry(b, row.side, row.channel);
        const float* run = fresh + row.fresh_at;
        if (row.ready == 0) {                    // (reads the fresh samples only: s0 == p)
            bank_copy(cur + row.p, row.n, cur, row.p, run, row.p);
        } else {
            const uint64_t used = (uint64_t)row.ready * b.hop;
            bank_copy(bank_carry(b, row.side ^ 1u, row.channel), (uint32_t)((uint64_t)row.p + row.n - used), cur, row.p, run, used);
        }
    }
}

// list[j] = (channel, ring slot of the oldest of its q rows) -> out[j][q][32 bytes]
__global__ __launch_bounds__(kBankThreads) void bank_window_kernel(BankDev b, const uint2* __restrict__ list, uint64_t n_list, uint32_t q,
                                                                   uint4* __restrict__ out) {
    const uint64_t per = 2ull * q, halves = n_list * per;
    const uint4* __restrict__ ring = reinterpret_cast<const uint4*>(b.ring);
    for (uint64_t t = (uint64_t)blockIdx.x * kBankThreads + threadIdx.x; t < halves; t += (uint64_t)gridDim.x * kBankThreads) {
        const uint64_t j = t / per, rem = t - j * per;
        const uint2 e = list[j];
        const uint64_t slot = ((uint64_t)e.y + (rem >> 1)) % b.history;
        out[t] = ring[((uint64_t)e.x * b.history + slot) * 2 + (rem & 1u)];
    }
}

inline uint64_t bank_blocks(uint64_t lanes) { return (lanes + kBankThreads - 1) / kBankThreads; }

}  // namespace

hipError_t launch_bank_stage(const BankDev& b, const BankRow* d_rows, uint32_t n_rows, const float* d_fresh, uint32_t g0, uint32_t nf,
                             float* d_clips, hipStream_t stream) {
    if (nf == 0) return hipSuccess;
    hipLaunchKernelGGL(bank_stage_kernel, dim3(strided_grid(nf, kBankMaxGrid)), dim3(kBankThreads), 0, stream, b, d_rows, n_rows, d_fresh,
                       g0, nf, d_clips);
    return hipGetLastError();
}

hipError_t launch_bank_commit_rows(const BankDev& b, const BankRow* d_rows, uint32_t n_rows, const uint32_t* d_packed, uint32_t total,
                                   void* d_out, hipStream_t stream) {
    if (n_rows == 0 || total == 0) return hipSuccess;
    hipLaunchKernelGGL(bank_commit_rows_kernel, dim3(strided_grid(bank_blocks(2ull * total), kBankMaxGrid)), dim3(kBankThreads), 0,
                       stream, b, d_rows, n_rows, reinterpret_cast<const uint4*>(d_packed), total, static_cast<uint4*>(d_out));
    return hipGetLastError();
}

hipError_t launch_bank_commit_carry(const BankDev& b, const BankRow* d_rows, uint32_t n_rows, const float* d_fresh, hipStream_t stream) {
    if (n_rows == 0) return hipSuccess;
    hipLaunchKernelGGL(bank_commit_carry_kernel, dim3(strided_grid(n_rows, kBankMaxGrid)), dim3(kBankThreads), 0, stream, b, d_rows,
                       n_rows, d_fresh);
    return hipGetLastError();
}

hipError_t launch_bank_commit(const BankDev& b, const BankRow* d_rows, uint32_t n_rows, const float* d_fresh, const uint32_t* d_packed,
                              uint32_t total, void* d_out, hipStream_t stream) {
    const hipError_t e = launch_bank_commit_rows(b, d_rows, n_rows, d_packed, total, d_out, stream);
    return e != hipSuccess ? e : launch_bank_commit_carry(b, d_rows, n_rows, d_fresh, stream);
}

hipError_t launch_bank_window(const BankDev& b, const uint2* d_list, uint64_t n_list, uint32_t q, void* d_out, hipStream_t stream) {
    if (n_list == 0 || q == 0) return hipSuccess;
    hipLaunchKernelGGL(bank_window_kernel, dim3(strided_grid(bank_blocks(2ull * n_list * q), kBankMaxGrid)), dim3(kBankThreads), 0, stream,
                       b, d_list, n_list, q, static_cast<uint4*>(d_out));
    return hipGetLastError();
}

}  // namespace lbad
