// k_records.hip -- the records of a ragged corpus (sliding_common.hpp has the layout): packed sub-fingerprints of whole entries
// -> records, records read from a file -> records with their derived fields recomputed, and the synthetic ragged corpus.
#include "sliding_common.hpp"

namespace lbad {
namespace {

// even-position bits of a 32-bit word, compacted into 16
__device__ __forceinline__ uint32_t even_bits(uint32_t x) {
    x &= 0x55555555u;
    x = (x | (x >> 1)) & 0x33333333u;
    x = (x | (x >> 2)) & 0x0F0F0F0Fu;
    x = (x | (x >> 4)) & 0x00FF00FFu;
    x = (x | (x >> 8)) & 0x0000FFFFu;
    return x;
}

// the record of the eight words P[0..3], N[0..3] (pairs beyond 99 cleared) with its derived fields: the full-range table
// row and its place (entry `ent`, sub-fingerprint i of it, r more behind it)
__device__ __forceinline__ void store_record(uint4* __restrict__ recs, uint64_t p, const uint32_t (&P)[4], const uint32_t (&N)[4],
                                             uint32_t ent, uint32_t i, uint32_t r) {
    const uint32_t p3 = P[3] & 0xFu, n3 = N[3] & 0xFu;
    const uint32_t possible = __popc(P[0] | N[0]) + __popc(P[1] | N[1]) + __popc(P[2] | N[2]) + __popc(p3 | n3);
    const uint32_t row = possible * (possible + 1u) / 2u;
    const uint32_t isat = i < 15u ? i : 15u, rsat = r < 15u ? r : 15u;
    recs[2 * p] = make_uint4(P[0], P[1], P[2], p3 | (row << 4) | ((ent >> 28) << 17) | (isat << 21) | (rsat << 25));
    recs[2 * p + 1] = make_uint4(N[0], N[1], N[2], n3 | (ent << 4));
}

// entry e with off[e] <= p < off[e + 1] among n entries (off: n + 1 increasing record positions)
__device__ __forceinline__ uint64_t entry_of(const uint32_t* __restrict__ off, uint64_t n, uint64_t p) {
    uint64_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) >> 1;
        if (off[mid] <= p) lo = mid; else hi = mid;
    }
    return lo;
}

// packed sub-fingerprints (8-word slots, Boolean b at bit b) of whole entries -> records.  off: ABSOLUTE record
// positions of the new entries (n_new + 1 values); slot t becomes record off[0] + t
__global__ __launch_bounds__(kSlThreads) void pack_records_kernel(const uint32_t* __restrict__ slots, uint64_t n_new_pos,
                                                                  const uint32_t* __restrict__ off, uint64_t n_new,
                                                                  uint32_t first_entry, uint4* __restrict__ recs) {
    const uint64_t t = (uint64_t)blockIdx.x * kSlThreads + threadIdx.x;
    if (t >= n_new_pos) return;
    const uint64_t p = (uint64_t)off[0] + t;
    const uint64_t e = entry_of(off, n_new, p);
    const uint4* s = reinterpret_cast<const uint4*>(slots + t * kPackedWords);
    const uint4 a = s[0], b = s[1];
    const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    // pairs 0..99 live in bits 0..199 = words 0..6 (word 6: 8 bits)
    uint32_t P[4], N[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t w0 = w[2 * k], w1 = 2 * k + 1 < 7 ? w[2 * k + 1] : 0u;
        P[k] = even_bits(w0) | (even_bits(w1) << 16);
        N[k] = even_bits(w0 >> 1) | (even_bits(w1 >> 1) << 16);
    }
    store_record(recs, p, P, N, first_entry + (uint32_t)e, (uint32_t)p - off[e], off[e + 1] - 1u - (uint32_t)p);
}

// Records that come from a FILE: keep the 200 Booleans, recompute everything derived (table row; place fields from the
// offsets the loader built out of the validated counts), clear everything reserved.
// old_layout: the round-3 file ("LBADCRP2": P at bits 0..99, N at bits 100..199, place fields above).
__global__ __launch_bounds__(kSlThreads) void restamp_records_kernel(uint4* __restrict__ recs, const uint32_t* __restrict__ off,
                                                                     uint64_t n_entries, uint64_t n, uint32_t old_layout,
                                                                     uint4 pair_mask) {
    const uint64_t t = (uint64_t)blockIdx.x * kSlThreads + threadIdx.x;
    if (t >= n) return;
    const uint4 a = recs[2 * t], b = recs[2 * t + 1];
    uint32_t P[4], N[4];
    if (old_layout) {
        P[0] = a.x; P[1] = a.y; P[2] = a.z; P[3] = a.w & 0xFu;
        N[0] = __funnelshift_r(a.w, b.x, 4);
        N[1] = __funnelshift_r(b.x, b.y, 4);
        N[2] = __funnelshift_r(b.y, b.z, 4);
        N[3] = (b.z >> 4) & 0xFu;
    } else {
        P[0] = a.x; P[1] = a.y; P[2] = a.z; P[3] = a.w & 0xFu;
        N[0] = b.x; N[1] = b.y; N[2] = b.z; N[3] = b.w & 0xFu;
    }
    const uint32_t pm[4] = {pair_mask.x, pair_mask.y, pair_mask.z, pair_mask.w};   // pairs the length has
#pragma unroll
    for (int k = 0; k < 4; ++k) { P[k] &= pm[k]; N[k] &= pm[k]; }
    const uint64_t e = entry_of(off, n_entries, t);
    store_record(recs, t, P, N, (uint32_t)e, (uint32_t)t - off[e], off[e + 1] - 1u - (uint32_t)t);
}

// synthetic ragged corpus: sub-fingerprint s of entry e is lbo_synth_entry's (oracle/lbad_oracle.c), entry e has
// lo + mix32(seed ^ 0x52414747 ^ e) % (hi - lo + 1) sub-fingerprints (the caller passes the prefix sums)
__device__ __forceinline__ uint32_t sl_mix32(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du;
    x ^= x >> 15; x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

__global__ __launch_bounds__(kSlThreads) void synth_ragged_kernel(uint32_t seed, uint64_t first_entry, uint64_t n_entries,
                                                                  const uint32_t* __restrict__ off, uint64_t n_pos,
                                                                  uint32_t subfp_len, uint32_t* __restrict__ out) {
    const uint64_t p = (uint64_t)blockIdx.x * kSlThreads + threadIdx.x;
    if (p >= n_pos) return;
    uint64_t lo = 0, hi = n_entries;
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) >> 1;
        if (off[mid] <= p) lo = mid; else hi = mid;
    }
    const uint64_t entry = first_entry + lo;
    const uint32_t s = (uint32_t)p - off[lo];
    const uint32_t key = sl_mix32(seed ^ sl_mix32((uint32_t)entry) ^ (uint32_t)(entry >> 32) * 0x632BE5ABu);
    const uint32_t pairs = (subfp_len + 1) / 2;
    uint32_t w[kPackedWords] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll 4
    for (uint32_t pr = 0; pr < pairs; ++pr) {
        const uint32_t r = sl_mix32(key + (s * 1024u + pr) * 0x9E3779B1u);
        uint32_t pos = 0, neg = 0;
        if (r % 100u != 0u) {
            if ((r >> 8) & 1u) pos = 1; else neg = 1;
        }
        const uint32_t b = 2 * pr;
        if (b + 1 >= subfp_len) neg = 0;
        const uint32_t two = pos | (neg << 1);
#pragma unroll
        for (uint32_t k = 0; k < kPackedWords; ++k)
            if (k == (b >> 5)) w[k] |= two << (b & 31);
    }
    uint4* dst = reinterpret_cast<uint4*>(out + p * kPackedWords);
    dst[0] = make_uint4(w[0], w[1], w[2], w[3]);
    dst[1] = make_uint4(w[4], w[5], w[6], w[7]);
}

}  // namespace

// d_off_new: ABSOLUTE record positions of the n_new new entries (n_new + 1 values, the first one = the position of slot 0)
hipError_t launch_pack_records(const uint32_t* d_slots, uint64_t n_new_pos, const uint32_t* d_off_new, uint64_t n_new,
                               uint32_t first_entry, uint4* d_recs, hipStream_t stream) {
    if (n_new_pos == 0) return hipSuccess;
    const uint64_t blocks = (n_new_pos + kSlThreads - 1) / kSlThreads;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pack_records_kernel, dim3((uint32_t)blocks), dim3(kSlThreads), 0, stream, d_slots, n_new_pos, d_off_new,
                       n_new, first_entry, d_recs);
    return hipGetLastError();
}

hipError_t launch_restamp_records(uint4* d_recs, const uint32_t* d_off, uint64_t n_entries, uint64_t n, uint32_t subfp_len,
                                  bool old_layout, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const uint64_t blocks = (n + kSlThreads - 1) / kSlThreads;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(restamp_records_kernel, dim3((uint32_t)blocks), dim3(kSlThreads), 0, stream, d_recs, d_off, n_entries, n,
                       old_layout ? 1u : 0u, pair_mask(subfp_len));
    return hipGetLastError();
}

hipError_t launch_synth_ragged(uint32_t seed, uint64_t first_entry, uint64_t n_entries, const uint32_t* d_off,
                               uint64_t n_pos, uint32_t subfp_len, uint32_t* d_out, hipStream_t stream) {
    if (n_pos == 0) return hipSuccess;
    const uint64_t blocks = (n_pos + kSlThreads - 1) / kSlThreads;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(synth_ragged_kernel, dim3((uint32_t)blocks), dim3(kSlThreads), 0, stream, seed, first_entry,
                       n_entries, d_off, n_pos, subfp_len, d_out);
    return hipGetLastError();
}

}  // namespace lbad
