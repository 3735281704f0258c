// k_query.hip -- the scans' query blocks built ON the device from packed sub-fingerprints (8 little-endian words each, the
// layout LBAudioDetectiveFingerprintClipsDevice writes and LBAudioDetectiveCorpusAppendPackedDevice reads): what the host
// builders build_plane_query (k_compare.hip), build_sliding_query (sliding.cpp) and build_align_query (k_align.hip) make from
// a fingerprint handle's Booleans, word for word, so that a query that is already in HBM never visits the host.  Every
// builder first clears the bits at or above the sub-fingerprint length: the result depends on the first `length` Booleans only.
// Not a hot loop -- a lane per output word or per sub-fingerprint, nothing kept in indexed arrays (no scratch memory).
#include "internal.hpp"

namespace lbad {
namespace {

constexpr int kQbThreads = 256;
// the specialised uniform scan's block (k_compare.hip: PlaneShape, kPlaneQueryWords); the launcher checks the size it names
constexpr uint32_t kLp = 200;
constexpr uint32_t kSubSpan = 7;
constexpr uint32_t kBlockWords = 144;

// the bits of word w of a row that lie below `lim`
__device__ __forceinline__ uint32_t below(uint32_t w, uint32_t lim) {
    const uint32_t base = 32u * w;
    return lim <= base ? 0u : (lim - base >= 32u ? 0xFFFFFFFFu : ((1u << (lim - base)) - 1u));
}

__device__ __forceinline__ uint32_t row_word(const uint32_t* __restrict__ r, int j, uint32_t lim) {
    return (j >= 0 && j < (int)kPackedWords) ? (r[j] & below((uint32_t)j, lim)) : 0u;
}

// 32 bits of a row from bit b on (b > -32 may be negative): bit i is the row's bit b + i where 0 <= b + i < lim, else 0
__device__ __forceinline__ uint32_t row_window(const uint32_t* __restrict__ r, int b, uint32_t lim) {
    const int j = b >> 5;                         // (arithmetic shift: the floor)
    const uint32_t sh = (uint32_t)b & 31u;
    const uint32_t lo = row_word(r, j, lim);
    if (sh == 0u) return lo;
    return (lo >> sh) | (row_word(r, j + 1, lim) << (32u - sh));
}

// bit p of the result = bit 2 p of x (p < 16)
__device__ __forceinline__ uint32_t even_bits(uint32_t x) {
    x &= 0x55555555u;
    x = (x | (x >> 1)) & 0x33333333u;
    x = (x | (x >> 2)) & 0x0F0F0F0Fu;
    x = (x | (x >> 4)) & 0x00FF00FFu;
    x = (x | (x >> 8)) & 0x0000FFFFu;
    return x;
}

// pairs (Booleans 2 p, 2 p + 1) of a word with at least one Boolean set, as bits at the even places (a pair never straddles a word)
__device__ __forceinline__ uint32_t live_pairs(uint32_t x) { return (x | (x >> 1)) & 0x55555555u; }

// ---- uniform corpus, specialised shape: build_plane_query, zero padded to kBlockWords -- one lane per output word ---------
__global__ __launch_bounds__(kQbThreads) void build_plane_queries_kernel(const uint32_t* __restrict__ rows, uint64_t n_queries,
                                                                         uint32_t n_sub, uint32_t pair_bits,
                                                                         uint32_t* __restrict__ blocks) {
    const uint64_t t = (uint64_t)blockIdx.x * kQbThreads + threadIdx.x;
    if (t >= n_queries * kBlockWords) return;
    const uint64_t q = t / kBlockWords;
    const uint32_t w = (uint32_t)(t - q * kBlockWords);
    const uint32_t* __restrict__ qrows = rows + q * n_sub * kPackedWords;
    const uint32_t words = ((n_sub * kLp + 127u) / 128u) * 4u;
    const uint32_t off_possible = words + n_sub * kSubSpan;
    uint32_t v = 0u;
    if (w < words) {
        // the tight bitstream: sub-fingerprint s at bits [200 s, 200 s + 200); a word may hold the end of one and the start of the next
        const uint32_t pos = 32u * w;
        const uint32_t s = pos / kLp, b = pos - s * kLp;
        if (s < n_sub) {
            v = row_window(qrows + s * kPackedWords, (int)b, kLp);
            const uint32_t got = kLp - b;
            if (got < 32u && s + 1u < n_sub) v |= row_window(qrows + (s + 1u) * kPackedWords, 0, kLp) << got;
        }
    } else if (w < off_possible) {
        // the pairs inside the range with a Boolean set, at the place of the pair's first bit in word w0 + j of the stream
        const uint32_t m = w - words;
        const uint32_t s = m / kSubSpan, j = m - s * kSubSpan;
        const uint32_t w0 = (s * kLp) >> 5;
        const int b = (int)(32u * (w0 + j)) - (int)(s * kLp);          // even: pairs keep their parity
        v = live_pairs(row_window(qrows + s * kPackedWords, b, pair_bits));
    } else if (w < off_possible + 3u * n_sub) {
        const uint32_t m = w - off_possible;
        const uint32_t kind = m / n_sub, s = m - kind * n_sub;
        const uint32_t* __restrict__ r = qrows + s * kPackedWords;
        uint32_t possible = 0u;
#pragma unroll
        for (uint32_t i = 0; i < kPackedWords; ++i) possible += __popc(live_pairs(r[i] & below(i, pair_bits)));
        // build_plane_query's own three expressions, correctly rounded: the scan's quotient relies on these bits
        const float pf = (float)possible;
        const float rh = possible ? __fdiv_rn(1.0f, pf) : 0.0f;
        const float rl = __fmul_rn(__fmaf_rn(-pf, rh, possible ? 1.0f : 0.0f), rh);
        v = __float_as_uint(kind == 0u ? pf : (kind == 1u ? rh : rl));
    }
    blocks[t] = v;
}

// ---- ragged corpus: build_sliding_query's block -- one lane per sub-fingerprint (and per block's zero slack) -----
__global__ __launch_bounds__(kQbThreads) void build_sliding_queries_kernel(const uint32_t* __restrict__ rows, uint64_t n_queries,
                                                                           uint32_t per, uint32_t subfp_len, uint4 rm,
                                                                           uint4* __restrict__ blocks) {
    const uint64_t t = (uint64_t)blockIdx.x * kQbThreads + threadIdx.x;
    const uint64_t per1 = (uint64_t)per + 1u;
    if (t >= n_queries * per1) return;
    const uint64_t q = t / per1;
    const uint32_t s = (uint32_t)(t - q * per1);
    uint4 P = make_uint4(0u, 0u, 0u, 0u), N = P, Z = P, T = P;
    if (s < per) {
        const uint32_t* __restrict__ r = rows + (q * per + s) * kPackedWords;
        uint32_t p[4], n[4];
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) {
            const uint32_t a = r[2u * k] & below(2u * k, subfp_len), b = r[2u * k + 1u] & below(2u * k + 1u, subfp_len);
            p[k] = even_bits(a) | (even_bits(b) << 16);
            n[k] = even_bits(a >> 1) | (even_bits(b >> 1) << 16);
        }
        P = make_uint4(p[0], p[1], p[2], p[3]);
        N = make_uint4(n[0], n[1], n[2], n[3]);
        Z = make_uint4((p[0] | n[0]) & rm.x, (p[1] | n[1]) & rm.y, (p[2] | n[2]) & rm.z, (p[3] | n[3]) & rm.w);
        const uint32_t possible = __popc(Z.x) + __popc(Z.y) + __popc(Z.z) + __popc(Z.w);
        T = make_uint4(possible * (possible + 1u) / 2u, possible, 0u, 0u);
    }
    uint4* __restrict__ o = blocks + t * 4u;
    o[0] = P; o[1] = N; o[2] = Z; o[3] = T;
}

// ---- rows as the generic uniform scan and the alignment read them -- one lane per sub-fingerprint -------------------------
// PAIRS: the first / second Booleans of the pairs (build_align_query's ragged form); otherwise the slot words themselves,
// cleared from the length on.  desc (optional): per query (first sub-fingerprint, count), launch_align_keys' table.
template <bool PAIRS>
__global__ __launch_bounds__(kQbThreads) void build_query_rows_kernel(const uint32_t* __restrict__ rows, uint64_t n_rows,
                                                                      uint32_t subfp_len, uint4* __restrict__ out,
                                                                      uint2* __restrict__ desc, uint32_t n_queries, uint32_t per) {
    const uint64_t t = (uint64_t)blockIdx.x * kQbThreads + threadIdx.x;
    if (t >= n_rows) return;
    const uint32_t* __restrict__ r = rows + t * kPackedWords;
    uint32_t x[8];
#pragma unroll
    for (uint32_t i = 0; i < 8u; ++i) x[i] = r[i] & below(i, subfp_len);
    if constexpr (PAIRS) {
        out[2u * t] = make_uint4(even_bits(x[0]) | (even_bits(x[1]) << 16), even_bits(x[2]) | (even_bits(x[3]) << 16),
                                 even_bits(x[4]) | (even_bits(x[5]) << 16), even_bits(x[6]) | (even_bits(x[7]) << 16));
        out[2u * t + 1u] = make_uint4(even_bits(x[0] >> 1) | (even_bits(x[1] >> 1) << 16), even_bits(x[2] >> 1) | (even_bits(x[3] >> 1) << 16),
                                      even_bits(x[4] >> 1) | (even_bits(x[5] >> 1) << 16), even_bits(x[6] >> 1) | (even_bits(x[7] >> 1) << 16));
    } else {
        out[2u * t] = make_uint4(x[0], x[1], x[2], x[3]);
        out[2u * t + 1u] = make_uint4(x[4], x[5], x[6], x[7]);
    }
    if (desc && t < n_queries) desc[t] = make_uint2((uint32_t)t * per, per);
}

bool grid_of(uint64_t lanes, uint32_t& grid) {
    const uint64_t blocks = (lanes + kQbThreads - 1) / kQbThreads;
    if (blocks == 0 || blocks > 0x7fffffffull) return false;
    grid = (uint32_t)blocks;
    return true;
}

}  // namespace

hipError_t launch_build_plane_queries(const uint32_t* d_rows, uint32_t n_queries, uint32_t n_sub, uint32_t range,
                                      uint32_t* d_blocks, hipStream_t stream) {
    if (plane_query_words() != kBlockWords || !planes_fast_supported(kLp, n_sub, n_sub) || planes_fast_const_words(n_sub) > kBlockWords)
        return hipErrorInvalidValue;
    const uint32_t lim = range < kLp ? range : kLp;
    uint32_t pair_bits = 2u * ((lim + 1u) / 2u);           // Booleans of the pairs inside the range ...
    if (pair_bits > kLp) pair_bits = kLp;                  // ... that exist
    uint32_t grid;
    if (!grid_of((uint64_t)n_queries * kBlockWords, grid)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(build_plane_queries_kernel, dim3(grid), dim3(kQbThreads), 0, stream, d_rows, (uint64_t)n_queries, n_sub,
                       pair_bits, d_blocks);
    return hipGetLastError();
}

hipError_t launch_build_sliding_queries(const uint32_t* d_rows, uint32_t n_queries, uint32_t per, uint32_t subfp_len, uint32_t range,
                                        uint32_t* d_blocks, hipStream_t stream) {
    if (!sliding_supported(subfp_len) || per == 0) return hipErrorInvalidValue;
    uint32_t grid;
    if (!grid_of((uint64_t)n_queries * ((uint64_t)per + 1u), grid)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(build_sliding_queries_kernel, dim3(grid), dim3(kQbThreads), 0, stream, d_rows, (uint64_t)n_queries, per,
                       subfp_len, sliding_range_mask(subfp_len, range), reinterpret_cast<uint4*>(d_blocks));
    return hipGetLastError();
}

hipError_t launch_build_query_rows(const uint32_t* d_rows, uint32_t n_queries, uint32_t per, uint32_t subfp_len, bool pairs,
                                   uint32_t* d_words, uint2* d_desc, hipStream_t stream) {
    const uint64_t n_rows = (uint64_t)n_queries * per;
    if (subfp_len == 0 || subfp_len > 32u * kPackedWords || n_rows > 0xFFFFFFFFull) return hipErrorInvalidValue;   // (the table counts in 32 bits)
    uint32_t grid;
    if (!grid_of(n_rows, grid)) return hipErrorInvalidValue;
    if (pairs)
        hipLaunchKernelGGL(build_query_rows_kernel<true>, dim3(grid), dim3(kQbThreads), 0, stream, d_rows, n_rows, subfp_len,
                           reinterpret_cast<uint4*>(d_words), d_desc, n_queries, per);
    else
        hipLaunchKernelGGL(build_query_rows_kernel<false>, dim3(grid), dim3(kQbThreads), 0, stream, d_rows, n_rows, subfp_len,
                           reinterpret_cast<uint4*>(d_words), d_desc, n_queries, per);
    return hipGetLastError();
}

}  // namespace lbad
