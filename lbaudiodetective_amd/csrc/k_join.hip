// k_join.hip -- corpus join: every ordered pair (row i of a uniform corpus, entry j of a uniform corpus of the same shape) whose
// score reaches a threshold, as CSR on the device.  Row i is entry i of the `queries` corpus used as the QUERY of the compare;
// its score against entry j is what the specialised uniform scan writes for that query (k_compare.hip: the batch scan's
// arithmetic, verbatim -- two three-input operations and a count per span word, hits / possible as two multiply-adds on
// (rh, rl), the sum in sub-fingerprint order, / NSUB, max(0, .)).  score(i -> j) != score(j -> i) in general: the query
// supplies the non-zero pairs.
//
// A chunk of rows (as many as the scratch holds) takes five launches and a workgroup never waits for another one:
//
//   build     the rows' query blocks (build_plane_query's layout, kJoinBlockWords words each) straight from the planes of
//             `queries`: the stream words are the plane words, the masks and counts follow from them; rh and rl by the three
//             correctly rounded expressions of k_query.hip
//   count     one workgroup per (tile of kJoinTileRows rows, tile of kJoinTileEntries entries): a lane owns ONE entry, its plane
//             words and their >> 1 stay in registers for the whole tile of rows; the row's words, masks and (rh, rl) are
//             wave-uniform (scalar loads).  Per row a ballot and a count per wave, the waves' sums through LDS, one word per
//             (row, entry tile) and one word per work item ("any match at all").  No atomics.
//   row scan  one workgroup per row: exclusive scan of the row's tile counts (32 bits: a row has < 2^32 matches), the row's
//             total as 64 bits
//   offsets   ONE workgroup: exclusive scan of the rows' totals on top of the total carried from the chunk before (device
//             memory): the CSR offsets of the chunk's rows, the running total behind them, the rows' bases for the scatter
//   scatter   the count kernel's work items: an item without a match returns after reading its one word, BEFORE it loads a
//             plane; otherwise the rows with a match in this entry tile are computed again (the same function: the same bits)
//             and a match's key goes to slot base + tile offset + rank where that is below the capacity; the rank inside a
//             wave is mbcnt under the ballot, the waves in front through LDS.  Plain vector stores.
//
// (The scan is two launches, not one: a single workgroup walking rows x tiles counts would move 12 bytes per count through one
// CU -- 10^9 counts in a self-join of a million entries.  Per row the tiles are scanned in parallel; the serial part is one
// word per row.)  The key slots are zeroed by the caller's hipMemsetAsync in front of the first chunk.
#include "internal.hpp"

namespace lbad {
namespace {

constexpr uint32_t kJoinTileEntries = 256;   // entries per work item = lanes of a workgroup
constexpr uint32_t kJoinTileRows = 64;       // rows an entry's words stay in registers for
constexpr uint32_t kJoinThreads = kJoinTileEntries;
constexpr uint32_t kJoinWaves = kJoinThreads / 64;
constexpr uint32_t kJoinMaxGrid = 1u << 20;  // work items beyond this many workgroups are walked with a grid stride
constexpr uint32_t kJoinScanThreads = 256;
constexpr uint32_t kJoinScanWaves = kJoinScanThreads / 64;
constexpr uint32_t kJoinScanPer = 4;         // counts per thread and step of the scans
constexpr uint32_t kJoinScanChunk = kJoinScanThreads * kJoinScanPer;
constexpr uint32_t kJoinScanMaxGrid = 4096;
static_assert(kJoinTileRows <= 64, "one wave writes a work item's row counts");

// the specialised uniform scan's shape and block (k_compare.hip: PlaneShape, kPlaneQueryWords); the launcher checks the size
constexpr uint32_t kLp = 200;
constexpr uint32_t kSubSpan = 7;
constexpr uint32_t kJoinBlockWords = 144;

template <int NSUB>
struct JoinShape {
    static constexpr uint32_t planes = (NSUB * kLp + 127) / 128;
    static constexpr uint32_t words = planes * 4;
    static constexpr uint32_t off_mask = words;
    static constexpr uint32_t off_possible = off_mask + NSUB * kSubSpan;
    static constexpr uint32_t off_rh = off_possible + NSUB;
    static constexpr uint32_t off_rl = off_rh + NSUB;
    static_assert(off_rl + NSUB <= kJoinBlockWords, "the block holds the shape");
};

// ---- the rows' query blocks from the planes of `queries` -- one lane per output word -------------------------------------------
// bits of stream word w (stream positions 32 w .. 32 w + 31) that lie in [lo, hi)
__device__ __forceinline__ uint32_t span_bits(uint32_t w, uint32_t lo, uint32_t hi) {
    const uint32_t base = 32u * w;
    const uint32_t below_hi = hi <= base ? 0u : (hi - base >= 32u ? 0xFFFFFFFFu : ((1u << (hi - base)) - 1u));
    const uint32_t below_lo = lo <= base ? 0u : (lo - base >= 32u ? 0xFFFFFFFFu : ((1u << (lo - base)) - 1u));
    return below_hi & ~below_lo;
}

// pairs of a word with at least one Boolean set, at the even places (sub-fingerprints start at even stream positions)
__device__ __forceinline__ uint32_t live_pairs(uint32_t x) { return (x | (x >> 1)) & 0x55555555u; }

__device__ __forceinline__ uint32_t plane_word(const uint32_t* __restrict__ planes32, uint64_t stride, uint64_t e, uint32_t w) {
    return planes32[((uint64_t)(w >> 2) * stride + e) * 4u + (w & 3u)];
}

__global__ __launch_bounds__(256) void join_build_rows_kernel(const uint32_t* __restrict__ qplanes32, uint64_t qstride,
                                                              uint64_t first_row, uint32_t rows, uint32_t n_sub, uint32_t pair_bits,
                                                              uint32_t* __restrict__ blocks) {
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (t >= (uint64_t)rows * kJoinBlockWords) return;
    const uint64_t r = t / kJoinBlockWords;
    const uint32_t w = (uint32_t)(t - r * kJoinBlockWords);
    const uint64_t e = first_row + r;
    const uint32_t words = ((n_sub * kLp + 127u) / 128u) * 4u;
    const uint32_t off_possible = words + n_sub * kSubSpan;
    uint32_t v = 0u;
    if (w < words) {
        v = plane_word(qplanes32, qstride, e, w);                 // the tight bitstream is the plane layout's own
    } else if (w < off_possible) {
        const uint32_t m = w - words;
        const uint32_t s = m / kSubSpan, j = m - s * kSubSpan;
        const uint32_t sw = ((s * kLp) >> 5) + j;                 // (< words: a sub-fingerprint's span ends inside the stream)
        v = live_pairs(plane_word(qplanes32, qstride, e, sw) & span_bits(sw, s * kLp, s * kLp + pair_bits));
    } else if (w < off_possible + 3u * n_sub) {
        const uint32_t m = w - off_possible;
        const uint32_t kind = m / n_sub, s = m - kind * n_sub;
        const uint32_t w0 = (s * kLp) >> 5;
        uint32_t possible = 0u;
#pragma unroll
        for (uint32_t j = 0; j < kSubSpan; ++j)
            possible += __popc(live_pairs(plane_word(qplanes32, qstride, e, w0 + j) & span_bits(w0 + j, s * kLp, s * kLp + pair_bits)));
        // build_plane_query's own three expressions, correctly rounded: the quotient relies on these bits
        const float pf = (float)possible;
        const float rh = possible ? __fdiv_rn(1.0f, pf) : 0.0f;
        const float rl = __fmul_rn(__fmaf_rn(-pf, rh, possible ? 1.0f : 0.0f), rh);
        v = __float_as_uint(kind == 0u ? pf : (kind == 1u ? rh : rl));
    }
    blocks[t] = v;
}

// ---- the pair loop ---------------------------------------------------------------------------------------------------------
template <int NSUB>
struct JoinEntry {
    uint32_t b[JoinShape<NSUB>::words], b1[JoinShape<NSUB>::words];
};

template <int NSUB>
__device__ __forceinline__ void join_load(const uint4* __restrict__ planes, uint64_t stride, uint64_t e, bool valid, JoinEntry<NSUB>& x) {
    using S = JoinShape<NSUB>;
    const uint4* __restrict__ at = planes + e;         // (a running address: no table of plane offsets in scalar registers)
#pragma unroll
    for (uint32_t p = 0; p < S::planes; ++p, at += stride) {
        const uint4 v = valid ? *at : make_uint4(0u, 0u, 0u, 0u);
        x.b[4 * p + 0] = v.x; x.b[4 * p + 1] = v.y; x.b[4 * p + 2] = v.z; x.b[4 * p + 3] = v.w;
    }
#pragma unroll
    for (uint32_t w = 0; w < S::words; ++w) x.b1[w] = x.b[w] >> 1;       // (pairs never straddle a word)
}

// the batch scan's score of the entry in x against the row whose block is qc (wave-uniform address)
//
// A row's block is up to 124 scalars and the scheduler would fetch all of them in front of the first vector instruction: more
// than the scalar file holds next to the kernel's own state.  So each sub-fingerprint reads at qc + a zero of its own that
// exists only once the sum of the sub-fingerprint TWO before it does (an empty statement, no instruction): the words of at most
// two sub-fingerprints -- the one being computed and the one being fetched -- are in scalar registers at a time.
template <int NSUB>
__device__ __forceinline__ float join_score(const JoinEntry<NSUB>& x, const uint32_t* __restrict__ qc) {
    using S = JoinShape<NSUB>;
    float sum = 0.0f;
    uint32_t zs = 0u, zn = 0u;                         // sub-fingerprint s reads at qc + zs, s + 1 at qc + zn
    asm("" : "+s"(zs));
    asm("" : "+s"(zn));
#pragma unroll
    for (uint32_t s = 0; s < (uint32_t)NSUB; ++s) {
        const uint32_t w0 = (s * kLp) >> 5;
        const uint32_t* __restrict__ qs = qc + zs;
        uint32_t h = 0x4B000000u;                      // hits counted on top of the bits of 2^23
#pragma unroll
        for (uint32_t j = 0; j < kSubSpan; ++j) {
            if (w0 + j < S::words) {
                const uint32_t qw = qs[w0 + j];
                const uint32_t u = __builtin_amdgcn_bitop3_b32(qs[S::off_mask + s * kSubSpan + j], x.b[w0 + j], qw, 0x90);   // a & ~(b ^ c)
                const uint32_t t = __builtin_amdgcn_bitop3_b32(u, x.b1[w0 + j], qw >> 1, 0x90);
                h += __popc(t);
            }
        }
        const float hf = __fsub_rn(__uint_as_float(h), 8388608.0f);
        const float rh = __uint_as_float(qs[S::off_rh + s]), rl = __uint_as_float(qs[S::off_rl + s]);
        uint32_t znn = 0u;
        asm("" : "+s"(znn) : "v"(sum));                // (sum: the sub-fingerprints before s)
        sum = __fadd_rn(sum, __fmaf_rn(hf, rh, __fmul_rn(hf, rl)));      // == hits / possible, 0 where nothing is possible
        zs = zn;
        zn = znn;
    }
    const float cand = __fdiv_rn(sum, (float)NSUB);
    return (0.0f < cand) ? cand : 0.0f;
}

// what the count and the scatter kernel share: the chunk's rows against the corpus
struct JoinPairs {
    const uint4* planes;          // the scanned corpus
    uint64_t stride, n_entries, etiles;
    const uint32_t* blocks;       // the chunk's row blocks
    uint32_t rows;                // rows of the chunk
    uint32_t skip;                // leave out the pair whose row index equals the entry's index
    uint64_t first_row;           // index of the chunk's first row in its own corpus
    float t;
};

// a lane's threshold: the call's, or one that nothing reaches where the lane has no entry
__device__ __forceinline__ float join_lane_threshold(const JoinPairs& a, bool valid) { return valid ? a.t : __builtin_inff(); }

// the row of the tile (0 .. kJoinTileRows - 1) whose index in its own corpus is entry e's index, where that pair is left out
__device__ __forceinline__ uint32_t join_self_row(const JoinPairs& a, uint64_t e, uint32_t row0) {
    const uint64_t d = e - (a.first_row + row0);           // (wraps to a huge value for rows behind the entry)
    return a.skip && d < kJoinTileRows ? (uint32_t)d : 0xFFFFFFFFu;
}

template <int NSUB>
__global__ __launch_bounds__(kJoinThreads) void join_count_kernel(const JoinPairs a, uint32_t* __restrict__ counts,
                                                                  uint32_t* __restrict__ any) {
    __shared__ uint32_t s_cnt[kJoinTileRows][kJoinWaves];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t rtiles = (a.rows + kJoinTileRows - 1) / kJoinTileRows;
    const uint64_t items = rtiles * a.etiles;
    for (uint64_t w = blockIdx.x; w < items; w += gridDim.x) {
        const uint64_t rt = w / a.etiles, et = w - rt * a.etiles;
        const uint64_t e = et * kJoinTileEntries + threadIdx.x;
        const bool valid = e < a.n_entries;
        JoinEntry<NSUB> x;
        join_load<NSUB>(a.planes, a.stride, e, valid, x);
        const uint32_t row0 = (uint32_t)rt * kJoinTileRows;
        const uint32_t nr = a.rows - row0 < kJoinTileRows ? a.rows - row0 : kJoinTileRows;
        const float t = join_lane_threshold(a, valid);
        const uint32_t self = join_self_row(a, e, row0);
        const uint32_t* __restrict__ qc = a.blocks + (size_t)row0 * kJoinBlockWords;
        for (uint32_t r = 0; r < nr; ++r, qc += kJoinBlockWords) {
            const float score = join_score<NSUB>(x, qc);
            const bool m = score >= t && r != self;
            const uint32_t c = (uint32_t)__popcll(__ballot(m));
            if (lane == 0) s_cnt[r][wave] = c;
        }
        __syncthreads();
        if (wave == 0) {
            uint32_t total = 0;
            if (lane < nr) {
#pragma unroll
                for (uint32_t i = 0; i < kJoinWaves; ++i) total += s_cnt[lane][i];
                counts[(uint64_t)(row0 + lane) * a.etiles + et] = total;
            }
            const unsigned long long some = __ballot(total != 0u);
            if (lane == 0) any[w] = some ? 1u : 0u;
        }
        __syncthreads();                       // (s_cnt is the next item's)
    }
}

template <int NSUB>
__global__ __launch_bounds__(kJoinThreads) void join_scatter_kernel(const JoinPairs a, const uint32_t* __restrict__ counts,
                                                                    const uint32_t* __restrict__ any,
                                                                    const uint32_t* __restrict__ tile_at,
                                                                    const unsigned long long* __restrict__ row_base,
                                                                    uint64_t capacity, uint64_t index_base,
                                                                    unsigned long long* __restrict__ keys) {
    __shared__ uint32_t s_w[kJoinWaves];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t rtiles = (a.rows + kJoinTileRows - 1) / kJoinTileRows;
    const uint64_t items = rtiles * a.etiles;
    for (uint64_t w = blockIdx.x; w < items; w += gridDim.x) {
        if (any[w] == 0u) continue;                                 // (the same word for the whole workgroup) nothing is loaded
        const uint64_t rt = w / a.etiles, et = w - rt * a.etiles;
        const uint32_t row0 = (uint32_t)rt * kJoinTileRows;
        const uint32_t nr = a.rows - row0 < kJoinTileRows ? a.rows - row0 : kJoinTileRows;
        if (row_base[row0] >= capacity) continue;                   // the list is full in front of this tile of rows
        const uint64_t e = et * kJoinTileEntries + threadIdx.x;
        const bool valid = e < a.n_entries;
        JoinEntry<NSUB> x;
        join_load<NSUB>(a.planes, a.stride, e, valid, x);
        const float t = join_lane_threshold(a, valid);
        const uint32_t self = join_self_row(a, e, row0);
        const uint32_t* __restrict__ qc = a.blocks + (size_t)row0 * kJoinBlockWords;
        uint64_t at_word = (uint64_t)row0 * a.etiles + et;
        for (uint32_t r = 0; r < nr; ++r, qc += kJoinBlockWords, at_word += a.etiles) {
            if (__builtin_amdgcn_readfirstlane(counts[at_word]) == 0u) continue;      // (uniform: one word per workgroup)
            const unsigned long long at = row_base[row0 + r] + tile_at[at_word];
            if (at >= capacity) continue;
            const float score = join_score<NSUB>(x, qc);
            const bool m = score >= t && r != self;
            const unsigned long long b = __ballot(m);
            const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
            if (lane == 0) s_w[wave] = (uint32_t)__popcll(b);
            __syncthreads();
            uint32_t before = 0;
#pragma unroll
            for (uint32_t i = 0; i < kJoinWaves; ++i) before += i < wave ? s_w[i] : 0u;
            const unsigned long long slot = at + before + below;
            if (m && slot < capacity)
                keys[slot] = ((unsigned long long)__float_as_uint(score) << 32) |
                             (unsigned long long)(0xFFFFFFFFu - (uint32_t)(index_base + e));
            __syncthreads();                   // (s_w is the next row's)
        }
    }
}

// ---- count -> offsets --------------------------------------------------------------------------------------------------------
// one workgroup per row: the row's tile counts to exclusive offsets inside the row, the row's total to row_total[row]
__global__ __launch_bounds__(kJoinScanThreads) void join_row_scan_kernel(const uint32_t* __restrict__ counts, uint64_t etiles,
                                                                         uint32_t rows, uint32_t* __restrict__ tile_at,
                                                                         unsigned long long* __restrict__ row_total) {
    __shared__ uint32_t wsum[kJoinScanWaves];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t row = blockIdx.x; row < rows; row += gridDim.x) {
        const uint32_t* cnt = counts + (size_t)row * etiles;
        uint32_t* off = tile_at + (size_t)row * etiles;
        uint32_t carry = 0u;                       // (a row has at most n_entries < 2^32 matches)
        for (uint64_t c0 = 0; c0 < etiles; c0 += kJoinScanChunk) {
            const uint64_t first = c0 + (uint64_t)threadIdx.x * kJoinScanPer;
            uint32_t c[kJoinScanPer], sum = 0;
#pragma unroll
            for (uint32_t j = 0; j < kJoinScanPer; ++j) {
                c[j] = first + j < etiles ? cnt[first + j] : 0u;
                sum += c[j];
            }
            uint32_t incl = sum;
#pragma unroll
            for (uint32_t d = 1; d < 64; d <<= 1) {
                const uint32_t up = __shfl_up(incl, d, 64);
                if (lane >= d) incl += up;
            }
            if (lane == 63) wsum[wave] = incl;
            __syncthreads();
            uint32_t before = 0, chunk = 0;
#pragma unroll
            for (uint32_t i = 0; i < kJoinScanWaves; ++i) {
                before += i < wave ? wsum[i] : 0u;
                chunk += wsum[i];
            }
            uint32_t at = carry + before + (incl - sum);
#pragma unroll
            for (uint32_t j = 0; j < kJoinScanPer; ++j) {
                if (first + j < etiles) off[first + j] = at;
                at += c[j];
            }
            carry += chunk;
            __syncthreads();                       // (wsum is the next step's)
        }
        if (threadIdx.x == 0) row_total[row] = carry;
    }
}

// ONE workgroup: the rows' totals (row_base on entry) to the rows' first slots (row_base on return, and the caller's CSR
// offsets), on top of the total of the chunks before; the running total to *state and behind the chunk's offsets
__global__ __launch_bounds__(kJoinScanThreads) void join_offsets_kernel(unsigned long long* __restrict__ row_base, uint32_t rows,
                                                                        unsigned long long* __restrict__ state, uint32_t first_chunk,
                                                                        unsigned long long* __restrict__ out_offsets) {
    __shared__ unsigned long long wsum[kJoinScanWaves];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    unsigned long long carry = first_chunk ? 0ull : *state;
    for (uint32_t c0 = 0; c0 < rows; c0 += kJoinScanChunk) {
        const uint32_t first = c0 + threadIdx.x * kJoinScanPer;
        unsigned long long c[kJoinScanPer], sum = 0ull;
#pragma unroll
        for (uint32_t j = 0; j < kJoinScanPer; ++j) {
            c[j] = first + j < rows ? row_base[first + j] : 0ull;
            sum += c[j];
        }
        unsigned long long incl = sum;
#pragma unroll
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const unsigned long long up = __shfl_up(incl, d, 64);
            if (lane >= d) incl += up;
        }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        unsigned long long before = 0ull, chunk = 0ull;
#pragma unroll
        for (uint32_t i = 0; i < kJoinScanWaves; ++i) {
            before += i < wave ? wsum[i] : 0ull;
            chunk += wsum[i];
        }
        unsigned long long at = carry + before + (incl - sum);
#pragma unroll
        for (uint32_t j = 0; j < kJoinScanPer; ++j) {
            if (first + j < rows) {
                row_base[first + j] = at;
                out_offsets[first + j] = at;
            }
            at += c[j];
        }
        carry += chunk;
        __syncthreads();                           // (wsum is the next step's; every thread has read *state by now)
    }
    if (threadIdx.x == 0) {
        *state = carry;
        out_offsets[rows] = carry;                 // the total so far: the next chunk's first offset, or the call's total
    }
}

// the scratch of a chunk of `rows` rows, in this order (every block 8-byte aligned)
struct JoinScratch {
    unsigned long long* state;       // 2 words: the total carried from chunk to chunk
    unsigned long long* row_base;    // rows
    uint32_t* blocks;                // rows x kJoinBlockWords
    uint32_t* counts;                // rows x etiles
    uint32_t* tile_at;               // rows x etiles
    uint32_t* any;                   // row tiles x etiles
};

uint64_t join_etiles(uint64_t n_entries) { return (n_entries + kJoinTileEntries - 1) / kJoinTileEntries; }

JoinScratch join_carve(void* d_scratch, uint64_t n_entries, uint32_t rows) {
    const uint64_t etiles = join_etiles(n_entries);
    JoinScratch s;
    s.state = static_cast<unsigned long long*>(d_scratch);
    s.row_base = s.state + 2;
    s.blocks = reinterpret_cast<uint32_t*>(s.row_base + rows);
    s.counts = s.blocks + (size_t)rows * kJoinBlockWords;
    s.tile_at = s.counts + (size_t)rows * etiles;
    s.any = s.tile_at + (size_t)rows * etiles;
    return s;
}

}  // namespace

// count -> offsets: the row scan and the offsets kernel, for this file's join and for k_join_ragged.hip's (the same counts layout)
void launch_join_scans(const uint32_t* counts, uint64_t etiles, uint32_t rows, uint32_t* tile_at, unsigned long long* row_base,
                       unsigned long long* state, uint32_t first_chunk, unsigned long long* out_offsets, hipStream_t stream) {
    hipLaunchKernelGGL(join_row_scan_kernel, dim3(strided_grid(rows, kJoinScanMaxGrid)), dim3(kJoinScanThreads), 0, stream,
                       counts, etiles, rows, tile_at, row_base);
    hipLaunchKernelGGL(join_offsets_kernel, dim3(1), dim3(kJoinScanThreads), 0, stream, row_base, rows, state, first_chunk, out_offsets);
}

namespace {

template <int NSUB>
hipError_t launch_join_n(const JoinCall& c, const JoinScratch& s, const JoinPairs& a, uint64_t items, uint32_t first_chunk,
                         unsigned long long* out_offsets) {
    const dim3 grid(strided_grid(items, kJoinMaxGrid));
    hipLaunchKernelGGL(join_count_kernel<NSUB>, grid, dim3(kJoinThreads), 0, c.stream, a, s.counts, s.any);
    launch_join_scans(s.counts, a.etiles, a.rows, s.tile_at, s.row_base, s.state, first_chunk, out_offsets, c.stream);
    hipLaunchKernelGGL(join_scatter_kernel<NSUB>, grid, dim3(kJoinThreads), 0, c.stream, a, s.counts, s.any, s.tile_at, s.row_base,
                       c.capacity, c.index_base, c.d_keys);
    return hipGetLastError();
}

}  // namespace

size_t join_scratch_bytes(uint64_t n_entries, uint64_t rows) {
    const uint64_t etiles = join_etiles(n_entries);
    const uint64_t rtiles = (rows + kJoinTileRows - 1) / kJoinTileRows;
    return (size_t)(16u + rows * (8u + 4u * kJoinBlockWords + 8u * etiles) + rtiles * etiles * 4u);
}

// rows of a chunk under a scratch limit: the largest whole number of row tiles that fits (0: not even one), at most 2^24
uint64_t join_chunk_rows(uint64_t n_entries, uint64_t limit_bytes) {
    const uint64_t etiles = join_etiles(n_entries);
    const uint64_t per_tile = kJoinTileRows * (8u + 4u * (uint64_t)kJoinBlockWords + 8u * etiles) + etiles * 4u;
    if (limit_bytes < 16u + per_tile) return 0;
    const uint64_t tiles = (limit_bytes - 16u) / per_tile;
    const uint64_t most = (1ull << 24) / kJoinTileRows;
    return (tiles < most ? tiles : most) * kJoinTileRows;
}

hipError_t launch_join_chunk(const JoinCall& c, void* d_scratch, uint32_t chunk_rows_max, uint64_t first_row, uint32_t rows,
                             uint32_t first_chunk, unsigned long long* out_offsets) {
    if (rows == 0 || c.n_entries == 0) return hipSuccess;
    // (the caller has checked the call; what is checked here ties this file to k_compare.hip's block and to the carved scratch)
    if (plane_query_words() != kJoinBlockWords || rows > chunk_rows_max) return hipErrorInvalidValue;
    const JoinScratch s = join_carve(d_scratch, c.n_entries, chunk_rows_max);
    const uint32_t lim = c.range < kLp ? c.range : kLp;
    uint32_t pair_bits = 2u * ((lim + 1u) / 2u);           // Booleans of the pairs inside the range ...
    if (pair_bits > kLp) pair_bits = kLp;                  // ... that exist
    const uint64_t lanes = (uint64_t)rows * kJoinBlockWords;
    hipLaunchKernelGGL(join_build_rows_kernel, dim3((uint32_t)((lanes + 255u) / 256u)), dim3(256), 0, c.stream,
                       reinterpret_cast<const uint32_t*>(c.d_qplanes), c.qstride, first_row, rows, c.n_sub, pair_bits, s.blocks);
    JoinPairs a;
    a.planes = c.d_planes; a.stride = c.stride; a.n_entries = c.n_entries; a.etiles = join_etiles(c.n_entries);
    a.blocks = s.blocks; a.rows = rows; a.skip = c.skip ? 1u : 0u; a.first_row = first_row; a.t = c.threshold;
    const uint64_t items = (uint64_t)((rows + kJoinTileRows - 1) / kJoinTileRows) * a.etiles;
    switch (c.n_sub) {
        case 1: return launch_join_n<1>(c, s, a, items, first_chunk, out_offsets);
        case 2: return launch_join_n<2>(c, s, a, items, first_chunk, out_offsets);
        case 3: return launch_join_n<3>(c, s, a, items, first_chunk, out_offsets);
        case 4: return launch_join_n<4>(c, s, a, items, first_chunk, out_offsets);
        case 5: return launch_join_n<5>(c, s, a, items, first_chunk, out_offsets);
        case 6: return launch_join_n<6>(c, s, a, items, first_chunk, out_offsets);
        case 7: return launch_join_n<7>(c, s, a, items, first_chunk, out_offsets);
        case 8: return launch_join_n<8>(c, s, a, items, first_chunk, out_offsets);
        default: return hipErrorNotSupported;
    }
}

}  // namespace lbad
