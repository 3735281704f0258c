// k_join_ragged.hip -- the corpus join of two RAGGED corpora: every ordered pair (row i of `queries`, entry j of the scanned
// corpus) whose score reaches a threshold, as CSR on the device, with each match's signed lag.  The score is the ragged scan's
// (k_align.hip:1-14 states it): fingerprint1 is the entry when n_i < n_j ("A"), the row otherwise ("B", equal lengths included);
// with n1 >= n2
//   q_o   = fl(fl(sum over s = 0 .. n2 - 1, in that order, of ratio(fp1[s + o], fp2[s])) / n2),   o = 0 .. n1 - n2
//   score = max(0, max_o q_o),  lag = +o in A, -o in B for the LOWEST o with q_o == score
// ratio = hits / possible correctly rounded (the table of sliding.cpp), possible = fingerprint1's non-zero pairs inside the range,
// hits = those on which both Booleans of both sides agree.  Both sides are RECORDS here (sliding_common.hpp): words 3 and 7
// carry derived fields above bit 3, so the non-zero pairs are never taken over raw words: under the pair mask where the range
// is shorter than the length, and where it covers the length (the FULL instances) under the mask of word 3's four pair bits
// alone -- words 0 .. 2 then need none, because the record builders (k_records.hip: pack_records_kernel, and the loader's
// restamp_records_kernel) leave every pair at or beyond ceil(length / 2) zero in P and in N; the table row in word 3 is counted
// over the raw words on that same invariant.  That table row (possible over the full range of that record) is used only for
// fingerprint1 and only when the range covers the length.
//
// The structure is k_join.hip's: count per (row, entry tile) -> the two scans (k_join.hip's own kernels, the counts have the same
// layout) -> a scatter that computes again only the rows that have a match in a tile, from which the lags fall out.  No
// workgroup waits for another and no result depends on which lane or workgroup finishes first.
//
// The pair loop.  A work item is (tile of kJoinRaggedTileRows rows, tile of kJoinRaggedTileEntries entries); its rows are
// taken one after the other, and one row against the tile's entries is |n_i - n_j| + 1 sliding offsets per entry, each of
// min(n_i, n_j) steps.  A lane owns TWO neighbouring offsets of one pair: fingerprint1's record of a step is the record the
// lane's other offset read one step earlier, so a step loads ONE record of fingerprint1 for two compares.  The pairs' units
// (ceil(offsets / 2)) are laid out by a prefix sum over the tile's entries, the A pairs first (padded to a whole wave), then
// the B pairs; a lane finds its pair by bisection in LDS.
//   A  the row is fingerprint2: its record of a step is the same for the whole wave (scalar loads), and so is the step count,
//      n_i: no divergence at all.  fingerprint1 is the entry: neighbouring lanes read neighbouring records.
//   B  the row is fingerprint1: it lies in LDS (one row, the cap's 1024 records at most, plus a zero record the odd unit's
//      second offset reads) and is indexed per lane; the entry's record of a step comes from memory.  A wave runs as many
//      steps as its longest entry.
// A lane's best (q_o bits << 32 | 0xFFFFFFFF - o) of its two offsets meets the pair's others in an LDS max: order-free, the
// lowest offset wins a tie.  The compare with the threshold is on the quotient.  Nothing is read beyond an entry's records
// plus one (inside the corpus' kRecordSlack); every loop is bounded by lengths from the record positions and by the cap.
#include "sliding_common.hpp"

namespace lbad {
namespace {

constexpr uint32_t kJoinRaggedTileEntries = 256;   // entries per work item = lanes of a workgroup
constexpr uint32_t kJoinRaggedTileRows = 64;       // rows per work item
constexpr uint32_t kJrThreads = kJoinRaggedTileEntries;
constexpr uint32_t kJrWaves = kJrThreads / 64;
constexpr uint32_t kJrMaxGrid = 1u << 20;          // work items beyond this many workgroups are walked with a grid stride
constexpr uint64_t kJrMaxWords = 0xFFFFFFFFull - kJrMaxGrid;   // rows x entry tiles of a chunk: 32-bit indices, strides included
constexpr uint32_t kJrCap = LBAD_JOIN_RAGGED_MAX_SUBFINGERPRINTS;
constexpr uint32_t kJrTriLast = kTriPairs * (kTriPairs + 1) / 2;   // the table's last row
static_assert(kJoinRaggedTileRows <= 64, "one wave writes a work item's row counts");
static_assert(kJrCap >= 1024 && (uint64_t)(kJrCap / 2 + 1) * kJoinRaggedTileEntries < (1ull << 32), "a tile's units fit 32 bits");
static_assert((kJrCap + 1) * 32u + 30u * 1024u <= 64u * 1024u, "one row and the tile's state fit the LDS of a workgroup");

struct JrArgs {
    const uint4* recs;            // the scanned corpus
    const uint32_t* off;
    uint32_t n_entries, etiles;   // (a ragged corpus has fewer than 2^32 entries; a chunk has fewer than 2^32 rows x entry tiles)
    const uint4* qrecs;           // the rows' corpus
    const uint32_t* qoff;
    uint32_t first_row;           // index of the chunk's first row in its own corpus
    uint32_t rows;                // rows of the chunk
    uint32_t skip;                // leave out the pair whose row index equals the entry's index
    uint32_t row_cap;             // longest row: the LDS row holds row_cap + 1 records
    uint32_t m[4];                // the pair mask of the range
    const float* tri;
    float t;
};

// the row's records as the scalar unit reads them: wave-uniform addresses in memory no kernel of the call writes
typedef const u32x4 __attribute__((address_space(4))) * JrUniformRecs;
__device__ __forceinline__ uint4 jr_uniform(JrUniformRecs p, uint32_t i) {
    const u32x4 v = p[i];
    return make_uint4(v.x, v.y, v.z, v.w);
}

// a workgroup's state in LDS (the row's records are the dynamic part)
struct JrTile {
    float tri[kTriSize];
    unsigned long long best[kJoinRaggedTileEntries];       // per entry: the row's best (q_o, offset) so far
    uint32_t start[2][kJoinRaggedTileEntries + 1];         // first unit of an entry's A / B pair; [tile entries] = the total
    uint32_t rec0[kJoinRaggedTileEntries], ne[kJoinRaggedTileEntries];     // the tile's entries (ne 0: no entry)
    unsigned long long wsum[kJrWaves];
};

// hits / possible of one step: (p1, n1) fingerprint1's record, (p2, n2) fingerprint2's
template <bool FULL>
__device__ __forceinline__ float jr_ratio(const float* tri, const uint4& p1, const uint4& n1, const uint4& p2, const uint4& n2,
                                          const uint32_t (&m)[4]) {
    const uint32_t a[4] = {p1.x, p1.y, p1.z, p1.w}, b[4] = {n1.x, n1.y, n1.z, n1.w};
    const uint32_t c[4] = {p2.x, p2.y, p2.z, p2.w}, d[4] = {n2.x, n2.y, n2.z, n2.w};
    uint32_t hits = 0u, possible = 0u;
#pragma unroll
    for (uint32_t w = 0; w < 4; ++w) {
        uint32_t u;
        if (FULL) {
            // every pair of the record is inside the range and the builders leave the pairs beyond the length zero (see the
            // head of the file): no mask but the one that keeps word 3's derived fields out
            u = __builtin_amdgcn_bitop3_b32(a[w], b[w], c[w], 0xA4);                       // (a | b) & ~(a ^ c)
            if (w == 3) u &= 0xFu;
        } else {
            const uint32_t nz = __builtin_amdgcn_bitop3_b32(a[w], b[w], m[w], 0xA8);       // (a | b) & c
            possible += __popc(nz);
            u = __builtin_amdgcn_bitop3_b32(nz, a[w], c[w], 0x90);                         // a & ~(b ^ c)
        }
        hits += __popc(__builtin_amdgcn_bitop3_b32(u, b[w], d[w], 0x90));
    }
    // FULL: the range covers the length, the record's own table row is possible's (bounded: whatever the word holds, the
    // read stays inside the table -- hits <= 100)
    uint32_t row = FULL ? (p1.w >> 4) & 0x1FFFu : (possible * (possible + 1u)) >> 1;
    if (FULL) row = row < kJrTriLast ? row : kJrTriLast;
    uint32_t at = row + hits;
    asm("" : "+v"(at));                                // (one index: the counts add up before the table's stride is applied)
    return tri[at];
}

__device__ __forceinline__ unsigned long long jr_key(float q, uint32_t o) {
    return ((unsigned long long)__float_as_uint(q) << 32) | (unsigned long long)(0xFFFFFFFFu - o);
}

// the last entry of the tile whose first unit is <= t (t below the total: an entry without units is never the answer)
__device__ __forceinline__ uint32_t jr_find(const uint32_t* start, uint32_t t) {
    uint32_t at = 0u;
#pragma unroll
    for (uint32_t step = kJoinRaggedTileEntries / 2; step; step >>= 1)
        if (start[at + step] <= t) at += step;
    return at;
}

// One row (records row_rec0 .. + n_r of the rows' corpus) against the tile's entries: thread x gets entry x's score and lag
// (0 / 0 without an entry).  Called by every thread of the workgroup; my_ne = s.ne[threadIdx.x].  SCALAR: the A pairs read the
// row's records through the scalar unit (the count kernel); otherwise from the LDS copy, one address per wave (the scatter
// kernel, which computes few rows again and has its scalar registers full of the lists' state).  The same arithmetic, the same bits.
template <bool FULL, bool SCALAR>
__device__ __forceinline__ void jr_row(const JrArgs& a, JrTile& s, uint4* s_row, uint32_t row_rec0, uint32_t n_r, uint32_t my_ne,
                                       float* score, int32_t* lag) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint4* __restrict__ rr = a.qrecs + 2u * (size_t)row_rec0;
    uint32_t m[4] = {a.m[0], a.m[1], a.m[2], a.m[3]};
    if (!SCALAR) {
#pragma unroll
        for (uint32_t w = 0; w < 4; ++w) asm("" : "+v"(m[w]));      // (the mask in vector registers)
    }
    // (the row before has left s_row, start and best: its last barrier stands in front of its result)
    for (uint32_t i = tid; i < 2u * (n_r + 1u); i += kJrThreads) s_row[i] = i < 2u * n_r ? rr[i] : make_uint4(0u, 0u, 0u, 0u);
    // units of this thread's pair, A in the low half and B in the high half of one word, and their prefix sums
    const bool is_a = my_ne > n_r;
    const uint32_t n_off = is_a ? my_ne - n_r + 1u : n_r - my_ne + 1u;
    const uint32_t units = my_ne ? (n_off + 1u) >> 1 : 0u;
    const unsigned long long mine = is_a ? (unsigned long long)units : (unsigned long long)units << 32;
    unsigned long long incl = mine;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const unsigned long long up = __shfl_up(incl, d, 64);
        if (lane >= d) incl += up;
    }
    if (lane == 63u) s.wsum[wave] = incl;
    s.best[tid] = 0ull;
    __syncthreads();
    unsigned long long before = 0ull, total = 0ull;
#pragma unroll
    for (uint32_t i = 0; i < kJrWaves; ++i) {
        before += i < wave ? s.wsum[i] : 0ull;
        total += s.wsum[i];
    }
    const unsigned long long excl = before + incl - mine;
    s.start[0][tid] = (uint32_t)excl;
    s.start[1][tid] = (uint32_t)(excl >> 32);
    if (tid == 0u) {
        s.start[0][kJoinRaggedTileEntries] = (uint32_t)total;
        s.start[1][kJoinRaggedTileEntries] = (uint32_t)(total >> 32);
    }
    __syncthreads();
    const uint32_t n_a = (uint32_t)total, n_b = (uint32_t)(total >> 32);
    const uint32_t a_end = (n_a + 63u) & ~63u;         // the B units start at a whole wave: a wave is all A or all B
    for (uint32_t t = tid; t < a_end + n_b; t += kJrThreads) {
        if (t < a_end) {
            if (t < n_a) {
                // A: the entry is fingerprint1, the row's record of a step is wave-uniform, n_r steps for every lane
                const uint32_t x = jr_find(s.start[0], t);
                const uint32_t o = 2u * (t - s.start[0][x]);
                const uint32_t offsets = s.ne[x] - n_r + 1u;
                const uint4* __restrict__ g = a.recs + 2u * ((size_t)s.rec0[x] + o);
                uint4 p = g[0], n = g[1];
                float s0 = 0.0f, s1 = 0.0f;
                const JrUniformRecs ru = (JrUniformRecs)(uintptr_t)rr;
                for (uint32_t i = 0; i < n_r; ++i) {
                    g += 2;
                    const uint4 cp = g[0], cn = g[1];          // (the last step: the record behind the entry, never scored)
                    uint4 rp, rn;
                    if (SCALAR) {
                        rp = jr_uniform(ru, 2u * i);
                        rn = jr_uniform(ru, 2u * i + 1u);
                    } else {
                        rp = s_row[2u * i];
                        rn = s_row[2u * i + 1u];
                    }
                    s0 = __fadd_rn(s0, jr_ratio<FULL>(s.tri, p, n, rp, rn, m));
                    s1 = __fadd_rn(s1, jr_ratio<FULL>(s.tri, cp, cn, rp, rn, m));
                    p = cp;
                    n = cn;
                }
                const float n2 = (float)n_r;
                const unsigned long long k0 = jr_key(__fdiv_rn(s0, n2), o);
                const unsigned long long k1 = o + 1u < offsets ? jr_key(__fdiv_rn(s1, n2), o + 1u) : 0ull;
                atomicMax(&s.best[x], k0 > k1 ? k0 : k1);
            }
        } else if (t - a_end < n_b) {
            // B: the row is fingerprint1, read from LDS at the lane's offsets; the entry's record of a step from memory
            const uint32_t tb = t - a_end;
            const uint32_t x = jr_find(s.start[1], tb);
            const uint32_t o = 2u * (tb - s.start[1][x]);
            const uint32_t n_e = s.ne[x];
            const uint32_t offsets = n_r - n_e + 1u;
            const uint4* __restrict__ g = a.recs + 2u * (size_t)s.rec0[x];
            const uint4* w = s_row + 2u * o;
            uint4 p = w[0], n = w[1];
            float s0 = 0.0f, s1 = 0.0f;
            for (uint32_t i = 0; i < n_e; ++i) {
                w += 2;
                const uint4 cp = w[0], cn = w[1];              // (the last step of the last unit: the zero record)
                const uint4 ep = g[2u * i], en = g[2u * i + 1u];
                s0 = __fadd_rn(s0, jr_ratio<FULL>(s.tri, p, n, ep, en, m));
                s1 = __fadd_rn(s1, jr_ratio<FULL>(s.tri, cp, cn, ep, en, m));
                p = cp;
                n = cn;
            }
            const float n2 = (float)n_e;
            const unsigned long long k0 = jr_key(__fdiv_rn(s0, n2), o);
            const unsigned long long k1 = o + 1u < offsets ? jr_key(__fdiv_rn(s1, n2), o + 1u) : 0ull;
            atomicMax(&s.best[x], k0 > k1 ? k0 : k1);
        }
    }
    __syncthreads();
    const unsigned long long best = s.best[tid];
    const uint32_t o = 0xFFFFFFFFu - (uint32_t)best;
    *score = my_ne ? __uint_as_float((uint32_t)(best >> 32)) : 0.0f;       // (a sum of quotients from +0: never below 0)
    *lag = my_ne ? (is_a ? (int32_t)o : -(int32_t)o) : 0;
}

// the table and the tile's entries into LDS; returns this thread's entry length (0: no entry)
__device__ __forceinline__ uint32_t jr_load_tile(const JrArgs& a, JrTile& s, uint32_t e) {
    uint32_t r0 = 0u, ne = 0u;
    if (e < a.n_entries) {
        r0 = a.off[e];
        ne = a.off[e + 1] - r0;
        ne = ne < kJrCap ? ne : kJrCap;
    }
    s.rec0[threadIdx.x] = r0;                          // (the item before has left them: jr_row's last barrier)
    s.ne[threadIdx.x] = ne;
    __syncthreads();
    return ne;
}

// the row of the tile whose index in its own corpus is entry e's index, where that pair is left out
__device__ __forceinline__ uint32_t jr_self_row(const JrArgs& a, uint32_t e, uint32_t row0) {
    const uint32_t d = e - (a.first_row + row0);           // (wraps to a huge value for rows behind the entry)
    return a.skip && d < kJoinRaggedTileRows ? d : 0xFFFFFFFFu;
}

// (records, length) of row r of the chunk, wave-uniform
__device__ __forceinline__ void jr_row_of(const JrArgs& a, uint32_t r, uint32_t* rec0, uint32_t* n_r) {
    const uint32_t at = __builtin_amdgcn_readfirstlane(a.qoff[a.first_row + r]);
    const uint32_t n = __builtin_amdgcn_readfirstlane(a.qoff[a.first_row + r + 1]) - at;
    *rec0 = at;
    *n_r = n < a.row_cap ? n : a.row_cap;
}

// Work item w = (entry tile w / row tiles, row tile w % row tiles): workgroups that run at the same time share their entry
// tile, whose records (256 entries x their lengths x 32 bytes, read again for every row) then stay in L2; with the row tile as
// the slow index every workgroup of a CU streamed a tile of its own from memory once per row.
template <bool FULL>
__global__ __launch_bounds__(kJrThreads) void join_ragged_count_kernel(const JrArgs a, uint32_t* __restrict__ counts,
                                                                       uint32_t* __restrict__ any) {
    extern __shared__ uint4 s_row[];
    __shared__ JrTile s;
    __shared__ uint32_t s_cnt[kJoinRaggedTileRows][kJrWaves];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t i = threadIdx.x; i < kTriSize; i += kJrThreads) s.tri[i] = a.tri[i];
    const uint32_t rtiles = (a.rows + kJoinRaggedTileRows - 1) / kJoinRaggedTileRows;
    const uint32_t items = rtiles * a.etiles;
    for (uint32_t w = blockIdx.x; w < items; w += gridDim.x) {
        const uint32_t et = w / rtiles, rt = w - et * rtiles;
        const uint32_t e = et * kJoinRaggedTileEntries + threadIdx.x;      // (at most 2^32 + 254: wraps only where no entry is)
        const uint32_t my_ne = jr_load_tile(a, s, e);
        const uint32_t row0 = rt * kJoinRaggedTileRows;
        const uint32_t nr = a.rows - row0 < kJoinRaggedTileRows ? a.rows - row0 : kJoinRaggedTileRows;
        const uint32_t self = jr_self_row(a, e, row0);
        for (uint32_t r = 0; r < nr; ++r) {
            uint32_t rec0, n_r;
            jr_row_of(a, row0 + r, &rec0, &n_r);
            float score;
            int32_t lag;
            jr_row<FULL, true>(a, s, s_row, rec0, n_r, my_ne, &score, &lag);
            const bool m = my_ne != 0u && score >= a.t && r != self;
            const uint32_t c = (uint32_t)__popcll(__ballot(m));
            if (lane == 0) s_cnt[r][wave] = c;
        }
        __syncthreads();
        if (wave == 0) {
            uint32_t total = 0;
            if (lane < nr) {
#pragma unroll
                for (uint32_t i = 0; i < kJrWaves; ++i) total += s_cnt[lane][i];
                counts[(row0 + lane) * a.etiles + et] = total;
            }
            const unsigned long long some = __ballot(total != 0u);
            if (lane == 0) any[w] = some ? 1u : 0u;
        }
        __syncthreads();                       // (s_cnt is the next item's)
    }
}

template <bool FULL>
__global__ __launch_bounds__(kJrThreads) void join_ragged_scatter_kernel(const JrArgs a, const uint32_t* __restrict__ counts,
                                                                         const uint32_t* __restrict__ any,
                                                                         const uint32_t* __restrict__ tile_at,
                                                                         const unsigned long long* __restrict__ row_base,
                                                                         uint32_t capacity, uint32_t key_base,
                                                                         unsigned long long* __restrict__ keys,
                                                                         int32_t* __restrict__ lags) {
    // (capacity <= 2^31; key_base = 0xFFFFFFFF - the low word of the index base: a key's low word is key_base - entry)
    extern __shared__ uint4 s_row[];
    __shared__ JrTile s;
    __shared__ uint32_t s_w[kJrWaves];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t i = threadIdx.x; i < kTriSize; i += kJrThreads) s.tri[i] = a.tri[i];
    const uint32_t rtiles = (a.rows + kJoinRaggedTileRows - 1) / kJoinRaggedTileRows;
    const uint32_t items = rtiles * a.etiles;
    for (uint32_t w = blockIdx.x; w < items; w += gridDim.x) {
        if (any[w] == 0u) continue;                                 // (the same word for the whole workgroup) nothing is loaded
        const uint32_t et = w / rtiles, rt = w - et * rtiles;         // (as in the count kernel)
        const uint32_t row0 = rt * kJoinRaggedTileRows;
        const uint32_t nr = a.rows - row0 < kJoinRaggedTileRows ? a.rows - row0 : kJoinRaggedTileRows;
        if (row_base[row0] >= capacity) continue;                   // the list is full in front of this tile of rows
        const uint32_t e = et * kJoinRaggedTileEntries + threadIdx.x;
        const uint32_t my_ne = jr_load_tile(a, s, e);
        const uint32_t self = jr_self_row(a, e, row0);
        uint32_t at_word = row0 * a.etiles + et;
        for (uint32_t r = 0; r < nr; ++r, at_word += a.etiles) {
            if (__builtin_amdgcn_readfirstlane(counts[at_word]) == 0u) continue;      // (uniform: one word per workgroup)
            const unsigned long long at = row_base[row0 + r] + tile_at[at_word];
            if (at >= capacity) continue;
            uint32_t rec0, n_r;
            jr_row_of(a, row0 + r, &rec0, &n_r);
            float score;
            int32_t lag;
            jr_row<FULL, false>(a, s, s_row, rec0, n_r, my_ne, &score, &lag);
            const bool m = my_ne != 0u && score >= a.t && r != self;
            const unsigned long long b = __ballot(m);
            const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
            if (lane == 0) s_w[wave] = (uint32_t)__popcll(b);
            __syncthreads();
            uint32_t before = 0;
#pragma unroll
            for (uint32_t i = 0; i < kJrWaves; ++i) before += i < wave ? s_w[i] : 0u;
            const unsigned long long slot = at + before + below;
            if (m && slot < capacity) {
                keys[slot] = ((unsigned long long)__float_as_uint(score) << 32) | (unsigned long long)(key_base - e);
                if (lags) lags[slot] = lag;
            }
            // (s_w is the next row's: jr_row's barriers stand in between)
        }
    }
}

// the scratch of a chunk of `rows` rows, in this order (every block 8-byte aligned)
struct JrScratch {
    unsigned long long* state;       // 2 words: the total carried from chunk to chunk
    unsigned long long* row_base;    // rows
    uint32_t* counts;                // rows x etiles
    uint32_t* tile_at;               // rows x etiles
    uint32_t* any;                   // row tiles x etiles
};

uint64_t jr_etiles(uint64_t n_entries) { return (n_entries + kJoinRaggedTileEntries - 1) / kJoinRaggedTileEntries; }

JrScratch jr_carve(void* d_scratch, uint64_t n_entries, uint32_t rows) {
    const uint64_t etiles = jr_etiles(n_entries);
    JrScratch s;
    s.state = static_cast<unsigned long long*>(d_scratch);
    s.row_base = s.state + 2;
    s.counts = reinterpret_cast<uint32_t*>(s.row_base + rows);
    s.tile_at = s.counts + (size_t)rows * etiles;
    s.any = s.tile_at + (size_t)rows * etiles;
    return s;
}

template <bool FULL>
hipError_t launch_jr(const JoinRaggedCall& c, const JrScratch& s, const JrArgs& a, uint32_t items, uint32_t first_chunk,
                     unsigned long long* out_offsets) {
    const dim3 grid(strided_grid(items, kJrMaxGrid));
    const size_t row_bytes = ((size_t)a.row_cap + 1u) * 32u;
    hipLaunchKernelGGL(join_ragged_count_kernel<FULL>, grid, dim3(kJrThreads), row_bytes, c.stream, a, s.counts, s.any);
    launch_join_scans(s.counts, a.etiles, a.rows, s.tile_at, s.row_base, s.state, first_chunk, out_offsets, c.stream);
    hipLaunchKernelGGL(join_ragged_scatter_kernel<FULL>, grid, dim3(kJrThreads), row_bytes, c.stream, a, s.counts, s.any, s.tile_at,
                       s.row_base, (uint32_t)c.capacity, 0xFFFFFFFFu - (uint32_t)c.index_base, c.d_keys, c.d_lags);
    return hipGetLastError();
}

}  // namespace

size_t join_ragged_scratch_bytes(uint64_t n_entries, uint64_t rows) {
    const uint64_t etiles = jr_etiles(n_entries);
    const uint64_t rtiles = (rows + kJoinRaggedTileRows - 1) / kJoinRaggedTileRows;
    return (size_t)(16u + rows * (8u + 8u * etiles) + rtiles * etiles * 4u);
}

// rows of a chunk under a scratch limit: the largest whole number of row tiles that fits (0: not even one), at most 2^24
// (with fewer than 2^32 entries there are fewer than 2^24 entry tiles: one row tile always stays within kJrMaxWords)
uint64_t join_ragged_chunk_rows(uint64_t n_entries, uint64_t limit_bytes) {
    const uint64_t etiles = jr_etiles(n_entries);
    const uint64_t per_tile = kJoinRaggedTileRows * (8u + 8u * etiles) + etiles * 4u;
    if (limit_bytes < 16u + per_tile) return 0;
    const uint64_t tiles = (limit_bytes - 16u) / per_tile;
    uint64_t most = (1ull << 24) / kJoinRaggedTileRows;                  // ... and rows x entry tiles within kJrMaxWords
    if (etiles && most > (kJrMaxWords / etiles) / kJoinRaggedTileRows) most = (kJrMaxWords / etiles) / kJoinRaggedTileRows;
    return (tiles < most ? tiles : most) * kJoinRaggedTileRows;
}

hipError_t launch_join_ragged_chunk(const JoinRaggedCall& c, void* d_scratch, uint32_t chunk_rows_max, uint64_t first_row,
                                    uint32_t rows, uint32_t first_chunk, unsigned long long* out_offsets) {
    if (rows == 0 || c.n_entries == 0) return hipSuccess;
    // (the caller has checked the call; what is checked here ties the launch to the LDS row and to the carved scratch.  A
    // corpus with entries has ne_max >= 1: both append calls refuse an entry without sub-fingerprints)
    if (rows > chunk_rows_max || c.q_ne_max == 0 || c.q_ne_max > kJrCap || c.n_entries > kMaxRaggedEntries ||
        (uint64_t)((rows + kJoinRaggedTileRows - 1) / kJoinRaggedTileRows) * kJoinRaggedTileRows * jr_etiles(c.n_entries) > kJrMaxWords ||
        first_row + rows > 0xFFFFFFFFull)
        return hipErrorInvalidValue;
    const float* tri = sliding_tri_table();
    if (!tri) return hipErrorOutOfMemory;
    const JrScratch s = jr_carve(d_scratch, c.n_entries, chunk_rows_max);
    const bool full = c.range >= c.subfp_len;
    const uint4 m = pair_mask(full ? c.subfp_len : c.range);
    JrArgs a;
    a.recs = c.d_recs; a.off = c.d_off; a.n_entries = (uint32_t)c.n_entries; a.etiles = (uint32_t)jr_etiles(c.n_entries);
    a.qrecs = c.d_qrecs; a.qoff = c.d_qoff; a.first_row = (uint32_t)first_row; a.rows = rows; a.skip = c.skip ? 1u : 0u;
    a.row_cap = c.q_ne_max; a.m[0] = m.x; a.m[1] = m.y; a.m[2] = m.z; a.m[3] = m.w; a.tri = tri; a.t = c.threshold;
    const uint32_t items = ((rows + kJoinRaggedTileRows - 1) / kJoinRaggedTileRows) * a.etiles;
    return full ? launch_jr<true>(c, s, a, items, first_chunk, out_offsets) : launch_jr<false>(c, s, a, items, first_chunk, out_offsets);
}

}  // namespace lbad
