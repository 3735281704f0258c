// k_occurrences.hip -- every place a recording matches a RAGGED corpus: for ONE query and every entry j, each cell q_o of the
// pair's profile (what LBAudioDetectiveCorpusMatchProfile returns, k_align.hip:1-14 states it) that reaches a threshold, as a
// list on the device in (entry, offset) order, with its signed lag.  fingerprint1 is the entry when the query is shorter ("A",
// lag +o), the query otherwise ("B", equal lengths included, lag -o); with n1 >= n2
//   q_o = fl(fl(sum over s = 0 .. n2 - 1, in that order, of ratio(fp1[s + o], fp2[s])) / n2),   o = 0 .. n1 - n2
// ratio = hits / possible correctly rounded (the table of sliding.cpp), possible = fingerprint1's non-zero pairs inside the
// range.  A cell matches when q_o >= threshold, and with `peaks` only when it is a local peak of its own profile:
// (o == 0 or q_o > q_(o-1)) and (o == last or q_o >= q_(o+1)) -- the first cell of a plateau.
//
// The structure is the joins': count per work item -> the two scans of k_join.hip (counts[entry][tile] has their layout, an
// entry is a "row") -> a scatter that computes again only the items that have a match.  No workgroup waits for another, no
// atomic touches memory, and every output location has one writer: nothing depends on which lane or workgroup finishes first.
//
// The pair loop steps over fingerprint2 and slides over fingerprint1.  A work item is (entry, tile of kOcKeep = 126 offsets);
// a wave takes an item and computes 128 cells, one more on each side of its tile: the neighbours the peak test of the tile's
// first and last cell needs (the recommended 128 kept cells would need the two edge cells from another pass over the pair).
// A lane owns TWO neighbouring offsets: fingerprint1's record of a step is the record the lane's other offset read one step
// earlier (k_join_ragged.hip's trick), so a step loads ONE record of fingerprint1 for two compares.  What a lane keeps of a
// fingerprint1 record is PREPARED once per record: P and N under the pair mask of the range and the quotient table's row of
// its `possible` -- the compare itself is then the same for every range.  fingerprint2's record of a step is the same for the
// whole wave and comes through the scalar unit.
//   B  the monitoring shape, a long recording against short entries.  The four waves of a workgroup take four neighbouring
//      tiles of ONE entry and walk a block of kOcBlock entries with them; the query records those tiles can touch for any
//      entry, [first offset - 1, first offset + 4 x 126 + 1 + longest B entry), are prepared ONCE per block into LDS (P, N and
//      the table row in separate arrays: a lane's stride of two records then meets no bank twice in a 16-byte read).  A pass
//      runs n_e steps, the entry's length: nothing is spent on pairs that do not exist.
//   A  the query is shorter: the entry's records are per lane, from memory, the query's uniform.  The table row is the
//      record's own where the range covers the length (FULL), a population count under the mask otherwise.
// Nothing is read beyond an entry's records plus one (inside kRecordSlack), or beyond the query's words; every loop is bounded
// by lengths from the record positions, clamped to the corpus' longest entry.
#include "sliding_common.hpp"

namespace lbad {
namespace {

constexpr uint32_t kOcKeep = 126;                      // cells a wave keeps of the 128 it computes
constexpr uint32_t kOcThreads = 256;
constexpr uint32_t kOcWaves = kOcThreads / 64;
constexpr uint32_t kOcGroup = kOcWaves * kOcKeep;      // offsets of one entry a workgroup takes
constexpr uint32_t kOcBlock = 64;                      // entries a workgroup walks with one window: what a chunk is a multiple of
constexpr uint32_t kOcMaxGrid = 1u << 16;              // units beyond this many workgroups are walked with a grid stride
constexpr uint64_t kOcMaxItems = 0xFFFFFFFFull - 4096; // entries x tiles of a chunk: 32-bit indices
constexpr uint32_t kOcCap = LBAD_OCCURRENCES_MAX_ENTRY_SUBFINGERPRINTS;
constexpr uint32_t kOcTriLast = kTriPairs * (kTriPairs + 1) / 2;   // the table's last row
constexpr uint32_t kOcRecBytes = 36;                   // a prepared record in LDS: P, N, the row
static_assert(kOcCap >= 1024, "the header promises 1024");
static_assert((kOcGroup + 2 + kOcCap) * kOcRecBytes + kTriSize * 4 + 64 <= 160 * 1024, "the window and the table fit a CU's LDS");

struct OcArgs {
    const uint4* recs;            // the corpus
    const uint32_t* off;
    uint32_t first, entries;      // the chunk: its first entry, its entries
    uint32_t tiles, groups;       // tiles per entry (the call's bound), groups of kOcWaves of them
    uint32_t ne_max;              // the corpus' longest entry
    const uint4* q;               // the query: P[4] N[4] per sub-fingerprint
    uint32_t nq;
    uint32_t win;                 // records of the LDS window
    uint32_t m[4];                // the pair mask of min(range, length)
    const float* tri;
    float t;
    uint32_t peaks;
};

typedef const u32x4 __attribute__((address_space(4))) * OcUniform;     // wave-uniform addresses no kernel of the call writes
__device__ __forceinline__ uint4 oc_uniform(OcUniform p, uint32_t i) {
    const u32x4 v = p[i];
    return make_uint4(v.x, v.y, v.z, v.w);
}

// a record of fingerprint1 as a lane keeps it
struct OcRec {
    uint4 p, n;
    uint32_t row;
};

__device__ __forceinline__ uint32_t oc_row_of(const uint4& p, const uint4& n) {
    const uint32_t possible = __popc(p.x | n.x) + __popc(p.y | n.y) + __popc(p.z | n.z) + __popc(p.w | n.w);
    return (possible * (possible + 1u)) >> 1;
}

// a corpus record prepared.  FULL: the range covers the length, the builders leave the pairs beyond it zero, and the record's
// own table row is possible's (bounded: whatever the word holds, the read stays inside the table -- hits <= 100)
template <bool FULL>
__device__ __forceinline__ OcRec oc_prepare(uint4 p, uint4 n, const uint32_t (&m)[4]) {
    OcRec r;
    if (FULL) {
        const uint32_t row = (p.w >> 4) & 0x1FFFu;
        r.row = row < kOcTriLast ? row : kOcTriLast;
        p.w &= 0xFu;
        n.w &= 0xFu;
        r.p = p;
        r.n = n;
    } else {
        r.p = make_uint4(p.x & m[0], p.y & m[1], p.z & m[2], p.w & m[3]);
        r.n = make_uint4(n.x & m[0], n.y & m[1], n.z & m[2], n.w & m[3]);
        r.row = oc_row_of(r.p, r.n);
    }
    return r;
}

// hits / possible of one step: f fingerprint1's prepared record, (p2, n2) fingerprint2's raw words (whatever they hold above
// the pairs never meets a set bit of f)
__device__ __forceinline__ float oc_ratio(const float* tri, const OcRec& f, const uint4& p2, const uint4& n2) {
    const uint32_t a[4] = {f.p.x, f.p.y, f.p.z, f.p.w}, b[4] = {f.n.x, f.n.y, f.n.z, f.n.w};
    const uint32_t c[4] = {p2.x, p2.y, p2.z, p2.w}, d[4] = {n2.x, n2.y, n2.z, n2.w};
    uint32_t at = f.row;
#pragma unroll
    for (uint32_t w = 0; w < 4; ++w) {
        const uint32_t u = __builtin_amdgcn_bitop3_b32(a[w], b[w], c[w], 0xA4);        // (a | b) & ~(a ^ c)
        at += __popc(__builtin_amdgcn_bitop3_b32(u, b[w], d[w], 0x90));                // u & ~(b ^ d)
    }
    asm("" : "+v"(at));                                // (one index: the counts add up before the table's stride is applied)
    return tri[at];
}

// the LDS of a workgroup: the table, then the window's three arrays (dynamic)
struct OcLds {
    float* tri;
    uint4 *p, *n;
    uint32_t* row;
};
__device__ __forceinline__ OcLds oc_lds(uint4* dyn, uint32_t win) {
    OcLds s;
    s.p = dyn;
    s.n = dyn + win;
    s.row = reinterpret_cast<uint32_t*>(dyn + 2u * (size_t)win);
    s.tri = reinterpret_cast<float*>(s.row + win);
    return s;
}

// the query records [wb, wb + win) prepared into LDS (wb = the group's first offset - 1, wrapping below 0; zero records
// where the query has none)
__device__ __forceinline__ void oc_stage(const OcArgs& a, const OcLds& s, uint32_t wb) {
    for (uint32_t r = threadIdx.x; r < a.win; r += kOcThreads) {
        const uint32_t qi = wb + r;
        OcRec f;
        f.p = make_uint4(0u, 0u, 0u, 0u);
        f.n = f.p;
        f.row = 0u;
        if (qi < a.nq) f = oc_prepare<false>(a.q[2u * (size_t)qi], a.q[2u * (size_t)qi + 1u], a.m);
        s.p[r] = f.p;
        s.n[r] = f.n;
        s.row[r] = f.row;
    }
}

// The 128 cells of one item: the lane's offsets are o and o + 1 with o = the tile's first offset - 1 + 2 x lane (o wraps to
// 0xFFFFFFFF for lane 0 of tile 0).  Returns the lane's match bits (bit 0: cell o, bit 1: cell o + 1) and the two quotients.
// Called by whole waves with wave-uniform (rec0, ne); n_off = the pair's offsets.
template <bool FULL>
__device__ __forceinline__ uint32_t oc_cells(const OcArgs& a, const OcLds& s, uint32_t wb, uint32_t rec0, uint32_t ne, uint32_t o,
                                             float* q0, float* q1) {
    const uint32_t lane = threadIdx.x & 63u;
    const bool is_a = a.nq < ne;
    float s0 = 0.0f, s1 = 0.0f, n2;
    uint32_t n_off;
    if (is_a) {
        // the entry is fingerprint1, per lane from memory (never beyond the record behind the entry); the query's record of a
        // step is wave-uniform
        n_off = ne - a.nq + 1u;
        const uint4* __restrict__ g = a.recs + 2u * (size_t)rec0;
        const uint32_t i0 = o + 1u == 0u ? 0u : (o < ne ? o : ne);
        OcRec f = oc_prepare<FULL>(g[2u * i0], g[2u * i0 + 1u], a.m);
        const OcUniform uq = (OcUniform)(uintptr_t)a.q;
        for (uint32_t i = 0; i < a.nq; ++i) {
            uint32_t at = o + 1u + i;
            at = at < ne ? at : ne;
            const OcRec c = oc_prepare<FULL>(g[2u * at], g[2u * at + 1u], a.m);
            const uint4 qp = oc_uniform(uq, 2u * i), qn = oc_uniform(uq, 2u * i + 1u);
            s0 = __fadd_rn(s0, oc_ratio(s.tri, f, qp, qn));
            s1 = __fadd_rn(s1, oc_ratio(s.tri, c, qp, qn));
            f = c;
        }
        n2 = (float)a.nq;
    } else {
        // the query is fingerprint1, prepared in LDS; the entry's record of a step is wave-uniform
        n_off = a.nq - ne + 1u;
        uint32_t r = o - wb;                                   // (o >= wb; at most kOcGroup + ne < win with the steps)
        OcRec f;
        f.p = s.p[r]; f.n = s.n[r]; f.row = s.row[r];
        const OcUniform ue = (OcUniform)(uintptr_t)(a.recs + 2u * (size_t)rec0);
        for (uint32_t i = 0; i < ne; ++i) {
            ++r;
            OcRec c;
            c.p = s.p[r]; c.n = s.n[r]; c.row = s.row[r];
            const uint4 ep = oc_uniform(ue, 2u * i), en = oc_uniform(ue, 2u * i + 1u);
            s0 = __fadd_rn(s0, oc_ratio(s.tri, f, ep, en));
            s1 = __fadd_rn(s1, oc_ratio(s.tri, c, ep, en));
            f = c;
        }
        n2 = (float)ne;
    }
    const float c0 = __fdiv_rn(s0, n2), c1 = __fdiv_rn(s1, n2);
    // (full EXEC: the whole wave is here) cell o - 1 is the left lane's second, cell o + 2 the right lane's first
    const float left = __uint_as_float(from_left_lane(__float_as_uint(c1)));
    const float right = __uint_as_float(from_right_lane(__float_as_uint(c0)));
    bool m0 = lane != 0u && o < n_off && c0 >= a.t;            // (lane 0's first and lane 63's second cell are the neighbours' only)
    bool m1 = lane != 63u && o + 1u < n_off && c1 >= a.t;
    if (a.peaks) {
        m0 = m0 && (o == 0u || c0 > left) && (o + 1u == n_off || c0 >= c1);
        m1 = m1 && (o + 1u == 0u || c1 > c0) && (o + 2u == n_off || c1 >= right);
    }
    *q0 = c0;
    *q1 = c1;
    return (m0 ? 1u : 0u) | (m1 ? 2u : 0u);
}

// (first record, length) of entry e of the chunk, wave-uniform
__device__ __forceinline__ void oc_entry(const OcArgs& a, uint32_t e, uint32_t* rec0, uint32_t* ne) {
    const uint32_t at = __builtin_amdgcn_readfirstlane(a.off[a.first + e]);
    const uint32_t n = __builtin_amdgcn_readfirstlane(a.off[a.first + e + 1u]) - at;
    *rec0 = at;
    *ne = n < a.ne_max ? n : a.ne_max;
}

// offsets of the pair (query, entry of ne sub-fingerprints)
__device__ __forceinline__ uint32_t oc_offsets(const OcArgs& a, uint32_t ne) { return a.nq < ne ? ne - a.nq + 1u : a.nq - ne + 1u; }

// Unit u = (entry block u / groups, tile group u % groups): workgroups that run at the same time share their entries' records.
// counts[entry][tile] for every tile below a.tiles; any[u]: the unit has a match.
template <bool FULL>
__global__ __launch_bounds__(kOcThreads) void occurrences_count_kernel(const OcArgs a, uint32_t* __restrict__ counts,
                                                                       uint32_t* __restrict__ any) {
    extern __shared__ uint4 s_dyn[];
    __shared__ uint32_t s_any;
    const OcLds s = oc_lds(s_dyn, a.win);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t i = threadIdx.x; i < kTriSize; i += kOcThreads) s.tri[i] = a.tri[i];
    const uint32_t units = ((a.entries + kOcBlock - 1u) / kOcBlock) * a.groups;
    for (uint32_t u = blockIdx.x; u < units; u += gridDim.x) {
        const uint32_t eb = u / a.groups, g = u - eb * a.groups;
        const uint32_t wb = g * kOcGroup - 1u;
        __syncthreads();                                       // (the unit before has left the window and s_any)
        oc_stage(a, s, wb);
        if (threadIdx.x == 0u) s_any = 0u;
        __syncthreads();
        const uint32_t tile = g * kOcWaves + wave;
        const uint32_t e0 = eb * kOcBlock, e1 = a.entries - e0 < kOcBlock ? a.entries : e0 + kOcBlock;
        uint32_t some = 0u;
        if (tile < a.tiles) {
            const uint32_t first = tile * kOcKeep;
            for (uint32_t e = e0; e < e1; ++e) {
                uint32_t rec0, ne, c = 0u;
                oc_entry(a, e, &rec0, &ne);
                if (first < oc_offsets(a, ne)) {
                    float q0, q1;
                    const uint32_t m = oc_cells<FULL>(a, s, wb, rec0, ne, first - 1u + 2u * lane, &q0, &q1);
                    c = (uint32_t)__popcll(__ballot(m & 1u)) + (uint32_t)__popcll(__ballot(m & 2u));
                }
                if (lane == 0u) counts[e * a.tiles + tile] = c;
                some |= c;
            }
        }
        if (lane == 0u && some) atomicOr(&s_any, 1u);          // (LDS: a flag, whoever sets it)
        __syncthreads();
        if (threadIdx.x == 0u) any[u] = s_any;
    }
}

template <bool FULL>
__global__ __launch_bounds__(kOcThreads) void occurrences_scatter_kernel(const OcArgs a, const uint32_t* __restrict__ counts,
                                                                         const uint32_t* __restrict__ any,
                                                                         const uint32_t* __restrict__ tile_at,
                                                                         const unsigned long long* __restrict__ row_base,
                                                                         unsigned long long capacity, uint32_t key_base,
                                                                         unsigned long long* __restrict__ keys,
                                                                         int32_t* __restrict__ lags) {
    // (key_base = 0xFFFFFFFF - the low word of the index base - the chunk's first entry: a key's low word is key_base - e)
    extern __shared__ uint4 s_dyn[];
    const OcLds s = oc_lds(s_dyn, a.win);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t i = threadIdx.x; i < kTriSize; i += kOcThreads) s.tri[i] = a.tri[i];
    const uint32_t units = ((a.entries + kOcBlock - 1u) / kOcBlock) * a.groups;
    for (uint32_t u = blockIdx.x; u < units; u += gridDim.x) {
        if (any[u] == 0u) continue;                            // (the same word for the whole workgroup) nothing is loaded
        const uint32_t eb = u / a.groups, g = u - eb * a.groups;
        const uint32_t e0 = eb * kOcBlock, e1 = a.entries - e0 < kOcBlock ? a.entries : e0 + kOcBlock;
        if (row_base[e0] >= capacity) continue;                // the list is full in front of this block
        const uint32_t wb = g * kOcGroup - 1u;
        __syncthreads();
        oc_stage(a, s, wb);
        __syncthreads();
        const uint32_t tile = g * kOcWaves + wave;
        if (tile >= a.tiles) continue;                         // (this wave meets no barrier of the unit any more)
        const uint32_t first = tile * kOcKeep;
        for (uint32_t e = e0; e < e1; ++e) {
            const uint32_t item = e * a.tiles + tile;
            if (__builtin_amdgcn_readfirstlane(counts[item]) == 0u) continue;
            const unsigned long long at = row_base[e] + tile_at[item];
            if (at >= capacity) continue;
            uint32_t rec0, ne;
            oc_entry(a, e, &rec0, &ne);
            const uint32_t o = first - 1u + 2u * lane;
            float q0, q1;
            const uint32_t m = oc_cells<FULL>(a, s, wb, rec0, ne, o, &q0, &q1);
            const unsigned long long b0 = __ballot(m & 1u), b1 = __ballot(m & 2u);
            const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(b0 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b0, 0u)) +
                                   __builtin_amdgcn_mbcnt_hi((uint32_t)(b1 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b1, 0u));
            const bool entry_long = a.nq < ne;
            const unsigned long long low = (unsigned long long)(key_base - e);
            unsigned long long slot = at + below;
            if ((m & 1u) && slot < capacity) {
                keys[slot] = ((unsigned long long)__float_as_uint(q0) << 32) | low;
                if (lags) lags[slot] = entry_long ? (int32_t)o : -(int32_t)o;
            }
            slot += m & 1u;
            if ((m & 2u) && slot < capacity) {
                keys[slot] = ((unsigned long long)__float_as_uint(q1) << 32) | low;
                if (lags) lags[slot] = entry_long ? (int32_t)(o + 1u) : -(int32_t)(o + 1u);
            }
        }
    }
}

// the scratch of a chunk of `entries` entries, in this order (every block 8-byte aligned)
struct OcScratch {
    unsigned long long* state;       // 2 words: the total carried from chunk to chunk
    unsigned long long* row_base;    // entries: an entry's first slot
    unsigned long long* offsets;     // entries + 1: what launch_join_scans hands a join's caller; nothing reads it here -- 8 bytes
                                     // per entry are the price of using the joins' scans as they are
    uint32_t* counts;                // entries x tiles
    uint32_t* tile_at;               // entries x tiles
    uint32_t* any;                   // entry blocks x tile groups
};

uint64_t oc_groups(uint64_t tiles) { return (tiles + kOcWaves - 1) / kOcWaves; }
uint64_t oc_blocks(uint64_t entries) { return (entries + kOcBlock - 1) / kOcBlock; }

OcScratch oc_carve(void* d_scratch, uint64_t entries, uint64_t tiles) {
    OcScratch s;
    s.state = static_cast<unsigned long long*>(d_scratch);
    s.row_base = s.state + 2;
    s.offsets = s.row_base + entries;
    s.counts = reinterpret_cast<uint32_t*>(s.offsets + entries + 1);
    s.tile_at = s.counts + (size_t)entries * tiles;
    s.any = s.tile_at + (size_t)entries * tiles;
    return s;
}

template <bool FULL>
hipError_t launch_oc(const OccurrencesCall& c, const OcScratch& s, const OcArgs& a, size_t lds, uint32_t first_chunk) {
    // (the largest size both kernels of this instance were set up for on each device, recorded once BOTH calls have succeeded)
    // (not PerDevice: that helper records before the set-up has succeeded.  Unsynchronised like it; two host threads that race
    // here set the attribute twice at worst)
    static size_t ready[kMaxDevices] = {};
    const int dev = current_device();
    if (dev < 0 || dev >= kMaxDevices) return hipErrorInvalidDevice;
    if (lds > 48 * 1024 && lds > ready[dev]) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(occurrences_count_kernel<FULL>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e == hipSuccess)
            e = hipFuncSetAttribute(reinterpret_cast<const void*>(occurrences_scatter_kernel<FULL>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
        ready[dev] = lds;
    }
    const uint64_t units = oc_blocks(a.entries) * a.groups;
    const dim3 grid((uint32_t)(units < kOcMaxGrid ? units : kOcMaxGrid));
    hipLaunchKernelGGL(occurrences_count_kernel<FULL>, grid, dim3(kOcThreads), lds, c.stream, a, s.counts, s.any);
    launch_join_scans(s.counts, a.tiles, a.entries, s.tile_at, s.row_base, s.state, first_chunk, s.offsets, c.stream);
    hipLaunchKernelGGL(occurrences_scatter_kernel<FULL>, grid, dim3(kOcThreads), lds, c.stream, a, s.counts, s.any, s.tile_at,
                       s.row_base, (unsigned long long)c.capacity, 0xFFFFFFFFu - (uint32_t)c.index_base - a.first, c.d_keys, c.d_lags);
    return hipGetLastError();
}

}  // namespace

uint32_t occurrences_block_entries() { return kOcBlock; }

uint64_t occurrences_tiles(uint32_t n_query, uint32_t ne_min, uint32_t ne_max) {
    uint64_t most = 1;
    if (ne_max > n_query) most = (uint64_t)ne_max - n_query + 1;
    if (ne_min <= n_query && (uint64_t)n_query - ne_min + 1 > most) most = (uint64_t)n_query - ne_min + 1;
    return (most + kOcKeep - 1) / kOcKeep;
}

size_t occurrences_scratch_bytes(uint64_t entries, uint64_t tiles) {
    return (size_t)(24u + entries * (16u + 8u * tiles) + oc_blocks(entries) * oc_groups(tiles) * 4u);
}

size_t occurrences_lds_bytes(uint32_t n_query, uint32_t ne_max) {
    const uint32_t ne_b = ne_max < n_query ? ne_max : n_query;
    return (size_t)(kOcGroup + 2u + ne_b) * kOcRecBytes + kTriSize * sizeof(float);
}

// entries of a chunk under a scratch limit: the largest whole number of entry blocks that fits (0: not even one), with
// entries x tiles within kOcMaxItems
uint64_t occurrences_chunk_entries(uint64_t tiles, uint64_t limit_bytes) {
    const uint64_t per_block = kOcBlock * (16u + 8u * tiles) + oc_groups(tiles) * 4u;
    if (limit_bytes < 24u + per_block) return 0;
    const uint64_t blocks = (limit_bytes - 24u) / per_block;
    const uint64_t most = (kOcMaxItems / tiles) / kOcBlock;
    return (blocks < most ? blocks : most) * kOcBlock;
}

hipError_t launch_occurrences_chunk(const OccurrencesCall& c, void* d_scratch, uint64_t chunk_entries_max, uint64_t first_entry,
                                    uint64_t entries, uint32_t first_chunk) {
    if (entries == 0) return hipSuccess;
    // (the caller has checked the call; what is checked here ties the launch to the LDS window and to the carved scratch)
    if (entries > chunk_entries_max || c.n_query == 0 || c.n_query > 0x7FFFFFFFu || c.ne_max == 0 || c.ne_max > kOcCap ||
        c.tiles == 0 || c.tiles != occurrences_tiles(c.n_query, c.ne_min, c.ne_max) || entries * c.tiles > kOcMaxItems ||
        first_entry + entries > kMaxRaggedEntries || c.index_base + first_entry + entries > 0x100000000ull)
        return hipErrorInvalidValue;
    const float* tri = sliding_tri_table();
    if (!tri) return hipErrorOutOfMemory;
    const OcScratch s = oc_carve(d_scratch, chunk_entries_max, c.tiles);
    const bool full = c.range >= c.subfp_len;
    const uint4 m = pair_mask(full ? c.subfp_len : c.range);
    const uint32_t ne_b = c.ne_max < c.n_query ? c.ne_max : c.n_query;
    OcArgs a;
    a.recs = c.d_recs; a.off = c.d_off; a.first = (uint32_t)first_entry; a.entries = (uint32_t)entries;
    a.tiles = (uint32_t)c.tiles; a.groups = (uint32_t)oc_groups(c.tiles); a.ne_max = c.ne_max;
    a.q = reinterpret_cast<const uint4*>(c.d_qwords); a.nq = c.n_query; a.win = kOcGroup + 2u + ne_b;
    a.m[0] = m.x; a.m[1] = m.y; a.m[2] = m.z; a.m[3] = m.w; a.tri = tri; a.t = c.threshold; a.peaks = c.peaks ? 1u : 0u;
    const size_t lds = occurrences_lds_bytes(c.n_query, c.ne_max);
    return full ? launch_oc<true>(c, s, a, lds, first_chunk) : launch_oc<false>(c, s, a, lds, first_chunk);
}

}  // namespace lbad
