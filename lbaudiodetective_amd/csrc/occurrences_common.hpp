// occurrences_common.hpp -- the pair loop of the occurrences pass, shared by the files whose kernels run it: k_occurrences.hip
// (the cells at or above a score as a list), k_recording.hip (the cells folded to a maximum per entry) and k_timeline.hip (to
// the best entry per offset) -- its device side, the head of their kernels and the launch side of a chunk -- and what the list
// families share beyond it (k_occurrences.hip, k_occurrences_batch.hip, k_occurrences_tail.hip): the count of an item, the emission
// of a lane's two cells, the scratch and the checks of a pass of rows.  k_occurrences.hip's
// head states the loop: a work item is (entry, tile of kOcTile offsets), a wave computes the tile's cells and one more on each
// side, a lane owns two neighbouring offsets, the query's window is prepared once per block of kOcEntries entries into LDS and
// fingerprint2's record of a step comes through the scalar unit.  Everything here is per file (an unnamed namespace), as in
// sliding_common.hpp.
#pragma once

#include "sliding_common.hpp"

namespace lbad {
namespace {

constexpr uint32_t kOcTile = 126;                      // cells a wave keeps of the 128 it computes (k_occurrences.hip: kOcKeep)
constexpr uint32_t kOcThreads = 256;
constexpr uint32_t kOcWaves = kOcThreads / 64;
constexpr uint32_t kOcTileGroup = kOcWaves * kOcTile;  // offsets of one entry a workgroup takes
constexpr uint32_t kOcEntries = 64;                    // entries a workgroup walks with one window (k_occurrences.hip: kOcBlock)
constexpr uint32_t kOcMaxGrid = 1u << 16;              // units beyond this many workgroups are walked with a grid stride
constexpr uint64_t kOcMaxItems = 0xFFFFFFFFull - 4096; // entries x tiles of a chunk: 32-bit indices
constexpr uint32_t kOcMaxRecs = 65535;                 // recordings of a pass, in every batch and tail family
constexpr uint32_t kOcCap = LBAD_OCCURRENCES_MAX_ENTRY_SUBFINGERPRINTS;
constexpr uint32_t kOcTriLast = kTriPairs * (kTriPairs + 1) / 2;   // the table's last row
constexpr uint32_t kOcRecBytes = 36;                   // a prepared record in LDS: P, N, the row
static_assert(kOcCap >= 1024, "the header promises 1024");
static_assert((kOcTileGroup + 2 + kOcCap) * kOcRecBytes + kTriSize * 4 + 64 <= 160 * 1024, "the window and the table fit a CU's LDS");

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
        uint32_t r = o - wb;                                   // (o >= wb; at most kOcTileGroup + ne < win with the steps)
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

// The count of one item (entry e of the chunk, the tile whose first offset is `first`): its matching cells, 0 where the pair has no
// offset in the tile.  a: the wave's recording (its query; the corpus and the chunk are the call's); lane: the kernel's own
// threadIdx.x & 63.  Called by whole waves.
template <bool FULL>
__device__ __forceinline__ uint32_t oc_count_cells(const OcArgs& a, const OcLds& s, uint32_t wb, uint32_t e, uint32_t first,
                                                   uint32_t lane) {
    uint32_t rec0, ne, c = 0u;
    oc_entry(a, e, &rec0, &ne);
    if (first < oc_offsets(a, ne)) {
        float q0, q1;
        const uint32_t m = oc_cells<FULL>(a, s, wb, rec0, ne, first - 1u + 2u * lane, &q0, &q1);
        c = (uint32_t)__popcll(__ballot(m & 1u)) + (uint32_t)__popcll(__ballot(m & 2u));
    }
    return c;
}

// The lane's two cells of one item (oc_cells' match bits m and quotients q0 and q1; offsets o and o1 = o + 1, the caller's sum:
// the value oc_cells tests) into the list: the item's first slot is `at`, a cell's slot that plus the matching cells in lower lanes
// (and the lane's own first cell), written where it is below the capacity.  A key is  quotient bits << 32 | key_base - e, a lag
// +offset where the entry is the longer (case A), -offset otherwise.  Called by whole waves (the ballots).
__device__ __forceinline__ void oc_emit(const OcArgs& a, uint32_t e, uint32_t ne, uint32_t m, uint32_t o, uint32_t o1, float q0, float q1,
                                        unsigned long long at, unsigned long long capacity, uint32_t key_base,
                                        unsigned long long* keys, int32_t* lags) {
    const unsigned long long b0 = __ballot(m & 1u), b1 = __ballot(m & 2u);
    const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(b0 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b0, 0u)) +
                           __builtin_amdgcn_mbcnt_hi((uint32_t)(b1 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b1, 0u));
    const bool entry_long = a.nq < ne;
    const unsigned long long low = (unsigned long long)(key_base - e);
    const auto put = [&](unsigned long long slot, float q, uint32_t off) {
        keys[slot] = ((unsigned long long)__float_as_uint(q) << 32) | low;
        if (lags) {
            // (tools/isa_diff.py asks for this form: with a plain `lags[slot] = ...` the six scatter kernels schedule the select in
            // front of the address and are no longer, instruction for instruction, the kernels that wrote this out themselves.
            // Passing o1 in, not adding 1 here, is for the same check.  Once that comparison no longer matters, write it plainly.)
            int32_t& lag = lags[slot];
            lag = entry_long ? (int32_t)off : -(int32_t)off;
        }
    };
    unsigned long long slot = at + below;
    if ((m & 1u) && slot < capacity) put(slot, q0, o);
    slot += m & 1u;
    if ((m & 2u) && slot < capacity) put(slot, q1, o1);
}

// The head of a pair-loop kernel.  The table into LDS (a unit's first barrier stands between this and the first read):
__device__ __forceinline__ void oc_load_tri(const OcArgs& a, const OcLds& s) {
    for (uint32_t i = threadIdx.x; i < kTriSize; i += kOcThreads) s.tri[i] = a.tri[i];
}
// units of a kernel whose units walk `walk` entries: unit u = (entry block u / groups, tile group u % groups), so workgroups
// that run at the same time share their entries' records
__device__ __forceinline__ uint32_t oc_units(const OcArgs& a, uint32_t walk) { return ((a.entries + walk - 1u) / walk) * a.groups; }
struct OcUnit {
    uint32_t eb, wb;              // the entry block; the window's first record (the group's first offset - 1, wrapping below 0)
    uint32_t tile;                // this wave's tile (`wave` is the kernel's threadIdx.x >> 6): it takes part when tile < a.tiles
    uint32_t e0, e1;              // the block's entries of the chunk
};
__device__ __forceinline__ OcUnit oc_unit(const OcArgs& a, uint32_t u, uint32_t walk, uint32_t wave) {
    OcUnit n;
    n.eb = u / a.groups;
    const uint32_t g = u - n.eb * a.groups;
    n.wb = g * kOcTileGroup - 1u;
    n.tile = g * kOcWaves + wave;
    n.e0 = n.eb * walk;
    n.e1 = a.entries - n.e0 < walk ? a.entries : n.e0 + walk;
    return n;
}
// the window of a unit staged once the unit before has left it
__device__ __forceinline__ void oc_stage_unit(const OcArgs& a, const OcLds& s, uint32_t wb) {
    __syncthreads();
    oc_stage(a, s, wb);
    __syncthreads();
}

inline uint64_t oc_groups(uint64_t tiles) { return (tiles + kOcWaves - 1) / kOcWaves; }
inline uint64_t oc_blocks(uint64_t entries) { return (entries + kOcEntries - 1) / kOcEntries; }
inline dim3 oc_grid(uint64_t units) { return dim3(strided_grid(units, kOcMaxGrid)); }

// The launch side of a chunk.  What every family checks of a call (the caller has checked it; this ties the launch to the LDS
// window and to the scratch): `tiles` is the family's bound for the call
inline bool oc_call_ok(const OcPassCall& c, uint64_t tiles, uint64_t first_entry, uint64_t entries) {
    return c.n_query != 0 && c.n_query <= 0x7FFFFFFFu && c.ne_max != 0 && c.ne_max <= kOcCap && c.tiles != 0 && c.tiles == tiles &&
           entries * c.tiles <= kOcMaxItems && first_entry + entries <= kMaxRaggedEntries;
}
// The scratch of the list families (k_occurrences.hip, k_occurrences_batch.hip, k_occurrences_tail.hip), in this order (every block
// 8-byte aligned; occurrences_scratch_bytes sizes it): `rows` rows of the joins' two scans -- the entries of a chunk, or recordings x
// entries of a pass -- of `tiles` columns each (the tail lists: one)
struct OcScratch {
    unsigned long long* state;       // 2 words: the total carried from chunk to chunk
    unsigned long long* row_base;    // rows: a row's first position
    unsigned long long* offsets;     // rows + 1: the same, and the total behind the last row (the single call reads none of it: 8
                                     // bytes per entry are the price of using the joins' scans as they are)
    uint32_t* counts;                // rows x tiles
    uint32_t* tile_at;               // rows x tiles
    uint32_t* any;                   // units
};
inline OcScratch oc_carve(void* d_scratch, uint64_t rows, uint64_t tiles) {
    OcScratch s;
    s.state = static_cast<unsigned long long*>(d_scratch);
    s.row_base = s.state + 2;
    s.offsets = s.row_base + rows;
    s.counts = reinterpret_cast<uint32_t*>(s.offsets + rows + 1);
    s.tile_at = s.counts + (size_t)rows * tiles;
    s.any = s.tile_at + (size_t)rows * tiles;
    return s;
}
// What ties a chunk of the rows-of-keys families (batch and tail lists) to its plan -- Plan: recordings_per_pass, entries_per_chunk,
// scratch_bytes -- behind oc_call_ok: the recordings against the plan's pass, the entries against its chunk, more than one recording
// takes the whole corpus in one chunk, the 32-bit item, row and slot indices, the scratch, the index base, the outputs
template <typename Plan>
inline bool oc_rows_call_ok(const OccurrencesCall& c, const Plan& plan, uint32_t recordings, uint64_t first_entry, uint64_t entries,
                            uint32_t first_chunk, const void* d_counts) {
    const bool chunked = plan.recordings_per_pass == 1;
    return recordings <= plan.recordings_per_pass && recordings <= kOcMaxRecs && entries <= plan.entries_per_chunk &&
           (chunked || (first_entry == 0 && first_chunk != 0)) && (uint64_t)recordings * entries * c.tiles <= kOcMaxItems &&
           (uint64_t)recordings * c.n_query <= 0x7FFFFFFFull && (uint64_t)recordings * c.capacity <= 0x80000000ull &&
           (uint64_t)recordings * occurrences_scratch_bytes(entries, c.tiles) <= plan.scratch_bytes &&
           c.index_base + first_entry + entries <= 0x100000000ull && c.d_keys && d_counts;
}
// the kernels' arguments for `entries` entries from `first_entry` (a.tri == nullptr: no table), and the LDS of a workgroup
inline OcArgs oc_args(const OcPassCall& c, uint64_t first_entry, uint64_t entries, float threshold, bool peaks, size_t* lds) {
    const uint4 m = pair_mask(c.range >= c.subfp_len ? c.subfp_len : c.range);
    const uint32_t ne_b = c.ne_max < c.n_query ? c.ne_max : c.n_query;
    OcArgs a;
    a.recs = c.d_recs; a.off = c.d_off; a.first = (uint32_t)first_entry; a.entries = (uint32_t)entries;
    a.tiles = (uint32_t)c.tiles; a.groups = (uint32_t)oc_groups(c.tiles); a.ne_max = c.ne_max;
    a.q = reinterpret_cast<const uint4*>(c.d_qwords); a.nq = c.n_query; a.win = kOcTileGroup + 2u + ne_b;
    a.m[0] = m.x; a.m[1] = m.y; a.m[2] = m.z; a.m[3] = m.w; a.tri = sliding_tri_table(); a.t = threshold; a.peaks = peaks ? 1u : 0u;
    *lds = occurrences_lds_bytes(c.n_query, c.ne_max);
    return a;
}
// Dynamic LDS above 48 KiB has to be allowed per kernel and device.  `ready`: the largest size every kernel of the set was set
// up for on each device -- the caller's static, one per kernel set -- recorded once EVERY call has succeeded (not PerDevice:
// that helper records before the set-up has succeeded.  Unsynchronised like it; two host threads that race here set the
// attribute twice at worst)
template <typename... Kernels>
hipError_t oc_allow_lds(size_t (&ready)[kMaxDevices], size_t lds, Kernels... kernels) {
    const int dev = current_device();
    if (dev < 0 || dev >= kMaxDevices) return hipErrorInvalidDevice;
    if (lds <= 48 * 1024 || lds <= ready[dev]) return hipSuccess;
    hipError_t e = hipSuccess;
    for (const void* k : {reinterpret_cast<const void*>(kernels)...})
        if (e == hipSuccess) e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e == hipSuccess) ready[dev] = lds;
    return e;
}

}  // namespace
}  // namespace lbad
