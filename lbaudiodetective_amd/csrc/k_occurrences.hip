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
#include "occurrences_common.hpp"

namespace lbad {
namespace {

constexpr uint32_t kOcKeep = 126;                      // cells a wave keeps of the 128 it computes
constexpr uint32_t kOcGroup = kOcWaves * kOcKeep;      // offsets of one entry a workgroup takes
constexpr uint32_t kOcBlock = 64;                      // entries a workgroup walks with one window: what a chunk is a multiple of
static_assert(kOcKeep == kOcTile && kOcBlock == kOcEntries, "occurrences_common.hpp's tile and entry block are these");

// Units of kOcBlock entries (oc_unit).  counts[entry][tile] for every tile below a.tiles; any[u]: the unit has a match.
template <bool FULL>
__global__ __launch_bounds__(kOcThreads) void occurrences_count_kernel(const OcArgs a, uint32_t* __restrict__ counts,
                                                                       uint32_t* __restrict__ any) {
    extern __shared__ uint4 s_dyn[];
    __shared__ uint32_t s_any;
    const OcLds s = oc_lds(s_dyn, a.win);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    oc_load_tri(a, s);
    const uint32_t units = oc_units(a, kOcBlock);
    for (uint32_t u = blockIdx.x; u < units; u += gridDim.x) {
        const OcUnit n = oc_unit(a, u, kOcBlock, wave);
        __syncthreads();                                       // (the unit before has left the window and s_any)
        oc_stage(a, s, n.wb);
        if (threadIdx.x == 0u) s_any = 0u;
        __syncthreads();
        uint32_t some = 0u;
        if (n.tile < a.tiles) {
            const uint32_t first = n.tile * kOcKeep;
            for (uint32_t e = n.e0; e < n.e1; ++e) {
                const uint32_t c = oc_count_cells<FULL>(a, s, n.wb, e, first, lane);
                if (lane == 0u) counts[e * a.tiles + n.tile] = c;
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
    oc_load_tri(a, s);
    const uint32_t units = oc_units(a, kOcBlock);
    for (uint32_t u = blockIdx.x; u < units; u += gridDim.x) {
        if (any[u] == 0u) continue;                            // (the same word for the whole workgroup) nothing is loaded
        const OcUnit n = oc_unit(a, u, kOcBlock, wave);
        if (row_base[n.e0] >= capacity) continue;              // the list is full in front of this block
        oc_stage_unit(a, s, n.wb);
        if (n.tile >= a.tiles) continue;                       // (this wave meets no barrier of the unit any more)
        const uint32_t first = n.tile * kOcKeep;
        for (uint32_t e = n.e0; e < n.e1; ++e) {
            const uint32_t item = e * a.tiles + n.tile;
            if (__builtin_amdgcn_readfirstlane(counts[item]) == 0u) continue;
            const unsigned long long at = row_base[e] + tile_at[item];
            if (at >= capacity) continue;
            uint32_t rec0, ne;
            oc_entry(a, e, &rec0, &ne);
            const uint32_t o = first - 1u + 2u * lane;
            float q0, q1;
            const uint32_t m = oc_cells<FULL>(a, s, n.wb, rec0, ne, o, &q0, &q1);
            oc_emit(a, e, ne, m, o, o + 1u, q0, q1, at, capacity, key_base, keys, lags);
        }
    }
}

// (the scratch of a chunk: OcScratch with a row per entry of the chunk)
template <bool FULL>
hipError_t launch_oc(const OccurrencesCall& c, const OcScratch& s, const OcArgs& a, size_t lds, uint32_t first_chunk) {
    static size_t ready[kMaxDevices] = {};                     // (both kernels of this instance)
    const hipError_t e = oc_allow_lds(ready, lds, occurrences_count_kernel<FULL>, occurrences_scatter_kernel<FULL>);
    if (e != hipSuccess) return e;
    const dim3 grid = oc_grid(oc_blocks(a.entries) * a.groups);
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
    // (oc_call_ok's, and what ties the launch to the carved scratch and to the keys)
    if (!oc_call_ok(c, occurrences_tiles(c.n_query, c.ne_min, c.ne_max), first_entry, entries) || entries > chunk_entries_max ||
        c.index_base + first_entry + entries > 0x100000000ull)
        return hipErrorInvalidValue;
    size_t lds = 0;
    const OcArgs a = oc_args(c, first_entry, entries, c.threshold, c.peaks, &lds);
    if (!a.tri) return hipErrorOutOfMemory;
    const OcScratch s = oc_carve(d_scratch, chunk_entries_max, c.tiles);
    return c.range >= c.subfp_len ? launch_oc<true>(c, s, a, lds, first_chunk) : launch_oc<false>(c, s, a, lds, first_chunk);
}

}  // namespace lbad
