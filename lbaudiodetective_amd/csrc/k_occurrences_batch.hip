// k_occurrences_batch.hip -- occurrences (k_occurrences.hip) for MANY recordings of one length in one call: for every recording r
// every cell (entry, offset) of a RAGGED corpus at or above a threshold, as r's own list in (entry, offset) order with its own
// count, row r what the single call gives for recording r alone, bit for bit.  And the sibling question on the batch scores
// (k_recording_batch.hip): per recording every ENTRY whose best cell reaches a threshold, in ascending index.  The shape is a
// detection service's: a stream bank's windows against a few thousand entries, where one recording alone gives the device a
// handful of workgroups.  The cells, the match and peak rules and the keys are k_occurrences.hip's; the pair loop is
// occurrences_common.hpp's as it is (oc_cells, oc_stage, oc_unit's numbering, the any[] flags), cases A and B.  What is new is the
// batch coordinate in the count / scan / scatter compaction, the plan (occurrences_batch_plan, the ONE place that decides form,
// passes, chunks and scratch) and the two forms of the batch family:
//   form S   (shared window) the single call's unit with the recording as one more coordinate: unit u = (entry block of kOcEntries,
//            recording of the pass, tile group), the entry block slowest.  The unit's query is q + 2 x rec x per.
//   form W   (window per wave) for recordings of fewer than kOcWaves tiles: the tiles of a pass are numbered through, gt =
//            recording x tiles + tile, a unit is (entry block, kOcWaves consecutive global tiles) and wave w takes gt = kOcWaves x g
//            + w.  The staging is k_recording_batch.hip's: every wave stages the records of its own tile, of ITS recording, into its
//            own sub-window -- zero records at or beyond that recording's length.  A wave whose gt lies beyond the pass stages zeros,
//            meets the unit's barriers and leaves.
// counts[recording of the pass][entry][tile] are rows = recordings x entries of the joins' two scans (launch_join_scans, as they
// are): row_base[rec x entries + e] is the global position in the pass, a recording's slot is that less the position of its first
// entry, its count the difference of two neighbouring recordings' first positions (the scans' offsets hold the total behind the
// last row).  A pass of ONE recording may run in entry chunks with the single call's carried total: its slots are the global
// positions themselves.  No atomics on memory, no workgroup waits for another, one writer per output word; the scatter computes
// again only the items with a match and skips what lies behind a full row.
// The threshold compaction takes rows of scores: a wave per (recording, 64 entries) counts with a ballot, the same two scans run
// over rows = recordings with the entry tiles as columns, and the same mapping scatters -- a fixed number of launches per pass.
// Nothing is read beyond an entry's records plus one (inside kRecordSlack), or beyond the recordings' words; every loop is bounded
// by lengths from the record positions, clamped to the corpus' longest entry, or by a count the host has checked.
#include "occurrences_common.hpp"

namespace lbad {
namespace {

constexpr uint64_t kObLdsBudget = 160 * 1024 - 64;     // occurrences_common.hpp's static assertion: a CU's LDS less 64 bytes
constexpr uint32_t kObThreads = 256;                   // the small kernels
constexpr uint32_t kObScoreTile = 64;                  // entries of a (recording, entry tile) of the threshold compaction: a wave's

// what a batch kernel needs beside OcArgs
struct ObPass {
    uint32_t recs;                // recordings of the pass, a.nq records each from a.q on
    uint32_t chunked;             // a pass of one recording in entry chunks: slots are the global positions
};

// a wave's place in a unit
struct ObUnit {
    uint32_t eb, rec, tile, wb;
    bool active;                  // the wave has an item of the pass
};

// form S: every wave of the unit shares the recording and the window; tile >= a.tiles: no item
__device__ __forceinline__ ObUnit ob_unit_shared(const OcArgs& a, uint32_t recs, uint32_t u, uint32_t wave) {
    const uint32_t per_block = recs * a.groups;
    ObUnit n;
    n.eb = u / per_block;
    const uint32_t v = u - n.eb * per_block;
    n.rec = v / a.groups;
    const uint32_t g = v - n.rec * a.groups;
    n.wb = g * kOcTileGroup - 1u;
    n.tile = g * kOcWaves + wave;
    n.active = n.tile < a.tiles;
    return n;
}

// form W: the wave's own global tile
__device__ __forceinline__ ObUnit ob_unit_wave(const OcArgs& a, uint32_t recs, uint32_t u, uint32_t wave) {
    const uint32_t gtiles = recs * a.tiles;
    const uint32_t ggroups = (gtiles + kOcWaves - 1u) / kOcWaves;
    ObUnit n;
    n.eb = u / ggroups;
    const uint32_t gt = (u - n.eb * ggroups) * kOcWaves + wave;
    n.active = gt < gtiles;
    n.rec = n.active ? gt / a.tiles : 0u;
    n.tile = n.active ? gt - n.rec * a.tiles : 0u;
    n.wb = n.tile * kOcTile - 1u;                              // (wraps below 0 for tile 0, as oc_unit's)
    return n;
}

template <bool WAVE>
__device__ __forceinline__ uint32_t ob_units(const OcArgs& a, uint32_t recs) {
    const uint32_t blocks = (a.entries + kOcEntries - 1u) / kOcEntries;
    return WAVE ? blocks * ((recs * a.tiles + kOcWaves - 1u) / kOcWaves) : blocks * recs * a.groups;
}

// the LDS of a wave.  Form S: oc_lds.  Form W: a.win records of ONE wave's sub-window; the LDS holds kOcWaves of them in each of the
// three arrays, then the table (k_recording_batch.hip's layout)
template <bool WAVE>
__device__ __forceinline__ OcLds ob_lds(uint4* dyn, uint32_t win, uint32_t wave) {
    if (!WAVE) return oc_lds(dyn, win);
    OcLds s;
    s.p = dyn + (size_t)wave * win;
    s.n = dyn + (size_t)(kOcWaves + wave) * win;
    uint32_t* const rows = reinterpret_cast<uint32_t*>(dyn + 2u * (size_t)kOcWaves * win);
    s.row = rows + (size_t)wave * win;
    s.tri = reinterpret_cast<float*>(rows + (size_t)kOcWaves * win);
    return s;
}

// the window(s) of a unit, between the caller's two barriers.  b: the wave's recording.  `want`: form W stages zeros otherwise
template <bool WAVE>
__device__ __forceinline__ void ob_stage(const OcArgs& b, const OcLds& s, uint32_t wb, bool want) {
    if (!WAVE) {
        oc_stage(b, s, wb);
        return;
    }
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t r = lane; r < b.win; r += 64u) {
        const uint32_t qi = wb + r;
        OcRec f;
        f.p = make_uint4(0u, 0u, 0u, 0u);
        f.n = f.p;
        f.row = 0u;
        if (want && qi < b.nq) f = oc_prepare<false>(b.q[2u * (size_t)qi], b.q[2u * (size_t)qi + 1u], b.m);   // (qi < nq: inside THIS recording)
        s.p[r] = f.p;
        s.n[r] = f.n;
        s.row[r] = f.row;
    }
}

// counts[rec][entry][tile] for every tile below a.tiles; any[u]: the unit has a match
template <bool FULL, bool WAVE>
__global__ __launch_bounds__(kOcThreads) void occurrences_batch_count_kernel(const OcArgs a, const ObPass p, uint32_t* __restrict__ counts,
                                                                             uint32_t* __restrict__ any) {
    extern __shared__ uint4 s_dyn[];
    __shared__ uint32_t s_any;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const OcLds s = ob_lds<WAVE>(s_dyn, a.win, wave);
    oc_load_tri(a, s);
    const uint32_t units = ob_units<WAVE>(a, p.recs);
    for (uint32_t u = blockIdx.x; u < units; u += gridDim.x) {
        const ObUnit n = WAVE ? ob_unit_wave(a, p.recs, u, wave) : ob_unit_shared(a, p.recs, u, wave);
        OcArgs b = a;                                          // the wave's recording: the window's and case A's query
        b.q = a.q + 2u * (size_t)n.rec * a.nq;
        __syncthreads();                                       // (the unit before has left the windows and s_any)
        ob_stage<WAVE>(b, s, n.wb, n.active);
        if (threadIdx.x == 0u) s_any = 0u;
        __syncthreads();
        uint32_t some = 0u;
        if (n.active) {
            const uint32_t first = n.tile * kOcTile;
            const uint32_t e0 = n.eb * kOcEntries, e1 = a.entries - e0 < kOcEntries ? a.entries : e0 + kOcEntries;
            uint32_t* __restrict__ row = counts + (size_t)n.rec * a.entries * a.tiles;
            for (uint32_t e = e0; e < e1; ++e) {
                const uint32_t c = oc_count_cells<FULL>(b, s, n.wb, e, first, lane);
                if (lane == 0u) row[(size_t)e * a.tiles + n.tile] = c;
                some |= c;
            }
        }
        if (lane == 0u && some) atomicOr(&s_any, 1u);          // (LDS: a flag, whoever sets it)
        __syncthreads();
        if (threadIdx.x == 0u) any[u] = s_any;
    }
}

// keys / lags: row 0 of the pass, rows `capacity` slots apart
template <bool FULL, bool WAVE>
__global__ __launch_bounds__(kOcThreads) void occurrences_batch_scatter_kernel(const OcArgs a, const ObPass p,
                                                                               const uint32_t* __restrict__ counts,
                                                                               const uint32_t* __restrict__ any,
                                                                               const uint32_t* __restrict__ tile_at,
                                                                               const unsigned long long* __restrict__ row_base,
                                                                               unsigned long long capacity, uint32_t key_base,
                                                                               unsigned long long* __restrict__ keys,
                                                                               int32_t* __restrict__ lags) {
    // (key_base = 0xFFFFFFFF - the low word of the index base - the chunk's first entry: a key's low word is key_base - e)
    extern __shared__ uint4 s_dyn[];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const OcLds s = ob_lds<WAVE>(s_dyn, a.win, wave);
    oc_load_tri(a, s);
    const uint32_t units = ob_units<WAVE>(a, p.recs);
    for (uint32_t u = blockIdx.x; u < units; u += gridDim.x) {
        if (any[u] == 0u) continue;                            // (the same word for the whole workgroup) nothing is loaded
        const ObUnit n = WAVE ? ob_unit_wave(a, p.recs, u, wave) : ob_unit_shared(a, p.recs, u, wave);
        const uint32_t row0 = n.rec * a.entries;               // the recording's first row of the scans
        const uint32_t e0 = n.eb * kOcEntries, e1 = a.entries - e0 < kOcEntries ? a.entries : e0 + kOcEntries;
        // the recording's first position in the pass; its list is full in front of this block of entries?
        const unsigned long long base = p.chunked ? 0ull : row_base[row0];
        const bool full = row_base[row0 + e0] - base >= capacity;
        if (!WAVE && full) continue;                           // (form S: the same recording for the whole workgroup)
        OcArgs b = a;
        b.q = a.q + 2u * (size_t)n.rec * a.nq;
        __syncthreads();                                       // (the unit before has left the windows)
        ob_stage<WAVE>(b, s, n.wb, n.active && !full);
        __syncthreads();
        if (!n.active || full) continue;                       // (this wave meets no barrier of the unit any more)
        const uint32_t first = n.tile * kOcTile;
        unsigned long long* __restrict__ out_keys = keys + (size_t)n.rec * capacity;
        int32_t* __restrict__ out_lags = lags ? lags + (size_t)n.rec * capacity : nullptr;
        for (uint32_t e = e0; e < e1; ++e) {
            const size_t item = (size_t)(row0 + e) * a.tiles + n.tile;
            if (__builtin_amdgcn_readfirstlane(counts[item]) == 0u) continue;
            const unsigned long long at = row_base[row0 + e] - base + tile_at[item];
            if (at >= capacity) continue;
            uint32_t rec0, ne;
            oc_entry(a, e, &rec0, &ne);
            const uint32_t o = first - 1u + 2u * lane;
            float q0, q1;
            const uint32_t m = oc_cells<FULL>(b, s, n.wb, rec0, ne, o, &q0, &q1);
            oc_emit(a, e, ne, m, o, o + 1u, q0, q1, at, capacity, key_base, out_keys, out_lags);
        }
    }
}

// out_counts[r] = the recording's matches: the difference of two neighbouring recordings' first positions (offsets[rows]: the total)
__global__ __launch_bounds__(kObThreads) void occurrences_batch_totals_kernel(const unsigned long long* __restrict__ offsets, uint32_t recs,
                                                                             uint32_t stride, unsigned long long* __restrict__ out_counts) {
    const uint32_t r = blockIdx.x * kObThreads + threadIdx.x;
    if (r < recs) out_counts[r] = offsets[(size_t)(r + 1u) * stride] - offsets[(size_t)r * stride];
}

// The threshold compaction.  Item (recording, tile of kObScoreTile entries) per wave, items numbered through over the grid's waves.
// counts[rec][tile]: the tile's scores >= t (a float compare: NaN never)
__global__ __launch_bounds__(kObThreads) void threshold_batch_count_kernel(const float* __restrict__ scores, uint32_t n, uint32_t recs,
                                                                          uint32_t etiles, float t, uint32_t* __restrict__ counts) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t waves = gridDim.x * (kObThreads / 64u);
    const uint32_t items = recs * etiles;
    for (uint32_t w = blockIdx.x * (kObThreads / 64u) + (threadIdx.x >> 6); w < items; w += waves) {
        const uint32_t rec = w / etiles;
        const uint32_t e = (w - rec * etiles) * kObScoreTile + lane;
        const bool m = e < n && scores[(size_t)rec * n + e] >= t;
        const uint32_t c = (uint32_t)__popcll(__ballot(m));
        if (lane == 0u) counts[w] = c;
    }
}

// the same items: a match's key to slot tile_at + matches in lower lanes where that is below the capacity; the wave of a
// recording's tile 0 writes its count
__global__ __launch_bounds__(kObThreads) void threshold_batch_scatter_kernel(const float* __restrict__ scores, uint32_t n, uint32_t recs,
                                                                            uint32_t etiles, float t, const uint32_t* __restrict__ counts,
                                                                            const uint32_t* __restrict__ tile_at,
                                                                            const unsigned long long* __restrict__ offsets,
                                                                            unsigned long long capacity, uint32_t key_base,
                                                                            unsigned long long* __restrict__ keys,
                                                                            unsigned long long* __restrict__ out_counts) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t waves = gridDim.x * (kObThreads / 64u);
    const uint32_t items = recs * etiles;
    for (uint32_t w = blockIdx.x * (kObThreads / 64u) + (threadIdx.x >> 6); w < items; w += waves) {
        const uint32_t rec = w / etiles;
        const uint32_t tile = w - rec * etiles;
        if (tile == 0u && lane == 0u) out_counts[rec] = offsets[rec + 1u] - offsets[rec];
        if (counts[w] == 0u) continue;
        const uint32_t at = tile_at[w];
        if (at >= capacity) continue;
        const uint32_t e = tile * kObScoreTile + lane;
        const float v = e < n ? scores[(size_t)rec * n + e] : 0.0f;
        const bool m = e < n && v >= t;
        const unsigned long long bal = __ballot(m);
        const unsigned long long slot =
            (unsigned long long)at + __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
        if (m && slot < capacity)
            keys[(size_t)rec * capacity + slot] = ((unsigned long long)__float_as_uint(v) << 32) | (unsigned long long)(key_base - e);
    }
}

// (the scratch of a pass: OcScratch with a row per (recording, entry); with one recording k_occurrences.hip's)
size_t ob_wave_lds(uint32_t ne_max) { return (size_t)kOcWaves * (kOcTile + 2u + ne_max) * kOcRecBytes + kTriSize * sizeof(float); }

template <bool FULL, bool WAVE>
hipError_t launch_ob(const OccurrencesCall& c, const OcScratch& s, const OcArgs& a, const ObPass& p, size_t lds, uint32_t first_chunk,
                     unsigned long long* d_counts) {
    static size_t ready[kMaxDevices] = {};                     // (both kernels of this instance)
    const hipError_t e = oc_allow_lds(ready, lds, occurrences_batch_count_kernel<FULL, WAVE>, occurrences_batch_scatter_kernel<FULL, WAVE>);
    if (e != hipSuccess) return e;
    const uint64_t units = WAVE ? oc_blocks(a.entries) * (((uint64_t)p.recs * a.tiles + kOcWaves - 1) / kOcWaves)
                                : oc_blocks(a.entries) * p.recs * a.groups;
    const dim3 grid = oc_grid(units);
    const uint32_t rows = p.recs * a.entries;
    hipLaunchKernelGGL((occurrences_batch_count_kernel<FULL, WAVE>), grid, dim3(kOcThreads), lds, c.stream, a, p, s.counts, s.any);
    launch_join_scans(s.counts, a.tiles, rows, s.tile_at, s.row_base, s.state, first_chunk, s.offsets, c.stream);
    hipLaunchKernelGGL((occurrences_batch_scatter_kernel<FULL, WAVE>), grid, dim3(kOcThreads), lds, c.stream, a, p, s.counts, s.any,
                       s.tile_at, s.row_base, (unsigned long long)c.capacity, 0xFFFFFFFFu - (uint32_t)c.index_base - a.first, c.d_keys,
                       c.d_lags);
    if (!p.chunked) return launch_occurrences_totals(s.offsets, p.recs, a.entries, d_counts, c.stream);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_occurrences_totals(const unsigned long long* d_offsets, uint32_t recordings, uint32_t stride, unsigned long long* d_counts,
                                     hipStream_t stream) {
    hipLaunchKernelGGL(occurrences_batch_totals_kernel, dim3((recordings + kObThreads - 1) / kObThreads), dim3(kObThreads), 0, stream,
                       d_offsets, recordings, stride, d_counts);
    return hipGetLastError();
}

bool occurrences_batch_plan(uint32_t recordings, uint32_t per, uint32_t ne_min, uint32_t ne_max, uint64_t entries, uint64_t limit_bytes,
                            bool force_shared, OccurrencesBatchPlan* plan) {
    *plan = OccurrencesBatchPlan();
    plan->form = kOccurrencesBatchFormShared;
    plan->tiles = 1;
    plan->recordings_per_pass = recordings;
    if (entries == 0) return true;
    const uint64_t limit = limit_bytes ? limit_bytes : kJoinScratchDefault;
    const uint64_t tiles = occurrences_tiles(per, ne_min, ne_max);
    // the entries of a chunk exactly as the single call has them (pass_plan)
    const uint64_t fit = occurrences_chunk_entries(tiles, limit);
    if (fit == 0) return false;                                // the limit holds no block of entries of ONE recording
    const uint64_t chunk = fit < entries ? fit : oc_blocks(entries) * kOcEntries;
    const uint64_t one = occurrences_scratch_bytes(chunk, tiles);
    uint64_t recs = 1;
    if (chunk >= entries) {                                    // one recording's whole-corpus scratch fits: several recordings a pass
        recs = limit / one;
        const uint64_t items = kOcMaxItems / (entries * tiles);            // (>= 1: occurrences_chunk_entries kept the chunk within it)
        if (recs > items) recs = items;
        if (recs > kOcMaxRecs) recs = kOcMaxRecs;
        if (recs > recordings) recs = recordings;
    }
    plan->tiles = tiles;
    plan->recordings_per_pass = (uint32_t)recs;
    plan->entries_per_chunk = chunk;
    plan->scratch_bytes = recs * one;
    const size_t wave_lds = ob_wave_lds(ne_max);
    const bool wave = tiles < kOcWaves && wave_lds <= kObLdsBudget && !force_shared;
    plan->form = wave ? kOccurrencesBatchFormWave : kOccurrencesBatchFormShared;
    plan->lds_bytes = wave ? wave_lds : occurrences_lds_bytes(per, ne_max);
    return true;
}

hipError_t launch_occurrences_batch_chunk(const OccurrencesCall& c, const OccurrencesBatchPlan& plan, uint32_t recordings, void* d_scratch,
                                          uint64_t first_entry, uint64_t entries, uint32_t first_chunk, unsigned long long* d_counts) {
    if (entries == 0 || recordings == 0) return hipSuccess;
    const bool chunked = plan.recordings_per_pass == 1;
    // (oc_call_ok's, and what ties the launch to the plan: oc_rows_call_ok's)
    if (!oc_call_ok(c, occurrences_tiles(c.n_query, c.ne_min, c.ne_max), first_entry, entries) || plan.tiles != c.tiles ||
        !oc_rows_call_ok(c, plan, recordings, first_entry, entries, first_chunk, d_counts))
        return hipErrorInvalidValue;
    size_t lds = 0;
    OcArgs a = oc_args(c, first_entry, entries, c.threshold, c.peaks, &lds);
    if (!a.tri) return hipErrorOutOfMemory;
    const bool wave = plan.form == kOccurrencesBatchFormWave;
    if (wave) {
        if (c.tiles >= kOcWaves || ob_wave_lds(c.ne_max) > kObLdsBudget) return hipErrorInvalidValue;
        a.win = kOcTile + 2u + c.ne_max;
        lds = ob_wave_lds(c.ne_max);
    }
    if (lds != plan.lds_bytes) return hipErrorInvalidValue;
    ObPass p;
    p.recs = recordings; p.chunked = chunked ? 1u : 0u;
    // (a chunked pass keeps ONE carving for all its chunks: the state word is carried)
    const OcScratch s = oc_carve(d_scratch, chunked ? plan.entries_per_chunk : (uint64_t)recordings * entries, c.tiles);
    const bool full = c.range >= c.subfp_len;
    if (wave) return full ? launch_ob<true, true>(c, s, a, p, lds, first_chunk, d_counts) : launch_ob<false, true>(c, s, a, p, lds, first_chunk, d_counts);
    return full ? launch_ob<true, false>(c, s, a, p, lds, first_chunk, d_counts) : launch_ob<false, false>(c, s, a, p, lds, first_chunk, d_counts);
}

size_t threshold_batch_scratch_bytes(uint64_t entries, uint32_t rows) {
    const uint64_t etiles = (entries + kObScoreTile - 1) / kObScoreTile;
    return (size_t)(8u * (2u + 2u * (uint64_t)rows + 1u) + 8u * (uint64_t)rows * etiles);
}

hipError_t launch_threshold_batch_keys(const float* d_scores, uint64_t n, uint32_t rows, float threshold, uint64_t capacity,
                                       uint64_t index_base, void* d_scratch, unsigned long long* d_keys, unsigned long long* d_counts,
                                       hipStream_t stream) {
    if (rows == 0) return hipSuccess;
    const uint64_t etiles = (n + kObScoreTile - 1) / kObScoreTile;
    if (!(threshold > 0.0f) || capacity == 0 || n == 0 || n > 0xFFFFFFFFull || index_base + n > 0x100000000ull || rows > kOcMaxRecs ||
        (uint64_t)rows * etiles > 0x7FFFFFFFull || (uint64_t)rows * capacity > 0x80000000ull)
        return hipErrorInvalidValue;
    unsigned long long* state = static_cast<unsigned long long*>(d_scratch);
    unsigned long long* row_base = state + 2;
    unsigned long long* offsets = row_base + rows;
    uint32_t* counts = reinterpret_cast<uint32_t*>(offsets + rows + 1);
    uint32_t* tile_at = counts + (size_t)rows * etiles;
    const uint64_t groups = ((uint64_t)rows * etiles + kObThreads / 64 - 1) / (kObThreads / 64);
    const dim3 grid(strided_grid(groups, kOcMaxGrid));
    hipLaunchKernelGGL(threshold_batch_count_kernel, grid, dim3(kObThreads), 0, stream, d_scores, (uint32_t)n, rows, (uint32_t)etiles, threshold,
                       counts);
    launch_join_scans(counts, etiles, rows, tile_at, row_base, state, 1u, offsets, stream);
    hipLaunchKernelGGL(threshold_batch_scatter_kernel, grid, dim3(kObThreads), 0, stream, d_scores, (uint32_t)n, rows, (uint32_t)etiles,
                       threshold, counts, tile_at, offsets, (unsigned long long)capacity, 0xFFFFFFFFu - (uint32_t)index_base, d_keys, d_counts);
    return hipGetLastError();
}

}  // namespace lbad
