// k_recording_batch.hip -- recording scores and lags (k_recording.hip) for MANY recordings of one length in one call: for every
// recording r and entry j of a RAGGED corpus the largest cell of the pair's profile and the lowest offset that reaches it, row r
// what the single call gives for recording r alone, bit for bit.  The shape is a broadcast monitor's: hundreds to thousands of
// short windows (StreamBank.window_device's block) against a few thousand entries, where one recording alone gives the device a
// handful of workgroups.  The cells, the 64-bit values and the fold are k_recording.hip's; the pair loop is
// occurrences_common.hpp's as it is, cases A and B: an entry LONGER than the recordings takes part (the recording slides along
// it), which is where this pass differs from the batch timeline.  What is new is the batch coordinate, and with it the plan
// (recording_batch_plan, the ONE place that decides form, passes, chunks and scratch) and two forms of the maxima kernel:
//   form S   (shared window) k_recording.hip's mapping with the recording as one more coordinate of a unit: unit u = (entry block
//            of kOcEntries, recording of the pass, tile group), the entry block slowest, so that workgroups that run together
//            share the entries' records.  The unit's query is q + 2 x rec x per, for the window AND for case A's scalar reads.
//   form W   (window per wave) for recordings of fewer than kOcWaves tiles, where form S leaves waves without a tile: the tiles of
//            a pass are numbered through, gt = recording x tiles + tile, a unit is (entry block, kOcWaves consecutive global tiles)
//            and wave w takes gt = kOcWaves x g + w.  Every wave stages the kOcTile + 2 + longest-entry records its own tile needs,
//            of ITS recording, into its own sub-window between the unit's two barriers -- zero records at or beyond that
//            recording's length: nothing of a neighbouring recording reaches a cell.  A wave whose gt lies beyond the pass stages
//            zeros, meets both barriers and leaves.  Case A reads the query of the wave's own recording.
// Partials [recording of the pass][entry][tile], one writer (lane 0 of the item's wave) per word, 0 where the (entry, tile) has no
// offset of the pair; no atomics, no workgroup waits for another, nothing is zeroed in front.  The fold is k_recording.hip's with
// the recording on blockIdx.y; the lag gather is its gather over rows of K slots.
// Nothing is read beyond an entry's records plus one (inside kRecordSlack), or beyond the recordings' words.
#include "occurrences_common.hpp"

namespace lbad {
namespace {

constexpr uint32_t kRbFoldThreads = 256;
constexpr uint32_t kRbMaxRecs = 65535;                 // recordings of a pass: the fold's gridDim.y, the selection's rows
constexpr uint64_t kRbLdsBudget = 160 * 1024 - 64;     // occurrences_common.hpp's static assertion: a CU's LDS less 64 bytes

// k_recording.hip's rec_row_max / rec_wave_max (per file, as everything of the pair loop)
template <int ROR>
__device__ __forceinline__ unsigned long long rb_row_max(unsigned long long v) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, 0x120 + ROR /* row_ror:ROR */, 0xF, 0xF, true);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v >> 32), 0x120 + ROR, 0xF, 0xF, true);
    const unsigned long long o = ((unsigned long long)hi << 32) | lo;
    return o > v ? o : v;
}

// the wave's maximum, wave-uniform.  Called by whole waves.
__device__ __forceinline__ unsigned long long rb_wave_max(unsigned long long v) {
    v = rb_row_max<1>(v);
    v = rb_row_max<2>(v);
    v = rb_row_max<4>(v);
    v = rb_row_max<8>(v);                                      // every lane: its row's maximum
    unsigned long long best = 0ull;
#pragma unroll
    for (int row = 0; row < 4; ++row) {
        const unsigned long long r = ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), row * 16) << 32) |
                                     (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, row * 16);
        best = r > best ? r : best;
    }
    return best;
}

// The entries [e0, e1) of the chunk against one tile of one recording (a.q: that recording; its window staged in s from record wb
// on): the tile's maximum per entry to row[entry x tiles + tile], `row` the recording's partials.  recording_maxima_kernel's walk.
template <bool FULL>
__device__ __forceinline__ void rb_walk(const OcArgs& a, const OcLds& s, uint32_t wb, uint32_t tile, uint32_t e0, uint32_t e1,
                                        unsigned long long* __restrict__ row) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t first = tile * kOcTile;
    const uint32_t o = first - 1u + 2u * lane;
    for (uint32_t e = e0; e < e1; ++e) {
        uint32_t rec0, ne;
        oc_entry(a, e, &rec0, &ne);
        const uint32_t n_off = oc_offsets(a, ne);
        unsigned long long best = 0ull;
        if (first < n_off) {
            float q0, q1;
            (void)oc_cells<FULL>(a, s, wb, rec0, ne, o, &q0, &q1);
            // (lane 0's first and lane 63's second cell are the neighbouring tiles')
            const unsigned long long v0 = lane != 0u && o < n_off ? ((unsigned long long)__float_as_uint(q0) << 32) | (0xFFFFFFFFu - o) : 0ull;
            const unsigned long long v1 =
                lane != 63u && o + 1u < n_off ? ((unsigned long long)__float_as_uint(q1) << 32) | (0xFFFFFFFFu - (o + 1u)) : 0ull;
            best = rb_wave_max(v0 > v1 ? v0 : v1);
        }
        if (lane == 0u) row[(size_t)e * a.tiles + tile] = best;
    }
}

// Form S.  a.q: the pass' first recording, `recs` recordings of a.nq records each; a.win: the shared window.
template <bool FULL>
__global__ __launch_bounds__(kOcThreads) void recording_batch_shared_kernel(const OcArgs a, uint32_t recs,
                                                                           unsigned long long* __restrict__ partials) {
    extern __shared__ uint4 s_dyn[];
    const OcLds s = oc_lds(s_dyn, a.win);
    const uint32_t wave = threadIdx.x >> 6;
    oc_load_tri(a, s);
    const uint32_t blocks = (a.entries + kOcEntries - 1u) / kOcEntries;
    const uint32_t per_block = recs * a.groups;
    const uint32_t units = blocks * per_block;
    for (uint32_t u = blockIdx.x; u < units; u += gridDim.x) {
        const uint32_t eb = u / per_block;
        const uint32_t v = u - eb * per_block;
        const uint32_t rec = v / a.groups;
        const uint32_t g = v - rec * a.groups;
        OcArgs b = a;                                          // the unit's recording (wave-uniform): the window's and case A's query
        b.q = a.q + 2u * (size_t)rec * a.nq;
        const uint32_t wb = g * kOcTileGroup - 1u;
        const uint32_t tile = g * kOcWaves + wave;
        oc_stage_unit(b, s, wb);
        if (tile >= a.tiles) continue;                         // (this wave meets no barrier of the unit any more)
        const uint32_t e0 = eb * kOcEntries, e1 = a.entries - e0 < kOcEntries ? a.entries : e0 + kOcEntries;
        rb_walk<FULL>(b, s, wb, tile, e0, e1, partials + (size_t)rec * a.entries * a.tiles);
    }
}

// Form W.  a.win: records of ONE wave's sub-window (kOcTile + 2 + the longest entry); the LDS holds kOcWaves of them in each of
// the three arrays, then the table.
template <bool FULL>
__global__ __launch_bounds__(kOcThreads) void recording_batch_wave_kernel(const OcArgs a, uint32_t recs,
                                                                         unsigned long long* __restrict__ partials) {
    extern __shared__ uint4 s_dyn[];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    OcLds s;
    s.p = s_dyn + (size_t)wave * a.win;
    s.n = s_dyn + (size_t)(kOcWaves + wave) * a.win;
    uint32_t* const rows = reinterpret_cast<uint32_t*>(s_dyn + 2u * (size_t)kOcWaves * a.win);
    s.row = rows + (size_t)wave * a.win;
    s.tri = reinterpret_cast<float*>(rows + (size_t)kOcWaves * a.win);
    oc_load_tri(a, s);
    const uint32_t blocks = (a.entries + kOcEntries - 1u) / kOcEntries;
    const uint32_t gtiles = recs * a.tiles;
    const uint32_t ggroups = (gtiles + kOcWaves - 1u) / kOcWaves;
    const uint32_t units = blocks * ggroups;
    for (uint32_t u = blockIdx.x; u < units; u += gridDim.x) {
        const uint32_t eb = u / ggroups;
        const uint32_t gt = (u - eb * ggroups) * kOcWaves + wave;
        const bool active = gt < gtiles;
        const uint32_t rec = active ? gt / a.tiles : 0u, tile = active ? gt - rec * a.tiles : 0u;
        const uint32_t wb = tile * kOcTile - 1u;               // (wraps below 0 for tile 0, as oc_unit's)
        OcArgs b = a;                                          // the wave's recording: the sub-window's and case A's query
        b.q = a.q + 2u * (size_t)rec * a.nq;
        __syncthreads();                                       // (the unit before has left the windows)
        for (uint32_t r = lane; r < a.win; r += 64u) {
            const uint32_t qi = wb + r;
            OcRec f;
            f.p = make_uint4(0u, 0u, 0u, 0u);
            f.n = f.p;
            f.row = 0u;
            if (active && qi < a.nq) f = oc_prepare<false>(b.q[2u * (size_t)qi], b.q[2u * (size_t)qi + 1u], a.m);   // (qi < nq: inside THIS recording)
            s.p[r] = f.p;
            s.n[r] = f.n;
            s.row[r] = f.row;
        }
        __syncthreads();
        if (!active) continue;                                 // (behind the unit's second barrier)
        const uint32_t e0 = eb * kOcEntries, e1 = a.entries - e0 < kOcEntries ? a.entries : e0 + kOcEntries;
        rb_walk<FULL>(b, s, wb, tile, e0, e1, partials + (size_t)rec * a.entries * a.tiles);
    }
}

// recording_fold_kernel with the recording on blockIdx.y: an entry's partials of that recording -> scores[rec][first + e] and,
// where asked for, lags[rec][first + e] (rows of `pitch` words).  `lanes` (a power of two, 1 .. 64) neighbouring lanes share an
// entry; whole waves, the lanes of entries beyond the chunk hold 0.
__global__ __launch_bounds__(kRbFoldThreads) void recording_batch_fold_kernel(const unsigned long long* __restrict__ partials,
                                                                            const uint32_t* __restrict__ off, uint32_t first,
                                                                            uint32_t entries, uint32_t tiles, uint32_t lanes, uint32_t nq,
                                                                            uint64_t pitch, float* __restrict__ scores,
                                                                            int32_t* __restrict__ lags) {
    const uint64_t t = (uint64_t)blockIdx.x * kRbFoldThreads + threadIdx.x;
    const uint64_t e = t / lanes;
    const uint32_t sub = (uint32_t)(t - e * lanes);
    const unsigned long long* __restrict__ src = partials + (size_t)blockIdx.y * entries * tiles;
    unsigned long long best = 0ull;
    if (e < entries)
        for (uint32_t tile = sub; tile < tiles; tile += lanes) {
            const unsigned long long v = src[(size_t)e * tiles + tile];
            best = v > best ? v : best;
        }
    for (uint32_t d = lanes >> 1; d != 0u; d >>= 1) {
        const unsigned long long o = __shfl_xor(best, (int)d, 64);
        best = o > best ? o : best;
    }
    if (e >= entries || sub != 0u) return;
    // (tile 0 holds offset 0 of every pair: best's low word is 0xFFFFFFFF - o of a cell that exists)
    const size_t at = (size_t)blockIdx.y * pitch + first + e;
    scores[at] = __uint_as_float((uint32_t)(best >> 32));
    if (lags) {
        const uint32_t o = 0xFFFFFFFFu - (uint32_t)best;
        const uint32_t ne = off[first + e + 1u] - off[first + e];
        lags[at] = nq < ne ? (int32_t)o : -(int32_t)o;
    }
}

// lags[r][slot] = row r's lag of the entry keys[r][slot] names; a zero key, or an index outside the corpus, gives 0
__global__ __launch_bounds__(kRbFoldThreads) void recording_batch_lag_gather_kernel(const unsigned long long* __restrict__ keys, uint64_t n,
                                                                                  uint32_t k, uint32_t base, uint64_t count,
                                                                                  const int32_t* __restrict__ entry_lags,
                                                                                  int32_t* __restrict__ lags) {
    const uint64_t slot = (uint64_t)blockIdx.x * kRbFoldThreads + threadIdx.x;
    if (slot >= n) return;
    const uint64_t r = slot / k;
    const unsigned long long key = keys[slot];
    const uint32_t j = 0xFFFFFFFFu - (uint32_t)key - base;     // (the low word is 0xFFFFFFFF - (index base + j))
    lags[slot] = key != 0ull && j < count ? entry_lags[(size_t)r * count + j] : 0;
}

size_t rb_wave_lds(uint32_t ne_max) { return (size_t)kOcWaves * (kOcTile + 2u + ne_max) * kOcRecBytes + kTriSize * sizeof(float); }

template <bool FULL>
hipError_t launch_rb_maxima(uint32_t form, const OcArgs& a, size_t lds, uint32_t recs, unsigned long long* partials, hipStream_t stream) {
    static size_t ready[2][kMaxDevices] = {};                  // (this instance, per form)
    if (form == kRecordingBatchFormWave) {
        const hipError_t e = oc_allow_lds(ready[1], lds, recording_batch_wave_kernel<FULL>);
        if (e != hipSuccess) return e;
        const uint64_t ggroups = ((uint64_t)recs * a.tiles + kOcWaves - 1) / kOcWaves;
        hipLaunchKernelGGL(recording_batch_wave_kernel<FULL>, oc_grid(oc_blocks(a.entries) * ggroups), dim3(kOcThreads), lds, stream, a, recs,
                           partials);
    } else {
        const hipError_t e = oc_allow_lds(ready[0], lds, recording_batch_shared_kernel<FULL>);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(recording_batch_shared_kernel<FULL>, oc_grid(oc_blocks(a.entries) * recs * a.groups), dim3(kOcThreads), lds, stream,
                           a, recs, partials);
    }
    return hipGetLastError();
}

}  // namespace

bool recording_batch_plan(uint32_t recordings, uint32_t per, uint32_t ne_min, uint32_t ne_max, uint64_t entries, uint64_t limit_bytes,
                          bool key_form, bool force_shared, RecordingBatchPlan* plan) {
    *plan = RecordingBatchPlan();
    plan->form = kRecordingBatchFormShared;
    plan->tiles = 1;
    plan->recordings_per_pass = recordings;
    if (entries == 0) return true;
    const uint64_t limit = limit_bytes ? limit_bytes : kJoinScratchDefault;
    const uint64_t tiles = occurrences_tiles(per, ne_min, ne_max);
    // the entries of a chunk exactly as the single call has them (pass_plan)
    const uint64_t fit = recording_chunk_entries(tiles, limit);
    if (fit == 0) return false;                                // the limit holds no block of entries of ONE recording
    const uint64_t chunk = fit < entries ? fit : oc_blocks(entries) * kOcEntries;
    const uint64_t one = recording_scratch_bytes(chunk, tiles);
    uint64_t recs = 1;
    if (chunk >= entries) {                                    // one recording's whole-corpus partials fit: several recordings a pass
        recs = limit / one;
        const uint64_t items = kOcMaxItems / (entries * tiles);            // (>= 1: recording_chunk_entries kept the chunk within it)
        if (recs > items) recs = items;
        if (recs > kRbMaxRecs) recs = kRbMaxRecs;
        if (key_form) {                                        // a score and a lag per entry and row of the selection, under the same limit
            const uint64_t rows = limit / (entries * 8u);
            if (recs > rows) recs = rows ? rows : 1;
        }
        if (recs > recordings) recs = recordings;
    }
    plan->tiles = tiles;
    plan->recordings_per_pass = (uint32_t)recs;
    plan->entries_per_chunk = chunk;
    plan->scratch_bytes = recs * one;
    const size_t wave_lds = rb_wave_lds(ne_max);
    const bool wave = tiles < kOcWaves && wave_lds <= kRbLdsBudget && !force_shared;
    plan->form = wave ? kRecordingBatchFormWave : kRecordingBatchFormShared;
    plan->lds_bytes = wave ? wave_lds : occurrences_lds_bytes(per, ne_max);
    return true;
}

hipError_t launch_recording_batch_chunk(const RecordingCall& c, const RecordingBatchPlan& plan, uint32_t recordings, uint64_t pitch,
                                        void* d_scratch, uint64_t first_entry, uint64_t entries) {
    if (entries == 0 || recordings == 0) return hipSuccess;
    // (oc_call_ok's, and what ties the launch to the plan: the scratch, the 32-bit unit indices, the fold's grid, the rows)
    if (!oc_call_ok(c, occurrences_tiles(c.n_query, c.ne_min, c.ne_max), first_entry, entries) || plan.tiles != c.tiles ||
        recordings > plan.recordings_per_pass || recordings > kRbMaxRecs || entries > plan.entries_per_chunk ||
        (uint64_t)recordings * entries * c.tiles > kOcMaxItems || (uint64_t)recordings * c.n_query > 0x7FFFFFFFull ||
        (uint64_t)recordings * recording_scratch_bytes(entries, c.tiles) > plan.scratch_bytes || first_entry + entries > pitch || !c.d_scores)
        return hipErrorInvalidValue;
    size_t lds = 0;
    OcArgs a = oc_args(c, first_entry, entries, 0.0f, false, &lds);                // (no cell is tested here)
    if (!a.tri) return hipErrorOutOfMemory;
    if (plan.form == kRecordingBatchFormWave) {
        if (c.tiles >= kOcWaves || rb_wave_lds(c.ne_max) > kRbLdsBudget) return hipErrorInvalidValue;
        a.win = kOcTile + 2u + c.ne_max;
        lds = rb_wave_lds(c.ne_max);
    }
    if (lds != plan.lds_bytes) return hipErrorInvalidValue;
    unsigned long long* partials = static_cast<unsigned long long*>(d_scratch);
    const hipError_t e = c.range >= c.subfp_len ? launch_rb_maxima<true>(plan.form, a, lds, recordings, partials, c.stream)
                                                : launch_rb_maxima<false>(plan.form, a, lds, recordings, partials, c.stream);
    if (e != hipSuccess) return e;
    uint32_t lanes = 1;
    while (lanes < 64u && lanes < c.tiles) lanes <<= 1;
    const uint64_t threads = entries * lanes;
    hipLaunchKernelGGL(recording_batch_fold_kernel, dim3((uint32_t)((threads + kRbFoldThreads - 1) / kRbFoldThreads), recordings),
                       dim3(kRbFoldThreads), 0, c.stream, partials, c.d_off, a.first, a.entries, a.tiles, lanes, c.n_query, pitch, c.d_scores,
                       c.d_lags);
    return hipGetLastError();
}

hipError_t launch_recording_batch_lag_gather(const unsigned long long* d_keys, uint32_t rows, uint32_t k, uint64_t index_base, uint64_t count,
                                             const int32_t* d_entry_lags, int32_t* d_lags, hipStream_t stream) {
    const uint64_t n = (uint64_t)rows * k;
    if (n == 0) return hipSuccess;
    if (n > 0x80000000ull || index_base + count > 0x100000000ull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(recording_batch_lag_gather_kernel, dim3((uint32_t)((n + kRbFoldThreads - 1) / kRbFoldThreads)), dim3(kRbFoldThreads), 0,
                       stream, d_keys, n, k, (uint32_t)index_base, count, d_entry_lags, d_lags);
    return hipGetLastError();
}

}  // namespace lbad
