// k_timeline_batch.hip -- the recording timeline (k_timeline.hip) for MANY recordings of one length in one call: the best entry of
// a RAGGED corpus at every offset of every recording, row r what the single call gives for recording r alone, bit for bit.  The
// shape is a broadcast monitor's: hundreds to thousands of short windows (StreamBank.window_device's block) against a few thousand
// entries, where one recording alone gives the device a handful of workgroups.  The cells, the keys and the fold are
// k_timeline.hip's; the pair loop is occurrences_common.hpp's as it is.  What is new is the batch coordinate, and with it the plan
// (timeline_batch_plan, the ONE place that decides form, passes, chunks and scratch) and two forms of the maxima kernel:
//   form S   (shared window) k_timeline.hip's mapping with the recording as one more coordinate of a unit: unit u = (entry block,
//            recording of the pass, tile group), the entry block slowest, so that workgroups that run together share the entries'
//            records.  The four waves share one window of kOcTileGroup + 2 + min(longest entry, recording) records of ONE recording.
//   form W   (window per wave) for recordings of fewer than kOcWaves tiles, where form S leaves waves without a tile: the tiles of
//            a pass are numbered through, gt = recording x tiles + tile, a unit is (entry block, kOcWaves consecutive global tiles)
//            and wave w takes gt = kOcWaves x g + w.  Every wave stages the kOcTile + 2 + longest-entry records its own tile needs,
//            of ITS recording, into its own sub-window between the unit's two barriers -- zero records wherever that recording has
//            none: the bound is the recording's length, not the packed block's, so nothing of a neighbouring recording is ever
//            read into a cell.  A wave whose gt lies beyond the pass stages zeros and still meets both barriers.
// Partials [recording of the pass][entry block][tiles x 126], every word below the call's tiles written by exactly one lane (0
// where nothing counted); no atomics, no workgroup waits for another.  The fold is k_timeline.hip's with the recording on
// blockIdx.z, one or two levels by the same rule; the lengths are k_timeline.hip's kernel over all the keys.
// Nothing is read beyond an entry's records plus one (inside kRecordSlack), or beyond the recordings' words.
#include "occurrences_common.hpp"

namespace lbad {
namespace {

constexpr uint32_t kTbEntries = 128;                   // entries a unit walks: k_timeline.hip's kTlEntries (timeline_block_entries())
constexpr uint32_t kTbFoldThreads = 256;
constexpr uint32_t kTbFoldWaves = kTbFoldThreads / 64;
constexpr uint32_t kTbFoldRows = 32;                   // k_timeline.hip's kTlFoldRows / kTlFoldSlices: the same one- or two-level rule
constexpr uint32_t kTbFoldSlices = 1024;
constexpr uint32_t kTbMaxGridZ = 65535;                // recordings of a pass: the fold's gridDim.z
constexpr uint64_t kTbLdsBudget = 160 * 1024 - 64;     // occurrences_common.hpp's static assertion: a CU's LDS less 64 bytes

// The entries [e0, e1) of the chunk against one tile of one recording whose window is staged in s from record wb on: the lane's
// two running maxima stored to `row`, the tile's 126 words of the partials.  k_timeline.hip's walk.
template <bool FULL>
__device__ __forceinline__ void tb_walk(const OcArgs& a, const OcLds& s, uint32_t wb, uint32_t tile, uint32_t e0, uint32_t e1,
                                        uint32_t key_low, unsigned long long* __restrict__ row) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t first = tile * kOcTile;
    const uint32_t o = first - 1u + 2u * lane;
    unsigned long long best0 = 0ull, best1 = 0ull;
    for (uint32_t e = e0; e < e1; ++e) {
        uint32_t rec0, ne;
        oc_entry(a, e, &rec0, &ne);
        if (ne > a.nq || first >= a.nq - ne + 1u) continue;                // (wave-uniform: no place inside the recording, or none in this tile)
        float q0, q1;
        const uint32_t bits = oc_cells<FULL>(a, s, wb, rec0, ne, o, &q0, &q1);
        const uint32_t low = key_low - e;
        const unsigned long long v0 = bits & 1u ? ((unsigned long long)__float_as_uint(q0) << 32) | low : 0ull;
        const unsigned long long v1 = bits & 2u ? ((unsigned long long)__float_as_uint(q1) << 32) | low : 0ull;
        best0 = v0 > best0 ? v0 : best0;
        best1 = v1 > best1 ? v1 : best1;
    }
    if (lane != 0u) row[2u * lane - 1u] = best0;
    if (lane != 63u) row[2u * lane] = best1;
}

// Form S.  a.q: the pass' first recording, `recs` recordings of a.nq records each; a.win: the shared window.
template <bool FULL>
__global__ __launch_bounds__(kOcThreads) void timeline_batch_shared_kernel(const OcArgs a, uint32_t recs, uint32_t key_low,
                                                                          unsigned long long* __restrict__ partials) {
    extern __shared__ uint4 s_dyn[];
    const OcLds s = oc_lds(s_dyn, a.win);
    const uint32_t wave = threadIdx.x >> 6;
    oc_load_tri(a, s);
    const uint32_t blocks = (a.entries + kTbEntries - 1u) / kTbEntries;
    const uint32_t per_block = recs * a.groups;
    const uint32_t units = blocks * per_block;
    for (uint32_t u = blockIdx.x; u < units; u += gridDim.x) {
        const uint32_t eb = u / per_block;
        const uint32_t v = u - eb * per_block;
        const uint32_t rec = v / a.groups;
        const uint32_t g = v - rec * a.groups;
        OcArgs b = a;                                          // the unit's recording (wave-uniform)
        b.q = a.q + 2u * (size_t)rec * a.nq;
        const uint32_t wb = g * kOcTileGroup - 1u;
        const uint32_t tile = g * kOcWaves + wave;
        oc_stage_unit(b, s, wb);
        if (tile >= a.tiles) continue;                         // (this wave meets no barrier of the unit any more)
        const uint32_t e0 = eb * kTbEntries, e1 = a.entries - e0 < kTbEntries ? a.entries : e0 + kTbEntries;
        tb_walk<FULL>(b, s, wb, tile, e0, e1, key_low, partials + (((size_t)rec * blocks + eb) * a.tiles + tile) * kOcTile);
    }
}

// Form W.  a.win: records of ONE wave's sub-window (kOcTile + 2 + the longest entry); the LDS holds kOcWaves of them in each of
// the three arrays, then the table.
template <bool FULL>
__global__ __launch_bounds__(kOcThreads) void timeline_batch_wave_kernel(const OcArgs a, uint32_t recs, uint32_t key_low,
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
    const uint32_t blocks = (a.entries + kTbEntries - 1u) / kTbEntries;
    const uint32_t gtiles = recs * a.tiles;
    const uint32_t ggroups = (gtiles + kOcWaves - 1u) / kOcWaves;
    const uint32_t units = blocks * ggroups;
    for (uint32_t u = blockIdx.x; u < units; u += gridDim.x) {
        const uint32_t eb = u / ggroups;
        const uint32_t gt = (u - eb * ggroups) * kOcWaves + wave;
        const bool active = gt < gtiles;
        const uint32_t rec = gt / a.tiles, tile = gt - rec * a.tiles;
        const uint32_t wb = tile * kOcTile - 1u;               // (wraps below 0 for tile 0, as oc_unit's)
        const uint4* __restrict__ q = a.q + 2u * (size_t)rec * a.nq;
        __syncthreads();                                       // (the unit before has left the windows)
        for (uint32_t r = lane; r < a.win; r += 64u) {
            const uint32_t qi = wb + r;
            OcRec f;
            f.p = make_uint4(0u, 0u, 0u, 0u);
            f.n = f.p;
            f.row = 0u;
            if (active && qi < a.nq) f = oc_prepare<false>(q[2u * (size_t)qi], q[2u * (size_t)qi + 1u], a.m);   // (qi < nq: inside THIS recording)
            s.p[r] = f.p;
            s.n[r] = f.n;
            s.row[r] = f.row;
        }
        __syncthreads();
        if (!active) continue;                                 // (behind the unit's second barrier)
        const uint32_t e0 = eb * kTbEntries, e1 = a.entries - e0 < kTbEntries ? a.entries : e0 + kTbEntries;
        tb_walk<FULL>(a, s, wb, tile, e0, e1, key_low, partials + (((size_t)rec * blocks + eb) * a.tiles + tile) * kOcTile);
    }
}

// k_timeline.hip's fold with the recording on blockIdx.z: src_rec / dst_rec words from one recording to the next
__global__ __launch_bounds__(kTbFoldThreads) void timeline_batch_fold_kernel(unsigned long long* src, uint32_t rows, uint32_t rows_per,
                                                                             uint64_t stride, uint64_t src_rec, uint32_t n,
                                                                             unsigned long long* dst, uint64_t dst_rec) {
    __shared__ unsigned long long s_best[kTbFoldWaves][64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t o = blockIdx.x * 64u + lane;
    const uint32_t r0 = blockIdx.y * rows_per, r1 = rows - r0 < rows_per ? rows : r0 + rows_per;
    src += (size_t)blockIdx.z * src_rec;
    unsigned long long best = 0ull;
    if (o < n)
        for (uint32_t r = r0 + wave; r < r1; r += kTbFoldWaves) {
            const unsigned long long v = src[(size_t)r * stride + o];
            best = v > best ? v : best;
        }
    s_best[wave][lane] = best;
    __syncthreads();                                           // (every thread of the workgroup is here)
    if (wave != 0u || o >= n) return;
#pragma unroll
    for (uint32_t w = 1; w < kTbFoldWaves; ++w) best = s_best[w][lane] > best ? s_best[w][lane] : best;
    if (dst) {
        unsigned long long* const d = dst + (size_t)blockIdx.z * dst_rec;
        const unsigned long long old = d[o];
        d[o] = old > best ? old : best;
    } else {
        src[(size_t)r0 * stride + o] = best;                   // (row r0's word o: read above by this very lane, by nobody else)
    }
}

inline uint64_t tb_blocks(uint64_t entries) { return (entries + kTbEntries - 1) / kTbEntries; }

size_t tb_wave_lds(uint32_t ne_max) { return (size_t)kOcWaves * (kOcTile + 2u + ne_max) * kOcRecBytes + kTriSize * sizeof(float); }

template <bool FULL>
hipError_t launch_tb_maxima(uint32_t form, const OcArgs& a, size_t lds, uint32_t recs, uint32_t key_low, unsigned long long* partials,
                            hipStream_t stream) {
    static size_t ready[2][kMaxDevices] = {};                  // (this instance, per form)
    if (form == kTimelineBatchFormWave) {
        const hipError_t e = oc_allow_lds(ready[1], lds, timeline_batch_wave_kernel<FULL>);
        if (e != hipSuccess) return e;
        const uint64_t ggroups = ((uint64_t)recs * a.tiles + kOcWaves - 1) / kOcWaves;
        hipLaunchKernelGGL(timeline_batch_wave_kernel<FULL>, oc_grid(tb_blocks(a.entries) * ggroups), dim3(kOcThreads), lds, stream, a, recs,
                           key_low, partials);
    } else {
        const hipError_t e = oc_allow_lds(ready[0], lds, timeline_batch_shared_kernel<FULL>);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(timeline_batch_shared_kernel<FULL>, oc_grid(tb_blocks(a.entries) * recs * a.groups), dim3(kOcThreads), lds, stream,
                           a, recs, key_low, partials);
    }
    return hipGetLastError();
}

}  // namespace

bool timeline_batch_plan(uint32_t recordings, uint32_t per, uint32_t ne_min, uint32_t ne_max, uint64_t entries, uint64_t limit_bytes,
                         bool force_shared, TimelineBatchPlan* plan) {
    *plan = TimelineBatchPlan();
    plan->form = kTimelineBatchFormShared;
    plan->tiles = 1;
    plan->recordings_per_pass = recordings;
    if (entries == 0) return true;
    const uint64_t limit = limit_bytes ? limit_bytes : kJoinScratchDefault;
    const uint64_t tiles = timeline_tiles(per, ne_min);
    // the entries of a chunk exactly as the single call has them (pass_plan)
    const uint64_t fit = timeline_chunk_entries(tiles, limit);
    if (fit == 0) return false;                                // the limit holds no block of entries of ONE recording
    const uint64_t chunk = fit < entries ? fit : tb_blocks(entries) * kTbEntries;
    const uint64_t one = timeline_scratch_bytes(chunk, tiles);
    uint64_t recs = 1;
    if (chunk >= entries) {                                    // one recording's whole-corpus partials fit: several recordings a pass
        recs = limit / one;
        const uint64_t items = kOcMaxItems / (entries * tiles);            // (>= 1: timeline_chunk_entries kept the chunk within it)
        if (recs > items) recs = items;
        if (recs > kTbMaxGridZ) recs = kTbMaxGridZ;
        if (recs > recordings) recs = recordings;
    }
    plan->tiles = tiles;
    plan->recordings_per_pass = (uint32_t)recs;
    plan->entries_per_chunk = chunk;
    plan->scratch_bytes = recs * one;
    const size_t wave_lds = tb_wave_lds(ne_max);
    const bool wave = tiles < kOcWaves && wave_lds <= kTbLdsBudget && !force_shared;
    plan->form = wave ? kTimelineBatchFormWave : kTimelineBatchFormShared;
    plan->lds_bytes = wave ? wave_lds : occurrences_lds_bytes(per, ne_max);
    return true;
}

hipError_t launch_timeline_batch_chunk(const TimelineCall& c, const TimelineBatchPlan& plan, uint32_t recordings, void* d_scratch,
                                       uint64_t first_entry, uint64_t entries) {
    if (entries == 0 || recordings == 0) return hipSuccess;
    // (oc_call_ok's, what ties the launch to the plan -- the scratch, the 32-bit unit indices, the fold's grid -- and to the keys)
    if (!oc_call_ok(c, timeline_tiles(c.n_query, c.ne_min), first_entry, entries) || c.ne_min > c.n_query || plan.tiles != c.tiles ||
        recordings > plan.recordings_per_pass || recordings > kTbMaxGridZ || entries > plan.entries_per_chunk ||
        (uint64_t)recordings * entries * c.tiles > kOcMaxItems || (uint64_t)recordings * c.n_query > 0x7FFFFFFFull ||
        c.index_base + first_entry + entries > 0x100000000ull || !c.d_keys)
        return hipErrorInvalidValue;
    size_t lds = 0;
    OcArgs a = oc_args(c, first_entry, entries, c.threshold, false, &lds);
    if (!a.tri) return hipErrorOutOfMemory;
    if (plan.form == kTimelineBatchFormWave) {
        if (c.tiles >= kOcWaves || tb_wave_lds(c.ne_max) > kTbLdsBudget) return hipErrorInvalidValue;
        a.win = kOcTile + 2u + c.ne_max;
        lds = tb_wave_lds(c.ne_max);
    }
    if (lds != plan.lds_bytes) return hipErrorInvalidValue;
    unsigned long long* partials = static_cast<unsigned long long*>(d_scratch);
    const uint32_t key_low = 0xFFFFFFFFu - (uint32_t)c.index_base - a.first;
    const hipError_t e = c.range >= c.subfp_len ? launch_tb_maxima<true>(plan.form, a, lds, recordings, key_low, partials, c.stream)
                                                : launch_tb_maxima<false>(plan.form, a, lds, recordings, key_low, partials, c.stream);
    if (e != hipSuccess) return e;
    // the offsets a pair reaches lie below tiles x 126; the words of a row of out beyond them stay the caller's zeros
    const uint64_t stride = c.tiles * kOcTile;
    const uint32_t n = (uint32_t)(stride < c.n_query ? stride : c.n_query);
    const uint32_t blocks = (uint32_t)tb_blocks(entries);
    const uint64_t src_rec = (uint64_t)blocks * stride;
    const uint32_t gx = (n + 63u) / 64u;
    if (blocks <= kTbFoldRows) {
        hipLaunchKernelGGL(timeline_batch_fold_kernel, dim3(gx, 1, recordings), dim3(kTbFoldThreads), 0, c.stream, partials, blocks, blocks,
                           stride, src_rec, n, c.d_keys, (uint64_t)c.n_query);
    } else {
        const uint32_t fit = (blocks + kTbFoldSlices - 1u) / kTbFoldSlices;
        const uint32_t rows_per = fit > kTbFoldRows ? fit : kTbFoldRows;
        const uint32_t slices = (blocks + rows_per - 1u) / rows_per;
        hipLaunchKernelGGL(timeline_batch_fold_kernel, dim3(gx, slices, recordings), dim3(kTbFoldThreads), 0, c.stream, partials, blocks,
                           rows_per, stride, src_rec, n, static_cast<unsigned long long*>(nullptr), (uint64_t)0);
        hipLaunchKernelGGL(timeline_batch_fold_kernel, dim3(gx, 1, recordings), dim3(kTbFoldThreads), 0, c.stream, partials, slices, slices,
                           stride * rows_per, src_rec, n, c.d_keys, (uint64_t)c.n_query);
    }
    return hipGetLastError();
}

}  // namespace lbad
