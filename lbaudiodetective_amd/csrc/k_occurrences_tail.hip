// k_occurrences_tail.hip -- the batch occurrences (k_occurrences_batch.hip) for the cells a push has COMPLETED: for every recording
// r of a pass only the cells (entry, offset) whose entry ends inside the recording's newest d_r sub-fingerprints, d_r = min(new
// count on the device, the host's bound, the length).  Entry j of n_j <= n_q sub-fingerprints has the offsets max(0, n_q - n_j -
// d_r + 1) .. n_q - n_j; a longer entry has no complete position and is skipped.  A cell's value is the pair loop's, case B, bit
// for bit (oc_prepare<false> for the recording's records, oc_ratio, the steps added in order from +0 and divided by n_j); a cell
// matches at or above the threshold, and there is no peak rule.  Keys, lags, order, counts and rows are the batch call's.
// The mapping is not the pair loop's (a wave per entry and 126 offsets would idle all but d_r of its cells):
//   lanes    are (recording, t) cells of ONE entry: D = the next power of two >= the bound lanes per recording, G = 256 / D
//            recordings per workgroup (fewer where their windows do not fit the LDS: the surplus lanes compute nothing).  Lane t of
//            recording r owns offset n_q - n_j - d_r + 1 + t, idle for t >= d_r or an offset below 0.  The entry and its step count
//            are the same for every lane of the workgroup, so the entry's record of a step comes through the scalar unit and no
//            lane waits for another's longer loop.
//   unit     u = (block of kOcEntries entries, group of G recordings), the entry block slowest.  The workgroup stages once per unit
//            the TAIL window of each of its recordings -- the last win = min(n_q, ne_b + D - 1) records -- as prepared records,
//            oc_stage's three arrays with one sub-window per recording.
// counts[recording of the pass][entry] (one column per row) are the rows of the joins' two scans as the batch call uses them; a
// cell's slot is its row's position less the position of its recording's first row plus the matching lanes below it among that
// recording's lanes.  A pass of ONE recording may run in entry chunks with the carried total.  No atomics on memory, no workgroup
// waits for another, one writer per output word; the scatter computes again only units with a match and skips rows already full.
// Nothing is read beyond an entry's records or a recording's words: every loop is bounded by a length from the record positions
// clamped to the corpus' longest entry, or by a count the host has checked.
// (OtPass, OtLane, ot_lane, ot_stage, ot_cell and ot_units: occurrences_tail_common.hpp, shared with k_recording_tail.hip; kOtMaxRecs,
// OtScratch and ot_carve: the same header, shared with k_occurrences_tail_peaks.hip)
#include "occurrences_tail_common.hpp"

namespace lbad {
namespace {

constexpr uint32_t kOtThreads = 256;                   // the totals kernel
constexpr uint32_t kOtCountFlight = 4;                 // steps of a cell whose reads are issued together: the count kernel's,
constexpr uint32_t kOtScatterFlight = 2;               // and the scatter kernel's, which has fewer scalar registers to spare
static_assert(kTriSize * sizeof(float) == 20604 && kOcRecBytes == 36 && kOcThreads == 256 && kOcEntries == 64,
              "occurrences_tail_shape (plan.cpp) counts the LDS and the lanes with these");

// counts[rec][entry] for every recording of the pass and entry of the chunk; any[u]: the unit has a match
__global__ __launch_bounds__(kOcThreads) void occurrences_tail_count_kernel(const OcArgs a, const OtPass p, uint32_t* __restrict__ counts,
                                                                            uint32_t* __restrict__ any) {
    extern __shared__ uint4 s_dyn[];
    __shared__ uint32_t s_any;
    const uint32_t lane = threadIdx.x & 63u;
    const OcLds s = oc_lds(s_dyn, p.per_group * a.win);
    oc_load_tri(a, s);
    const uint32_t units = ot_units(a, p);
    for (uint32_t u = blockIdx.x; u < units; u += gridDim.x) {
        const uint32_t eb = u / p.groups, group = u - eb * p.groups;
        const OtLane n = ot_lane(a, p, group);
        __syncthreads();                                       // (the unit before has left the windows and s_any)
        ot_stage(a, p, s, group);
        if (threadIdx.x == 0u) s_any = 0u;
        __syncthreads();
        const uint32_t e0 = eb * kOcEntries, e1 = a.entries - e0 < kOcEntries ? a.entries : e0 + kOcEntries;
        uint32_t* __restrict__ row = counts + (size_t)n.rec * a.entries;
        bool some = false;
        for (uint32_t e = e0; e < e1; ++e) {
            uint32_t rec0, ne, c = 0u;
            oc_entry(a, e, &rec0, &ne);
            if (ne != 0u && ne <= a.nq) {
                uint32_t o;
                float q;
                const bool m = ot_cell<kOtCountFlight>(a, s, n, rec0, ne, &o, &q);
                c = (uint32_t)__popcll(__ballot(m) & n.seg);
                some = some || m;
            }
            if (n.has && n.t == 0u) row[e] = c;
        }
        if (__ballot(some) != 0ull && lane == 0u) atomicOr(&s_any, 1u);        // (LDS: a flag, whoever sets it)
        __syncthreads();
        if (threadIdx.x == 0u) any[u] = s_any;
    }
}

// keys / lags: row 0 of the pass, rows `capacity` slots apart
__global__ __launch_bounds__(kOcThreads) void occurrences_tail_scatter_kernel(const OcArgs a, const OtPass p,
                                                                              const uint32_t* __restrict__ counts,
                                                                              const uint32_t* __restrict__ any,
                                                                              const unsigned long long* __restrict__ row_base,
                                                                              unsigned long long capacity, uint32_t key_base,
                                                                              unsigned long long* __restrict__ keys,
                                                                              int32_t* __restrict__ lags) {
    // (key_base = 0xFFFFFFFF - the low word of the index base - the chunk's first entry: a key's low word is key_base - e)
    extern __shared__ uint4 s_dyn[];
    const uint32_t lane = threadIdx.x & 63u;
    const OcLds s = oc_lds(s_dyn, p.per_group * a.win);
    oc_load_tri(a, s);
    const uint32_t units = ot_units(a, p);
    for (uint32_t u = blockIdx.x; u < units; u += gridDim.x) {
        if (any[u] == 0u) continue;                            // (the same word for the whole workgroup) nothing is loaded
        const uint32_t eb = u / p.groups, group = u - eb * p.groups;
        const OtLane n = ot_lane(a, p, group);
        __syncthreads();                                       // (the unit before has left the windows)
        ot_stage(a, p, s, group);
        __syncthreads();
        const uint32_t e0 = eb * kOcEntries, e1 = a.entries - e0 < kOcEntries ? a.entries : e0 + kOcEntries;
        const uint32_t row0 = n.rec * a.entries;               // the recording's first row of the scans
        // the recording's first position in the pass; its list is full in front of this block of entries?
        const unsigned long long base = p.chunked ? 0ull : row_base[row0];
        const bool open = n.has && row_base[row0 + e0] - base < capacity;
        if (__ballot(open) == 0ull) continue;                  // (this wave meets no barrier of the unit any more)
        unsigned long long* __restrict__ out_keys = keys + (size_t)n.rec * capacity;
        int32_t* __restrict__ out_lags = lags ? lags + (size_t)n.rec * capacity : nullptr;
        for (uint32_t e = e0; e < e1; ++e) {
            const bool want = open && counts[row0 + e] != 0u;
            if (__ballot(want) == 0ull) continue;              // (a count above 0: the entry takes part)
            uint32_t rec0, ne, o;
            oc_entry(a, e, &rec0, &ne);
            if (ne == 0u || ne > a.nq) continue;               // (never with a count above 0: the reads stay inside the windows)
            float q;
            const bool m = ot_cell<kOtScatterFlight>(a, s, n, rec0, ne, &o, &q);
            const unsigned long long mine = __ballot(m) & n.seg & ((1ull << lane) - 1ull);
            if (!want || !m) continue;
            const unsigned long long slot = row_base[row0 + e] - base + (uint32_t)__popcll(mine);
            if (slot >= capacity) continue;
            out_keys[slot] = ((unsigned long long)__float_as_uint(q) << 32) | (unsigned long long)(key_base - e);
            if (out_lags) out_lags[slot] = -(int32_t)o;
        }
    }
}

// out_counts[r] = the recording's matches: the difference of two neighbouring recordings' first positions (offsets[rows]: the total)
__global__ __launch_bounds__(kOtThreads) void occurrences_tail_totals_kernel(const unsigned long long* __restrict__ offsets, uint32_t recs,
                                                                            uint32_t stride, unsigned long long* __restrict__ out_counts) {
    const uint32_t r = blockIdx.x * kOtThreads + threadIdx.x;
    if (r < recs) out_counts[r] = offsets[(size_t)(r + 1u) * stride] - offsets[(size_t)r * stride];
}

}  // namespace

hipError_t launch_occurrences_tail_chunk(const OccurrencesCall& c, const OccurrencesTailPlan& plan, uint32_t recordings,
                                         const uint32_t* d_new_counts, uint32_t max_new, void* d_scratch, uint64_t first_entry,
                                         uint64_t entries, uint32_t first_chunk, unsigned long long* d_counts) {
    if (entries == 0 || recordings == 0) return hipSuccess;
    const bool chunked = plan.recordings_per_pass == 1;
    // (oc_call_ok's with one tile, and what ties the launch to the plan: the lanes, the sub-windows and the LDS, the scratch, the
    // 32-bit row and unit indices, the keys' rows; more than one recording takes the whole corpus in one chunk)
    OccurrencesTailPlan again;
    if (!oc_call_ok(c, 1, first_entry, entries) || max_new == 0 || max_new > LBAD_OCCURRENCES_TAIL_MAX_NEW) return hipErrorInvalidValue;
    occurrences_tail_shape(c.n_query, c.ne_max, max_new, &again);
    if (again.lanes != plan.lanes || again.recordings_per_workgroup != plan.recordings_per_workgroup ||
        again.window_records != plan.window_records || again.lds_bytes != plan.lds_bytes || plan.lds_bytes > 160 * 1024 - 64 ||
        plan.window_records > c.n_query || recordings > plan.recordings_per_pass || recordings > kOtMaxRecs ||
        entries > plan.entries_per_chunk || (!chunked && (first_entry != 0 || first_chunk == 0)) ||
        (uint64_t)recordings * entries > kOcMaxItems || (uint64_t)recordings * c.n_query > 0x7FFFFFFFull ||
        (uint64_t)recordings * c.capacity > 0x80000000ull ||
        (uint64_t)recordings * occurrences_scratch_bytes(entries, 1) > plan.scratch_bytes ||
        c.index_base + first_entry + entries > 0x100000000ull || !c.d_keys || !d_counts || !d_new_counts)
        return hipErrorInvalidValue;
    size_t lds = 0;
    OcArgs a = oc_args(c, first_entry, entries, c.threshold, false, &lds);
    if (!a.tri) return hipErrorOutOfMemory;
    a.win = plan.window_records;
    lds = (size_t)plan.lds_bytes;
    OtPass p;
    p.fresh = d_new_counts; p.recs = recordings; p.chunked = chunked ? 1u : 0u; p.max_new = max_new; p.lanes = plan.lanes;
    p.shift = (uint32_t)__builtin_ctz(plan.lanes); p.per_group = plan.recordings_per_workgroup;
    p.groups = (recordings + p.per_group - 1u) / p.per_group;
    static size_t ready[kMaxDevices] = {};                     // (both kernels)
    const hipError_t e = oc_allow_lds(ready, lds, occurrences_tail_count_kernel, occurrences_tail_scatter_kernel);
    if (e != hipSuccess) return e;
    // (a chunked pass keeps ONE carving for all its chunks: the state word is carried)
    const OtScratch s = ot_carve(d_scratch, chunked ? 1 : recordings, chunked ? plan.entries_per_chunk : entries);
    const dim3 grid = oc_grid(oc_blocks(entries) * p.groups);
    const uint32_t rows = recordings * a.entries;
    hipLaunchKernelGGL(occurrences_tail_count_kernel, grid, dim3(kOcThreads), lds, c.stream, a, p, s.counts, s.any);
    launch_join_scans(s.counts, 1, rows, s.tile_at, s.row_base, s.state, first_chunk, s.offsets, c.stream);
    hipLaunchKernelGGL(occurrences_tail_scatter_kernel, grid, dim3(kOcThreads), lds, c.stream, a, p, s.counts, s.any, s.row_base,
                       (unsigned long long)c.capacity, 0xFFFFFFFFu - (uint32_t)c.index_base - a.first, c.d_keys, c.d_lags);
    if (!chunked) return launch_occurrences_tail_totals(s.offsets, recordings, a.entries, d_counts, c.stream);
    return hipGetLastError();
}

hipError_t launch_occurrences_tail_totals(const unsigned long long* d_offsets, uint32_t recordings, uint32_t stride,
                                          unsigned long long* d_counts, hipStream_t stream) {
    hipLaunchKernelGGL(occurrences_tail_totals_kernel, dim3((recordings + kOtThreads - 1) / kOtThreads), dim3(kOtThreads), 0, stream, d_offsets,
                       recordings, stride, d_counts);
    return hipGetLastError();
}

}  // namespace lbad
