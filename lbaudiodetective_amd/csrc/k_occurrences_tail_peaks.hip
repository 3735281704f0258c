// k_occurrences_tail_peaks.hip -- the tail occurrences (k_occurrences_tail.hip) with the occurrences' peak rule, each cell judged
// ONE sub-fingerprint late: by then its right neighbour exists.  For recording r of a pass with d_r = min(new count on the device,
// the host's bound, the length) and entry j of n_j <= n_q sub-fingerprints, last = n_q - n_j, the JUDGED cells are the offsets
// max(0, last - d_r) .. last - 1 -- those whose entry ends inside the d_r sub-fingerprints in front of the newest one --, and with
// `final` the newest cell `last` as well.  A judged cell matches when q_o >= the threshold, (o == 0 or q_o > q_(o-1)) and (o == last
// or q_o >= q_(o+1)): k_occurrences.hip's rule on the window's own profile, so a plateau reports its first cell and a neighbour below
// the threshold still takes part.  A cell's value is the pair loop's, bit for bit, as in the tail kernels (ot_cell).  Keys, lags,
// order, counts and rows are the batch call's with peaks on.
// The mapping is the tail kernels' (occurrences_tail_common.hpp) with two more cells a pair:
//   lanes    D = the next power of two >= the bound + 2 lanes per recording (so the bound is at most 62: D stays inside a wave).
//            Lane t of recording r owns offset last - d_r - 1 + t, t = 0 .. d_r + 1, idle for an offset below 0: ot_cell as it is
//            with d_r + 2 cells.  Lane 0 only SUPPLIES q_(o-1) to lane 1, lane d_r + 1 only supplies q_(o+1) to lane d_r unless
//            the call is final; neither matches otherwise.
//   exchange a lane takes its two neighbours' values with one shuffle each, D wide, right behind ot_cell: there the whole wave is
//            converged -- the entry and its step count are the same for every lane, and the scatter's exits in front of it are
//            ballots of the whole wave.  A judged lane with o > 0 has t >= 1 and lane t - 1 holds cell o - 1; one with o < last has
//            t <= d_r and lane t + 1 <= D - 1 holds cell o + 1: both inside the recording's D lanes.  At o == 0 and at o == last the
//            rule's "does not exist" branch decides and the fetched value is not looked at.
//   window   min(n_q, min(longest, n_q) + D - 1) records, the plan's at bound + 2: a cell at offset o >= last - D + 1 reads
//            records o - (n_q - win) .. + n_j - 1 of it, at least win - n_j - D + 1 >= 0 and at most win - 1 (ot_cell's bounds).
// Nothing is carried from call to call: the d_r + 2 cells are computed again, (d + 2) / d of the tail kernels' cell work, and D
// doubles where bound + 2 crosses a power of two.  Counts, scans and scatter are k_occurrences_tail.hip's scheme, the totals its
// kernel (launch_occurrences_tail_totals): no atomics on memory, no workgroup waits for another, one writer per output word.
#include "occurrences_tail_common.hpp"

namespace lbad {
namespace {

constexpr uint32_t kOpCountFlight = 4;                 // k_occurrences_tail.hip's two
constexpr uint32_t kOpScatterFlight = 2;
static_assert(kTriSize * sizeof(float) == 20604 && kOcRecBytes == 36 && kOcThreads == 256 && kOcEntries == 64,
              "occurrences_tail_shape (plan.cpp) counts the LDS and the lanes with these");
static_assert(LBAD_OCCURRENCES_TAIL_PEAKS_MAX_NEW + 2 <= LBAD_OCCURRENCES_TAIL_MAX_NEW && LBAD_OCCURRENCES_TAIL_MAX_NEW == 64,
              "a recording's lanes, the bound + 2 rounded up, stay inside one wave");

// ot_lane with the pair's d + 2 cells: n.d is what ot_cell spreads over the lanes, *d the recording's own count
__device__ __forceinline__ OtLane op_lane(const OcArgs& a, const OtPass& p, uint32_t group, uint32_t* d) {
    OtLane n = ot_lane(a, p, group);
    *d = n.d;
    n.d = n.has ? n.d + 2u : 0u;
    return n;
}

// The lane's cell of one entry (ot_cell: offset to *o, quotient to *q) and the peak rule; true where the cell is judged and
// matches.  The WHOLE WAVE calls this together: the shuffles read the neighbours' registers.
template <uint32_t FLIGHT>
__device__ __forceinline__ bool op_cell(const OcArgs& a, const OtPass& p, const OcLds& s, const OtLane& n, uint32_t d, uint32_t final,
                                        uint32_t rec0, uint32_t ne, uint32_t* o, float* q) {
    const uint32_t last = a.nq - ne;
    ot_cell<FLIGHT>(a, s, n, rec0, ne, o, q);
    const float left = __shfl_up(*q, 1u, (int)p.lanes), right = __shfl_down(*q, 1u, (int)p.lanes);
    const bool cell = n.t < n.d && last + 1u + n.t >= n.d;     // (ot_cell's: the lane has an offset >= 0)
    const bool judged = cell && n.t != 0u && (final != 0u || n.t <= d);
    return judged && *q >= a.t && (*o == 0u || *q > left) && (*o == last || *q >= right);
}

// counts[rec][entry] for every recording of the pass and entry of the chunk; any[u]: the unit has a match
__global__ __launch_bounds__(kOcThreads) void occurrences_tail_peaks_count_kernel(const OcArgs a, const OtPass p, const uint32_t final,
                                                                                  uint32_t* __restrict__ counts,
                                                                                  uint32_t* __restrict__ any) {
    extern __shared__ uint4 s_dyn[];
    __shared__ uint32_t s_any;
    const uint32_t lane = threadIdx.x & 63u;
    const OcLds s = oc_lds(s_dyn, p.per_group * a.win);
    oc_load_tri(a, s);
    const uint32_t units = ot_units(a, p);
    for (uint32_t u = blockIdx.x; u < units; u += gridDim.x) {
        const uint32_t eb = u / p.groups, group = u - eb * p.groups;
        uint32_t d;
        const OtLane n = op_lane(a, p, group, &d);
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
            if (ne != 0u && ne <= a.nq) {                      // (the same for every lane)
                uint32_t o;
                float q;
                const bool m = op_cell<kOpCountFlight>(a, p, s, n, d, final, rec0, ne, &o, &q);
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
__global__ __launch_bounds__(kOcThreads) void occurrences_tail_peaks_scatter_kernel(const OcArgs a, const OtPass p, const uint32_t final,
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
        uint32_t d;
        const OtLane n = op_lane(a, p, group, &d);
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
            if (__ballot(want) == 0ull) continue;              // (the whole wave leaves or stays: a count above 0, the entry takes part)
            uint32_t rec0, ne, o;
            oc_entry(a, e, &rec0, &ne);
            if (ne == 0u || ne > a.nq) continue;               // (the same for every lane; never with a count above 0)
            float q;
            const bool m = op_cell<kOpScatterFlight>(a, p, s, n, d, final, rec0, ne, &o, &q);      // (the exchange: before any lane's own exit)
            const unsigned long long mine = __ballot(m) & n.seg & ((1ull << lane) - 1ull);
            if (!want || !m) continue;
            const unsigned long long slot = row_base[row0 + e] - base + (uint32_t)__popcll(mine);
            if (slot >= capacity) continue;
            out_keys[slot] = ((unsigned long long)__float_as_uint(q) << 32) | (unsigned long long)(key_base - e);
            if (out_lags) out_lags[slot] = -(int32_t)o;
        }
    }
}

}  // namespace

hipError_t launch_occurrences_tail_peaks_chunk(const OccurrencesCall& c, const OccurrencesTailPlan& plan, uint32_t recordings,
                                               const uint32_t* d_new_counts, uint32_t max_new, bool final, void* d_scratch,
                                               uint64_t first_entry, uint64_t entries, uint32_t first_chunk, unsigned long long* d_counts) {
    if (entries == 0 || recordings == 0) return hipSuccess;
    const bool chunked = plan.recordings_per_pass == 1;
    // (launch_occurrences_tail_chunk's checks, the shape at max_new + 2: a recording's lanes hold its two neighbour cells)
    OccurrencesTailPlan again;
    if (!oc_call_ok(c, 1, first_entry, entries) || max_new == 0 || max_new > LBAD_OCCURRENCES_TAIL_PEAKS_MAX_NEW) return hipErrorInvalidValue;
    occurrences_tail_shape(c.n_query, c.ne_max, max_new + 2u, &again);
    if (again.lanes != plan.lanes || again.lanes < max_new + 2u || again.lanes > 64u ||
        again.recordings_per_workgroup != plan.recordings_per_workgroup || again.window_records != plan.window_records ||
        again.lds_bytes != plan.lds_bytes || plan.lds_bytes > 160 * 1024 - 64 || plan.window_records > c.n_query ||
        recordings > plan.recordings_per_pass || recordings > kOtMaxRecs || entries > plan.entries_per_chunk ||
        (!chunked && (first_entry != 0 || first_chunk == 0)) || (uint64_t)recordings * entries > kOcMaxItems ||
        (uint64_t)recordings * c.n_query > 0x7FFFFFFFull || (uint64_t)recordings * c.capacity > 0x80000000ull ||
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
    const hipError_t e = oc_allow_lds(ready, lds, occurrences_tail_peaks_count_kernel, occurrences_tail_peaks_scatter_kernel);
    if (e != hipSuccess) return e;
    // (a chunked pass keeps ONE carving for all its chunks: the state word is carried)
    const OtScratch s = ot_carve(d_scratch, chunked ? 1 : recordings, chunked ? plan.entries_per_chunk : entries);
    const dim3 grid = oc_grid(oc_blocks(entries) * p.groups);
    const uint32_t rows = recordings * a.entries;
    const uint32_t fin = final ? 1u : 0u;
    hipLaunchKernelGGL(occurrences_tail_peaks_count_kernel, grid, dim3(kOcThreads), lds, c.stream, a, p, fin, s.counts, s.any);
    launch_join_scans(s.counts, 1, rows, s.tile_at, s.row_base, s.state, first_chunk, s.offsets, c.stream);
    hipLaunchKernelGGL(occurrences_tail_peaks_scatter_kernel, grid, dim3(kOcThreads), lds, c.stream, a, p, fin, s.counts, s.any, s.row_base,
                       (unsigned long long)c.capacity, 0xFFFFFFFFu - (uint32_t)c.index_base - a.first, c.d_keys, c.d_lags);
    if (!chunked) return launch_occurrences_tail_totals(s.offsets, recordings, a.entries, d_counts, c.stream);
    return hipGetLastError();
}

}  // namespace lbad
