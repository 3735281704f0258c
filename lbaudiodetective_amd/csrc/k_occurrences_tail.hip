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
// (OtPass, OtLane, ot_lane, ot_stage, ot_cell and ot_units: occurrences_tail_common.hpp, shared with k_recording_tail.hip; the
// scratch, the checks of a pass of rows and the totals: occurrences_common.hpp and k_occurrences_batch.hip)
//
// THE PEAKS LIST (the kernels' PEAKS instances) is the list above under the occurrences' peak rule, each cell judged
// ONE sub-fingerprint late: by then its right neighbour exists.  For recording r of a pass with d_r = min(new count on the device,
// the host's bound, the length) and entry j of n_j <= n_q sub-fingerprints, last = n_q - n_j, the JUDGED cells are the offsets
// max(0, last - d_r) .. last - 1 -- those whose entry ends inside the d_r sub-fingerprints in front of the newest one --, and with
// `final` the newest cell `last` as well.  A judged cell matches when q_o >= the threshold, (o == 0 or q_o > q_(o-1)) and (o == last
// or q_o >= q_(o+1)): k_occurrences.hip's rule on the window's own profile, so a plateau reports its first cell and a neighbour below
// the threshold still takes part.  A cell's value is the pair loop's, bit for bit, as in the plain instances (ot_cell).  Keys, lags,
// order, counts and rows are the batch call's with peaks on.
// The mapping is the one above with two more cells a pair:
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
// Nothing is carried from call to call: the d_r + 2 cells are computed again, (d + 2) / d of the plain list's cell work, and D
// doubles where bound + 2 crosses a power of two.  Counts, scans, scatter and totals are the same code: one kernel pair, two instances.
#include "occurrences_tail_common.hpp"

namespace lbad {
namespace {

constexpr uint32_t kOtCountFlight = 4;                 // steps of a cell whose reads are issued together: the count kernel's,
constexpr uint32_t kOtScatterFlight = 2;               // and the scatter kernel's, which has fewer scalar registers to spare
static_assert(kTriSize * sizeof(float) == 20604 && kOcRecBytes == 36 && kOcThreads == 256 && kOcEntries == 64,
              "occurrences_tail_shape (plan.cpp) counts the LDS and the lanes with these");
static_assert(LBAD_OCCURRENCES_TAIL_PEAKS_MAX_NEW + 2 <= LBAD_OCCURRENCES_TAIL_MAX_NEW && LBAD_OCCURRENCES_TAIL_MAX_NEW == 64,
              "a recording's lanes, the peaks bound + 2 rounded up, stay inside one wave");

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
__device__ __forceinline__ bool op_cell(const OcArgs& a, const OtPass& p, const OcLds& s, const OtLane& n, uint32_t d, uint32_t rec0,
                                        uint32_t ne, uint32_t* o, float* q) {
    const uint32_t last = a.nq - ne;
    ot_cell<FLIGHT>(a, s, n, rec0, ne, o, q);
    const float left = __shfl_up(*q, 1u, (int)p.lanes), right = __shfl_down(*q, 1u, (int)p.lanes);
    const bool cell = n.t < n.d && last + 1u + n.t >= n.d;     // (ot_cell's: the lane has an offset >= 0)
    const bool judged = cell && n.t != 0u && (p.final != 0u || n.t <= d);
    return judged && *q >= a.t && (*o == 0u || *q > left) && (*o == last || *q >= right);
}

// The lane and its cell under the call's rule: ot_lane and ot_cell as they are, or the peaks list's pair (*d: its recording's own count)
template <bool PEAKS>
__device__ __forceinline__ OtLane ot_rule_lane(const OcArgs& a, const OtPass& p, uint32_t group, uint32_t* d) {
    if (PEAKS) return op_lane(a, p, group, d);
    *d = 0u;
    return ot_lane(a, p, group);
}
template <bool PEAKS, uint32_t FLIGHT>
__device__ __forceinline__ bool ot_rule_cell(const OcArgs& a, const OtPass& p, const OcLds& s, const OtLane& n, uint32_t d, uint32_t rec0,
                                             uint32_t ne, uint32_t* o, float* q) {
    if (PEAKS) return op_cell<FLIGHT>(a, p, s, n, d, rec0, ne, o, q);
    return ot_cell<FLIGHT>(a, s, n, rec0, ne, o, q);
}

// counts[rec][entry] for every recording of the pass and entry of the chunk; any[u]: the unit has a match
template <bool PEAKS>
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
        uint32_t d;
        const OtLane n = ot_rule_lane<PEAKS>(a, p, group, &d);
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
                const bool m = ot_rule_cell<PEAKS, kOtCountFlight>(a, p, s, n, d, rec0, ne, &o, &q);
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
template <bool PEAKS>
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
        uint32_t d;
        OtLane n = ot_rule_lane<PEAKS>(a, p, group, &d);
        // (the peaks instance takes t afresh per unit: `t != 0` held as a mask from the kernel's head across every unit was the one
        // scalar pair it had no register for, and went to a vector lane and back)
        if (PEAKS) asm("" : "+v"(n.t));
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
            // (the same for every lane; never with a count above 0: the reads stay inside the windows)
            if (ne == 0u || ne > a.nq) continue;
            float q;
            const bool m = ot_rule_cell<PEAKS, kOtScatterFlight>(a, p, s, n, d, rec0, ne, &o, &q);     // (before any lane's own exit)
            const unsigned long long mine = __ballot(m) & n.seg & ((1ull << lane) - 1ull);
            if (!want || !m) continue;
            const unsigned long long slot = row_base[row0 + e] - base + (uint32_t)__popcll(mine);
            if (slot >= capacity) continue;
            out_keys[slot] = ((unsigned long long)__float_as_uint(q) << 32) | (unsigned long long)(key_base - e);
            if (out_lags) out_lags[slot] = -(int32_t)o;
        }
    }
}

// one instance's launches: count, the joins' scans over rows = recordings x entries of one column, scatter, totals
template <bool PEAKS>
hipError_t launch_ot(const OccurrencesCall& c, const OcScratch& s, const OcArgs& a, const OtPass& p, size_t lds, uint32_t first_chunk,
                     unsigned long long* d_counts) {
    static size_t ready[kMaxDevices] = {};                     // (both kernels of this instance)
    const hipError_t e = oc_allow_lds(ready, lds, occurrences_tail_count_kernel<PEAKS>, occurrences_tail_scatter_kernel<PEAKS>);
    if (e != hipSuccess) return e;
    const dim3 grid = oc_grid(oc_blocks(a.entries) * p.groups);
    const uint32_t rows = p.recs * a.entries;
    hipLaunchKernelGGL(occurrences_tail_count_kernel<PEAKS>, grid, dim3(kOcThreads), lds, c.stream, a, p, s.counts, s.any);
    launch_join_scans(s.counts, 1, rows, s.tile_at, s.row_base, s.state, first_chunk, s.offsets, c.stream);
    hipLaunchKernelGGL(occurrences_tail_scatter_kernel<PEAKS>, grid, dim3(kOcThreads), lds, c.stream, a, p, s.counts, s.any, s.row_base,
                       (unsigned long long)c.capacity, 0xFFFFFFFFu - (uint32_t)c.index_base - a.first, c.d_keys, c.d_lags);
    if (!p.chunked) return launch_occurrences_totals(s.offsets, p.recs, a.entries, d_counts, c.stream);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_occurrences_tail_chunk(const OccurrencesCall& c, const OccurrencesTailPlan& plan, uint32_t recordings,
                                         const uint32_t* d_new_counts, uint32_t max_new, bool peaks, bool final, void* d_scratch,
                                         uint64_t first_entry, uint64_t entries, uint32_t first_chunk, unsigned long long* d_counts) {
    if (entries == 0 || recordings == 0) return hipSuccess;
    const bool chunked = plan.recordings_per_pass == 1;
    // (oc_call_ok's with one tile, and what ties the launch to the plan: the lanes, the sub-windows and the LDS (ot_shape_ok) -- the
    // peaks list's shape at max_new + 2: a recording's lanes hold its two neighbour cells --, and oc_rows_call_ok's)
    const uint32_t cells = max_new + (peaks ? 2u : 0u);
    if (!oc_call_ok(c, 1, first_entry, entries) || max_new == 0 ||
        max_new > (peaks ? LBAD_OCCURRENCES_TAIL_PEAKS_MAX_NEW : LBAD_OCCURRENCES_TAIL_MAX_NEW))
        return hipErrorInvalidValue;
    if (!ot_shape_ok(c, plan, cells) || (peaks && (plan.lanes < cells || plan.lanes > 64u)) ||
        !oc_rows_call_ok(c, plan, recordings, first_entry, entries, first_chunk, d_counts) || !d_new_counts)
        return hipErrorInvalidValue;
    size_t lds = 0;
    OcArgs a = oc_args(c, first_entry, entries, c.threshold, false, &lds);
    if (!a.tri) return hipErrorOutOfMemory;
    a.win = plan.window_records;
    lds = (size_t)plan.lds_bytes;
    const OtPass p = ot_pass(plan, recordings, d_new_counts, max_new, chunked, peaks && final);
    // (a chunked pass keeps ONE carving for all its chunks: the state word is carried)
    const OcScratch s = oc_carve(d_scratch, chunked ? plan.entries_per_chunk : (uint64_t)recordings * entries, 1);
    return peaks ? launch_ot<true>(c, s, a, p, lds, first_chunk, d_counts) : launch_ot<false>(c, s, a, p, lds, first_chunk, d_counts);
}

}  // namespace lbad
