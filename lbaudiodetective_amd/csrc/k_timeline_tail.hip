// k_timeline_tail.hip -- the tail occurrences' cells (k_occurrences_tail.hip) folded to ONE key per (recording, offset): of the
// cells a push has completed -- entry j of n_j <= n_q sub-fingerprints at the offsets max(0, n_q - n_j - d_r + 1) .. n_q - n_j, d_r =
// min(new count on the device, the host's bound, the length) -- that reach the threshold, per offset the largest key  q_o bits <<
// 32 | 0xFFFFFFFF - (index base + j): the batch timeline's key of that cell (k_timeline_batch.hip), a cell's value being ot_cell's,
// the pair loop's bit for bit.  A second kernel merges them by unsigned maximum with the previous timeline shifted left by the
// recording's new count, which is the timeline of the window after the push: a cell's value depends on the entry and the
// sub-fingerprints under it alone, so the cells the window had before the push are the previous timeline's, d_r places further left.
// The mapping is recording_tail_kernel's as it is (occurrences_tail_common.hpp): lanes are (recording, t) cells of ONE entry, D
// lanes per recording, the unit's tail windows staged once, the entry's records through the scalar unit.  The fold differs: a
// lane's offset moves with n_j, so a lane owns no output slot.
//   strip     per recording of the group `width` = min(longest entry, n_q) - shortest entry + D 64-bit accumulators in LDS, zeroed
//             with the windows; the cell of an entry of n_j at offset o has slot (n_q - o) - shortest entry = n_j - shortest + (d_r
//             - 1 - t), below the width since t < d_r <= D.  A cell that counts does atomicMax on its slot: no cross-lane ordering
//             is argued, lanes of several recordings and waves meet in no slot but their own recording's
//   flush     behind the unit's entries (a barrier), the non-zero slots go to the recording's strip in the pass' scratch
//             [recordings of the pass][width], zeroed by the host in front of the pass, with a global unsigned 64-bit atomicMax
//   finish    one thread per (recording, offset): the strip's slot (0 outside the strip), the previous row at o + min(new count,
//             n_q) (0 beyond the row), the larger of the two, and the length of the entry it names
// A maximum is commutative and associative, so the result does not depend on the grid, the order of units or of lanes.  No
// workgroup waits for another.  Nothing is read beyond an entry's records, a recording's words or a row of the previous keys:
// every loop is bounded as in the tail kernels, every slot is held against the width before it is touched.
#include "occurrences_tail_common.hpp"

namespace lbad {
namespace {

constexpr uint32_t kTtFlight = 4;                      // steps of a cell whose reads are issued together: the count kernel's
constexpr uint32_t kTtFinishThreads = 256;
constexpr uint32_t kTtFinishMaxGrid = 1u << 16;
static_assert(kTriSize * sizeof(float) == 20604 && kOcRecBytes == 36 && kOcThreads == 256 && kOcEntries == 64,
              "timeline_tail_shape (plan.cpp) counts the LDS and the lanes with these");

// strips[rec][slot] for every recording of the pass: the largest key of the cells at or above a.t, by atomic maxima
__global__ __launch_bounds__(kOcThreads) void timeline_tail_cells_kernel(const OcArgs a, const OtPass p, uint32_t ne_min, uint32_t width,
                                                                         uint32_t key_low, unsigned long long* __restrict__ strips) {
    extern __shared__ uint4 s_dyn[];
    const uint32_t records = p.per_group * a.win;
    const OcLds s = oc_lds(s_dyn, records);
    // behind the table, on the next 8-byte boundary (the windows are 36 bytes a record, the table 20604)
    unsigned long long* const acc =
        reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(s_dyn) + (((size_t)records * kOcRecBytes + kTriSize * sizeof(float) + 7u) & ~(size_t)7u));
    const uint32_t slots = p.per_group * width;
    oc_load_tri(a, s);
    const uint32_t units = ot_units(a, p);
    for (uint32_t u = blockIdx.x; u < units; u += gridDim.x) {
        const uint32_t eb = u / p.groups, group = u - eb * p.groups;
        const OtLane n = ot_lane(a, p, group);
        __syncthreads();                                       // (the unit before has left the windows and flushed the strips)
        ot_stage(a, p, s, group);
        for (uint32_t at = threadIdx.x; at < slots; at += kOcThreads) acc[at] = 0ull;
        __syncthreads();
        const uint32_t e0 = eb * kOcEntries, e1 = a.entries - e0 < kOcEntries ? a.entries : e0 + kOcEntries;
        unsigned long long* const mine = acc + (size_t)(n.has ? threadIdx.x >> p.shift : 0u) * width;
        for (uint32_t e = e0; e < e1; ++e) {
            uint32_t rec0, ne;
            oc_entry(a, e, &rec0, &ne);
            if (ne == 0u || ne > a.nq) continue;               // (wave-uniform)
            uint32_t o;
            float q;
            if (!ot_cell<kTtFlight>(a, s, n, rec0, ne, &o, &q)) continue;
            const uint32_t slot = (a.nq - o) - ne_min;         // (a cell: o <= n_q - n_j, n_j >= the shortest entry)
            if (slot < width) atomicMax(mine + slot, ((unsigned long long)__float_as_uint(q) << 32) | (unsigned long long)(key_low - e));
        }
        __syncthreads();
        for (uint32_t at = threadIdx.x; at < slots; at += kOcThreads) {
            const unsigned long long v = acc[at];
            const uint32_t slot_rec = at / width, rec = group * p.per_group + slot_rec;
            if (v != 0ull && rec < p.recs) atomicMax(strips + (size_t)rec * width + (at - slot_rec * width), v);
        }
    }
}

// keys[r][o] and lengths[r][o] of the pass' rows; `cells` = recordings x per
__global__ __launch_bounds__(kTtFinishThreads) void timeline_tail_finish_kernel(const unsigned long long* __restrict__ strips, uint32_t width,
                                                                                uint32_t ne_min, uint32_t cells, uint32_t per,
                                                                                const uint32_t* __restrict__ fresh,
                                                                                const unsigned long long* __restrict__ prev, uint32_t base,
                                                                                uint64_t count, const uint32_t* __restrict__ off,
                                                                                unsigned long long* __restrict__ keys,
                                                                                uint32_t* __restrict__ lengths) {
    const uint32_t step = gridDim.x * kTtFinishThreads;
    for (uint32_t at = blockIdx.x * kTtFinishThreads + threadIdx.x; at < cells; at += step) {
        const uint32_t r = at / per, o = at - r * per;
        unsigned long long best = 0ull;
        const uint32_t slot = (per - o) - ne_min;              // (wraps for an offset no entry reaches the end from)
        if (strips && slot < width) best = strips[(size_t)r * width + slot];
        if (prev) {
            const uint32_t d = fresh[r];
            const uint32_t shift = d < per ? d : per;
            if (shift < per - o) {                             // o + shift < per: inside row r
                const unsigned long long old = prev[(size_t)r * per + o + shift];
                best = old > best ? old : best;
            }
        }
        keys[at] = best;
        if (lengths) {
            const uint32_t j = 0xFFFFFFFFu - (uint32_t)best - base;        // (the low word is 0xFFFFFFFF - (index base + j))
            lengths[at] = best != 0ull && j < count ? off[j + 1u] - off[j] : 0u;
        }
    }
}

}  // namespace

hipError_t launch_timeline_tail_cells(const TimelineCall& c, const TimelineTailPlan& plan, uint32_t recordings, const uint32_t* d_new_counts,
                                      uint32_t max_new, uint64_t entries, unsigned long long* d_strips) {
    if (entries == 0 || recordings == 0) return hipSuccess;
    // (oc_call_ok's with one tile, and what ties the launch to the plan: the lanes, the sub-windows, the strips and the LDS, the
    // 32-bit unit indices, the keys)
    if (!oc_call_ok(c, 1, 0, entries) || max_new == 0 || max_new > LBAD_OCCURRENCES_TAIL_MAX_NEW || c.ne_min == 0 || c.ne_min > c.n_query ||
        c.ne_min > c.ne_max)
        return hipErrorInvalidValue;
    TimelineTailPlan again;
    timeline_tail_shape(c.n_query, c.ne_min, c.ne_max, max_new, &again);
    if (again.lanes != plan.lanes || again.recordings_per_workgroup != plan.recordings_per_workgroup ||
        again.window_records != plan.window_records || again.strip_width != plan.strip_width || again.lds_bytes != plan.lds_bytes ||
        plan.lds_bytes > 160 * 1024 - 64 || plan.window_records > c.n_query || plan.strip_width == 0 || plan.lanes == 0 || plan.lanes > 64 ||
        (plan.lanes & (plan.lanes - 1u)) != 0 || plan.recordings_per_workgroup == 0 ||
        plan.recordings_per_workgroup * plan.lanes > kOcThreads || recordings > plan.recordings_per_pass || recordings > kOcMaxRecs ||
        oc_blocks(entries) * recordings > kOcMaxItems || (uint64_t)recordings * c.n_query > 0x7FFFFFFFull ||
        (uint64_t)recordings * plan.strip_width * 8u > plan.scratch_bytes || c.index_base + entries > 0x100000000ull || !d_strips ||
        !d_new_counts)
        return hipErrorInvalidValue;
    size_t lds = 0;
    OcArgs a = oc_args(c, 0, entries, c.threshold, false, &lds);
    if (!a.tri) return hipErrorOutOfMemory;
    a.win = plan.window_records;
    lds = (size_t)plan.lds_bytes;
    const OtPass p = ot_pass(plan, recordings, d_new_counts, max_new, false, false);
    static size_t ready[kMaxDevices] = {};
    const hipError_t e = oc_allow_lds(ready, lds, timeline_tail_cells_kernel);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(timeline_tail_cells_kernel, oc_grid(oc_blocks(entries) * p.groups), dim3(kOcThreads), lds, c.stream, a, p, c.ne_min,
                       plan.strip_width, 0xFFFFFFFFu - (uint32_t)c.index_base, d_strips);
    return hipGetLastError();
}

hipError_t launch_timeline_tail_finish(const unsigned long long* d_strips, uint32_t strip_width, uint32_t ne_min, uint32_t recordings,
                                       uint32_t per, const uint32_t* d_new_counts, const unsigned long long* d_prev, uint64_t index_base,
                                       uint64_t count, const uint32_t* d_off, unsigned long long* d_keys, uint32_t* d_lengths,
                                       hipStream_t stream) {
    if (recordings == 0 || per == 0) return hipSuccess;
    if ((uint64_t)recordings * per > 0x7FFFFFFFull || index_base + count > 0x100000000ull || !d_keys || (d_prev && !d_new_counts) ||
        (d_strips && (strip_width == 0 || ne_min == 0)) || (d_lengths && count != 0 && !d_off))
        return hipErrorInvalidValue;
    const uint32_t cells = recordings * per;
    hipLaunchKernelGGL(timeline_tail_finish_kernel, dim3(strided_grid((cells + kTtFinishThreads - 1u) / kTtFinishThreads, kTtFinishMaxGrid)),
                       dim3(kTtFinishThreads), 0, stream, d_strips, strip_width, ne_min, cells, per, d_new_counts, d_prev,
                       (uint32_t)index_base, count, d_off, d_keys, d_lengths);
    return hipGetLastError();
}

}  // namespace lbad
