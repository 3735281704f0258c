// k_recording_tail.hip -- the tail occurrences' cells (k_occurrences_tail.hip) folded to ONE value per (recording, entry): of the
// cells a push has completed -- entry j of n_j <= n_q sub-fingerprints at the offsets max(0, n_q - n_j - d_r + 1) .. n_q - n_j, d_r =
// min(new count on the device, the host's bound, the length) -- the largest q_o, floored at +0, and minus the LOWEST offset that
// reaches it; +0 and 0 for a pair without a tail cell (d_r == 0, an empty entry, an entry longer than the recording).  A cell's
// value is ot_cell's, the pair loop's bit for bit.  The output has a fixed shape, so there is no count, no `any` flag, no scan and
// no scatter: one launch per pass over ALL entries, and the project's selections (launch_topk_keys, launch_threshold_batch_keys)
// read the rows.
// The mapping is occurrences_tail_count_kernel's as it is (occurrences_tail_common.hpp): lanes are (recording, t) cells of ONE
// entry, D lanes per recording, the unit's tail windows staged once, the entry's records through the scalar unit, a lane without a
// cell computes the newest cell and drops it.  Behind ot_cell:
//   own cell  whether the lane HAS a cell comes from t, d and the offset alone (never from a comparison of the value); a lane
//             with one forms max(+0, q), a lane without one contributes the word 0
//   reduce    the D lanes of a recording hold  value bits << 32 | 0xFFFFFFFF - t  and take the largest in log2(D) __shfl_xor
//             steps (none for D == 1): non-negative floats order as their bit patterns, a tie goes to the lowest t, that is the
//             lowest offset; D is a power of two <= 64 and a recording's lanes are an aligned run of one wave, so a step never
//             leaves the recording
//   write     lane t == 0 of a recording writes scores[rec][e] and, where wanted, lags[rec][e]: one writer per word, every word
// No atomics on memory, no workgroup waits for another.  Nothing is read beyond an entry's records or a recording's words: every
// loop is bounded as in the count kernel.
#include "occurrences_tail_common.hpp"

namespace lbad {
namespace {

constexpr uint32_t kRtFlight = 4;                      // steps of a cell whose reads are issued together: the count kernel's
static_assert(kTriSize * sizeof(float) == 20604 && kOcRecBytes == 36 && kOcThreads == 256 && kOcEntries == 64,
              "occurrences_tail_shape (plan.cpp) counts the LDS and the lanes with these");

// scores[rec][e] (and lags[rec][e]) for every recording of the pass and entry of the corpus, rows `pitch` words apart
__global__ __launch_bounds__(kOcThreads) void recording_tail_kernel(const OcArgs a, const OtPass p, size_t pitch, float* __restrict__ scores,
                                                                    int32_t* __restrict__ lags) {
    extern __shared__ uint4 s_dyn[];
    const OcLds s = oc_lds(s_dyn, p.per_group * a.win);
    oc_load_tri(a, s);
    const uint32_t units = ot_units(a, p);
    for (uint32_t u = blockIdx.x; u < units; u += gridDim.x) {
        const uint32_t eb = u / p.groups, group = u - eb * p.groups;
        const OtLane n = ot_lane(a, p, group);
        __syncthreads();                                       // (the unit before has left the windows)
        ot_stage(a, p, s, group);
        __syncthreads();
        const uint32_t e0 = eb * kOcEntries, e1 = a.entries - e0 < kOcEntries ? a.entries : e0 + kOcEntries;
        float* __restrict__ row = scores + (size_t)n.rec * pitch;
        int32_t* __restrict__ lag_row = lags ? lags + (size_t)n.rec * pitch : nullptr;
        const bool writer = n.has && n.t == 0u;
        for (uint32_t e = e0; e < e1; ++e) {
            uint32_t rec0, ne;
            oc_entry(a, e, &rec0, &ne);
            unsigned long long best = 0ull;                    // (no cell)
            uint32_t last = 0u;
            if (ne != 0u && ne <= a.nq) {
                uint32_t o;
                float q;
                ot_cell<kRtFlight>(a, s, n, rec0, ne, &o, &q);
                last = a.nq - ne;                              // the newest cell's offset
                const bool cell = n.t < n.d && last + 1u + n.t >= n.d;         // ot_cell's: from t, d and the offset
                if (cell && !(q < 0.0f))                       // (a value below 0 equals no score: lag 0, as the reference has it)
                    best = ((unsigned long long)__float_as_uint(q > 0.0f ? q : 0.0f) << 32) | (unsigned long long)(0xFFFFFFFFu - n.t);
                for (uint32_t m = 1u; m < p.lanes; m <<= 1) {
                    const unsigned long long other = __shfl_xor(best, (int)m, 64);
                    best = other > best ? other : best;
                }
            }
            if (writer) {
                row[e] = __uint_as_float((uint32_t)(best >> 32));
                // the winner's offset: last + 1 + t - d, t = 0xFFFFFFFF - the low word
                if (lag_row) lag_row[e] = best != 0ull ? -(int32_t)(last + 1u + (0xFFFFFFFFu - (uint32_t)best) - n.d) : 0;
            }
        }
    }
}

}  // namespace

hipError_t launch_recording_tail(const RecordingCall& c, const RecordingTailPlan& plan, uint32_t recordings, const uint32_t* d_new_counts,
                                 uint32_t max_new, uint64_t entries, uint64_t pitch) {
    if (entries == 0 || recordings == 0) return hipSuccess;
    // (oc_call_ok's with one tile, and what ties the launch to the plan: the lanes, the sub-windows and the LDS (ot_shape_ok), the
    // 32-bit unit indices, the rows)
    if (!oc_call_ok(c, 1, 0, entries) || max_new == 0 || max_new > LBAD_OCCURRENCES_TAIL_MAX_NEW) return hipErrorInvalidValue;
    if (!ot_shape_ok(c, plan, max_new) || plan.lanes == 0 || plan.lanes > 64 || (plan.lanes & (plan.lanes - 1u)) != 0 ||
        plan.recordings_per_workgroup == 0 || plan.recordings_per_workgroup * plan.lanes > kOcThreads ||
        recordings > plan.recordings_per_pass || recordings > kOcMaxRecs || oc_blocks(entries) * recordings > kOcMaxItems ||
        (uint64_t)recordings * c.n_query > 0x7FFFFFFFull || entries > pitch || !c.d_scores || !d_new_counts)
        return hipErrorInvalidValue;
    size_t lds = 0;
    OcArgs a = oc_args(c, 0, entries, 0.0f, false, &lds);                          // (no cell is tested here)
    if (!a.tri) return hipErrorOutOfMemory;
    a.win = plan.window_records;
    lds = (size_t)plan.lds_bytes;
    const OtPass p = ot_pass(plan, recordings, d_new_counts, max_new, false, false);
    static size_t ready[kMaxDevices] = {};
    const hipError_t e = oc_allow_lds(ready, lds, recording_tail_kernel);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(recording_tail_kernel, oc_grid(oc_blocks(entries) * p.groups), dim3(kOcThreads), lds, c.stream, a, p, (size_t)pitch,
                       c.d_scores, c.d_lags);
    return hipGetLastError();
}

}  // namespace lbad
