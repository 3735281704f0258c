// occurrences_tail_common.hpp -- what the tail kernels share: k_occurrences_tail.hip (the cells a push has completed as a list, and
// that list under the peak rule, one sub-fingerprint late) and k_recording_tail.hip (the same cells folded to the best per
// (recording, entry)) -- the device side, and on the host the plan's shape held against the call and the pass' arguments.
// k_occurrences_tail.hip's head states the mapping: lanes are (recording, t) cells of ONE entry, D lanes per recording, a unit is
// (block of kOcEntries entries, group of recordings) whose tail windows are staged once.  Everything here is per file (an unnamed
// namespace), as in occurrences_common.hpp.
#pragma once

#include "occurrences_common.hpp"

namespace lbad {
namespace {

// what a tail kernel needs beside OcArgs (a.win: records of ONE recording's sub-window; a.tiles = a.groups = 1)
struct OtPass {
    const uint32_t* fresh;        // the pass' new counts, one per recording
    uint32_t recs;                // recordings of the pass, a.nq records each from a.q on
    uint32_t chunked;             // a pass of one recording in entry chunks: slots are the global positions
    uint32_t max_new;             // the host's bound: 1 .. D
    uint32_t lanes, shift;        // D = 1 << shift
    uint32_t per_group;           // recordings of a workgroup: 1 .. kOcThreads / D
    uint32_t groups;              // groups of per_group recordings in the pass
    uint32_t final;               // the peaks list: the newest cell is judged too (the last of eight words: 40 bytes with or without it)
};
static_assert(sizeof(OtPass) == 40, "a pointer and eight words: the kernels' arguments lie where they lay with seven");

// a lane's place in a unit
struct OtLane {
    uint32_t rec;                 // its recording of the pass (0 where it has none)
    uint32_t t;                   // its cell among the recording's
    uint32_t d;                   // the recording's new sub-fingerprints, clamped (0: the lane has no recording)
    uint32_t sub;                 // its recording's sub-window: the first record in the LDS arrays
    unsigned long long seg;       // the lanes of its recording in the wave
    bool has;                     // the lane has a recording of the pass
};

__device__ __forceinline__ OtLane ot_lane(const OcArgs& a, const OtPass& p, uint32_t group) {
    const uint32_t slot = threadIdx.x >> p.shift;              // the recording's place in the workgroup
    const uint32_t lane = threadIdx.x & 63u;
    OtLane n;
    n.t = threadIdx.x & (p.lanes - 1u);
    n.rec = group * p.per_group + slot;
    n.has = slot < p.per_group && n.rec < p.recs;
    if (!n.has) n.rec = 0u;
    uint32_t d = n.has ? p.fresh[n.rec] : 0u;
    d = d < p.max_new ? d : p.max_new;
    n.d = d < a.nq ? d : a.nq;
    n.sub = (slot < p.per_group ? slot : 0u) * a.win;
    const unsigned long long all = p.lanes == 64u ? ~0ull : (1ull << p.lanes) - 1ull;
    n.seg = all << (lane & ~(p.lanes - 1u));
    return n;
}

// the sub-windows of a unit, between the caller's two barriers: record r of sub-window s is record n_q - win + r of recording
// group x per_group + s (inside THAT recording), zero where the pass has no such recording
__device__ __forceinline__ void ot_stage(const OcArgs& a, const OtPass& p, const OcLds& s, uint32_t group) {
    const uint32_t records = p.per_group * a.win;
    const uint32_t q0 = a.nq - a.win;
    for (uint32_t at = threadIdx.x; at < records; at += kOcThreads) {
        const uint32_t slot = at / a.win, r = at - slot * a.win;
        const uint32_t rec = group * p.per_group + slot;
        OcRec f;
        f.p = make_uint4(0u, 0u, 0u, 0u);
        f.n = f.p;
        f.row = 0u;
        if (rec < p.recs) {
            const uint4* __restrict__ q = a.q + 2u * ((size_t)rec * a.nq + q0 + r);
            f = oc_prepare<false>(q[0], q[1], a.m);
        }
        s.p[at] = f.p;
        s.n[at] = f.n;
        s.row[at] = f.row;
    }
}

// The lane's cell of one entry (rec0, ne), 1 <= ne <= n_q, wave-uniform: its offset to *o, its quotient to *q; true where the cell
// exists and matches.  A lane without a cell computes the newest one and drops it, so every read stays inside the sub-window: a
// cell at offset o reads records o - (n_q - win) .. + ne - 1 of it, at least win - ne_b - D + 1 >= 0 and at most win - 1.
template <uint32_t FLIGHT>
__device__ __forceinline__ bool ot_cell(const OcArgs& a, const OcLds& s, const OtLane& n, uint32_t rec0, uint32_t ne, uint32_t* o, float* q) {
    const uint32_t last = a.nq - ne;                           // the newest cell's offset
    const uint32_t at = last + 1u + n.t;                       // the lane's offset + d
    const bool cell = n.t < n.d && at >= n.d;
    const uint32_t off = cell ? at - n.d : last;
    uint32_t r = n.sub + off - (a.nq - a.win);
    const OcUniform ue = (OcUniform)(uintptr_t)(a.recs + 2u * (size_t)rec0);
    float sum = 0.0f;
    // FLIGHT steps in flight: their window records, entry records and quotients are independent reads; the sum stays in order
    uint32_t i = 0;
    for (; i + FLIGHT <= ne; i += FLIGHT) {
        float v[FLIGHT];
#pragma unroll
        for (uint32_t k = 0; k < FLIGHT; ++k) {
            OcRec f;
            f.p = s.p[r + k]; f.n = s.n[r + k]; f.row = s.row[r + k];
            const uint4 ep = oc_uniform(ue, 2u * (i + k)), en = oc_uniform(ue, 2u * (i + k) + 1u);
            v[k] = oc_ratio(s.tri, f, ep, en);
        }
#pragma unroll
        for (uint32_t k = 0; k < FLIGHT; ++k) sum = __fadd_rn(sum, v[k]);
        r += FLIGHT;
    }
    for (; i < ne; ++i) {
        OcRec f;
        f.p = s.p[r]; f.n = s.n[r]; f.row = s.row[r];
        ++r;
        const uint4 ep = oc_uniform(ue, 2u * i), en = oc_uniform(ue, 2u * i + 1u);
        sum = __fadd_rn(sum, oc_ratio(s.tri, f, ep, en));
    }
    const float c = __fdiv_rn(sum, (float)ne);
    *o = off;
    *q = c;
    return cell && c >= a.t;
}

__device__ __forceinline__ uint32_t ot_units(const OcArgs& a, const OtPass& p) { return ((a.entries + kOcEntries - 1u) / kOcEntries) * p.groups; }

// ---- the host side
// the plan's shape is occurrences_tail_shape's for this call at `shape_max_new` cells a recording (1 .. 64, the caller's check), and
// a workgroup's windows fit the LDS and the recordings
template <typename Plan>
inline bool ot_shape_ok(const OcPassCall& c, const Plan& plan, uint32_t shape_max_new) {
    OccurrencesTailPlan again;
    occurrences_tail_shape(c.n_query, c.ne_max, shape_max_new, &again);
    return again.lanes == plan.lanes && again.recordings_per_workgroup == plan.recordings_per_workgroup &&
           again.window_records == plan.window_records && again.lds_bytes == plan.lds_bytes && plan.lds_bytes <= 160 * 1024 - 64 &&
           plan.window_records <= c.n_query;
}

// the pass of `recordings` recordings under a plan whose shape ot_shape_ok has accepted
template <typename Plan>
inline OtPass ot_pass(const Plan& plan, uint32_t recordings, const uint32_t* d_new_counts, uint32_t max_new, bool chunked, bool final) {
    OtPass p;
    p.fresh = d_new_counts; p.recs = recordings; p.chunked = chunked ? 1u : 0u; p.max_new = max_new; p.lanes = plan.lanes;
    p.shift = (uint32_t)__builtin_ctz(plan.lanes); p.per_group = plan.recordings_per_workgroup;
    p.groups = (recordings + p.per_group - 1u) / p.per_group; p.final = final ? 1u : 0u;
    return p;
}

}  // namespace
}  // namespace lbad
