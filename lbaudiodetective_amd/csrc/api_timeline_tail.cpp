// api_timeline_tail.cpp -- the timeline tail (k_timeline_tail.hip): every channel's timeline kept current from a push -- the
// previous timeline shifted left by the channel's new count, merged by unsigned maximum with the cells the push completed (the
// tail occurrences', api_occurrences_tail.cpp) folded per offset.  The plan is timeline_tail_plan's, here and in the debug symbol;
// the corpus' checks, the events and the staging buffer are the tail calls' (recording_pass.cpp); the strips of a pass live in the
// join scratch.
#include "internal.hpp"

#include <cmath>

namespace lbad {
namespace {

// a cell of this call is one offset of an entry not longer than the recording: ONE tile, whatever the lengths
uint64_t tail_tiles(uint32_t, uint32_t, uint32_t) { return 1; }
// (the strips do not grow with the entries: whatever the limit, the "chunk" is the corpus; timeline_tail_plan judges the limit)
uint64_t tail_chunk_entries(uint64_t, uint64_t) { return kMaxRaggedEntries; }
const PassFamily kFamily = {tail_tiles, tail_chunk_entries, occurrences_block_entries};

struct TailRows {
    const uint32_t* d_rows = nullptr;    // [recordings][per][8]
    const uint32_t* d_new = nullptr;     // [recordings]
    const unsigned long long* prev = nullptr;    // optional: [recordings][per]
    unsigned long long* keys = nullptr;  // [recordings][per]
    uint32_t* lengths = nullptr;         // optional: likewise
    uint32_t recordings = 0, max_new = 0;
};

// everything behind the wait, on the call's stream: pass by pass the recordings' rows, zero strips, the cells, the rows
OSStatus tail_launch(LBAudioDetectiveCorpus* c, const TimelineTailPlan& plan, TimelineCall call, const TailRows& rows) {
    const uint32_t per = call.n_query;
    if (c->append_event.ev) LBAD_HIP(hipStreamWaitEvent(call.stream, c->append_event, 0));
    unsigned long long* strips = static_cast<unsigned long long*>(c->d_join_scratch.get());
    for (uint32_t r0 = 0; r0 < rows.recordings; r0 += plan.recordings_per_pass) {
        const uint32_t n = rows.recordings - r0 < plan.recordings_per_pass ? rows.recordings - r0 : plan.recordings_per_pass;
        LBAD_HIP(launch_build_query_rows(rows.d_rows + (size_t)r0 * per * kPackedWords, n, per, c->subfp_len, true, c->d_pq, nullptr,
                                         call.stream));
        LBAD_HIP(hipMemsetAsync(strips, 0, (size_t)n * plan.strip_width * sizeof(unsigned long long), call.stream));
        LBAD_HIP(launch_timeline_tail_cells(call, plan, n, rows.d_new + r0, rows.max_new, c->count, strips));
        LBAD_HIP(launch_timeline_tail_finish(strips, plan.strip_width, call.ne_min, n, per, rows.d_new + r0,
                                             rows.prev ? rows.prev + (size_t)r0 * per : nullptr, call.index_base, c->count, c->d_off,
                                             rows.keys + (size_t)r0 * per, rows.lengths ? rows.lengths + (size_t)r0 * per : nullptr,
                                             call.stream));
    }
    return noErr;
}

// One call.  The caller has checked what needs no handle, and the device.
OSStatus tail_impl(LBAudioDetectiveCorpus* c, const TailRows& rows, uint32_t per, uint32_t range, float threshold, uint64_t index_base,
                   hipStream_t stream) {
    // what the corpus decides (pass_plan's checks, the tail occurrences call's), before anything is reserved or launched
    PassQuery pq;
    pq.d_rows = rows.d_rows; pq.per = per; pq.range = range;
    PassPlan single;
    OSStatus st = pass_plan(c, pq, index_base, kFamily, &single);
    if (st != noErr) return st;
    TimelineTailPlan plan;
    if (!timeline_tail_plan(rows.recordings, per, single.call.ne_min, c->ne_max, c->count, rows.max_new, c->join_scratch_limit, &plan))
        return kLBAudioDetectiveArgumentInvalid;
    if (c->count == 0 || !single.any) {
        // no cell: the shifted previous rows (zeros without them), on the stream behind the corpus' latest append like every result
        if (c->append_event.ev) LBAD_HIP(hipStreamWaitEvent(stream, c->append_event, 0));
        LBAD_HIP(launch_timeline_tail_finish(nullptr, 0, 0, rows.recordings, per, rows.d_new, rows.prev, index_base, c->count, c->d_off,
                                             rows.keys, rows.lengths, stream));
        return noErr;
    }
    PassGuard guard(c, pq, false);
    st = guard.wait();                                     // (the scratch and the staged rows are the previous call's until then)
    if (st == noErr) st = c->d_join_scratch.reserve(plan.scratch_bytes);
    if (st == noErr) st = c->d_pq.reserve((size_t)plan.recordings_per_pass * per * kPackedWords);
    if (st != noErr) return st;
    TimelineCall call;
    static_cast<OcPassCall&>(call) = single.call;
    call.tiles = 1; call.stream = stream;
    call.d_qwords = c->d_pq;
    call.threshold = threshold; call.index_base = index_base;
    return guard.finish(stream, tail_launch(c, plan, call, rows));
}

}  // namespace
}  // namespace lbad

extern "C" {

OSStatus LBAudioDetectiveCorpusRecordingPackedTimelineTailBatchKeysDevice(LBAudioDetectiveCorpusRef c, const void* inPackedQueries,
                                                                          UInt32 inRecordings, UInt32 inSubfingerprints,
                                                                          const void* inNewCounts, UInt32 inMaxNew, UInt32 inRange,
                                                                          Float32 inThreshold, UInt64 inIndexBase, const void* inPrevKeys,
                                                                          void* outKeys, void* outLengths, void* inStream) {
    LBAD_GUARD_BEGIN
    // what needs neither handle nor device, in the tail calls' order
    if (!c || !inPackedQueries || !inNewCounts || (reinterpret_cast<uintptr_t>(inNewCounts) & 3u) != 0 || inMaxNew == 0 ||
        inMaxNew > LBAD_OCCURRENCES_TAIL_MAX_NEW || inRecordings == 0 || inSubfingerprints == 0 ||
        (uint64_t)inRecordings * inSubfingerprints > 0x7FFFFFFFull || !outKeys || !std::isfinite(inThreshold) || !(inThreshold > 0.0f) ||
        inIndexBase > 0x100000000ull)
        return kLBAudioDetectiveArgumentInvalid;
    if (inPrevKeys) {                                      // the previous rows are read while the new ones are written
        const uint64_t bytes = (uint64_t)inRecordings * inSubfingerprints * sizeof(unsigned long long);
        const uintptr_t a = reinterpret_cast<uintptr_t>(inPrevKeys), b = reinterpret_cast<uintptr_t>(outKeys);
        if (a < b ? b - a < bytes : a - b < bytes) return kLBAudioDetectiveArgumentInvalid;
    }
    if (!lbad::device_ready()) return kLBAudioDetectiveDeviceUnavailable;
    lbad::TailRows rows;
    rows.d_rows = static_cast<const uint32_t*>(inPackedQueries); rows.d_new = static_cast<const uint32_t*>(inNewCounts);
    rows.prev = static_cast<const unsigned long long*>(inPrevKeys); rows.keys = static_cast<unsigned long long*>(outKeys);
    rows.lengths = static_cast<uint32_t*>(outLengths); rows.recordings = inRecordings; rows.max_new = inMaxNew;
    return lbad::tail_impl(c, rows, inSubfingerprints, inRange, inThreshold, inIndexBase, static_cast<hipStream_t>(inStream));
    LBAD_GUARD_END
}

OSStatus LBAudioDetectiveDebugTimelineTailPlan(UInt32 inRecordings, UInt32 inSubfingerprints, UInt32 inShortestEntry, UInt32 inLongestEntry,
                                               UInt64 inEntries, UInt32 inMaxNew, UInt64 inScratchLimit, UInt32* outLanes,
                                               UInt32* outRecordingsPerWorkgroup, UInt32* outWindowRecords, UInt32* outStripWidth,
                                               UInt64* outLdsBytes, UInt32* outRecordingsPerPass, UInt64* outScratchBytes) {
    if (!outLanes || !outRecordingsPerWorkgroup || !outWindowRecords || !outStripWidth || !outLdsBytes || !outRecordingsPerPass ||
        !outScratchBytes || inRecordings == 0 || inSubfingerprints == 0 || (uint64_t)inRecordings * inSubfingerprints > 0x7FFFFFFFull ||
        inShortestEntry > inLongestEntry || inLongestEntry > LBAD_OCCURRENCES_MAX_ENTRY_SUBFINGERPRINTS ||
        (inEntries != 0 && inShortestEntry == 0) || inEntries > 0x100000000ull || inMaxNew == 0 || inMaxNew > LBAD_OCCURRENCES_TAIL_MAX_NEW)
        return kLBAudioDetectiveArgumentInvalid;
    lbad::TimelineTailPlan plan;
    if (!lbad::timeline_tail_plan(inRecordings, inSubfingerprints, inShortestEntry, inLongestEntry, inEntries, inMaxNew, inScratchLimit, &plan))
        return kLBAudioDetectiveArgumentInvalid;
    *outLanes = plan.lanes;
    *outRecordingsPerWorkgroup = plan.recordings_per_workgroup;
    *outWindowRecords = plan.window_records;
    *outStripWidth = plan.strip_width;
    *outLdsBytes = plan.lds_bytes;
    *outRecordingsPerPass = plan.recordings_per_pass;
    *outScratchBytes = plan.scratch_bytes;
    return noErr;
}

}  // extern "C"
