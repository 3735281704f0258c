// api_timeline_batch.cpp -- the batch recording timeline (k_timeline_batch.hip): the best entry of a ragged corpus at every offset
// of MANY recordings of one length, packed sub-fingerprints on the device (a stream bank's windows above all), as keys and lengths
// on the device.  The plan is timeline_batch_plan's, here and in the debug symbol; the events, the staging buffer and the scratch
// are the single call's (recording_pass.cpp, api_timeline.cpp), which stays as it is.
#include "internal.hpp"

#include <atomic>
#include <cmath>

namespace lbad {
namespace {

std::atomic<uint32_t> g_force_shared{0};       // LBAudioDetectiveDebugSetTimelineBatchForm: measurements and tests take form S where W is legal

// everything behind the wait, on the call's stream: pass by pass the recordings' rows, the chunks into the keys, then the lengths
OSStatus timeline_batch_launch(LBAudioDetectiveCorpus* c, const TimelineBatchPlan& plan, TimelineCall call, const uint32_t* d_rows,
                               uint32_t recordings, unsigned long long* keys, uint32_t* lengths) {
    const uint32_t per = call.n_query;
    if (c->append_event.ev) LBAD_HIP(hipStreamWaitEvent(call.stream, c->append_event, 0));
    for (uint32_t r0 = 0; r0 < recordings; r0 += plan.recordings_per_pass) {
        const uint32_t n = recordings - r0 < plan.recordings_per_pass ? recordings - r0 : plan.recordings_per_pass;
        LBAD_HIP(launch_build_query_rows(d_rows + (size_t)r0 * per * kPackedWords, n, per, c->subfp_len, true, c->d_pq, nullptr, call.stream));
        call.d_keys = keys + (size_t)r0 * per;
        LBAD_HIP(pass_chunks(c->count, plan.entries_per_chunk,
                             [&](uint64_t e0, uint64_t m) { return launch_timeline_batch_chunk(call, plan, n, c->d_join_scratch, e0, m); }));
    }
    if (lengths)
        LBAD_HIP(launch_timeline_lengths(keys, recordings * per, call.index_base, c->count, c->d_off, lengths, call.stream));
    return noErr;
}

OSStatus timeline_batch_impl(LBAudioDetectiveCorpus* c, const uint32_t* d_rows, uint32_t recordings, uint32_t per, uint32_t range,
                             float threshold, uint64_t index_base, unsigned long long* keys, uint32_t* lengths, hipStream_t stream) {
    // what needs neither handle nor device
    if (!c || !d_rows || !keys || recordings == 0 || per == 0 || (uint64_t)recordings * per > 0x7FFFFFFFull || !std::isfinite(threshold) ||
        !(threshold > 0.0f) || index_base > 0x100000000ull)
        return kLBAudioDetectiveArgumentInvalid;
    if (!device_ready()) return kLBAudioDetectiveDeviceUnavailable;
    // what the corpus decides (pass_plan's checks), before anything is reserved or launched
    if (!c->ragged || c->ne_max > LBAD_OCCURRENCES_MAX_ENTRY_SUBFINGERPRINTS || index_base + c->count > 0x100000000ull)
        return kLBAudioDetectiveArgumentInvalid;
    const uint32_t ne_min = c->count ? c->len_hist.begin()->first : 0;
    TimelineBatchPlan plan;
    if (!timeline_batch_plan(recordings, per, ne_min, c->ne_max, c->count, c->join_scratch_limit, g_force_shared.load() != 0, &plan))
        return kLBAudioDetectiveArgumentInvalid;
    // the keys carry the running maximum from chunk to chunk: zeros in front of the first.  Where no entry takes part these
    // zeros (and the lengths') are the answer.
    const size_t cells = (size_t)recordings * per;
    LBAD_HIP(hipMemsetAsync(keys, 0, cells * sizeof(unsigned long long), stream));
    if (c->count == 0 || ne_min > per) {
        if (lengths) LBAD_HIP(hipMemsetAsync(lengths, 0, cells * sizeof(uint32_t), stream));
        return noErr;
    }
    PassQuery pq;
    pq.d_rows = d_rows; pq.per = per; pq.range = range;
    PassGuard guard(c, pq, false);
    OSStatus st = guard.wait();                            // (the scratch and the staged rows are the previous call's until then)
    if (st == noErr) st = c->d_join_scratch.reserve(plan.scratch_bytes);
    if (st == noErr) st = c->d_pq.reserve((size_t)plan.recordings_per_pass * per * kPackedWords);
    if (st != noErr) return st;
    TimelineCall call;
    call.d_recs = c->d_recs; call.d_off = c->d_off; call.ne_min = ne_min; call.ne_max = c->ne_max; call.subfp_len = c->subfp_len;
    call.range = range ? range : c->subfp_len; call.n_query = per; call.tiles = plan.tiles; call.stream = stream;
    call.d_qwords = c->d_pq;
    call.threshold = threshold; call.index_base = index_base;
    return guard.finish(stream, timeline_batch_launch(c, plan, call, d_rows, recordings, keys, lengths));
}

}  // namespace
}  // namespace lbad

extern "C" {

OSStatus LBAudioDetectiveCorpusRecordingPackedTimelineBatchKeysDevice(LBAudioDetectiveCorpusRef c, const void* inPackedQueries,
                                                                      UInt32 inRecordings, UInt32 inSubfingerprints, UInt32 inRange,
                                                                      Float32 inThreshold, UInt64 inIndexBase, void* outKeys,
                                                                      void* outLengths, void* inStream) {
    LBAD_GUARD_BEGIN
    return lbad::timeline_batch_impl(c, static_cast<const uint32_t*>(inPackedQueries), inRecordings, inSubfingerprints, inRange, inThreshold,
                                     inIndexBase, static_cast<unsigned long long*>(outKeys), static_cast<uint32_t*>(outLengths),
                                     static_cast<hipStream_t>(inStream));
    LBAD_GUARD_END
}

OSStatus LBAudioDetectiveDebugTimelineBatchPlan(UInt32 inRecordings, UInt32 inSubfingerprints, UInt32 inShortestEntry, UInt32 inLongestEntry,
                                                UInt64 inEntries, UInt64 inScratchLimit, UInt32* outForm, UInt64* outTiles,
                                                UInt32* outRecordingsPerPass, UInt64* outEntriesPerChunk, UInt64* outScratchBytes,
                                                UInt64* outLdsBytes) {
    if (!outForm || !outTiles || !outRecordingsPerPass || !outEntriesPerChunk || !outScratchBytes || !outLdsBytes || inRecordings == 0 ||
        inSubfingerprints == 0 || (uint64_t)inRecordings * inSubfingerprints > 0x7FFFFFFFull || inShortestEntry > inLongestEntry ||
        inLongestEntry > LBAD_OCCURRENCES_MAX_ENTRY_SUBFINGERPRINTS || (inEntries != 0 && inShortestEntry == 0) ||
        inEntries > 0x100000000ull)
        return kLBAudioDetectiveArgumentInvalid;
    lbad::TimelineBatchPlan plan;
    if (!lbad::timeline_batch_plan(inRecordings, inSubfingerprints, inShortestEntry, inLongestEntry, inEntries, inScratchLimit,
                                   lbad::g_force_shared.load() != 0, &plan))
        return kLBAudioDetectiveArgumentInvalid;
    *outForm = plan.form;
    *outTiles = plan.tiles;
    *outRecordingsPerPass = plan.recordings_per_pass;
    *outEntriesPerChunk = plan.entries_per_chunk;
    *outScratchBytes = plan.scratch_bytes;
    *outLdsBytes = plan.lds_bytes;
    return noErr;
}

OSStatus LBAudioDetectiveDebugSetTimelineBatchForm(UInt32 inForceShared) {
    lbad::g_force_shared.store(inForceShared ? 1u : 0u);
    return noErr;
}

}  // extern "C"
