// api_occurrences_batch.cpp -- the batch occurrences and the batch recording threshold (k_occurrences_batch.hip): for MANY
// recordings of one length, packed sub-fingerprints on the device (a stream bank's windows above all), every cell of a ragged
// corpus at or above a score per recording, and every entry whose best cell reaches a score per recording, as rows of keys and
// lags with a count per recording.  The plan is occurrences_batch_plan's, here and in the debug symbol (the threshold form runs the
// batch scores pass under recording_batch_plan's key form, as the batch top-K does); the corpus' checks, the events, the staging
// buffer and the scratch are the single calls' (recording_pass.cpp, api_occurrences.cpp, api_recording.cpp), which stay as they are;
// the argument checks, the zeros and the occurrences' pass loop are recording_pass.cpp's for every list of key rows (key_rows_call).
#include "internal.hpp"

#include <atomic>

namespace lbad {
namespace {

std::atomic<uint32_t> g_force_shared{0};       // LBAudioDetectiveDebugSetOccurrencesBatchForm: measurements and tests take form S where W is legal

const PassFamily kFamily = {occurrences_tiles, occurrences_chunk_entries, occurrences_block_entries};
const PassFamily kScoresFamily = {occurrences_tiles, recording_chunk_entries, occurrences_block_entries};

OSStatus occurrences_batch_impl(LBAudioDetectiveCorpus* c, const uint32_t* d_rows, uint32_t recordings, uint32_t per, uint32_t range,
                                float threshold, uint32_t peaks, uint64_t capacity, uint64_t index_base, unsigned long long* keys,
                                int32_t* lags, unsigned long long* counts, hipStream_t stream) {
    if (!key_rows_args_ok(c, d_rows, keys, counts, recordings, per, threshold, capacity, index_base)) return kLBAudioDetectiveArgumentInvalid;
    if (!device_ready()) return kLBAudioDetectiveDeviceUnavailable;
    // what the corpus decides (pass_plan's checks, the single call's), before anything is reserved or launched
    PassQuery pq;
    pq.d_rows = d_rows; pq.per = per; pq.range = range;
    PassPlan single;
    OSStatus st = pass_plan(c, pq, index_base, kFamily, &single);
    if (st != noErr) return st;
    OccurrencesBatchPlan plan;
    if (!occurrences_batch_plan(recordings, per, single.call.ne_min, c->ne_max, c->count, c->join_scratch_limit, g_force_shared.load() != 0,
                                &plan))
        return kLBAudioDetectiveArgumentInvalid;
    if (c->count == 0) return zero_key_rows(recordings, capacity, keys, lags, counts, stream);    // nothing to compare: zeros
    KeyRows rows;
    rows.d_rows = d_rows; rows.recordings = recordings; rows.threshold = threshold; rows.peaks = peaks != 0; rows.capacity = capacity;
    rows.index_base = index_base; rows.keys = keys; rows.lags = lags; rows.counts = counts; rows.stream = stream;
    const KeyRowsPasses passes = {plan.recordings_per_pass, plan.entries_per_chunk, plan.scratch_bytes};
    return key_rows_call(c, pq, single, passes, plan.tiles, rows,
                         [&](const OccurrencesCall& call, uint32_t, uint32_t n, uint64_t e0, uint64_t m, uint32_t first,
                             unsigned long long* d_counts) {
                             return launch_occurrences_batch_chunk(call, plan, n, c->d_join_scratch, e0, m, first, d_counts);
                         });
}

// the threshold form behind the wait: pass by pass the recordings' rows, the batch scores pass into the pass' score (and lag)
// rows, the per-row compaction and its lags
OSStatus threshold_batch_launch(LBAudioDetectiveCorpus* c, const RecordingBatchPlan& plan, RecordingCall call, const uint32_t* d_rows,
                                uint32_t recordings, float threshold, uint64_t capacity, uint64_t index_base, unsigned long long* keys,
                                int32_t* lags, unsigned long long* counts) {
    const uint32_t per = call.n_query;
    const uint64_t count = c->count;
    if (c->append_event.ev) LBAD_HIP(hipStreamWaitEvent(call.stream, c->append_event, 0));
    LBAD_HIP(hipMemsetAsync(keys, 0, (size_t)recordings * capacity * sizeof(unsigned long long), call.stream));
    call.d_scores = c->d_topk_scores;
    call.d_lags = lags ? reinterpret_cast<int32_t*>(c->d_topk_scores + (size_t)plan.recordings_per_pass * count) : nullptr;
    for (uint32_t r0 = 0; r0 < recordings; r0 += plan.recordings_per_pass) {
        const uint32_t n = recordings - r0 < plan.recordings_per_pass ? recordings - r0 : plan.recordings_per_pass;
        LBAD_HIP(launch_build_query_rows(d_rows + (size_t)r0 * per * kPackedWords, n, per, c->subfp_len, true, c->d_pq, nullptr, call.stream));
        LBAD_HIP(pass_chunks(count, plan.entries_per_chunk, [&](uint64_t e0, uint64_t m) {
            return launch_recording_batch_chunk(call, plan, n, count, c->d_join_scratch, e0, m);
        }));
        unsigned long long* row_keys = keys + (size_t)r0 * capacity;
        LBAD_HIP(launch_threshold_batch_keys(call.d_scores, count, n, threshold, capacity, index_base, c->d_threshold_scratch, row_keys,
                                             counts + r0, call.stream));
        if (lags)
            LBAD_HIP(launch_recording_batch_lag_gather(row_keys, n, (uint32_t)capacity, index_base, count, call.d_lags,
                                                       lags + (size_t)r0 * capacity, call.stream));
    }
    return noErr;
}

OSStatus threshold_batch_impl(LBAudioDetectiveCorpus* c, const uint32_t* d_rows, uint32_t recordings, uint32_t per, uint32_t range,
                              float threshold, uint64_t capacity, uint64_t index_base, unsigned long long* keys,
                              unsigned long long* counts, int32_t* lags, hipStream_t stream) {
    if (!key_rows_args_ok(c, d_rows, keys, counts, recordings, per, threshold, capacity, index_base)) return kLBAudioDetectiveArgumentInvalid;
    if (!device_ready()) return kLBAudioDetectiveDeviceUnavailable;
    PassQuery pq;
    pq.d_rows = d_rows; pq.per = per; pq.range = range;
    PassPlan single;
    OSStatus st = pass_plan(c, pq, index_base, kScoresFamily, &single);
    if (st != noErr) return st;
    RecordingBatchPlan plan;
    if (!recording_batch_plan(recordings, per, single.call.ne_min, c->ne_max, c->count, c->join_scratch_limit, true,
                              g_force_shared.load() != 0, &plan))
        return kLBAudioDetectiveArgumentInvalid;
    if (c->count == 0) return zero_key_rows(recordings, capacity, keys, lags, counts, stream);    // nothing to score: zeros
    PassGuard guard(c, pq, true);
    st = guard.wait();                                     // (the scratch and the staged rows are the previous call's until then)
    if (st == noErr) st = c->d_join_scratch.reserve(plan.scratch_bytes);
    if (st == noErr) st = c->d_pq.reserve((size_t)plan.recordings_per_pass * per * kPackedWords);
    if (st == noErr) st = c->d_topk_scores.reserve((size_t)plan.recordings_per_pass * c->count * (lags ? 2 : 1));
    if (st == noErr) st = c->d_threshold_scratch.reserve(threshold_batch_scratch_bytes(c->count, plan.recordings_per_pass));
    if (st != noErr) return st;
    RecordingCall call;
    static_cast<OcPassCall&>(call) = single.call;
    call.tiles = plan.tiles; call.stream = stream;
    call.d_qwords = c->d_pq;
    return guard.finish(stream, threshold_batch_launch(c, plan, call, d_rows, recordings, threshold, capacity, index_base, keys, lags, counts));
}

}  // namespace
}  // namespace lbad

extern "C" {

OSStatus LBAudioDetectiveCorpusQueryPackedOccurrencesBatchKeysDevice(LBAudioDetectiveCorpusRef c, const void* inPackedQueries,
                                                                     UInt32 inRecordings, UInt32 inSubfingerprints, UInt32 inRange,
                                                                     Float32 inThreshold, UInt32 inPeaksOnly, UInt64 inCapacity,
                                                                     UInt64 inIndexBase, void* outKeys, void* outLags, void* outCounts,
                                                                     void* inStream) {
    LBAD_GUARD_BEGIN
    return lbad::occurrences_batch_impl(c, static_cast<const uint32_t*>(inPackedQueries), inRecordings, inSubfingerprints, inRange,
                                        inThreshold, inPeaksOnly, inCapacity, inIndexBase, static_cast<unsigned long long*>(outKeys),
                                        static_cast<int32_t*>(outLags), static_cast<unsigned long long*>(outCounts),
                                        static_cast<hipStream_t>(inStream));
    LBAD_GUARD_END
}

OSStatus LBAudioDetectiveCorpusQueryPackedRecordingThresholdBatchKeysDevice(LBAudioDetectiveCorpusRef c, const void* inPackedQueries,
                                                                            UInt32 inRecordings, UInt32 inSubfingerprints, UInt32 inRange,
                                                                            Float32 inThreshold, UInt64 inCapacity, UInt64 inIndexBase,
                                                                            void* outKeys, void* outCounts, void* outLags, void* inStream) {
    LBAD_GUARD_BEGIN
    return lbad::threshold_batch_impl(c, static_cast<const uint32_t*>(inPackedQueries), inRecordings, inSubfingerprints, inRange,
                                      inThreshold, inCapacity, inIndexBase, static_cast<unsigned long long*>(outKeys),
                                      static_cast<unsigned long long*>(outCounts), static_cast<int32_t*>(outLags),
                                      static_cast<hipStream_t>(inStream));
    LBAD_GUARD_END
}

OSStatus LBAudioDetectiveDebugOccurrencesBatchPlan(UInt32 inRecordings, UInt32 inSubfingerprints, UInt32 inShortestEntry, UInt32 inLongestEntry,
                                                   UInt64 inEntries, UInt64 inScratchLimit, UInt32* outForm, UInt64* outTiles,
                                                   UInt32* outRecordingsPerPass, UInt64* outEntriesPerChunk, UInt64* outScratchBytes,
                                                   UInt64* outLdsBytes) {
    if (!outForm || !outTiles || !outRecordingsPerPass || !outEntriesPerChunk || !outScratchBytes || !outLdsBytes || inRecordings == 0 ||
        inSubfingerprints == 0 || (uint64_t)inRecordings * inSubfingerprints > 0x7FFFFFFFull || inShortestEntry > inLongestEntry ||
        inLongestEntry > LBAD_OCCURRENCES_MAX_ENTRY_SUBFINGERPRINTS || (inEntries != 0 && inShortestEntry == 0) ||
        inEntries > 0x100000000ull)
        return kLBAudioDetectiveArgumentInvalid;
    lbad::OccurrencesBatchPlan plan;
    if (!lbad::occurrences_batch_plan(inRecordings, inSubfingerprints, inShortestEntry, inLongestEntry, inEntries, inScratchLimit,
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

OSStatus LBAudioDetectiveDebugSetOccurrencesBatchForm(UInt32 inForceShared) {
    lbad::g_force_shared.store(inForceShared ? 1u : 0u);
    return noErr;
}

}  // extern "C"
