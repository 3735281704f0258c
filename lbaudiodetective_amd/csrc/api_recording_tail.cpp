// api_recording_tail.cpp -- the recording tail (k_recording_tail.hip): of the cells a push has completed (the tail occurrences',
// api_occurrences_tail.cpp) the best per (recording, entry) -- as score and lag rows, as the K best keys per recording, or as every
// entry at or above a score per recording.  The plan is recording_tail_plan's, here and in the debug symbol; the corpus' checks,
// the events and the staging buffer are the tail occurrences call's (recording_pass.cpp); what follows a pass in the key forms is
// the batch calls' (api_recording_batch.cpp, api_occurrences_batch.cpp): launch_topk_keys, launch_threshold_batch_keys and
// launch_recording_batch_lag_gather as they are, one row per recording of a pass.
#include "internal.hpp"

#include <cmath>

namespace lbad {
namespace {

// a cell of this call is one offset of an entry not longer than the recording: ONE tile, whatever the lengths
uint64_t tail_tiles(uint32_t, uint32_t, uint32_t) { return 1; }
const PassFamily kFamily = {tail_tiles, occurrences_chunk_entries, occurrences_block_entries};

enum class Form { Scores, TopK, Threshold };

// what follows a pass, and where the results go
struct TailSelect {
    Form form = Form::Scores;
    float* scores = nullptr;             // Scores: [recordings][entries]
    uint32_t k = 0;                      // TopK
    float threshold = 0.0f;              // Threshold
    uint64_t capacity = 0;               // Threshold: slots of a row (TopK: k)
    uint64_t index_base = 0;
    unsigned long long* keys = nullptr;  // [recordings][slots]
    unsigned long long* counts = nullptr;    // Threshold: [recordings]
    int32_t* lags = nullptr;             // optional: the scores' or the keys' shape
    uint64_t slots() const { return form == Form::TopK ? k : capacity; }
};

// what needs neither handle nor device: the recordings, the new counts and their bound
bool tail_args_ok(const void* c, const void* d_rows, const void* d_new, uint32_t recordings, uint32_t per, uint32_t max_new) {
    return c && d_rows && d_new && (reinterpret_cast<uintptr_t>(d_new) & 3u) == 0 && max_new != 0 && max_new <= LBAD_OCCURRENCES_TAIL_MAX_NEW &&
           recordings != 0 && per != 0 && (uint64_t)recordings * per <= 0x7FFFFFFFull;
}

// nothing to compare, or no entry with a complete position inside the recordings: +0 scores and 0 lags, zero keys, lags and counts
OSStatus zero_outputs(const TailSelect& sel, uint32_t recordings, uint64_t entries, hipStream_t stream) {
    if (sel.form == Form::Scores) {
        const size_t words = (size_t)recordings * entries;
        if (words == 0) return noErr;                          // an empty corpus writes nothing
        LBAD_HIP(hipMemsetAsync(sel.scores, 0, words * sizeof(float), stream));
        if (sel.lags) LBAD_HIP(hipMemsetAsync(sel.lags, 0, words * sizeof(int32_t), stream));
        return noErr;
    }
    return zero_key_rows(recordings, sel.slots(), sel.keys, sel.lags, sel.counts, stream);
}

// everything behind the wait, on the call's stream: pass by pass the recordings' rows, the fold into the pass' score (and lag)
// rows -- the caller's in the scores form, the corpus' scores scratch in the key forms -- then the selection and its lags
OSStatus tail_launch(LBAudioDetectiveCorpus* c, const RecordingTailPlan& plan, RecordingCall call, const uint32_t* d_rows,
                     const uint32_t* d_new, uint32_t max_new, uint32_t recordings, const TailSelect& sel) {
    const uint32_t per = call.n_query;
    const uint64_t count = c->count;
    if (c->append_event.ev) LBAD_HIP(hipStreamWaitEvent(call.stream, c->append_event, 0));
    if (sel.form == Form::Threshold)                           // (launch_threshold_batch_keys: the caller has zeroed the keys)
        LBAD_HIP(hipMemsetAsync(sel.keys, 0, (size_t)recordings * sel.capacity * sizeof(unsigned long long), call.stream));
    for (uint32_t r0 = 0; r0 < recordings; r0 += plan.recordings_per_pass) {
        const uint32_t n = recordings - r0 < plan.recordings_per_pass ? recordings - r0 : plan.recordings_per_pass;
        LBAD_HIP(launch_build_query_rows(d_rows + (size_t)r0 * per * kPackedWords, n, per, c->subfp_len, true, c->d_pq, nullptr, call.stream));
        if (sel.form == Form::Scores) {
            call.d_scores = sel.scores + (size_t)r0 * count;
            call.d_lags = sel.lags ? sel.lags + (size_t)r0 * count : nullptr;
        } else {
            // the pass' score rows and, behind them, its lag rows
            call.d_scores = c->d_topk_scores;
            call.d_lags = sel.lags ? reinterpret_cast<int32_t*>(c->d_topk_scores + (size_t)plan.recordings_per_pass * count) : nullptr;
        }
        LBAD_HIP(launch_recording_tail(call, plan, n, d_new + r0, max_new, count, count));
        if (sel.form == Form::Scores) continue;
        const uint64_t slots = sel.slots();
        unsigned long long* keys = sel.keys + (size_t)r0 * slots;
        if (sel.form == Form::TopK)
            LBAD_HIP(launch_topk_keys(call.d_scores, count, n, sel.k, sel.index_base, c->d_topk_scratch, keys, call.stream));
        else
            LBAD_HIP(launch_threshold_batch_keys(call.d_scores, count, n, sel.threshold, sel.capacity, sel.index_base, c->d_threshold_scratch,
                                                 keys, sel.counts + r0, call.stream));
        if (sel.lags)
            LBAD_HIP(launch_recording_batch_lag_gather(keys, n, (uint32_t)slots, sel.index_base, count, call.d_lags,
                                                       sel.lags + (size_t)r0 * slots, call.stream));
    }
    return noErr;
}

// One call.  The caller has checked what needs no handle, and the device.
OSStatus tail_impl(LBAudioDetectiveCorpus* c, const uint32_t* d_rows, uint32_t recordings, uint32_t per, const uint32_t* d_new,
                   uint32_t max_new, uint32_t range, const TailSelect& sel, hipStream_t stream) {
    const bool keyed = sel.form != Form::Scores;
    // what the corpus decides (pass_plan's checks, the tail occurrences call's), before anything is reserved or launched
    PassQuery pq;
    pq.d_rows = d_rows; pq.per = per; pq.range = range;
    PassPlan single;
    OSStatus st = pass_plan(c, pq, keyed ? sel.index_base : 0, kFamily, &single);
    if (st != noErr) return st;
    if (!keyed && (uint64_t)recordings * c->count > 0x7FFFFFFFull) return kLBAudioDetectiveArgumentInvalid;
    RecordingTailPlan plan;
    recording_tail_plan(recordings, per, c->ne_max, c->count, max_new, c->join_scratch_limit, keyed, &plan);
    if (c->count == 0 || !single.any) return zero_outputs(sel, recordings, c->count, stream);
    PassGuard guard(c, pq, keyed);
    st = guard.wait();                                     // (the scratch and the staged rows are the previous call's until then)
    if (st == noErr) st = c->d_pq.reserve((size_t)plan.recordings_per_pass * per * kPackedWords);
    if (st == noErr && keyed) {
        st = c->d_topk_scores.reserve((size_t)plan.recordings_per_pass * c->count * (sel.lags ? 2 : 1));
        if (st == noErr)
            st = sel.form == Form::TopK ? c->d_topk_scratch.reserve(topk_scratch_bytes(plan.recordings_per_pass))
                                        : c->d_threshold_scratch.reserve(threshold_batch_scratch_bytes(c->count, plan.recordings_per_pass));
    }
    if (st != noErr) return st;
    RecordingCall call;
    static_cast<OcPassCall&>(call) = single.call;
    call.tiles = 1; call.stream = stream;
    call.d_qwords = c->d_pq;
    return guard.finish(stream, tail_launch(c, plan, call, d_rows, d_new, max_new, recordings, sel));
}

}  // namespace
}  // namespace lbad

extern "C" {

OSStatus LBAudioDetectiveCorpusRecordingPackedScoresTailBatchDevice(LBAudioDetectiveCorpusRef c, const void* inPackedQueries, UInt32 inRecordings,
                                                                    UInt32 inSubfingerprints, const void* inNewCounts, UInt32 inMaxNew,
                                                                    UInt32 inRange, Float32* outScores, SInt32* outLags, void* inStream) {
    LBAD_GUARD_BEGIN
    if (!lbad::tail_args_ok(c, inPackedQueries, inNewCounts, inRecordings, inSubfingerprints, inMaxNew) || !outScores)
        return kLBAudioDetectiveArgumentInvalid;
    if (!lbad::device_ready()) return kLBAudioDetectiveDeviceUnavailable;
    lbad::TailSelect sel;
    sel.form = lbad::Form::Scores; sel.scores = outScores; sel.lags = outLags;
    return lbad::tail_impl(c, static_cast<const uint32_t*>(inPackedQueries), inRecordings, inSubfingerprints,
                           static_cast<const uint32_t*>(inNewCounts), inMaxNew, inRange, sel, static_cast<hipStream_t>(inStream));
    LBAD_GUARD_END
}

OSStatus LBAudioDetectiveCorpusQueryPackedRecordingTopKTailBatchKeysDevice(LBAudioDetectiveCorpusRef c, const void* inPackedQueries,
                                                                           UInt32 inRecordings, UInt32 inSubfingerprints,
                                                                           const void* inNewCounts, UInt32 inMaxNew, UInt32 inRange,
                                                                           UInt32 inK, UInt64 inIndexBase, void* outKeys, void* outLags,
                                                                           void* inStream) {
    LBAD_GUARD_BEGIN
    if (!lbad::tail_args_ok(c, inPackedQueries, inNewCounts, inRecordings, inSubfingerprints, inMaxNew) || !outKeys || inK == 0 ||
        inK > lbad::kTopKMax || inIndexBase > 0x100000000ull || (uint64_t)inRecordings * inK > 0x80000000ull)
        return kLBAudioDetectiveArgumentInvalid;
    if (!lbad::device_ready()) return kLBAudioDetectiveDeviceUnavailable;
    lbad::TailSelect sel;
    sel.form = lbad::Form::TopK; sel.k = inK; sel.index_base = inIndexBase;
    sel.keys = static_cast<unsigned long long*>(outKeys); sel.lags = static_cast<int32_t*>(outLags);
    return lbad::tail_impl(c, static_cast<const uint32_t*>(inPackedQueries), inRecordings, inSubfingerprints,
                           static_cast<const uint32_t*>(inNewCounts), inMaxNew, inRange, sel, static_cast<hipStream_t>(inStream));
    LBAD_GUARD_END
}

OSStatus LBAudioDetectiveCorpusQueryPackedRecordingThresholdTailBatchKeysDevice(LBAudioDetectiveCorpusRef c, const void* inPackedQueries,
                                                                                UInt32 inRecordings, UInt32 inSubfingerprints,
                                                                                const void* inNewCounts, UInt32 inMaxNew, UInt32 inRange,
                                                                                Float32 inThreshold, UInt64 inCapacity, UInt64 inIndexBase,
                                                                                void* outKeys, void* outCounts, void* outLags, void* inStream) {
    LBAD_GUARD_BEGIN
    // (the threshold and capacity limits are the batch recording threshold's)
    if (!lbad::tail_args_ok(c, inPackedQueries, inNewCounts, inRecordings, inSubfingerprints, inMaxNew) || !outKeys || !outCounts ||
        !std::isfinite(inThreshold) || !(inThreshold > 0.0f) || inCapacity == 0 || inCapacity > 0x80000000ull ||
        (uint64_t)inRecordings * inCapacity > 0x80000000ull || inIndexBase > 0x100000000ull)
        return kLBAudioDetectiveArgumentInvalid;
    if (!lbad::device_ready()) return kLBAudioDetectiveDeviceUnavailable;
    lbad::TailSelect sel;
    sel.form = lbad::Form::Threshold; sel.threshold = inThreshold; sel.capacity = inCapacity; sel.index_base = inIndexBase;
    sel.keys = static_cast<unsigned long long*>(outKeys); sel.counts = static_cast<unsigned long long*>(outCounts);
    sel.lags = static_cast<int32_t*>(outLags);
    return lbad::tail_impl(c, static_cast<const uint32_t*>(inPackedQueries), inRecordings, inSubfingerprints,
                           static_cast<const uint32_t*>(inNewCounts), inMaxNew, inRange, sel, static_cast<hipStream_t>(inStream));
    LBAD_GUARD_END
}

OSStatus LBAudioDetectiveDebugRecordingTailPlan(UInt32 inRecordings, UInt32 inSubfingerprints, UInt32 inLongestEntry, UInt64 inEntries,
                                                UInt32 inMaxNew, UInt64 inScratchLimit, UInt32 inKeyForm, UInt32* outLanes,
                                                UInt32* outRecordingsPerWorkgroup, UInt32* outWindowRecords, UInt64* outLdsBytes,
                                                UInt32* outRecordingsPerPass, UInt64* outScratchBytes) {
    if (!outLanes || !outRecordingsPerWorkgroup || !outWindowRecords || !outLdsBytes || !outRecordingsPerPass || !outScratchBytes ||
        inRecordings == 0 || inSubfingerprints == 0 || (uint64_t)inRecordings * inSubfingerprints > 0x7FFFFFFFull ||
        inLongestEntry > LBAD_OCCURRENCES_MAX_ENTRY_SUBFINGERPRINTS || (inEntries != 0 && inLongestEntry == 0) ||
        inEntries > 0x100000000ull || inMaxNew == 0 || inMaxNew > LBAD_OCCURRENCES_TAIL_MAX_NEW ||
        (!inKeyForm && (uint64_t)inRecordings * inEntries > 0x7FFFFFFFull))
        return kLBAudioDetectiveArgumentInvalid;
    lbad::RecordingTailPlan plan;
    lbad::recording_tail_plan(inRecordings, inSubfingerprints, inLongestEntry, inEntries, inMaxNew, inScratchLimit, inKeyForm != 0, &plan);
    *outLanes = plan.lanes;
    *outRecordingsPerWorkgroup = plan.recordings_per_workgroup;
    *outWindowRecords = plan.window_records;
    *outLdsBytes = plan.lds_bytes;
    *outRecordingsPerPass = plan.recordings_per_pass;
    *outScratchBytes = plan.scratch_bytes;
    return noErr;
}

}  // extern "C"
