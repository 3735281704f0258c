// api_recording_batch.cpp -- the batch recording scores and the batch recording top-K (k_recording_batch.hip): scores and lags
// of a ragged corpus for MANY recordings of one length, packed sub-fingerprints on the device (a stream bank's windows above all),
// per entry or as the K best keys per recording with their lags.  The plan is recording_batch_plan's, here and in the debug symbol;
// the corpus' checks, the events, the staging buffer and the scratch are the single call's (recording_pass.cpp, api_recording.cpp),
// which stays as it is; the selection is launch_topk_keys as it is, one row per recording of a pass.
#include "internal.hpp"

#include <atomic>

namespace lbad {
namespace {

std::atomic<uint32_t> g_force_shared{0};       // LBAudioDetectiveDebugSetRecordingBatchForm: measurements and tests take form S where W is legal

const PassFamily kFamily = {occurrences_tiles, recording_chunk_entries, occurrences_block_entries};

// what follows a pass in the key form
struct BatchSelect {
    uint32_t k = 0;
    uint64_t index_base = 0;
    unsigned long long* keys = nullptr;  // [recordings][k]
    int32_t* lags = nullptr;             // optional, the same shape
};

// everything behind the wait, on the call's stream: pass by pass the recordings' rows, the chunks into the pass' score (and lag)
// rows, then the selection and its lags
OSStatus recording_batch_launch(LBAudioDetectiveCorpus* c, const RecordingBatchPlan& plan, RecordingCall call, const uint32_t* d_rows,
                                uint32_t recordings, float* out_scores, int32_t* out_lags, const BatchSelect* sel) {
    const uint32_t per = call.n_query;
    const uint64_t count = c->count;
    if (c->append_event.ev) LBAD_HIP(hipStreamWaitEvent(call.stream, c->append_event, 0));
    for (uint32_t r0 = 0; r0 < recordings; r0 += plan.recordings_per_pass) {
        const uint32_t n = recordings - r0 < plan.recordings_per_pass ? recordings - r0 : plan.recordings_per_pass;
        LBAD_HIP(launch_build_query_rows(d_rows + (size_t)r0 * per * kPackedWords, n, per, c->subfp_len, true, c->d_pq, nullptr, call.stream));
        if (sel) {
            // the pass' score rows and, behind them, its lag rows
            call.d_scores = c->d_topk_scores;
            call.d_lags = sel->lags ? reinterpret_cast<int32_t*>(c->d_topk_scores + (size_t)plan.recordings_per_pass * count) : nullptr;
        } else {
            call.d_scores = out_scores + (size_t)r0 * count;
            call.d_lags = out_lags ? out_lags + (size_t)r0 * count : nullptr;
        }
        LBAD_HIP(pass_chunks(count, plan.entries_per_chunk, [&](uint64_t e0, uint64_t m) {
            return launch_recording_batch_chunk(call, plan, n, count, c->d_join_scratch, e0, m);
        }));
        if (!sel) continue;
        unsigned long long* keys = sel->keys + (size_t)r0 * sel->k;
        LBAD_HIP(launch_topk_keys(call.d_scores, count, n, sel->k, sel->index_base, c->d_topk_scratch, keys, call.stream));
        if (sel->lags)
            LBAD_HIP(launch_recording_batch_lag_gather(keys, n, sel->k, sel->index_base, count, call.d_lags, sel->lags + (size_t)r0 * sel->k,
                                                       call.stream));
    }
    return noErr;
}

// One call.  The caller has checked what needs no handle, and the device.  sel == nullptr: the per-entry form, out_scores (and
// out_lags, optional) the caller's.  Otherwise the passes' scores and entry lags lie in the corpus' scores scratch, under topk_ev.
OSStatus recording_batch_impl(LBAudioDetectiveCorpus* c, const uint32_t* d_rows, uint32_t recordings, uint32_t per, uint32_t range,
                              float* out_scores, int32_t* out_lags, const BatchSelect* sel, hipStream_t stream) {
    // what the corpus decides (pass_plan's checks, the single call's), before anything is reserved or launched
    PassQuery pq;
    pq.d_rows = d_rows; pq.per = per; pq.range = range;
    PassPlan single;
    OSStatus st = pass_plan(c, pq, sel ? sel->index_base : 0, kFamily, &single);
    if (st != noErr) return st;
    if (!sel && (uint64_t)recordings * c->count > 0x7FFFFFFFull) return kLBAudioDetectiveArgumentInvalid;
    RecordingBatchPlan plan;
    if (!recording_batch_plan(recordings, per, single.call.ne_min, c->ne_max, c->count, c->join_scratch_limit, sel != nullptr,
                              g_force_shared.load() != 0, &plan))
        return kLBAudioDetectiveArgumentInvalid;
    if (c->count == 0) {                                   // nothing to score: the scores form writes nothing, the key form zeros
        if (!sel) return noErr;
        const size_t slots = (size_t)recordings * sel->k;
        LBAD_HIP(hipMemsetAsync(sel->keys, 0, slots * sizeof(unsigned long long), stream));
        if (sel->lags) LBAD_HIP(hipMemsetAsync(sel->lags, 0, slots * sizeof(int32_t), stream));
        return noErr;
    }
    PassGuard guard(c, pq, sel != nullptr);
    st = guard.wait();                                     // (the scratch and the staged rows are the previous call's until then)
    if (st == noErr) st = c->d_join_scratch.reserve(plan.scratch_bytes);
    if (st == noErr) st = c->d_pq.reserve((size_t)plan.recordings_per_pass * per * kPackedWords);
    if (st == noErr && sel) {
        st = c->d_topk_scores.reserve((size_t)plan.recordings_per_pass * c->count * (sel->lags ? 2 : 1));
        if (st == noErr) st = c->d_topk_scratch.reserve(topk_scratch_bytes(plan.recordings_per_pass));
    }
    if (st != noErr) return st;
    RecordingCall call;
    static_cast<OcPassCall&>(call) = single.call;
    call.tiles = plan.tiles; call.stream = stream;
    call.d_qwords = c->d_pq;
    return guard.finish(stream, recording_batch_launch(c, plan, call, d_rows, recordings, out_scores, out_lags, sel));
}

bool batch_ok(const void* c, const void* d_rows, uint32_t recordings, uint32_t per) {
    return c && d_rows && recordings != 0 && per != 0 && (uint64_t)recordings * per <= 0x7FFFFFFFull;
}

OSStatus scores_batch_impl(LBAudioDetectiveCorpus* c, const uint32_t* d_rows, uint32_t recordings, uint32_t per, uint32_t range, float* scores,
                           int32_t* lags, hipStream_t stream) {
    if (!batch_ok(c, d_rows, recordings, per) || !scores) return kLBAudioDetectiveArgumentInvalid;
    if (!device_ready()) return kLBAudioDetectiveDeviceUnavailable;
    return recording_batch_impl(c, d_rows, recordings, per, range, scores, lags, nullptr, stream);
}

OSStatus topk_batch_impl(LBAudioDetectiveCorpus* c, const uint32_t* d_rows, uint32_t recordings, uint32_t per, uint32_t range, uint32_t k,
                         uint64_t index_base, unsigned long long* keys, int32_t* lags, hipStream_t stream) {
    if (!batch_ok(c, d_rows, recordings, per) || !keys || k == 0 || k > kTopKMax || index_base > 0x100000000ull ||
        (uint64_t)recordings * k > 0x80000000ull)
        return kLBAudioDetectiveArgumentInvalid;
    if (!device_ready()) return kLBAudioDetectiveDeviceUnavailable;
    BatchSelect sel;
    sel.k = k; sel.index_base = index_base; sel.keys = keys; sel.lags = lags;
    return recording_batch_impl(c, d_rows, recordings, per, range, nullptr, nullptr, &sel, stream);
}

}  // namespace
}  // namespace lbad

extern "C" {

OSStatus LBAudioDetectiveCorpusRecordingPackedScoresBatchDevice(LBAudioDetectiveCorpusRef c, const void* inPackedQueries, UInt32 inRecordings,
                                                                UInt32 inSubfingerprints, UInt32 inRange, Float32* outScores,
                                                                SInt32* outLags, void* inStream) {
    LBAD_GUARD_BEGIN
    return lbad::scores_batch_impl(c, static_cast<const uint32_t*>(inPackedQueries), inRecordings, inSubfingerprints, inRange, outScores,
                                   outLags, static_cast<hipStream_t>(inStream));
    LBAD_GUARD_END
}

OSStatus LBAudioDetectiveCorpusQueryPackedRecordingTopKBatchKeysDevice(LBAudioDetectiveCorpusRef c, const void* inPackedQueries,
                                                                       UInt32 inRecordings, UInt32 inSubfingerprints, UInt32 inRange,
                                                                       UInt32 inK, UInt64 inIndexBase, void* outKeys, void* outLags,
                                                                       void* inStream) {
    LBAD_GUARD_BEGIN
    return lbad::topk_batch_impl(c, static_cast<const uint32_t*>(inPackedQueries), inRecordings, inSubfingerprints, inRange, inK,
                                 inIndexBase, static_cast<unsigned long long*>(outKeys), static_cast<int32_t*>(outLags),
                                 static_cast<hipStream_t>(inStream));
    LBAD_GUARD_END
}

OSStatus LBAudioDetectiveDebugRecordingBatchPlan(UInt32 inRecordings, UInt32 inSubfingerprints, UInt32 inShortestEntry, UInt32 inLongestEntry,
                                                 UInt64 inEntries, UInt64 inScratchLimit, UInt32 inKeyForm, UInt32* outForm,
                                                 UInt64* outTiles, UInt32* outRecordingsPerPass, UInt64* outEntriesPerChunk,
                                                 UInt64* outScratchBytes, UInt64* outLdsBytes) {
    if (!outForm || !outTiles || !outRecordingsPerPass || !outEntriesPerChunk || !outScratchBytes || !outLdsBytes || inRecordings == 0 ||
        inSubfingerprints == 0 || (uint64_t)inRecordings * inSubfingerprints > 0x7FFFFFFFull || inShortestEntry > inLongestEntry ||
        inLongestEntry > LBAD_OCCURRENCES_MAX_ENTRY_SUBFINGERPRINTS || (inEntries != 0 && inShortestEntry == 0) ||
        inEntries > 0x100000000ull || (!inKeyForm && (uint64_t)inRecordings * inEntries > 0x7FFFFFFFull))
        return kLBAudioDetectiveArgumentInvalid;
    lbad::RecordingBatchPlan plan;
    if (!lbad::recording_batch_plan(inRecordings, inSubfingerprints, inShortestEntry, inLongestEntry, inEntries, inScratchLimit,
                                    inKeyForm != 0, lbad::g_force_shared.load() != 0, &plan))
        return kLBAudioDetectiveArgumentInvalid;
    *outForm = plan.form;
    *outTiles = plan.tiles;
    *outRecordingsPerPass = plan.recordings_per_pass;
    *outEntriesPerChunk = plan.entries_per_chunk;
    *outScratchBytes = plan.scratch_bytes;
    *outLdsBytes = plan.lds_bytes;
    return noErr;
}

OSStatus LBAudioDetectiveDebugSetRecordingBatchForm(UInt32 inForceShared) {
    lbad::g_force_shared.store(inForceShared ? 1u : 0u);
    return noErr;
}

}  // extern "C"
