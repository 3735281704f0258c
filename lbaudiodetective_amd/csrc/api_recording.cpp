// api_recording.cpp -- scores and lags of a ragged corpus for ONE query of any length, a long recording above all
// (k_recording.hip): the per-entry forms from a handle or from packed sub-fingerprints on the device, and the top-K and threshold
// forms, which run that pass into the corpus' scores scratch, then the EXISTING selections of k_topk.hip / k_threshold.hip, then
// the gather of the selected entries' lags.  The plan, the query's staging, the events and the key block are recording_pass.cpp's.
#include "internal.hpp"

#include <cmath>

namespace lbad {
namespace {

const PassFamily kFamily = {occurrences_tiles, recording_chunk_entries, occurrences_block_entries};

// what follows the pass in the key forms
struct RecSelect {
    bool threshold = false;              // false: top-K
    uint32_t k = 0;
    float t = 0.0f;
    uint64_t capacity = 0;               // threshold: slots; top-K: k
    uint64_t index_base = 0;
    unsigned long long* keys = nullptr;
    unsigned long long* count = nullptr; // threshold only
    int32_t* lags = nullptr;             // optional
};

bool threshold_ok(float t, uint64_t capacity) {
    return std::isfinite(t) && t > 0.0f && capacity != 0 && capacity <= 0x80000000ull;
}

// everything behind the staging of the query, on the call's stream: the pass chunk by chunk, then the selection and its lags
OSStatus recording_launch(LBAudioDetectiveCorpus* c, const RecordingCall& call, uint64_t chunk, const RecSelect* sel) {
    LBAD_HIP(pass_chunks(c->count, chunk, [&](uint64_t e0, uint64_t n) { return launch_recording_chunk(call, c->d_join_scratch, e0, n); }));
    if (!sel) return noErr;
    if (sel->threshold)
        LBAD_HIP(launch_threshold_keys(call.d_scores, c->count, 1, sel->t, sel->capacity, sel->index_base, c->d_threshold_scratch, sel->keys,
                                       sel->count, call.stream));
    else
        LBAD_HIP(launch_topk_keys(call.d_scores, c->count, 1, sel->k, sel->index_base, c->d_topk_scratch, sel->keys, call.stream));
    if (sel->lags)
        LBAD_HIP(launch_recording_lag_gather(sel->keys, sel->capacity, sel->index_base, c->count, call.d_lags, sel->lags, call.stream));
    return noErr;
}

// One call.  The caller has checked what needs no handle, and the device.  sel == nullptr: the per-entry form, out_scores (and
// out_lags, optional) the caller's.  Otherwise scores and entry lags lie in the corpus' scores scratch, under topk_ev.
OSStatus recording_impl(LBAudioDetectiveCorpus* c, const PassQuery& q, float* out_scores, int32_t* out_lags, const RecSelect* sel,
                        hipStream_t stream) {
    PassPlan plan;
    OSStatus st = pass_plan(c, q, sel ? sel->index_base : 0, kFamily, &plan);
    if (st != noErr) return st;
    if (c->count == 0) {                                   // nothing to score: the scores forms write nothing, the key forms zeros
        if (!sel) return noErr;
        LBAD_HIP(hipMemsetAsync(sel->keys, 0, (size_t)sel->capacity * sizeof(unsigned long long), stream));
        if (sel->lags) LBAD_HIP(hipMemsetAsync(sel->lags, 0, (size_t)sel->capacity * sizeof(int32_t), stream));
        if (sel->count) LBAD_HIP(hipMemsetAsync(sel->count, 0, sizeof(unsigned long long), stream));
        return noErr;
    }
    PassGuard guard(c, q, sel != nullptr);
    st = guard.wait();                                     // (the scratch is the previous call's until then)
    if (st == noErr) st = c->d_join_scratch.reserve(recording_scratch_bytes(plan.chunk, plan.call.tiles));
    RecordingCall call;
    static_cast<OcPassCall&>(call) = plan.call;
    call.d_scores = out_scores; call.d_lags = out_lags;
    if (st == noErr && sel) {
        // one row of scores and, behind it, the entries' lags
        st = c->d_topk_scores.reserve((size_t)c->count * (sel->lags ? 2 : 1));
        if (st == noErr)
            st = sel->threshold ? c->d_threshold_scratch.reserve(threshold_scratch_bytes(c->count, 1)) : c->d_topk_scratch.reserve(topk_scratch_bytes(1));
        call.d_scores = c->d_topk_scores;
        call.d_lags = sel->lags ? reinterpret_cast<int32_t*>(c->d_topk_scores + c->count) : nullptr;
    }
    if (st != noErr) return st;
    st = pass_stage_query(c, q, stream, &call);
    if (st == noErr) st = recording_launch(c, call, plan.chunk, sel);
    return guard.finish(stream, st);
}

OSStatus scores_handle_impl(LBAudioDetectiveCorpus* c, const LBAudioDetectiveFingerprint* q, uint32_t range, float* scores, int32_t* lags,
                            hipStream_t stream) {
    if (!c || !q || !scores) return kLBAudioDetectiveArgumentInvalid;
    if (!device_ready()) return kLBAudioDetectiveDeviceUnavailable;
    PassQuery pq;
    pq.fp = q; pq.range = range;
    return recording_impl(c, pq, scores, lags, nullptr, stream);
}

bool packed_ok(const void* c, const void* d_rows, uint32_t per) { return c && d_rows && per != 0 && per <= 0x7FFFFFFFu; }

OSStatus scores_packed_impl(LBAudioDetectiveCorpus* c, const uint32_t* d_rows, uint32_t per, uint32_t range, float* scores, int32_t* lags,
                            hipStream_t stream) {
    if (!packed_ok(c, d_rows, per) || !scores) return kLBAudioDetectiveArgumentInvalid;
    if (!device_ready()) return kLBAudioDetectiveDeviceUnavailable;
    PassQuery pq;
    pq.d_rows = d_rows; pq.per = per; pq.range = range;
    return recording_impl(c, pq, scores, lags, nullptr, stream);
}

OSStatus topk_packed_impl(LBAudioDetectiveCorpus* c, const uint32_t* d_rows, uint32_t per, uint32_t range, uint32_t k, uint64_t index_base,
                          unsigned long long* keys, int32_t* lags, hipStream_t stream) {
    if (!packed_ok(c, d_rows, per) || !keys || k == 0 || k > kTopKMax || index_base > 0x100000000ull) return kLBAudioDetectiveArgumentInvalid;
    if (!device_ready()) return kLBAudioDetectiveDeviceUnavailable;
    PassQuery pq;
    pq.d_rows = d_rows; pq.per = per; pq.range = range;
    RecSelect sel;
    sel.k = k; sel.capacity = k; sel.index_base = index_base; sel.keys = keys; sel.lags = lags;
    return recording_impl(c, pq, nullptr, nullptr, &sel, stream);
}

OSStatus threshold_packed_impl(LBAudioDetectiveCorpus* c, const uint32_t* d_rows, uint32_t per, uint32_t range, float t, uint64_t capacity,
                               uint64_t index_base, unsigned long long* keys, unsigned long long* count, int32_t* lags,
                               hipStream_t stream) {
    if (!packed_ok(c, d_rows, per) || !keys || !count || !threshold_ok(t, capacity) || index_base > 0x100000000ull)
        return kLBAudioDetectiveArgumentInvalid;
    if (!device_ready()) return kLBAudioDetectiveDeviceUnavailable;
    PassQuery pq;
    pq.d_rows = d_rows; pq.per = per; pq.range = range;
    RecSelect sel;
    sel.threshold = true; sel.t = t; sel.capacity = capacity; sel.index_base = index_base; sel.keys = keys; sel.count = count;
    sel.lags = lags;
    return recording_impl(c, pq, nullptr, nullptr, &sel, stream);
}

// host-returning form: keys and (out_lags given) lags in ONE block of the corpus' key buffer on the null stream, then decoded
OSStatus topk_host_impl(LBAudioDetectiveCorpus* c, const LBAudioDetectiveFingerprint* q, uint32_t range, uint32_t k, SInt64* out_idx,
                        Float32* out_scores, SInt32* out_lags, UInt32* out_count) {
    if (!c || !q || !out_idx || !out_scores || !out_count || k == 0 || k > kTopKMax) return kLBAudioDetectiveArgumentInvalid;
    if (!device_ready()) return kLBAudioDetectiveDeviceUnavailable;
    PassQuery pq;
    pq.fp = q; pq.range = range;
    PassPlan plan;
    OSStatus st = pass_plan(c, pq, 0, kFamily, &plan);     // (a refused call reserves nothing)
    if (st != noErr) return st;
    KeyBlock b;
    st = key_block_reserve(c, k, out_lags ? k : 0, &b);
    if (st != noErr) return st;
    RecSelect sel;
    sel.k = k; sel.capacity = k; sel.keys = b.d_keys; sel.lags = reinterpret_cast<int32_t*>(b.d_words);
    st = recording_impl(c, pq, nullptr, nullptr, &sel, nullptr);
    if (st != noErr) return key_block_failed(st);
    std::vector<unsigned long long> host;
    st = key_block_read(b, k, &host);
    if (st != noErr) return st;
    const int32_t* lags = reinterpret_cast<const int32_t*>(host.data() + k);
    UInt32 got = 0;
    for (uint32_t i = 0; i < k; ++i) {
        LBAudioDetectiveCorpusDecodeKey(host[i], out_idx + i, out_scores + i);
        if (out_idx[i] >= 0) ++got;
        if (out_lags) out_lags[i] = out_idx[i] >= 0 ? lags[i] : 0;
    }
    *out_count = got;
    return noErr;
}

}  // namespace
}  // namespace lbad

extern "C" {

OSStatus LBAudioDetectiveCorpusRecordingScoresDevice(LBAudioDetectiveCorpusRef c, LBAudioDetectiveFingerprintRef inQuery, UInt32 inRange,
                                                     Float32* outScores, SInt32* outLags, void* inStream) {
    LBAD_GUARD_BEGIN
    return lbad::scores_handle_impl(c, inQuery, inRange, outScores, outLags, static_cast<hipStream_t>(inStream));
    LBAD_GUARD_END
}

OSStatus LBAudioDetectiveCorpusRecordingPackedScoresDevice(LBAudioDetectiveCorpusRef c, const void* inPackedQuery, UInt32 inSubfingerprints,
                                                           UInt32 inRange, Float32* outScores, SInt32* outLags, void* inStream) {
    LBAD_GUARD_BEGIN
    return lbad::scores_packed_impl(c, static_cast<const uint32_t*>(inPackedQuery), inSubfingerprints, inRange, outScores, outLags,
                                    static_cast<hipStream_t>(inStream));
    LBAD_GUARD_END
}

OSStatus LBAudioDetectiveCorpusQueryRecordingTopK(LBAudioDetectiveCorpusRef c, LBAudioDetectiveFingerprintRef inQuery, UInt32 inRange,
                                                  UInt32 inK, SInt64* outIndices, Float32* outScores, SInt32* outLags, UInt32* outCount) {
    LBAD_GUARD_BEGIN
    return lbad::topk_host_impl(c, inQuery, inRange, inK, outIndices, outScores, outLags, outCount);
    LBAD_GUARD_END
}

OSStatus LBAudioDetectiveCorpusQueryPackedRecordingTopKKeysDevice(LBAudioDetectiveCorpusRef c, const void* inPackedQuery,
                                                                  UInt32 inSubfingerprints, UInt32 inRange, UInt32 inK, UInt64 inIndexBase,
                                                                  void* outKeys, void* outLags, void* inStream) {
    LBAD_GUARD_BEGIN
    return lbad::topk_packed_impl(c, static_cast<const uint32_t*>(inPackedQuery), inSubfingerprints, inRange, inK, inIndexBase,
                                  static_cast<unsigned long long*>(outKeys), static_cast<int32_t*>(outLags),
                                  static_cast<hipStream_t>(inStream));
    LBAD_GUARD_END
}

OSStatus LBAudioDetectiveCorpusQueryPackedRecordingThresholdKeysDevice(LBAudioDetectiveCorpusRef c, const void* inPackedQuery,
                                                                       UInt32 inSubfingerprints, UInt32 inRange, Float32 inThreshold,
                                                                       UInt64 inCapacity, UInt64 inIndexBase, void* outKeys, void* outCount,
                                                                       void* outLags, void* inStream) {
    LBAD_GUARD_BEGIN
    return lbad::threshold_packed_impl(c, static_cast<const uint32_t*>(inPackedQuery), inSubfingerprints, inRange, inThreshold, inCapacity,
                                       inIndexBase, static_cast<unsigned long long*>(outKeys), static_cast<unsigned long long*>(outCount),
                                       static_cast<int32_t*>(outLags), static_cast<hipStream_t>(inStream));
    LBAD_GUARD_END
}

}  // extern "C"
