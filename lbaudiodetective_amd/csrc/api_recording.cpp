// api_recording.cpp -- scores and lags of a ragged corpus for ONE query of any length, a long recording above all
// (k_recording.hip): the per-entry forms from a handle or from packed sub-fingerprints on the device, and the top-K and threshold
// forms, which run that pass into the corpus' scores scratch, then the EXISTING selections of k_topk.hip / k_threshold.hip, then
// the gather of the selected entries' lags.
#include "internal.hpp"

#include <cmath>
#include <cstring>

namespace lbad {
namespace {

// the query of a call: a handle (staged through the alignment's pair, under its event) or packed sub-fingerprints on the device
// (through the builder of k_query.hip, under the packed calls' event)
struct RecQuery {
    const LBAudioDetectiveFingerprint* fp = nullptr;
    const uint32_t* d_rows = nullptr;
    uint32_t per = 0;
};

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

// what the corpus decides, before anything is reserved or launched (the occurrences calls' own restrictions): a ragged corpus
// of the query's sub-fingerprint length with no entry above the cap, the indices in range, the entries per chunk under the limit
OSStatus recording_plan(const LBAudioDetectiveCorpus* c, uint32_t q_length, uint32_t n_query, uint64_t index_base, uint64_t* out_tiles,
                        uint64_t* out_chunk) {
    if (!c->ragged || q_length != c->subfp_len || n_query == 0 || n_query > 0x7FFFFFFFu ||
        c->ne_max > LBAD_OCCURRENCES_MAX_ENTRY_SUBFINGERPRINTS || index_base + c->count > 0x100000000ull)
        return kLBAudioDetectiveArgumentInvalid;
    *out_tiles = 1;
    *out_chunk = 0;
    if (c->count == 0) return noErr;
    const uint64_t tiles = occurrences_tiles(n_query, c->len_hist.begin()->first, c->ne_max);
    const uint64_t limit = c->join_scratch_limit ? c->join_scratch_limit : kJoinScratchDefault;
    const uint64_t chunk = recording_chunk_entries(tiles, limit);
    if (chunk == 0) return kLBAudioDetectiveArgumentInvalid;          // the limit holds no block of entries at this query length
    const uint64_t block = occurrences_block_entries();
    *out_tiles = tiles;
    *out_chunk = chunk < c->count ? chunk : (c->count + block - 1) / block * block;
    return noErr;
}

// everything behind the staging of the query, on `stream`: the pass chunk by chunk, then the selection and its lags
OSStatus recording_launch(LBAudioDetectiveCorpus* c, const uint32_t* d_qwords, uint32_t n_query, uint32_t range, uint64_t tiles,
                          uint64_t chunk, float* scores, int32_t* lags, const RecSelect* sel, hipStream_t stream) {
    // the corpus' latest append, awaited on the device
    if (c->append_event.ev) LBAD_HIP(hipStreamWaitEvent(stream, c->append_event, 0));
    RecordingCall call;
    call.d_recs = c->d_recs; call.d_off = c->d_off; call.ne_min = c->len_hist.begin()->first; call.ne_max = c->ne_max;
    call.subfp_len = c->subfp_len; call.range = range ? range : c->subfp_len; call.d_qwords = d_qwords; call.n_query = n_query;
    call.tiles = tiles; call.d_scores = scores; call.d_lags = lags; call.stream = stream;
    hipError_t e = hipSuccess;
    for (uint64_t e0 = 0; e0 < c->count && e == hipSuccess; e0 += chunk)
        e = launch_recording_chunk(call, c->d_join_scratch, e0, c->count - e0 < chunk ? c->count - e0 : chunk);
    LBAD_HIP(e);
    if (!sel) return noErr;
    if (sel->threshold)
        LBAD_HIP(launch_threshold_keys(scores, c->count, 1, sel->t, sel->capacity, sel->index_base, c->d_threshold_scratch, sel->keys,
                                       sel->count, stream));
    else
        LBAD_HIP(launch_topk_keys(scores, c->count, 1, sel->k, sel->index_base, c->d_topk_scratch, sel->keys, stream));
    if (sel->lags) LBAD_HIP(launch_recording_lag_gather(sel->keys, sel->capacity, sel->index_base, c->count, lags, sel->lags, stream));
    return noErr;
}

// One call.  The caller has checked what needs no handle, and the device.  sel == nullptr: the per-entry form, out_scores (and
// out_lags, optional) the caller's.  Otherwise scores and entry lags lie in the corpus' scores scratch, under topk_ev.
OSStatus recording_impl(LBAudioDetectiveCorpus* c, const RecQuery& q, uint32_t range, float* out_scores, int32_t* out_lags,
                        const RecSelect* sel, hipStream_t stream) {
    const uint32_t n_query = q.fp ? q.fp->count : q.per;
    uint64_t tiles = 0, chunk = 0;
    OSStatus st = recording_plan(c, q.fp ? q.fp->length : c->subfp_len, n_query, sel ? sel->index_base : 0, &tiles, &chunk);
    if (st != noErr) return st;
    if (c->count == 0) {                                   // nothing to score: the scores forms write nothing, the key forms zeros
        if (!sel) return noErr;
        LBAD_HIP(hipMemsetAsync(sel->keys, 0, (size_t)sel->capacity * sizeof(unsigned long long), stream));
        if (sel->lags) LBAD_HIP(hipMemsetAsync(sel->lags, 0, (size_t)sel->capacity * sizeof(int32_t), stream));
        if (sel->count) LBAD_HIP(hipMemsetAsync(sel->count, 0, sizeof(unsigned long long), stream));
        return noErr;
    }
    // the scratch is the previous call's until its event: the partials (join_ev), the query's words (align_ev / pq_ev), the score
    // row and the selection's words (topk_ev)
    Event& q_ev = q.fp ? c->align_ev : c->pq_ev;
    st = c->join_ev.wait_or_create();
    if (st == noErr) st = q_ev.wait_or_create();
    if (st == noErr && sel) st = c->topk_ev.wait_or_create();
    if (st == noErr) st = c->d_join_scratch.reserve(recording_scratch_bytes(chunk, tiles));
    int32_t* lags = out_lags;
    if (st == noErr && sel) {
        // one row of scores and, behind it, the entries' lags
        st = c->d_topk_scores.reserve((size_t)c->count * (sel->lags ? 2 : 1));
        if (st == noErr)
            st = sel->threshold ? c->d_threshold_scratch.reserve(threshold_scratch_bytes(c->count, 1)) : c->d_topk_scratch.reserve(topk_scratch_bytes(1));
        out_scores = c->d_topk_scores;
        lags = sel->lags ? reinterpret_cast<int32_t*>(c->d_topk_scores + c->count) : nullptr;
    }
    if (st != noErr) return st;
    const uint32_t* d_qwords = nullptr;
    if (q.fp) {
        std::vector<uint32_t> words;
        build_align_query(q.fp, true, words);
        st = c->align_q.reserve(words.size());
        if (st != noErr) return st;
        std::memcpy(c->align_q.host, words.data(), words.size() * sizeof(uint32_t));
        d_qwords = c->align_q.dev;
        st = hip_status(hipMemcpyAsync(c->align_q.dev, c->align_q.host, words.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream),
                        "query words", __LINE__);
    } else {
        st = c->d_pq.reserve((size_t)q.per * kPackedWords);
        if (st != noErr) return st;
        d_qwords = c->d_pq;
        st = hip_status(launch_build_query_rows(q.d_rows, 1, q.per, c->subfp_len, true, c->d_pq, nullptr, stream), "query words", __LINE__);
    }
    if (st == noErr) st = recording_launch(c, d_qwords, n_query, range, tiles, chunk, out_scores, lags, sel, stream);
    // behind whatever was launched, also after a failure: the scratch and the staged words are in use until then
    const OSStatus rec = q_ev.record(stream);
    const OSStatus rec2 = c->join_ev.record(stream);
    const OSStatus rec3 = sel ? c->topk_ev.record(stream) : noErr;
    return st != noErr ? st : (rec != noErr ? rec : (rec2 != noErr ? rec2 : rec3));
}

OSStatus scores_handle_impl(LBAudioDetectiveCorpus* c, const LBAudioDetectiveFingerprint* q, uint32_t range, float* scores, int32_t* lags,
                            hipStream_t stream) {
    if (!c || !q || !scores) return kLBAudioDetectiveArgumentInvalid;
    if (!device_ready()) return kLBAudioDetectiveDeviceUnavailable;
    RecQuery rq;
    rq.fp = q;
    return recording_impl(c, rq, range, scores, lags, nullptr, stream);
}

bool packed_ok(const void* c, const void* d_rows, uint32_t per) { return c && d_rows && per != 0 && per <= 0x7FFFFFFFu; }

OSStatus scores_packed_impl(LBAudioDetectiveCorpus* c, const uint32_t* d_rows, uint32_t per, uint32_t range, float* scores, int32_t* lags,
                            hipStream_t stream) {
    if (!packed_ok(c, d_rows, per) || !scores) return kLBAudioDetectiveArgumentInvalid;
    if (!device_ready()) return kLBAudioDetectiveDeviceUnavailable;
    RecQuery rq;
    rq.d_rows = d_rows; rq.per = per;
    return recording_impl(c, rq, range, scores, lags, nullptr, stream);
}

OSStatus topk_packed_impl(LBAudioDetectiveCorpus* c, const uint32_t* d_rows, uint32_t per, uint32_t range, uint32_t k, uint64_t index_base,
                          unsigned long long* keys, int32_t* lags, hipStream_t stream) {
    if (!packed_ok(c, d_rows, per) || !keys || k == 0 || k > kTopKMax || index_base > 0x100000000ull) return kLBAudioDetectiveArgumentInvalid;
    if (!device_ready()) return kLBAudioDetectiveDeviceUnavailable;
    RecQuery rq;
    rq.d_rows = d_rows; rq.per = per;
    RecSelect sel;
    sel.k = k; sel.capacity = k; sel.index_base = index_base; sel.keys = keys; sel.lags = lags;
    return recording_impl(c, rq, range, nullptr, nullptr, &sel, stream);
}

OSStatus threshold_packed_impl(LBAudioDetectiveCorpus* c, const uint32_t* d_rows, uint32_t per, uint32_t range, float t, uint64_t capacity,
                               uint64_t index_base, unsigned long long* keys, unsigned long long* count, int32_t* lags,
                               hipStream_t stream) {
    if (!packed_ok(c, d_rows, per) || !keys || !count || !threshold_ok(t, capacity) || index_base > 0x100000000ull)
        return kLBAudioDetectiveArgumentInvalid;
    if (!device_ready()) return kLBAudioDetectiveDeviceUnavailable;
    RecQuery rq;
    rq.d_rows = d_rows; rq.per = per;
    RecSelect sel;
    sel.threshold = true; sel.t = t; sel.capacity = capacity; sel.index_base = index_base; sel.keys = keys; sel.count = count;
    sel.lags = lags;
    return recording_impl(c, rq, range, nullptr, nullptr, &sel, stream);
}

// host-returning form: keys and (out_lags given) lags in ONE block of the corpus' key buffer on the null stream, then decoded
OSStatus topk_host_impl(LBAudioDetectiveCorpus* c, const LBAudioDetectiveFingerprint* q, uint32_t range, uint32_t k, SInt64* out_idx,
                        Float32* out_scores, SInt32* out_lags, UInt32* out_count) {
    if (!c || !q || !out_idx || !out_scores || !out_count || k == 0 || k > kTopKMax) return kLBAudioDetectiveArgumentInvalid;
    if (!device_ready()) return kLBAudioDetectiveDeviceUnavailable;
    uint64_t tiles = 0, chunk = 0;
    OSStatus st = recording_plan(c, q->length, q->count, 0, &tiles, &chunk);       // (a refused call reserves nothing)
    if (st != noErr) return st;
    st = c->topk_ev.wait();             // (the key buffer is the previous top-K, threshold or join call's until then)
    const size_t words = (size_t)k + (out_lags ? (k + 1) / 2 : 0);
    if (st == noErr) st = c->d_topk_keys.reserve(words);
    if (st != noErr) return st;
    RecQuery rq;
    rq.fp = q;
    RecSelect sel;
    sel.k = k; sel.capacity = k; sel.keys = c->d_topk_keys;
    sel.lags = out_lags ? reinterpret_cast<int32_t*>(c->d_topk_keys + k) : nullptr;
    st = recording_impl(c, rq, range, nullptr, nullptr, &sel, nullptr);
    if (st != noErr) {
        (void)hipStreamSynchronize(nullptr);       // whatever was launched has left the key buffer before its next user
        return st;
    }
    std::vector<unsigned long long> host(words);
    LBAD_HIP(hipMemcpy(host.data(), c->d_topk_keys, words * sizeof(unsigned long long), hipMemcpyDeviceToHost));
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
