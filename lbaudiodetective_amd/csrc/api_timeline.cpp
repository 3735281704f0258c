// api_timeline.cpp -- the recording timeline (k_timeline.hip): the best entry of a ragged corpus at every offset of ONE query, a
// long recording above all, as keys and lengths on the device, from a handle or from packed sub-fingerprints on the device, and
// the host-returning form.
#include "internal.hpp"

#include <cmath>
#include <cstring>

namespace lbad {
namespace {

// the query of a call: a handle (staged through the alignment's pair, under its event) or packed sub-fingerprints on the device
// (through the builder of k_query.hip, under the packed calls' event)
struct TlQuery {
    const LBAudioDetectiveFingerprint* fp = nullptr;
    const uint32_t* d_rows = nullptr;
    uint32_t per = 0;
};

// what needs neither handle nor device: a finite threshold above 0, an index base a corpus can lie behind
bool timeline_args_ok(float threshold, uint64_t index_base) {
    return std::isfinite(threshold) && threshold > 0.0f && index_base <= 0x100000000ull;
}

// what the corpus decides, before anything is reserved or launched (the occurrences calls' own restrictions): a ragged corpus
// of the query's sub-fingerprint length with no entry above the cap, the indices in range, the entries per chunk under the
// limit.  *out_any: an entry takes part (the shortest is not longer than the query).
OSStatus timeline_plan(const LBAudioDetectiveCorpus* c, uint32_t q_length, uint32_t n_query, uint64_t index_base, uint64_t* out_tiles,
                       uint64_t* out_chunk, bool* out_any) {
    if (!c->ragged || q_length != c->subfp_len || n_query == 0 || n_query > 0x7FFFFFFFu ||
        c->ne_max > LBAD_OCCURRENCES_MAX_ENTRY_SUBFINGERPRINTS || index_base + c->count > 0x100000000ull)
        return kLBAudioDetectiveArgumentInvalid;
    *out_tiles = 1;
    *out_chunk = 0;
    *out_any = false;
    if (c->count == 0) return noErr;
    const uint32_t ne_min = c->len_hist.begin()->first;
    const uint64_t tiles = timeline_tiles(n_query, ne_min);
    const uint64_t limit = c->join_scratch_limit ? c->join_scratch_limit : kJoinScratchDefault;
    const uint64_t chunk = timeline_chunk_entries(tiles, limit);
    if (chunk == 0) return kLBAudioDetectiveArgumentInvalid;          // the limit holds no block of entries at this query length
    const uint64_t block = timeline_block_entries();
    *out_tiles = tiles;
    *out_chunk = chunk < c->count ? chunk : (c->count + block - 1) / block * block;
    *out_any = ne_min <= n_query;
    return noErr;
}

// everything behind the staging of the query, on `stream`: the pass chunk by chunk into the keys, then the lengths
OSStatus timeline_launch(LBAudioDetectiveCorpus* c, const uint32_t* d_qwords, uint32_t n_query, uint32_t range, float threshold,
                         uint64_t index_base, uint64_t tiles, uint64_t chunk, unsigned long long* keys, uint32_t* lengths,
                         hipStream_t stream) {
    // the corpus' latest append, awaited on the device
    if (c->append_event.ev) LBAD_HIP(hipStreamWaitEvent(stream, c->append_event, 0));
    TimelineCall call;
    call.d_recs = c->d_recs; call.d_off = c->d_off; call.ne_min = c->len_hist.begin()->first; call.ne_max = c->ne_max;
    call.subfp_len = c->subfp_len; call.range = range ? range : c->subfp_len; call.d_qwords = d_qwords; call.n_query = n_query;
    call.tiles = tiles; call.threshold = threshold; call.index_base = index_base; call.d_keys = keys; call.stream = stream;
    hipError_t e = hipSuccess;
    for (uint64_t e0 = 0; e0 < c->count && e == hipSuccess; e0 += chunk)
        e = launch_timeline_chunk(call, c->d_join_scratch, e0, c->count - e0 < chunk ? c->count - e0 : chunk);
    LBAD_HIP(e);
    if (lengths) LBAD_HIP(launch_timeline_lengths(keys, n_query, index_base, c->count, c->d_off, lengths, stream));
    return noErr;
}

// One call.  The caller has checked what needs no handle, and the device.
OSStatus timeline_impl(LBAudioDetectiveCorpus* c, const TlQuery& q, uint32_t range, float threshold, uint64_t index_base,
                       unsigned long long* keys, uint32_t* lengths, hipStream_t stream) {
    const uint32_t n_query = q.fp ? q.fp->count : q.per;
    uint64_t tiles = 0, chunk = 0;
    bool any = false;
    OSStatus st = timeline_plan(c, q.fp ? q.fp->length : c->subfp_len, n_query, index_base, &tiles, &chunk, &any);
    if (st != noErr) return st;
    // the keys carry the running maximum from chunk to chunk: zeros in front of the first.  Where no entry takes part these
    // zeros (and the lengths') are the answer.
    LBAD_HIP(hipMemsetAsync(keys, 0, (size_t)n_query * sizeof(unsigned long long), stream));
    if (!any) {
        if (lengths) LBAD_HIP(hipMemsetAsync(lengths, 0, (size_t)n_query * sizeof(uint32_t), stream));
        return noErr;
    }
    // the scratch is the previous call's until its event: the partials (join_ev), the query's words (align_ev / pq_ev)
    Event& q_ev = q.fp ? c->align_ev : c->pq_ev;
    st = c->join_ev.wait_or_create();
    if (st == noErr) st = q_ev.wait_or_create();
    if (st == noErr) st = c->d_join_scratch.reserve(timeline_scratch_bytes(chunk, tiles));
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
    if (st == noErr) st = timeline_launch(c, d_qwords, n_query, range, threshold, index_base, tiles, chunk, keys, lengths, stream);
    // behind whatever was launched, also after a failure: the scratch and the staged words are in use until then
    const OSStatus rec = q_ev.record(stream);
    const OSStatus rec2 = c->join_ev.record(stream);
    return st != noErr ? st : (rec != noErr ? rec : rec2);
}

OSStatus timeline_handle_impl(LBAudioDetectiveCorpus* c, const LBAudioDetectiveFingerprint* q, uint32_t range, float threshold,
                              uint64_t index_base, unsigned long long* keys, uint32_t* lengths, hipStream_t stream) {
    if (!c || !q || !keys || !timeline_args_ok(threshold, index_base)) return kLBAudioDetectiveArgumentInvalid;
    if (!device_ready()) return kLBAudioDetectiveDeviceUnavailable;
    TlQuery tq;
    tq.fp = q;
    return timeline_impl(c, tq, range, threshold, index_base, keys, lengths, stream);
}

OSStatus timeline_packed_impl(LBAudioDetectiveCorpus* c, const uint32_t* d_rows, uint32_t per, uint32_t range, float threshold,
                              uint64_t index_base, unsigned long long* keys, uint32_t* lengths, hipStream_t stream) {
    if (!c || !d_rows || !keys || per == 0 || per > 0x7FFFFFFFu || !timeline_args_ok(threshold, index_base))
        return kLBAudioDetectiveArgumentInvalid;
    if (!device_ready()) return kLBAudioDetectiveDeviceUnavailable;
    TlQuery tq;
    tq.d_rows = d_rows; tq.per = per;
    return timeline_impl(c, tq, range, threshold, index_base, keys, lengths, stream);
}

// host-returning form: keys and (out_lengths given) lengths in ONE block of the corpus' key buffer on the null stream, then
// decoded
OSStatus timeline_host_impl(LBAudioDetectiveCorpus* c, const LBAudioDetectiveFingerprint* q, uint32_t range, float threshold,
                            SInt64* out_idx, Float32* out_scores, UInt32* out_lengths, UInt64* out_count) {
    if (!c || !q || !out_idx || !out_scores || !out_count || !timeline_args_ok(threshold, 0)) return kLBAudioDetectiveArgumentInvalid;
    if (!device_ready()) return kLBAudioDetectiveDeviceUnavailable;
    uint64_t tiles = 0, chunk = 0;
    bool any = false;
    OSStatus st = timeline_plan(c, q->length, q->count, 0, &tiles, &chunk, &any);      // (a refused call reserves nothing)
    if (st != noErr) return st;
    const size_t n = q->count;
    st = c->topk_ev.wait();             // (the key buffer is the previous top-K, threshold or join call's until then)
    const size_t words = n + (out_lengths ? (n + 1) / 2 : 0);
    if (st == noErr) st = c->d_topk_keys.reserve(words);
    if (st != noErr) return st;
    unsigned long long* d_keys = c->d_topk_keys;
    uint32_t* d_lengths = out_lengths ? reinterpret_cast<uint32_t*>(d_keys + n) : nullptr;
    st = timeline_handle_impl(c, q, range, threshold, 0, d_keys, d_lengths, nullptr);
    if (st != noErr) {
        (void)hipStreamSynchronize(nullptr);       // whatever was launched has left the key buffer before its next user
        return st;
    }
    std::vector<unsigned long long> host(words);
    LBAD_HIP(hipMemcpy(host.data(), d_keys, words * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    const uint32_t* lengths = reinterpret_cast<const uint32_t*>(host.data() + n);
    UInt64 got = 0;
    for (size_t o = 0; o < n; ++o) {
        LBAudioDetectiveCorpusDecodeKey(host[o], out_idx + o, out_scores + o);
        if (out_idx[o] >= 0) ++got;
        if (out_lengths) out_lengths[o] = out_idx[o] >= 0 ? lengths[o] : 0;
    }
    *out_count = got;
    return noErr;
}

}  // namespace
}  // namespace lbad

extern "C" {

OSStatus LBAudioDetectiveCorpusRecordingTimelineKeysDevice(LBAudioDetectiveCorpusRef c, LBAudioDetectiveFingerprintRef inQuery,
                                                           UInt32 inRange, Float32 inThreshold, UInt64 inIndexBase, void* outKeys,
                                                           void* outLengths, void* inStream) {
    LBAD_GUARD_BEGIN
    return lbad::timeline_handle_impl(c, inQuery, inRange, inThreshold, inIndexBase, static_cast<unsigned long long*>(outKeys),
                                      static_cast<uint32_t*>(outLengths), static_cast<hipStream_t>(inStream));
    LBAD_GUARD_END
}

OSStatus LBAudioDetectiveCorpusRecordingPackedTimelineKeysDevice(LBAudioDetectiveCorpusRef c, const void* inPackedQuery,
                                                                 UInt32 inSubfingerprints, UInt32 inRange, Float32 inThreshold,
                                                                 UInt64 inIndexBase, void* outKeys, void* outLengths, void* inStream) {
    LBAD_GUARD_BEGIN
    return lbad::timeline_packed_impl(c, static_cast<const uint32_t*>(inPackedQuery), inSubfingerprints, inRange, inThreshold,
                                      inIndexBase, static_cast<unsigned long long*>(outKeys), static_cast<uint32_t*>(outLengths),
                                      static_cast<hipStream_t>(inStream));
    LBAD_GUARD_END
}

OSStatus LBAudioDetectiveCorpusQueryRecordingTimeline(LBAudioDetectiveCorpusRef c, LBAudioDetectiveFingerprintRef inQuery, UInt32 inRange,
                                                      Float32 inThreshold, SInt64* outIndices, Float32* outScores, UInt32* outLengths,
                                                      UInt64* outCount) {
    LBAD_GUARD_BEGIN
    return lbad::timeline_host_impl(c, inQuery, inRange, inThreshold, outIndices, outScores, outLengths, outCount);
    LBAD_GUARD_END
}

}  // extern "C"
