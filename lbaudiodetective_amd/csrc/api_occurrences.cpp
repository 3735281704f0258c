// api_occurrences.cpp -- every place a recording matches a ragged corpus (k_occurrences.hip): the cells of every entry's
// profile at or above a score, as keys and lags on the device, from a handle or from packed sub-fingerprints on the device,
// and the host-returning form.
#include "internal.hpp"

#include <cmath>
#include <cstring>

namespace lbad {
namespace {

// what needs neither handle nor device: a finite threshold above 0, 1 .. 2^31 slots, an index base a corpus can lie behind
bool occurrences_args_ok(float threshold, uint64_t capacity, uint64_t index_base) {
    return std::isfinite(threshold) && threshold > 0.0f && capacity != 0 && capacity <= 0x80000000ull && index_base <= 0x100000000ull;
}

// what the corpus decides, before anything is reserved or launched: a ragged corpus of the query's sub-fingerprint length with
// no entry above the cap (ne_max: the host knows it), the indices in range, and the entries per chunk under the scratch limit
OSStatus occurrences_plan(const LBAudioDetectiveCorpus* c, uint32_t q_length, uint32_t n_query, uint64_t index_base, uint64_t* out_tiles,
                          uint64_t* out_chunk) {
    if (!c->ragged || q_length != c->subfp_len || n_query == 0 || n_query > 0x7FFFFFFFu ||
        c->ne_max > LBAD_OCCURRENCES_MAX_ENTRY_SUBFINGERPRINTS || index_base + c->count > 0x100000000ull)
        return kLBAudioDetectiveArgumentInvalid;
    *out_tiles = 1;
    *out_chunk = 0;
    if (c->count == 0) return noErr;
    const uint64_t tiles = occurrences_tiles(n_query, c->len_hist.begin()->first, c->ne_max);
    const uint64_t limit = c->join_scratch_limit ? c->join_scratch_limit : kJoinScratchDefault;
    const uint64_t chunk = occurrences_chunk_entries(tiles, limit);
    if (chunk == 0) return kLBAudioDetectiveArgumentInvalid;          // the limit holds no block of entries at this query length
    *out_tiles = tiles;
    *out_chunk = chunk < c->count ? chunk : (c->count + occurrences_block_entries() - 1) / occurrences_block_entries() * occurrences_block_entries();
    return noErr;
}

// the call itself on `stream`: the query's words are on the device (or on their way there on `stream`).  The caller has
// waited for join_ev and records it behind this.
OSStatus occurrences_run(LBAudioDetectiveCorpus* c, const uint32_t* d_qwords, uint32_t n_query, uint32_t range, float threshold,
                         bool peaks, uint64_t capacity, uint64_t index_base, uint64_t tiles, uint64_t chunk, unsigned long long* keys,
                         int32_t* lags, unsigned long long* count, hipStream_t stream) {
    // the corpus' latest append, awaited on the device
    if (c->append_event.ev) LBAD_HIP(hipStreamWaitEvent(stream, c->append_event, 0));
    LBAD_HIP(hipMemsetAsync(keys, 0, (size_t)capacity * sizeof(unsigned long long), stream));
    if (lags) LBAD_HIP(hipMemsetAsync(lags, 0, (size_t)capacity * sizeof(int32_t), stream));
    if (c->count == 0) {
        LBAD_HIP(hipMemsetAsync(count, 0, sizeof(unsigned long long), stream));
        return noErr;
    }
    OSStatus st = c->d_join_scratch.reserve(occurrences_scratch_bytes(chunk, tiles));
    if (st != noErr) return st;
    OccurrencesCall call;
    call.d_recs = c->d_recs; call.d_off = c->d_off; call.ne_min = c->len_hist.begin()->first; call.ne_max = c->ne_max;
    call.subfp_len = c->subfp_len; call.range = range ? range : c->subfp_len; call.d_qwords = d_qwords; call.n_query = n_query;
    call.tiles = tiles; call.threshold = threshold; call.peaks = peaks; call.capacity = capacity; call.index_base = index_base;
    call.d_keys = keys; call.d_lags = lags; call.stream = stream;
    hipError_t e = hipSuccess;
    for (uint64_t e0 = 0; e0 < c->count && e == hipSuccess; e0 += chunk) {
        const uint64_t n = c->count - e0 < chunk ? c->count - e0 : chunk;
        e = launch_occurrences_chunk(call, c->d_join_scratch, chunk, e0, n, e0 == 0 ? 1u : 0u);
    }
    LBAD_HIP(e);
    // the running total behind the last chunk is the call's count
    LBAD_HIP(hipMemcpyAsync(count, c->d_join_scratch.get(), sizeof(unsigned long long), hipMemcpyDeviceToDevice, stream));
    return noErr;
}

// from a handle: the query's words through the alignment's staging pair, under its event
OSStatus occurrences_handle_impl(LBAudioDetectiveCorpus* c, const LBAudioDetectiveFingerprint* q, uint32_t range, float threshold,
                                 uint32_t peaks, uint64_t capacity, uint64_t index_base, unsigned long long* keys, int32_t* lags,
                                 unsigned long long* count, hipStream_t stream) {
    if (!c || !q || !keys || !count || !occurrences_args_ok(threshold, capacity, index_base)) return kLBAudioDetectiveArgumentInvalid;
    if (!device_ready()) return kLBAudioDetectiveDeviceUnavailable;
    uint64_t tiles = 0, chunk = 0;
    OSStatus st = occurrences_plan(c, q->length, q->count, index_base, &tiles, &chunk);
    if (st != noErr) return st;
    st = c->join_ev.wait_or_create();                 // (the scratch is the previous call's until then)
    if (st == noErr) st = c->align_ev.wait_or_create();
    if (st != noErr) return st;
    std::vector<uint32_t> words;
    build_align_query(q, true, words);
    st = c->align_q.reserve(words.size());
    if (st != noErr) return st;
    std::memcpy(c->align_q.host, words.data(), words.size() * sizeof(uint32_t));
    st = hip_status(hipMemcpyAsync(c->align_q.dev, c->align_q.host, words.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream),
                    "query words", __LINE__);
    if (st == noErr)
        st = occurrences_run(c, c->align_q.dev, q->count, range, threshold, peaks != 0, capacity, index_base, tiles, chunk, keys, lags,
                             count, stream);
    // behind whatever was launched, also after a failure: the scratch and the staged words are in use until then
    const OSStatus rec = c->align_ev.record(stream);
    const OSStatus rec2 = c->join_ev.record(stream);
    return st != noErr ? st : (rec != noErr ? rec : rec2);
}

// from packed sub-fingerprints on the device: the builder of k_query.hip writes the words, under the packed calls' event
OSStatus occurrences_packed_impl(LBAudioDetectiveCorpus* c, const uint32_t* d_rows, uint32_t per, uint32_t range, float threshold,
                                 uint32_t peaks, uint64_t capacity, uint64_t index_base, unsigned long long* keys, int32_t* lags,
                                 unsigned long long* count, hipStream_t stream) {
    if (!c || !d_rows || !keys || !count || per == 0 || per > 0x7FFFFFFFu || !occurrences_args_ok(threshold, capacity, index_base))
        return kLBAudioDetectiveArgumentInvalid;
    if (!device_ready()) return kLBAudioDetectiveDeviceUnavailable;
    uint64_t tiles = 0, chunk = 0;
    OSStatus st = occurrences_plan(c, c->subfp_len, per, index_base, &tiles, &chunk);
    if (st != noErr) return st;
    st = c->join_ev.wait_or_create();
    if (st == noErr) st = c->pq_ev.wait_or_create();
    if (st == noErr) st = c->d_pq.reserve((size_t)per * kPackedWords);
    if (st != noErr) return st;
    st = hip_status(launch_build_query_rows(d_rows, 1, per, c->subfp_len, true, c->d_pq, nullptr, stream), "query words", __LINE__);
    if (st == noErr)
        st = occurrences_run(c, c->d_pq, per, range, threshold, peaks != 0, capacity, index_base, tiles, chunk, keys, lags, count, stream);
    const OSStatus rec = c->pq_ev.record(stream);
    const OSStatus rec2 = c->join_ev.record(stream);
    return st != noErr ? st : (rec != noErr ? rec : rec2);
}

// host-returning form: keys, the count and the lags in ONE block of the corpus' key buffer on the null stream; the count is
// read back first, then min(count, capacity) keys and lags
OSStatus occurrences_host_impl(LBAudioDetectiveCorpus* c, const LBAudioDetectiveFingerprint* q, uint32_t range, float threshold,
                               uint32_t peaks, uint64_t capacity, SInt64* out_idx, Float32* out_scores, SInt32* out_lags,
                               UInt64* out_count) {
    if (!c || !q || !out_idx || !out_scores || !out_count || !occurrences_args_ok(threshold, capacity, 0))
        return kLBAudioDetectiveArgumentInvalid;
    if (!device_ready()) return kLBAudioDetectiveDeviceUnavailable;
    uint64_t tiles = 0, chunk = 0;
    OSStatus st = occurrences_plan(c, q->length, q->count, 0, &tiles, &chunk);     // (a refused call reserves nothing)
    if (st != noErr) return st;
    st = c->topk_ev.wait();             // (the key buffer is the previous top-K, threshold or join call's until then)
    const size_t words = (size_t)capacity + 1 + (out_lags ? (capacity + 1) / 2 : 0);
    if (st == noErr) st = c->d_topk_keys.reserve(words);
    if (st != noErr) return st;
    unsigned long long* d_keys = c->d_topk_keys;
    int32_t* d_lags = out_lags ? reinterpret_cast<int32_t*>(d_keys + capacity + 1) : nullptr;
    st = occurrences_handle_impl(c, q, range, threshold, peaks, capacity, 0, d_keys, d_lags, d_keys + capacity, nullptr);
    if (st != noErr) {
        (void)hipStreamSynchronize(nullptr);       // whatever was launched has left the key buffer before its next user
        return st;
    }
    // the count first, then only the matches that exist: a generous capacity costs the device block and its memsets, no copy
    unsigned long long total = 0;
    LBAD_HIP(hipMemcpy(&total, d_keys + capacity, sizeof(total), hipMemcpyDeviceToHost));
    const size_t m = (size_t)(total < capacity ? total : capacity);
    std::vector<unsigned long long> keys(m);
    std::vector<int32_t> lags(out_lags ? m : 0);
    if (m) LBAD_HIP(hipMemcpy(keys.data(), d_keys, m * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    if (m && out_lags) LBAD_HIP(hipMemcpy(lags.data(), d_lags, m * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (uint64_t at = 0; at < capacity; ++at) {
        if (at < m) {
            LBAudioDetectiveCorpusDecodeKey(keys[at], out_idx + at, out_scores + at);
            if (out_lags) out_lags[at] = lags[at];
        } else {
            out_idx[at] = -1; out_scores[at] = 0.0f;
            if (out_lags) out_lags[at] = 0;
        }
    }
    *out_count = total;
    return noErr;
}

}  // namespace
}  // namespace lbad

extern "C" {

OSStatus LBAudioDetectiveCorpusQueryOccurrencesKeysDevice(LBAudioDetectiveCorpusRef c, LBAudioDetectiveFingerprintRef inQuery, UInt32 inRange,
                                                          Float32 inThreshold, UInt32 inPeaksOnly, UInt64 inCapacity, UInt64 inIndexBase,
                                                          void* outKeys, void* outLags, void* outCount, void* inStream) {
    LBAD_GUARD_BEGIN
    return lbad::occurrences_handle_impl(c, inQuery, inRange, inThreshold, inPeaksOnly, inCapacity, inIndexBase,
                                         static_cast<unsigned long long*>(outKeys), static_cast<int32_t*>(outLags),
                                         static_cast<unsigned long long*>(outCount), static_cast<hipStream_t>(inStream));
    LBAD_GUARD_END
}

OSStatus LBAudioDetectiveCorpusQueryPackedOccurrencesKeysDevice(LBAudioDetectiveCorpusRef c, const void* inPackedQuery,
                                                                UInt32 inSubfingerprints, UInt32 inRange, Float32 inThreshold,
                                                                UInt32 inPeaksOnly, UInt64 inCapacity, UInt64 inIndexBase, void* outKeys,
                                                                void* outLags, void* outCount, void* inStream) {
    LBAD_GUARD_BEGIN
    return lbad::occurrences_packed_impl(c, static_cast<const uint32_t*>(inPackedQuery), inSubfingerprints, inRange, inThreshold,
                                         inPeaksOnly, inCapacity, inIndexBase, static_cast<unsigned long long*>(outKeys),
                                         static_cast<int32_t*>(outLags), static_cast<unsigned long long*>(outCount),
                                         static_cast<hipStream_t>(inStream));
    LBAD_GUARD_END
}

OSStatus LBAudioDetectiveCorpusQueryOccurrences(LBAudioDetectiveCorpusRef c, LBAudioDetectiveFingerprintRef inQuery, UInt32 inRange,
                                                Float32 inThreshold, UInt32 inPeaksOnly, UInt64 inCapacity, SInt64* outIndices,
                                                Float32* outScores, SInt32* outLags, UInt64* outCount) {
    LBAD_GUARD_BEGIN
    return lbad::occurrences_host_impl(c, inQuery, inRange, inThreshold, inPeaksOnly, inCapacity, outIndices, outScores, outLags,
                                       outCount);
    LBAD_GUARD_END
}

}  // extern "C"
