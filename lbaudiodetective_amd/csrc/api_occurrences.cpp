// api_occurrences.cpp -- every place a recording matches a ragged corpus (k_occurrences.hip): the cells of every entry's
// profile at or above a score, as keys and lags on the device, from a handle or from packed sub-fingerprints on the device,
// and the host-returning form.  The plan, the query's staging, the events and the key block are recording_pass.cpp's.
#include "internal.hpp"

#include <cmath>

namespace lbad {
namespace {

const PassFamily kFamily = {occurrences_tiles, occurrences_chunk_entries, occurrences_block_entries};

// what needs neither handle nor device: a finite threshold above 0, 1 .. 2^31 slots, an index base a corpus can lie behind
bool occurrences_args_ok(float threshold, uint64_t capacity, uint64_t index_base) {
    return std::isfinite(threshold) && threshold > 0.0f && capacity != 0 && capacity <= 0x80000000ull && index_base <= 0x100000000ull;
}

// everything behind the staging of the query, on the call's stream: the zeros, the pass chunk by chunk, the count
OSStatus occurrences_launch(LBAudioDetectiveCorpus* c, const OccurrencesCall& call, uint64_t chunk, unsigned long long* count) {
    LBAD_HIP(hipMemsetAsync(call.d_keys, 0, (size_t)call.capacity * sizeof(unsigned long long), call.stream));
    if (call.d_lags) LBAD_HIP(hipMemsetAsync(call.d_lags, 0, (size_t)call.capacity * sizeof(int32_t), call.stream));
    LBAD_HIP(pass_chunks(c->count, chunk, [&](uint64_t e0, uint64_t n) {
        return launch_occurrences_chunk(call, c->d_join_scratch, chunk, e0, n, e0 == 0 ? 1u : 0u);
    }));
    // the running total behind the last chunk is the call's count
    LBAD_HIP(hipMemcpyAsync(count, c->d_join_scratch.get(), sizeof(unsigned long long), hipMemcpyDeviceToDevice, call.stream));
    return noErr;
}

// One call.  The caller has checked what needs no handle, and the device.
OSStatus occurrences_impl(LBAudioDetectiveCorpus* c, const PassQuery& q, float threshold, uint32_t peaks, uint64_t capacity,
                          uint64_t index_base, unsigned long long* keys, int32_t* lags, unsigned long long* count, hipStream_t stream) {
    PassPlan plan;
    OSStatus st = pass_plan(c, q, index_base, kFamily, &plan);
    if (st != noErr) return st;
    if (c->count == 0) {                                   // nothing to compare: zeros
        LBAD_HIP(hipMemsetAsync(keys, 0, (size_t)capacity * sizeof(unsigned long long), stream));
        if (lags) LBAD_HIP(hipMemsetAsync(lags, 0, (size_t)capacity * sizeof(int32_t), stream));
        LBAD_HIP(hipMemsetAsync(count, 0, sizeof(unsigned long long), stream));
        return noErr;
    }
    PassGuard guard(c, q, false);
    st = guard.wait();                                     // (the scratch is the previous call's until then)
    if (st == noErr) st = c->d_join_scratch.reserve(occurrences_scratch_bytes(plan.chunk, plan.call.tiles));
    if (st != noErr) return st;
    OccurrencesCall call;
    static_cast<OcPassCall&>(call) = plan.call;
    call.threshold = threshold; call.peaks = peaks != 0; call.capacity = capacity; call.index_base = index_base;
    call.d_keys = keys; call.d_lags = lags;
    st = pass_stage_query(c, q, stream, &call);
    if (st == noErr) st = occurrences_launch(c, call, plan.chunk, count);
    return guard.finish(stream, st);
}

OSStatus occurrences_handle_impl(LBAudioDetectiveCorpus* c, const LBAudioDetectiveFingerprint* q, uint32_t range, float threshold,
                                 uint32_t peaks, uint64_t capacity, uint64_t index_base, unsigned long long* keys, int32_t* lags,
                                 unsigned long long* count, hipStream_t stream) {
    if (!c || !q || !keys || !count || !occurrences_args_ok(threshold, capacity, index_base)) return kLBAudioDetectiveArgumentInvalid;
    if (!device_ready()) return kLBAudioDetectiveDeviceUnavailable;
    PassQuery pq;
    pq.fp = q; pq.range = range;
    return occurrences_impl(c, pq, threshold, peaks, capacity, index_base, keys, lags, count, stream);
}

OSStatus occurrences_packed_impl(LBAudioDetectiveCorpus* c, const uint32_t* d_rows, uint32_t per, uint32_t range, float threshold,
                                 uint32_t peaks, uint64_t capacity, uint64_t index_base, unsigned long long* keys, int32_t* lags,
                                 unsigned long long* count, hipStream_t stream) {
    if (!c || !d_rows || !keys || !count || per == 0 || per > 0x7FFFFFFFu || !occurrences_args_ok(threshold, capacity, index_base))
        return kLBAudioDetectiveArgumentInvalid;
    if (!device_ready()) return kLBAudioDetectiveDeviceUnavailable;
    PassQuery pq;
    pq.d_rows = d_rows; pq.per = per; pq.range = range;
    return occurrences_impl(c, pq, threshold, peaks, capacity, index_base, keys, lags, count, stream);
}

// host-returning form: keys, the count and the lags in ONE block of the corpus' key buffer on the null stream; the count is
// read back first, then min(count, capacity) keys and lags
OSStatus occurrences_host_impl(LBAudioDetectiveCorpus* c, const LBAudioDetectiveFingerprint* q, uint32_t range, float threshold,
                               uint32_t peaks, uint64_t capacity, SInt64* out_idx, Float32* out_scores, SInt32* out_lags,
                               UInt64* out_count) {
    if (!c || !q || !out_idx || !out_scores || !out_count || !occurrences_args_ok(threshold, capacity, 0))
        return kLBAudioDetectiveArgumentInvalid;
    if (!device_ready()) return kLBAudioDetectiveDeviceUnavailable;
    PassQuery pq;
    pq.fp = q; pq.range = range;
    PassPlan plan;
    OSStatus st = pass_plan(c, pq, 0, kFamily, &plan);     // (a refused call reserves nothing)
    if (st != noErr) return st;
    KeyBlock b;                                            // the keys, then the count
    st = key_block_reserve(c, (size_t)capacity + 1, out_lags ? (size_t)capacity : 0, &b);
    if (st != noErr) return st;
    st = occurrences_impl(c, pq, threshold, peaks, capacity, 0, b.d_keys, reinterpret_cast<int32_t*>(b.d_words), b.d_keys + capacity,
                          nullptr);
    if (st != noErr) return key_block_failed(st);
    // the count first, then only the matches that exist: a generous capacity costs the device block and its memsets, no copy
    unsigned long long total = 0;
    LBAD_HIP(hipMemcpy(&total, b.d_keys + capacity, sizeof(total), hipMemcpyDeviceToHost));
    const size_t m = (size_t)(total < capacity ? total : capacity);
    std::vector<unsigned long long> host;
    st = key_block_read(b, m, &host);
    if (st != noErr) return st;
    const int32_t* lags = reinterpret_cast<const int32_t*>(host.data() + m);
    for (uint64_t at = 0; at < capacity; ++at) {
        if (at < m) {
            LBAudioDetectiveCorpusDecodeKey(host[at], out_idx + at, out_scores + at);
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
