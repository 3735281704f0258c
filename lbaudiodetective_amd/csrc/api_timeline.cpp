// api_timeline.cpp -- the recording timeline (k_timeline.hip): the best entry of a ragged corpus at every offset of ONE query, a
// long recording above all, as keys and lengths on the device, from a handle or from packed sub-fingerprints on the device, and
// the host-returning form.  The plan, the query's staging, the events and the key block are recording_pass.cpp's.
#include "internal.hpp"

#include <cmath>

namespace lbad {
namespace {

const PassFamily kFamily = {[](uint32_t n_query, uint32_t ne_min, uint32_t) { return timeline_tiles(n_query, ne_min); }, timeline_chunk_entries,
                            timeline_block_entries};

// what needs neither handle nor device: a finite threshold above 0, an index base a corpus can lie behind
bool timeline_args_ok(float threshold, uint64_t index_base) {
    return std::isfinite(threshold) && threshold > 0.0f && index_base <= 0x100000000ull;
}

// everything behind the staging of the query, on the call's stream: the pass chunk by chunk into the keys, then the lengths
OSStatus timeline_launch(LBAudioDetectiveCorpus* c, const TimelineCall& call, uint64_t chunk, uint32_t* lengths) {
    LBAD_HIP(pass_chunks(c->count, chunk, [&](uint64_t e0, uint64_t n) { return launch_timeline_chunk(call, c->d_join_scratch, e0, n); }));
    if (lengths) LBAD_HIP(launch_timeline_lengths(call.d_keys, call.n_query, call.index_base, c->count, c->d_off, lengths, call.stream));
    return noErr;
}

// One call.  The caller has checked what needs no handle, and the device.
OSStatus timeline_impl(LBAudioDetectiveCorpus* c, const PassQuery& q, float threshold, uint64_t index_base, unsigned long long* keys,
                       uint32_t* lengths, hipStream_t stream) {
    PassPlan plan;
    OSStatus st = pass_plan(c, q, index_base, kFamily, &plan);
    if (st != noErr) return st;
    const uint32_t n_query = plan.call.n_query;
    // the keys carry the running maximum from chunk to chunk: zeros in front of the first.  Where no entry takes part these
    // zeros (and the lengths') are the answer.
    LBAD_HIP(hipMemsetAsync(keys, 0, (size_t)n_query * sizeof(unsigned long long), stream));
    if (!plan.any) {
        if (lengths) LBAD_HIP(hipMemsetAsync(lengths, 0, (size_t)n_query * sizeof(uint32_t), stream));
        return noErr;
    }
    PassGuard guard(c, q, false);
    st = guard.wait();                                     // (the scratch is the previous call's until then)
    if (st == noErr) st = c->d_join_scratch.reserve(timeline_scratch_bytes(plan.chunk, plan.call.tiles));
    if (st != noErr) return st;
    TimelineCall call;
    static_cast<OcPassCall&>(call) = plan.call;
    call.threshold = threshold; call.index_base = index_base; call.d_keys = keys;
    st = pass_stage_query(c, q, stream, &call);
    if (st == noErr) st = timeline_launch(c, call, plan.chunk, lengths);
    return guard.finish(stream, st);
}

OSStatus timeline_handle_impl(LBAudioDetectiveCorpus* c, const LBAudioDetectiveFingerprint* q, uint32_t range, float threshold,
                              uint64_t index_base, unsigned long long* keys, uint32_t* lengths, hipStream_t stream) {
    if (!c || !q || !keys || !timeline_args_ok(threshold, index_base)) return kLBAudioDetectiveArgumentInvalid;
    if (!device_ready()) return kLBAudioDetectiveDeviceUnavailable;
    PassQuery pq;
    pq.fp = q; pq.range = range;
    return timeline_impl(c, pq, threshold, index_base, keys, lengths, stream);
}

OSStatus timeline_packed_impl(LBAudioDetectiveCorpus* c, const uint32_t* d_rows, uint32_t per, uint32_t range, float threshold,
                              uint64_t index_base, unsigned long long* keys, uint32_t* lengths, hipStream_t stream) {
    if (!c || !d_rows || !keys || per == 0 || per > 0x7FFFFFFFu || !timeline_args_ok(threshold, index_base))
        return kLBAudioDetectiveArgumentInvalid;
    if (!device_ready()) return kLBAudioDetectiveDeviceUnavailable;
    PassQuery pq;
    pq.d_rows = d_rows; pq.per = per; pq.range = range;
    return timeline_impl(c, pq, threshold, index_base, keys, lengths, stream);
}

// host-returning form: keys and (out_lengths given) lengths in ONE block of the corpus' key buffer on the null stream, then
// decoded
OSStatus timeline_host_impl(LBAudioDetectiveCorpus* c, const LBAudioDetectiveFingerprint* q, uint32_t range, float threshold,
                            SInt64* out_idx, Float32* out_scores, UInt32* out_lengths, UInt64* out_count) {
    if (!c || !q || !out_idx || !out_scores || !out_count || !timeline_args_ok(threshold, 0)) return kLBAudioDetectiveArgumentInvalid;
    if (!device_ready()) return kLBAudioDetectiveDeviceUnavailable;
    PassQuery pq;
    pq.fp = q; pq.range = range;
    PassPlan plan;
    OSStatus st = pass_plan(c, pq, 0, kFamily, &plan);     // (a refused call reserves nothing)
    if (st != noErr) return st;
    const size_t n = q->count;
    KeyBlock b;
    st = key_block_reserve(c, n, out_lengths ? n : 0, &b);
    if (st != noErr) return st;
    st = timeline_impl(c, pq, threshold, 0, b.d_keys, b.d_words, nullptr);
    if (st != noErr) return key_block_failed(st);
    std::vector<unsigned long long> host;
    st = key_block_read(b, n, &host);
    if (st != noErr) return st;
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
