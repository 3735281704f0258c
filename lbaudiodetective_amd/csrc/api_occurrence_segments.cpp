// api_occurrence_segments.cpp -- occurrence segments (k_occurrence_segments.hip): the non-overlapping spans over
// ALL cells of an occurrences call's rows, for one recording or a batch, from keys, lags and entry lengths on the device to a key
// block on the device -- no handle, no scratch, no event: one launch on the caller's stream -- and the call that makes the
// lengths from the keys, which does take the corpus: each shard computes the lengths of its own keys before rows are joined.
#include "internal.hpp"

namespace lbad {
namespace {

bool aligned_to(const void* p, uintptr_t bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0; }

// what needs no device
bool occurrence_segments_args_ok(const void* in_keys, const void* in_lags, const void* in_lengths, const void* in_counts,
                                 uint32_t recordings, uint32_t cap_in, uint32_t per, uint32_t cap_out, const void* out_starts,
                                 const void* out_keys, const void* out_lags, const void* out_lengths, const void* out_counts) {
    if (!in_keys || !in_lags || !in_lengths || !out_starts || !out_keys || !out_counts) return false;
    if (recordings == 0 || cap_in == 0 || per == 0 || cap_out == 0) return false;
    if (per > LBAD_SEGMENTS_MAX_SUBFINGERPRINTS || cap_in > LBAD_OCCURRENCE_SEGMENTS_MAX_CANDIDATES) return false;
    if ((uint64_t)recordings * cap_in > 0x7FFFFFFFull || (uint64_t)recordings * per > 0x7FFFFFFFull ||
        (uint64_t)recordings * cap_out > 0x7FFFFFFFull)
        return false;
    if (!aligned_to(in_keys, 8) || !aligned_to(in_counts, 8) || !aligned_to(out_keys, 8) || !aligned_to(in_lags, 4) ||
        !aligned_to(in_lengths, 4) || !aligned_to(out_starts, 4) || !aligned_to(out_lags, 4) || !aligned_to(out_lengths, 4) ||
        !aligned_to(out_counts, 4))
        return false;
    return out_keys != in_keys && out_lags != in_lags && out_lengths != in_lengths;
}

}  // namespace
}  // namespace lbad

extern "C" {

OSStatus LBAudioDetectiveOccurrenceSegmentsFromKeysDevice(const void* inKeys, const void* inLags, const void* inLengths, const void* inCounts,
                                                          UInt32 inRecordings, UInt32 inCapacity, UInt32 inSubfingerprints,
                                                          UInt32 inOutCapacity, void* outStarts, void* outKeys, void* outLags,
                                                          void* outLengths, void* outCounts, void* inStream) {
    LBAD_GUARD_BEGIN
    if (!lbad::occurrence_segments_args_ok(inKeys, inLags, inLengths, inCounts, inRecordings, inCapacity, inSubfingerprints, inOutCapacity,
                                           outStarts, outKeys, outLags, outLengths, outCounts))
        return kLBAudioDetectiveArgumentInvalid;
    if (!lbad::device_ready()) return kLBAudioDetectiveDeviceUnavailable;
    LBAD_HIP(lbad::launch_occurrence_segments(static_cast<const unsigned long long*>(inKeys), static_cast<const int32_t*>(inLags),
                                              static_cast<const uint32_t*>(inLengths), static_cast<const unsigned long long*>(inCounts),
                                              inRecordings, inCapacity, inSubfingerprints, inOutCapacity, static_cast<uint32_t*>(outStarts),
                                              static_cast<unsigned long long*>(outKeys), static_cast<int32_t*>(outLags),
                                              static_cast<uint32_t*>(outLengths), static_cast<uint32_t*>(outCounts),
                                              static_cast<hipStream_t>(inStream)));
    return noErr;
    LBAD_GUARD_END
}

OSStatus LBAudioDetectiveCorpusEntryLengthsFromKeysDevice(LBAudioDetectiveCorpusRef inCorpus, const void* inKeys, UInt64 inCount,
                                                          UInt64 inIndexBase, void* outLengths, void* inStream) {
    LBAD_GUARD_BEGIN
    // what needs neither handle nor device
    if (!inCorpus || !inKeys || !outLengths || inCount == 0 || inCount > 0x7FFFFFFFull || inIndexBase > 0x100000000ull ||
        !lbad::aligned_to(inKeys, 8) || !lbad::aligned_to(outLengths, 4))
        return kLBAudioDetectiveArgumentInvalid;
    if (!lbad::device_ready()) return kLBAudioDetectiveDeviceUnavailable;
    LBAudioDetectiveCorpus* c = inCorpus;
    if (inIndexBase + c->count > 0x100000000ull) return kLBAudioDetectiveArgumentInvalid;
    hipStream_t stream = static_cast<hipStream_t>(inStream);
    if (c->append_event.ev) LBAD_HIP(hipStreamWaitEvent(stream, c->append_event, 0));     // the latest append, awaited on the device
    const unsigned long long* keys = static_cast<const unsigned long long*>(inKeys);
    uint32_t* lengths = static_cast<uint32_t*>(outLengths);
    if (c->ragged)
        LBAD_HIP(lbad::launch_timeline_lengths(keys, (uint32_t)inCount, inIndexBase, c->count, c->d_off, lengths, stream));
    else
        LBAD_HIP(lbad::launch_entry_lengths_uniform(keys, (uint32_t)inCount, inIndexBase, c->count, c->n_sub, lengths, stream));
    return noErr;
    LBAD_GUARD_END
}

}  // extern "C"
