// api_segments.cpp -- recording segments (k_segments.hip): the non-overlapping spans of a timeline's per-offset winners, for one
// recording or a batch, from keys and lengths on the device to a key block on the device.  No handle, no scratch, no event: one
// launch on the caller's stream.
#include "internal.hpp"

namespace lbad {
namespace {

bool aligned_to(const void* p, uintptr_t bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0; }

// what needs no device
bool segments_args_ok(const void* in_keys, const void* in_lengths, uint32_t recordings, uint32_t per, uint32_t capacity,
                      const void* out_starts, const void* out_keys, const void* out_lengths, const void* out_counts) {
    if (!in_keys || !in_lengths || !out_starts || !out_keys || !out_counts) return false;
    if (recordings == 0 || per == 0 || capacity == 0 || per > LBAD_SEGMENTS_MAX_SUBFINGERPRINTS) return false;
    if ((uint64_t)recordings * per > 0x7FFFFFFFull || (uint64_t)recordings * capacity > 0x7FFFFFFFull) return false;
    if (!aligned_to(in_keys, 8) || !aligned_to(out_keys, 8) || !aligned_to(in_lengths, 4) || !aligned_to(out_starts, 4) ||
        !aligned_to(out_lengths, 4) || !aligned_to(out_counts, 4))
        return false;
    return out_keys != in_keys && out_lengths != in_lengths;
}

}  // namespace
}  // namespace lbad

extern "C" {

OSStatus LBAudioDetectiveTimelineSegmentsFromKeysDevice(const void* inKeys, const void* inLengths, UInt32 inRecordings,
                                                        UInt32 inSubfingerprints, UInt32 inCapacity, void* outStarts, void* outKeys,
                                                        void* outLengths, void* outCounts, void* inStream) {
    LBAD_GUARD_BEGIN
    if (!lbad::segments_args_ok(inKeys, inLengths, inRecordings, inSubfingerprints, inCapacity, outStarts, outKeys, outLengths, outCounts))
        return kLBAudioDetectiveArgumentInvalid;
    if (!lbad::device_ready()) return kLBAudioDetectiveDeviceUnavailable;
    LBAD_HIP(lbad::launch_timeline_segments(static_cast<const unsigned long long*>(inKeys), static_cast<const uint32_t*>(inLengths),
                                            inRecordings, inSubfingerprints, inCapacity, static_cast<uint32_t*>(outStarts),
                                            static_cast<unsigned long long*>(outKeys), static_cast<uint32_t*>(outLengths),
                                            static_cast<uint32_t*>(outCounts), static_cast<hipStream_t>(inStream)));
    return noErr;
    LBAD_GUARD_END
}

}  // extern "C"
