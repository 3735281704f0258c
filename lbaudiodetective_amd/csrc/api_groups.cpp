// api_groups.cpp -- duplicate groups out of match keys: the host side of k_groups.hip.
// The labels call turns the keys of a join or of a threshold batch into the connected components of the match graph where the
// keys lie: asynchronous on the caller's stream, no read-back, no scratch beyond the caller's buffers.  The extra-keys call
// turns labels into the key list "everything except the first entry of each group", which the removal takes as it is; like
// LBAudioDetectiveThresholdKeysFromScoresDevice it owns its scratch and returns once the keys are written.
#include "internal.hpp"

namespace lbad {
namespace {

constexpr uint64_t kTwo32 = 0x100000000ull, kTwo31 = 0x80000000ull;

bool aligned_to(const void* p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) == 0; }

// what needs neither device nor memory
bool labels_args_ok(const void* keys, uint64_t n_slots, const void* offsets, uint64_t pitch, uint64_t n_rows, uint64_t first_row,
                    const void* row_keys, uint64_t index_base, uint64_t n, const void* labels, const void* group_count) {
    if (!labels || (n_slots && !keys)) return false;
    if (index_base > kTwo32 || n > kTwo32 || index_base + n > kTwo32) return false;
    if (n_slots > kTwo31 || n_rows > kTwo32) return false;
    if (!row_keys && (first_row > kTwo32 || first_row + n_rows > n)) return false;
    // (rows of more than 2^31 slots hold more than n_slots can be; below that the product is at most 2^63)
    if (!offsets && (pitch == 0 || (n_rows != 0 && pitch > kTwo31) || (n_rows == 0 ? 0 : n_rows * pitch) != n_slots)) return false;
    return aligned_to(keys, 7u) && aligned_to(offsets, 7u) && aligned_to(row_keys, 7u) && aligned_to(labels, 3u) &&
           aligned_to(group_count, 7u);
}

bool extra_args_ok(const void* labels, uint64_t n, uint64_t index_base, uint64_t capacity, const void* keys, const void* count) {
    if (!labels || !keys || !count) return false;
    if (capacity == 0 || capacity > kTwo31) return false;
    if (index_base > kTwo32 || n > kTwo32 || index_base + n > kTwo32) return false;
    return aligned_to(labels, 3u) && aligned_to(keys, 7u);
}

}  // namespace
}  // namespace lbad

extern "C" {

OSStatus LBAudioDetectiveGroupLabelsFromKeysDevice(const void* inKeys, UInt64 inSlotCount, const void* inOffsets, UInt64 inRowPitch,
                                                   UInt64 inRowCount, UInt64 inFirstRow, const void* inRowKeys, UInt64 inIndexBase,
                                                   UInt64 inEntryCount, UInt32 inReset, void* ioLabels, void* outGroupCount,
                                                   void* inStream) {
    LBAD_GUARD_BEGIN
    if (!lbad::labels_args_ok(inKeys, inSlotCount, inOffsets, inRowPitch, inRowCount, inFirstRow, inRowKeys, inIndexBase, inEntryCount,
                              ioLabels, outGroupCount))
        return kLBAudioDetectiveArgumentInvalid;
    if (!lbad::device_ready()) return kLBAudioDetectiveDeviceUnavailable;
    hipStream_t stream = static_cast<hipStream_t>(inStream);
    // the flatten launch adds the roots it finds to the count
    if (outGroupCount) LBAD_HIP(hipMemsetAsync(outGroupCount, 0, sizeof(unsigned long long), stream));
    if (inEntryCount == 0) return noErr;
    return lbad::hip_status(lbad::launch_group_labels(static_cast<const unsigned long long*>(inKeys), inSlotCount,
                                                      static_cast<const unsigned long long*>(inOffsets), inOffsets ? 0 : inRowPitch,
                                                      inRowCount, inFirstRow, static_cast<const unsigned long long*>(inRowKeys),
                                                      inIndexBase, inEntryCount, inReset != 0, static_cast<uint32_t*>(ioLabels),
                                                      static_cast<unsigned long long*>(outGroupCount), stream),
                            "groups", __LINE__);
    LBAD_GUARD_END
}

OSStatus LBAudioDetectiveGroupExtraKeysFromLabelsDevice(const void* inLabels, UInt64 inEntryCount, UInt64 inIndexBase, UInt64 inCapacity,
                                                        void* outKeys, UInt64* outCount, void* inStream) {
    LBAD_GUARD_BEGIN
    if (!lbad::extra_args_ok(inLabels, inEntryCount, inIndexBase, inCapacity, outKeys, outCount)) return kLBAudioDetectiveArgumentInvalid;
    *outCount = 0;
    if (!lbad::device_ready()) return kLBAudioDetectiveDeviceUnavailable;
    hipStream_t stream = static_cast<hipStream_t>(inStream);
    unsigned long long* keys = static_cast<unsigned long long*>(outKeys);
    // the zero keys behind the list (and under it: the scatter launch writes the keys over them)
    LBAD_HIP(hipMemsetAsync(keys, 0, (size_t)inCapacity * sizeof(unsigned long long), stream));
    if (inEntryCount == 0) {
        LBAD_HIP(hipStreamSynchronize(stream));
        return noErr;
    }
    lbad::DeviceBuffer<void> scratch;                      // (its own: freed on return, behind the synchronisation below)
    OSStatus st = scratch.reserve(lbad::group_extra_scratch_bytes(inEntryCount));
    if (st != noErr) return st;
    st = lbad::hip_status(lbad::launch_group_extra_keys(static_cast<const uint32_t*>(inLabels), inEntryCount, inIndexBase, inCapacity, scratch,
                                                        keys, stream),
                          "group extra keys", __LINE__);
    unsigned long long count = 0;
    const char* last = static_cast<const char*>(scratch.get()) + lbad::group_extra_scratch_bytes(inEntryCount) - sizeof(count);
    if (st == noErr) st = lbad::hip_status(hipMemcpyAsync(&count, last, sizeof(count), hipMemcpyDeviceToHost, stream), "group extra keys", __LINE__);
    const OSStatus done = lbad::hip_status(hipStreamSynchronize(stream), "group extra keys", __LINE__);
    if (st != noErr || done != noErr) return st != noErr ? st : done;
    *outCount = count;
    return noErr;
    LBAD_GUARD_END
}

}  // extern "C"
