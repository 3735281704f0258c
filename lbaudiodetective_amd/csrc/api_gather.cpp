// api_gather.cpp -- entries handed back out of a corpus: the host side of k_gather.hip.
// The entries a key list names come back in list order in the packed layout -- what LBAudioDetectiveFingerprintClipsDevice
// writes and every ...Packed...Device call reads -- with the rows' offsets beside them.  The device form is asynchronous on the
// caller's stream; the host form and LBAudioDetectiveCorpusCopyFingerprint are that form on the null stream with one read-back.
#include "internal.hpp"

#include <cstring>

namespace lbad {
namespace {

// what needs neither handle nor device (the packed rows go out as 16-byte stores, keys and offsets as 8-byte words)
bool gather_args_ok(const void* corpus, const void* list, uint64_t n, uint64_t index_base, const void* packed, uint64_t capacity,
                    const void* offsets) {
    if (!corpus || !offsets || (n && !list) || (capacity && !packed)) return false;
    if (n > 0x80000000ull || index_base > 0x100000000ull) return false;
    return (reinterpret_cast<uintptr_t>(packed) & 15u) == 0 && (reinterpret_cast<uintptr_t>(offsets) & 7u) == 0 &&
           (reinterpret_cast<uintptr_t>(list) & 7u) == 0;
}

// the device form behind its argument checks
OSStatus gather_keys(LBAudioDetectiveCorpus* c, const unsigned long long* d_keys, uint64_t n, uint64_t index_base, void* d_packed,
                     uint64_t capacity, unsigned long long* d_offsets, hipStream_t stream) {
    if (n == 0) {
        LBAD_HIP(hipMemsetAsync(d_offsets, 0, sizeof(unsigned long long), stream));
        return noErr;
    }
    OSStatus st = c->gather_ev.wait_or_create();                      // (the scratch is the previous call's until then)
    if (st == noErr) st = c->d_gather_scratch.reserve(gather_scratch_bytes(n));
    if (st != noErr) return st;
    if (c->append_event.ev) LBAD_HIP(hipStreamWaitEvent(stream, c->append_event, 0));     // the latest append, awaited on the device
    GatherSource src;
    src.ragged = c->ragged;
    src.recs = c->d_recs; src.off = c->d_off; src.ne_max = c->ne_max;
    src.planes = c->d_planes; src.stride = c->capacity; src.n_planes = c->n_planes; src.n_sub = c->n_sub;
    src.count = c->count; src.subfp_len = c->subfp_len;
    st = hip_status(launch_gather(src, d_keys, n, index_base, c->d_gather_scratch, d_packed, capacity, d_offsets, stream), "gather", __LINE__);
    // behind whatever was launched, also after a failure: the scratch and the corpus' blocks are in use until then
    const OSStatus rec = c->gather_ev.record(stream);
    return st != noErr ? st : rec;
}

// host form: keys, offsets and packed rows in ONE block of its own on the null stream, one read-back
OSStatus gather_indices(LBAudioDetectiveCorpus* c, const UInt64* indices, uint64_t n, void* out_packed, uint64_t capacity,
                        UInt64* out_offsets) {
    for (uint64_t i = 0; i < n; ++i)
        if (indices[i] >= c->count) return kLBAudioDetectiveArgumentInvalid;            // nothing has been written
    if (n == 0) {
        out_offsets[0] = 0;
        return noErr;
    }
    // rows that can exist: the copy back never moves more than the rows' true total
    uint64_t total = 0;
    for (uint64_t i = 0; i < n; ++i) total += c->ragged ? (uint64_t)(c->h_off[indices[i] + 1] - c->h_off[indices[i]]) : (uint64_t)c->n_sub;
    const uint64_t rows = total < capacity ? total : capacity;
    const size_t packed_at = (size_t)((2 * n + 1 + 1) & ~1ull);                         // (16-byte aligned)
    std::vector<unsigned long long> host(packed_at + (size_t)(4 * rows));               // keys | offsets | packed (32 bytes a row)
    for (uint64_t i = 0; i < n; ++i) host[i] = 0xFFFFFFFFull - indices[i];
    DeviceBuffer<unsigned long long> block;
    OSStatus st = block.reserve(host.size());
    if (st != noErr) return st;
    LBAD_HIP(hipMemcpy(block, host.data(), (size_t)n * sizeof(unsigned long long), hipMemcpyHostToDevice));
    st = gather_keys(c, block, n, 0, rows ? block + packed_at : nullptr, rows, block + n, nullptr);
    if (st != noErr) {
        (void)hipStreamSynchronize(nullptr);       // whatever was launched has left the block before it goes
        return st;
    }
    LBAD_HIP(hipMemcpy(host.data() + n, block + n, (host.size() - (size_t)n) * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    if (host[(size_t)(2 * n)] != total) return kLBAudioDetectiveDeviceError;            // (the host's offsets say otherwise)
    std::memcpy(out_offsets, host.data() + n, (size_t)(n + 1) * sizeof(UInt64));
    if (rows) std::memcpy(out_packed, host.data() + packed_at, (size_t)rows * LBAD_PACKED_BYTES);
    return noErr;
}

}  // namespace
}  // namespace lbad

extern "C" {

OSStatus LBAudioDetectiveCorpusGatherKeysDevice(LBAudioDetectiveCorpusRef inCorpus, const void* inKeys, UInt64 inCount, UInt64 inIndexBase,
                                                void* outPacked, UInt64 inCapacity, void* outOffsets, void* inStream) {
    LBAD_GUARD_BEGIN
    if (!lbad::gather_args_ok(inCorpus, inKeys, inCount, inIndexBase, outPacked, inCapacity, outOffsets)) return kLBAudioDetectiveArgumentInvalid;
    if (!lbad::device_ready()) return kLBAudioDetectiveDeviceUnavailable;
    if (inIndexBase + inCorpus->count > 0x100000000ull) return kLBAudioDetectiveArgumentInvalid;
    return lbad::gather_keys(inCorpus, static_cast<const unsigned long long*>(inKeys), inCount, inIndexBase, outPacked, inCapacity,
                             static_cast<unsigned long long*>(outOffsets), static_cast<hipStream_t>(inStream));
    LBAD_GUARD_END
}

OSStatus LBAudioDetectiveCorpusGatherIndices(LBAudioDetectiveCorpusRef inCorpus, const UInt64* inIndices, UInt64 inCount, void* outPacked,
                                             UInt64 inCapacity, UInt64* outOffsets) {
    LBAD_GUARD_BEGIN
    // (host memory: no alignment is asked of it)
    if (!inCorpus || !outOffsets || (inCount && !inIndices) || (inCapacity && !outPacked) || inCount > 0x80000000ull)
        return kLBAudioDetectiveArgumentInvalid;
    if (!lbad::device_ready()) return kLBAudioDetectiveDeviceUnavailable;
    return lbad::gather_indices(inCorpus, inIndices, inCount, outPacked, inCapacity, outOffsets);
    LBAD_GUARD_END
}

LBAudioDetectiveFingerprintRef LBAudioDetectiveCorpusCopyFingerprint(LBAudioDetectiveCorpusRef inCorpus, UInt64 inIndex) {
    try {
        if (!inCorpus || !lbad::device_ready()) return NULL;
        LBAudioDetectiveCorpus* c = inCorpus;
        if (inIndex >= c->count) return NULL;
        const uint64_t n_sub = c->ragged ? (uint64_t)(c->h_off[inIndex + 1] - c->h_off[inIndex]) : (uint64_t)c->n_sub;
        std::vector<uint32_t> words((size_t)n_sub * lbad::kPackedWords);
        UInt64 offsets[2] = {0, 0};
        if (lbad::gather_indices(c, &inIndex, 1, words.data(), n_sub, offsets) != noErr || offsets[1] != n_sub) return NULL;
        LBAudioDetectiveFingerprint* fp = new LBAudioDetectiveFingerprint();
        fp->length = c->subfp_len;
        fp->count = (uint32_t)n_sub;
        try {
            fp->data.assign((size_t)n_sub * c->subfp_len, 0);
        } catch (const std::bad_alloc&) {
            delete fp;
            return NULL;
        }
        for (uint64_t s = 0; s < n_sub; ++s)
            LBAudioDetectiveUnpackSubfingerprint(words.data() + (size_t)s * lbad::kPackedWords, c->subfp_len,
                                                 fp->data.data() + (size_t)s * c->subfp_len);
        return fp;
    } catch (const std::exception&) {
        return NULL;
    }
}

}  // extern "C"
