// api_ids.cpp -- the caller's 64-bit ids of corpus entries: the host side of k_ids.hip.
// A corpus starts without ids; the first ids set turn them on: `capacity` words on the device, zero (no id) wherever nothing was
// set, zero at and above the count -- so no append has to know of them.  The ids move with their entries when a removal closes
// the corpus up, are stored behind the payload of the corpus file, come back for any key list (IdsFromKeys) and name entries in
// the key format every taking call reads (KeysFromIds, through an index built on first use).  ids_ev orders every use of the
// id block, the index and their scratch.
#include "internal.hpp"

#include <cstring>

namespace lbad {
namespace {

constexpr char kIdsMagic[8] = {'L', 'B', 'A', 'D', 'I', 'D', 'S', '1'};
constexpr size_t kIdsPiece = 1u << 20;           // ids per staging piece of the file calls (8 MiB)

bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }

// what needs neither handle nor device, for the two list calls
bool list_args_ok(const void* corpus, const void* in, uint64_t n, uint64_t index_base, const void* out) {
    if (!corpus || (n && (!in || !out))) return false;
    if (n > 0x80000000ull || index_base > 0x100000000ull) return false;
    return aligned8(in) && aligned8(out);
}

// ... and for a range of entries
bool range_args_ok(const void* corpus, uint64_t first, uint64_t n, const void* p) {
    return corpus && !(n && !p) && first <= 0x100000000ull && n <= 0x100000000ull;
}

// the id block of a corpus that had none: `capacity` zero words, zeroed on `stream` in front of the caller's first copy
OSStatus turn_on(LBAudioDetectiveCorpus* c, hipStream_t stream) {
    OSStatus st = c->d_ids.reserve((size_t)c->capacity);
    if (st != noErr) return st;
    st = hip_status(hipMemsetAsync(c->d_ids, 0, (size_t)c->capacity * sizeof(unsigned long long), stream), "entry ids", __LINE__);
    if (st != noErr) c->d_ids.reset();
    return st;
}

// src: n ids on the device, or on the host in memory the copy may read until the stream has passed it (pinned)
OSStatus set_ids(LBAudioDetectiveCorpus* c, uint64_t first, uint64_t n, const void* src, hipMemcpyKind kind, hipStream_t stream) {
    const bool fresh = c->d_ids.get() == nullptr;
    OSStatus st = fresh ? turn_on(c, stream) : noErr;
    if (st != noErr) return st;
    st = hip_status(hipMemcpyAsync(c->d_ids + first, src, (size_t)n * sizeof(unsigned long long), kind, stream), "entry ids", __LINE__);
    if (st != noErr && fresh) {                  // (a block that may not be zero is no id block)
        (void)hipStreamSynchronize(stream);
        c->d_ids.reset();
    }
    c->ids_index_valid = false;
    // behind whatever was launched, also after a failure
    const OSStatus rec = c->ids_ev.record(stream);
    return st != noErr ? st : rec;
}

}  // namespace

OSStatus ids_compact(LBAudioDetectiveCorpus* c, const uint32_t* d_map, uint64_t first, uint64_t kept, hipStream_t stream) {
    if (!c->d_ids) return noErr;
    OSStatus st = c->ids_ev.wait_or_create();
    if (st == noErr) st = c->d_ids_scratch.reserve((size_t)(c->count - first));
    if (st != noErr) return st;
    st = hip_status(launch_ids_compact(c->d_ids, d_map, first, kept, c->count, c->d_ids_scratch, stream), "entry ids", __LINE__);
    c->ids_index_valid = false;
    const OSStatus rec = c->ids_ev.record(stream);
    return st != noErr ? st : rec;
}

OSStatus ids_save_trailer(LBAudioDetectiveCorpus* c, FILE* f) {
    if (!c->d_ids) return noErr;
    OSStatus st = c->ids_ev.wait();
    if (st != noErr) return st;
    const uint64_t count = c->count;
    if (std::fwrite(kIdsMagic, 8, 1, f) != 1 || std::fwrite(&count, sizeof(count), 1, f) != 1) return kLBAudioDetectiveDeviceError;
    std::vector<unsigned long long> host((size_t)(count < kIdsPiece ? count : kIdsPiece));
    for (uint64_t at = 0; at < count; at += kIdsPiece) {
        const size_t n = (size_t)(count - at < kIdsPiece ? count - at : kIdsPiece);
        st = hip_status(hipMemcpy(host.data(), c->d_ids + at, n * sizeof(unsigned long long), hipMemcpyDeviceToHost), "entry ids D2H", __LINE__);
        if (st != noErr) return st;
        if (std::fwrite(host.data(), sizeof(unsigned long long), n, f) != n) return kLBAudioDetectiveDeviceError;
    }
    return noErr;
}

// f stands behind the payload.  Untrusted: the count must be the payload's and the file must hold what it announces.
bool ids_load_trailer(LBAudioDetectiveCorpus* c, FILE* f, uint64_t count) {
    char magic[8];
    if (std::fread(magic, 1, 8, f) != 8 || std::memcmp(magic, kIdsMagic, 8) != 0) return true;      // no trailer: whatever follows is ignored
    uint64_t announced = 0;
    if (std::fread(&announced, sizeof(announced), 1, f) != 1 || announced != count || count > c->capacity) return false;
    const long at = std::ftell(f);
    if (at < 0 || std::fseek(f, 0, SEEK_END) != 0) return false;
    const long end = std::ftell(f);
    if (end < at || (uint64_t)(end - at) / sizeof(unsigned long long) < count || std::fseek(f, at, SEEK_SET) != 0) return false;
    if (c->d_ids.reserve((size_t)c->capacity) != noErr) return false;
    bool ok = hip_status(hipMemset(c->d_ids, 0, (size_t)c->capacity * sizeof(unsigned long long)), "entry ids", __LINE__) == noErr;
    unsigned long long* host = static_cast<unsigned long long*>(std::malloc(sizeof(unsigned long long) * (size_t)(count < kIdsPiece ? (count ? count : 1) : kIdsPiece)));
    if (!host) ok = false;
    for (uint64_t e = 0; ok && e < count; e += kIdsPiece) {
        const size_t n = (size_t)(count - e < kIdsPiece ? count - e : kIdsPiece);
        ok = std::fread(host, sizeof(unsigned long long), n, f) == n &&
             hip_status(hipMemcpy(c->d_ids + e, host, n * sizeof(unsigned long long), hipMemcpyHostToDevice), "entry ids H2D", __LINE__) == noErr;
    }
    std::free(host);
    c->ids_index_valid = false;
    return ok;
}

}  // namespace lbad

extern "C" {

OSStatus LBAudioDetectiveCorpusSetEntryIdsDevice(LBAudioDetectiveCorpusRef inCorpus, UInt64 inFirst, UInt64 inCount, const void* inIds,
                                                 void* inStream) {
    LBAD_GUARD_BEGIN
    if (!lbad::range_args_ok(inCorpus, inFirst, inCount, inIds) || !lbad::aligned8(inIds)) return kLBAudioDetectiveArgumentInvalid;
    if (!lbad::device_ready()) return kLBAudioDetectiveDeviceUnavailable;
    LBAudioDetectiveCorpus* c = inCorpus;
    if (inFirst + inCount > c->count) return kLBAudioDetectiveArgumentInvalid;          // nothing has changed
    if (inCount == 0) return noErr;
    OSStatus st = c->ids_ev.wait_or_create();
    if (st != noErr) return st;
    return lbad::set_ids(c, inFirst, inCount, inIds, hipMemcpyDeviceToDevice, static_cast<hipStream_t>(inStream));
    LBAD_GUARD_END
}

OSStatus LBAudioDetectiveCorpusSetEntryIds(LBAudioDetectiveCorpusRef inCorpus, UInt64 inFirst, UInt64 inCount, const UInt64* inIds) {
    LBAD_GUARD_BEGIN
    if (!lbad::range_args_ok(inCorpus, inFirst, inCount, inIds)) return kLBAudioDetectiveArgumentInvalid;
    if (!lbad::device_ready()) return kLBAudioDetectiveDeviceUnavailable;
    LBAudioDetectiveCorpus* c = inCorpus;
    if (inFirst + inCount > c->count) return kLBAudioDetectiveArgumentInvalid;
    if (inCount == 0) return noErr;
    OSStatus st = c->ids_ev.wait_or_create();                     // (the staging is the previous call's until then)
    if (st == noErr) st = c->h_ids_stage.reserve((size_t)inCount);
    if (st != noErr) return st;
    std::memcpy(c->h_ids_stage.get(), inIds, (size_t)inCount * sizeof(UInt64));
    return lbad::set_ids(c, inFirst, inCount, c->h_ids_stage.get(), hipMemcpyHostToDevice, nullptr);
    LBAD_GUARD_END
}

OSStatus LBAudioDetectiveCorpusGetEntryIds(LBAudioDetectiveCorpusRef inCorpus, UInt64 inFirst, UInt64 inCount, UInt64* outIds) {
    LBAD_GUARD_BEGIN
    if (!lbad::range_args_ok(inCorpus, inFirst, inCount, outIds)) return kLBAudioDetectiveArgumentInvalid;
    if (!lbad::device_ready()) return kLBAudioDetectiveDeviceUnavailable;
    LBAudioDetectiveCorpus* c = inCorpus;
    if (inFirst + inCount > c->capacity) return kLBAudioDetectiveArgumentInvalid;
    if (inCount == 0) return noErr;
    if (!c->d_ids) {
        std::memset(outIds, 0, (size_t)inCount * sizeof(UInt64));
        return noErr;
    }
    OSStatus st = c->ids_ev.wait();
    if (st != noErr) return st;
    LBAD_HIP(hipMemcpy(outIds, c->d_ids + inFirst, (size_t)inCount * sizeof(UInt64), hipMemcpyDeviceToHost));
    return noErr;
    LBAD_GUARD_END
}

UInt32 LBAudioDetectiveCorpusHasEntryIds(LBAudioDetectiveCorpusRef inCorpus) { return inCorpus && inCorpus->d_ids ? 1u : 0u; }

OSStatus LBAudioDetectiveCorpusIdsFromKeysDevice(LBAudioDetectiveCorpusRef inCorpus, const void* inKeys, UInt64 inCount, UInt64 inIndexBase,
                                                 void* outIds, void* inStream) {
    LBAD_GUARD_BEGIN
    if (!lbad::list_args_ok(inCorpus, inKeys, inCount, inIndexBase, outIds)) return kLBAudioDetectiveArgumentInvalid;
    if (!lbad::device_ready()) return kLBAudioDetectiveDeviceUnavailable;
    LBAudioDetectiveCorpus* c = inCorpus;
    if (inIndexBase + c->count > 0x100000000ull) return kLBAudioDetectiveArgumentInvalid;
    if (inCount == 0) return noErr;
    hipStream_t stream = static_cast<hipStream_t>(inStream);
    if (!c->d_ids) {                                              // no ids: zeros, and nothing of the corpus is touched
        LBAD_HIP(hipMemsetAsync(outIds, 0, (size_t)inCount * sizeof(UInt64), stream));
        return noErr;
    }
    OSStatus st = c->ids_ev.wait_or_create();
    if (st != noErr) return st;
    if (c->append_event.ev) LBAD_HIP(hipStreamWaitEvent(stream, c->append_event, 0));     // the latest append, awaited on the device
    st = lbad::hip_status(lbad::launch_ids_from_keys(static_cast<const unsigned long long*>(inKeys), inCount, inIndexBase, c->count, c->d_ids,
                                                     static_cast<unsigned long long*>(outIds), stream), "ids from keys", __LINE__);
    const OSStatus rec = c->ids_ev.record(stream);
    return st != noErr ? st : rec;
    LBAD_GUARD_END
}

OSStatus LBAudioDetectiveCorpusKeysFromIdsDevice(LBAudioDetectiveCorpusRef inCorpus, const void* inIds, UInt64 inCount, UInt64 inIndexBase,
                                                 void* outKeys, void* inStream) {
    LBAD_GUARD_BEGIN
    if (!lbad::list_args_ok(inCorpus, inIds, inCount, inIndexBase, outKeys)) return kLBAudioDetectiveArgumentInvalid;
    if (!lbad::device_ready()) return kLBAudioDetectiveDeviceUnavailable;
    LBAudioDetectiveCorpus* c = inCorpus;
    if (inIndexBase + c->count > 0x100000000ull) return kLBAudioDetectiveArgumentInvalid;
    if (inCount == 0) return noErr;
    hipStream_t stream = static_cast<hipStream_t>(inStream);
    if (!c->d_ids) {                                              // no ids: no entry has any, every key is the zero key
        LBAD_HIP(hipMemsetAsync(outKeys, 0, (size_t)inCount * sizeof(UInt64), stream));
        return noErr;
    }
    OSStatus st = c->ids_ev.wait_or_create();
    if (st != noErr) return st;
    if (c->append_event.ev) LBAD_HIP(hipStreamWaitEvent(stream, c->append_event, 0));
    if (!c->ids_index_valid) {                                    // stale: rebuilt whole, on this call's stream
        const uint64_t slots = lbad::ids_index_slots(c->count);
        st = c->d_ids_slot_ids.reserve((size_t)slots);
        if (st == noErr) st = c->d_ids_slot_index.reserve((size_t)slots);
        if (st != noErr) return st;                               // (nothing was launched)
        st = lbad::hip_status(lbad::launch_ids_index_build(c->d_ids, c->count, c->d_ids_slot_ids, c->d_ids_slot_index, slots, stream),
                              "id index", __LINE__);
        c->ids_slots = slots;
        c->ids_index_valid = st == noErr;
    }
    if (st == noErr)
        st = lbad::hip_status(lbad::launch_keys_from_ids(static_cast<const unsigned long long*>(inIds), inCount, inIndexBase, c->count,
                                                         c->d_ids_slot_ids, c->d_ids_slot_index, c->ids_slots,
                                                         static_cast<unsigned long long*>(outKeys), stream), "keys from ids", __LINE__);
    const OSStatus rec = c->ids_ev.record(stream);
    return st != noErr ? st : rec;
    LBAD_GUARD_END
}

}  // extern "C"
