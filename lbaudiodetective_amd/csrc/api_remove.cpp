// api_remove.cpp -- entries taken out of a corpus: the host side of k_remove.hip.
// The entries a call names go, the others keep their order and close up; afterwards the corpus is what a fresh one of the same
// capacities would be after appending the kept entries in order.  A removal is a synchronous maintenance call: it waits for
// everything the corpus has in flight, moves the planes or records through the bounce buffer in ascending chunks, and returns
// when the device is done and count, offsets and histogram on the host are up to date.
#include "internal.hpp"

#include <algorithm>

namespace lbad {
namespace {

constexpr uint64_t kRemoveScratchDefault = 256ull << 20;
constexpr uint32_t kGone = 0xFFFFFFFFu;

// items (entries of a uniform corpus, records of a ragged one) the bounce buffer may hold under the corpus' limit: a whole
// number of tiles, 0 when the limit holds no tile
uint64_t chunk_items(const LBAudioDetectiveCorpus* c) {
    const uint64_t limit = c->remove_scratch_limit ? c->remove_scratch_limit : kRemoveScratchDefault;
    const uint64_t item_bytes = c->ragged ? 32u : (uint64_t)c->n_planes * sizeof(uint4);
    const uint64_t tile = remove_tile_entries();
    return limit / item_bytes / tile * tile;
}

// Everything that may still read or write the corpus' planes, records, offsets or plan is done, on whatever stream it ran;
// the latest append is awaited on the device
OSStatus await_in_flight(LBAudioDetectiveCorpus* c, hipStream_t stream) {
    OSStatus st = c->plan_built.wait();
    for (const Event& e : c->query_ev)
        if (st == noErr) st = e.wait();
    if (st == noErr) st = c->topk_ev.wait();
    if (st == noErr) st = c->align_ev.wait();
    if (st == noErr) st = c->pq_ev.wait();
    if (st == noErr) st = c->join_ev.wait();
    if (st == noErr) st = c->gather_ev.wait();
    if (st == noErr) st = c->ids_ev.wait();
    if (st != noErr) return st;
    if (c->stream) LBAD_HIP(hipStreamSynchronize(c->stream));        // the polled top-1 query's own stream
    if (c->append_event.ev) LBAD_HIP(hipStreamWaitEvent(stream, c->append_event, 0));
    return noErr;
}

// uniform: the planes of the entries from `first` on, chunk by chunk.  host: the index block's head and tile offsets
OSStatus move_planes(LBAudioDetectiveCorpus* c, const RemoveIndex& ix, const uint32_t* tile_off, uint64_t first, uint64_t kept,
                     uint64_t chunk, hipStream_t stream) {
    const uint64_t tile = remove_tile_entries();
    const uint64_t from = first / tile * tile;
    const uint64_t need = (c->count - from + tile - 1) / tile * tile;
    const uint64_t slots = need < chunk ? need : chunk;
    OSStatus st = c->d_remove_bounce.reserve((size_t)slots * c->n_planes);
    if (st != noErr) return st;
    uint64_t e0 = first, base = first;                       // (every entry below `first` stays: it is its own new index)
    while (e0 < c->count && base < kept) {                   // (base == kept: nothing above e0 is kept)
        const uint64_t e1 = std::min<uint64_t>(c->count, e0 / tile * tile + slots);
        const uint64_t k = tile_off[e1 == c->count ? ix.tiles : e1 / tile] - base;
        if (k > e1 - e0) return kLBAudioDetectiveDeviceError;     // (a chunk keeps at most its own entries)
        LBAD_HIP(launch_remove_gather_planes(c->d_planes, c->capacity, c->n_planes, ix.map, e0, e1, (uint32_t)base, c->d_remove_bounce,
                                             slots, stream));
        LBAD_HIP(launch_remove_scatter(c->d_remove_bounce, slots, c->n_planes, c->d_planes, c->capacity, base, k, stream));
        base += k;
        e0 = e1;
    }
    return noErr;
}

// ragged: the records of the entries from `first` on.  map: the call's map on the host; new_off: the kept entries' record
// positions (kept + 1 values)
OSStatus move_records(LBAudioDetectiveCorpus* c, const RemoveIndex& ix, const uint32_t* map, const std::vector<uint32_t>& new_off,
                      uint64_t first, uint64_t kept, uint64_t chunk, hipStream_t stream) {
    const uint64_t tile = remove_tile_entries();
    const std::vector<uint32_t>& old_off = c->h_off;
    const uint64_t r_first = old_off[first], new_pos = new_off[kept];
    OSStatus st = c->d_remove_off.reserve((size_t)c->capacity + 1);
    if (st != noErr) return st;
    // the new offsets beside the old ones: the gather launches read both.  Entries below `first` keep theirs.
    LBAD_HIP(hipMemcpyAsync(c->d_remove_off + first, new_off.data() + first, (kept + 1 - first) * sizeof(uint32_t), hipMemcpyHostToDevice,
                            stream));
    if (kept > first) {
        const uint64_t need = (c->n_pos - r_first + tile - 1) / tile * tile;
        const uint64_t slots = need < chunk ? need : chunk;
        st = c->d_remove_bounce.reserve((size_t)slots * 2);
        if (st != noErr) return st;
        // new position of the first kept record at or behind record r
        uint64_t e = first;                                   // (r only grows: so does the entry that holds it)
        auto new_position = [&](uint64_t r) -> uint64_t {
            if (r >= c->n_pos) return new_pos;
            while (old_off[e + 1] <= r) ++e;
            if (map[e] != kGone) return (uint64_t)new_off[map[e]] + (r - old_off[e]);
            uint64_t n = e + 1;
            while (n < c->count && map[n] == kGone) ++n;
            return n < c->count ? new_off[map[n]] : new_pos;
        };
        uint64_t r0 = r_first, base = r_first;
        while (r0 < c->n_pos && base < new_pos) {
            const uint64_t r1 = std::min<uint64_t>(c->n_pos, r0 + slots);
            const uint64_t k = new_position(r1) - base;
            if (k > r1 - r0) return kLBAudioDetectiveDeviceError;     // (a chunk keeps at most its own records)
            LBAD_HIP(launch_remove_gather_records(c->d_recs, c->d_off, c->d_remove_off, ix.map, c->count, r0, r1, base, c->d_remove_bounce,
                                                  slots, stream));
            LBAD_HIP(launch_remove_scatter(c->d_remove_bounce, 0, 1, c->d_recs, 0, 2 * base, 2 * k, stream));
            base += k;
            r0 = r1;
        }
    }
    // behind the last gather: the offsets, and kRecordSlack zero records behind the new end (inside the block: it has that many
    // behind its capacity)
    LBAD_HIP(hipMemcpyAsync(c->d_off + first, c->d_remove_off + first, (kept + 1 - first) * sizeof(uint32_t), hipMemcpyDeviceToDevice,
                            stream));
    LBAD_HIP(hipMemsetAsync(c->d_recs + 2 * new_pos, 0, (size_t)kRecordSlack * 32, stream));
    return noErr;
}

// d_list: n_list keys or indices ON THE DEVICE.  out_map_host / out_map_dev (either may be null): one word per old entry
OSStatus remove_impl(LBAudioDetectiveCorpus* c, const unsigned long long* d_list, uint64_t n_list, bool keys, uint64_t index_base,
                     uint32_t* out_map_host, uint32_t* out_map_dev, UInt64* out_removed, hipStream_t stream) {
    *out_removed = 0;
    const uint64_t count = c->count;
    if (count == 0) return noErr;
    const uint64_t chunk = chunk_items(c);
    if (chunk == 0) return kLBAudioDetectiveArgumentInvalid;          // the limit holds no tile
    if (n_list == 0) {                                                // nothing goes: the identity map, nothing is launched
        if (out_map_host)
            for (uint64_t e = 0; e < count; ++e) out_map_host[e] = (uint32_t)e;
        if (!out_map_dev) return noErr;
    }
    OSStatus st = await_in_flight(c, stream);
    if (st != noErr) return st;
    RemoveIndex ix = remove_index_layout(nullptr, count);
    st = c->d_remove_index.reserve((size_t)ix.words);
    if (st != noErr) return st;
    ix = remove_index_layout(c->d_remove_index, count);
    LBAD_HIP(launch_remove_index(d_list, n_list, keys, index_base, count, ix, stream));
    // ONE read-back: kept, first removed, the tile offsets -- and the map where the host needs it (its caller wants it, or the
    // corpus is ragged: the host's offsets and histogram follow from it)
    const bool want_map = out_map_host != nullptr || c->ragged;
    std::vector<uint32_t> host((size_t)(want_map ? ix.map_words : ix.head_words));
    LBAD_HIP(hipMemcpyAsync(host.data(), ix.head, host.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    LBAD_HIP(hipStreamSynchronize(stream));
    const uint64_t kept = host[0], first = host[1];
    const uint32_t* tile_off = host.data() + 4;
    const uint32_t* map = want_map ? host.data() + ix.map_at : nullptr;
    if (kept > count || (kept < count && first >= count)) return kLBAudioDetectiveDeviceError;
    if (out_map_host) std::copy(map, map + count, out_map_host);
    if (out_map_dev) LBAD_HIP(hipMemcpyAsync(out_map_dev, ix.map, count * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream));
    if (kept == count) {                                              // the list named nothing valid
        LBAD_HIP(hipStreamSynchronize(stream));
        return noErr;
    }
    if (c->d_ids) {                                                   // the ids' scratch, before anything moves
        st = c->d_ids_scratch.reserve((size_t)(count - first));
        if (st != noErr) return st;
    }
    if (c->ragged) {
        std::vector<uint32_t> new_off((size_t)kept + 1);
        std::map<uint32_t, uint64_t> hist;
        uint32_t longest = 0;
        new_off[0] = 0;
        for (uint64_t e = 0; e < count; ++e) {
            if (map[e] == kGone) continue;
            if (map[e] >= kept) return kLBAudioDetectiveDeviceError;
            const uint32_t len = c->h_off[e + 1] - c->h_off[e];
            new_off[(size_t)map[e] + 1] = new_off[map[e]] + len;
            ++hist[len];
            longest = len > longest ? len : longest;
        }
        st = move_records(c, ix, map, new_off, first, kept, chunk, stream);
        const OSStatus done = hip_status(hipStreamSynchronize(stream), "removal", __LINE__);   // (new_off is read by a copy until then)
        if (st != noErr || done != noErr) return st != noErr ? st : done;
        c->n_pos = new_off[kept];
        c->h_off.swap(new_off);
        c->len_hist.swap(hist);
        c->ne_max = longest;
        c->plan_nq = 0;                                               // the scan's plan is of the old entries
        c->plan_count = 0;
    } else {
        if (kept > first) st = move_planes(c, ix, tile_off, first, kept, chunk, stream);
        if (st != noErr) {
            (void)hipStreamSynchronize(stream);
            return st;
        }
    }
    // the ids of a corpus that has them go with their entries, by the same device map (a corpus without ids: nothing happens)
    st = ids_compact(c, ix.map, first, kept, stream);
    if (st != noErr) {
        (void)hipStreamSynchronize(stream);
        return st;
    }
    c->count = kept;
    *out_removed = count - kept;
    // every device-side waiter waits for the append event: the removal leaves it behind itself, and the polled top-1 path
    // learns that the entries changed, as after an append
    st = c->append_event.create();
    if (st == noErr) st = c->append_event.record(stream);
    if (st == noErr && c->stream) st = hip_status(hipStreamWaitEvent(c->stream, c->append_event, 0), "removal", __LINE__);
    c->appended = true;
    const OSStatus done = hip_status(hipStreamSynchronize(stream), "removal", __LINE__);
    return st != noErr ? st : done;
}

}  // namespace
}  // namespace lbad

extern "C" {

OSStatus LBAudioDetectiveCorpusRemoveIndices(LBAudioDetectiveCorpusRef inCorpus, const UInt64* inIndices, UInt64 inCount,
                                             UInt32* outNewIndices, UInt64* outRemoved) {
    LBAD_GUARD_BEGIN
    if (!inCorpus || !outRemoved || (inCount && !inIndices)) return kLBAudioDetectiveArgumentInvalid;
    *outRemoved = 0;                                    // (also where the call is refused from here on)
    if (!lbad::device_ready()) return kLBAudioDetectiveDeviceUnavailable;
    LBAudioDetectiveCorpus* c = inCorpus;
    for (UInt64 i = 0; i < inCount; ++i)
        if (inIndices[i] >= c->count) return kLBAudioDetectiveArgumentInvalid;      // nothing has changed
    if (inCount && c->count) {
        OSStatus st = c->d_remove_list.reserve((size_t)inCount);
        if (st != noErr) return st;
        LBAD_HIP(hipMemcpy(c->d_remove_list, inIndices, (size_t)inCount * sizeof(UInt64), hipMemcpyHostToDevice));
    }
    return lbad::remove_impl(c, c->d_remove_list, inCount, false, 0, outNewIndices, nullptr, outRemoved, nullptr);
    LBAD_GUARD_END
}

OSStatus LBAudioDetectiveCorpusRemoveKeysDevice(LBAudioDetectiveCorpusRef inCorpus, const void* inKeys, UInt64 inCount, UInt64 inIndexBase,
                                                void* outNewIndices, UInt64* outRemoved, void* inStream) {
    LBAD_GUARD_BEGIN
    if (!inCorpus || !outRemoved || (inCount && !inKeys) || inIndexBase > 0x100000000ull) return kLBAudioDetectiveArgumentInvalid;
    *outRemoved = 0;
    if (!lbad::device_ready()) return kLBAudioDetectiveDeviceUnavailable;
    if (inIndexBase + inCorpus->count > 0x100000000ull) return kLBAudioDetectiveArgumentInvalid;
    return lbad::remove_impl(inCorpus, static_cast<const unsigned long long*>(inKeys), inCount, true, inIndexBase, nullptr,
                             static_cast<uint32_t*>(outNewIndices), outRemoved, static_cast<hipStream_t>(inStream));
    LBAD_GUARD_END
}

OSStatus LBAudioDetectiveCorpusSetRemoveScratchLimit(LBAudioDetectiveCorpusRef inCorpus, UInt64 inBytes) {
    if (!inCorpus) return kLBAudioDetectiveArgumentInvalid;
    inCorpus->remove_scratch_limit = inBytes;
    // a block above the new limit goes (a removal is synchronous: nothing uses it now)
    const uint64_t limit = inBytes ? inBytes : lbad::kRemoveScratchDefault;
    if (inCorpus->d_remove_bounce.capacity() * sizeof(uint4) > limit) inCorpus->d_remove_bounce.reset();
    return noErr;
}

}  // extern "C"
