// api_corpus.cpp -- device-resident reference-fingerprint corpus and its top-1 query.
// Scales the best-match loop of LBAudioDetectiveTests/LBAudioDetectiveTests.m:57-91 (one original
// against N candidates, strict '<', first maximum wins) to an HBM-resident database.
#include "internal.hpp"

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <functional>

namespace lbad {
namespace {

// ragged corpus: the sliding scan (sliding.cpp decides and launches; any query length, any entry lengths).  A launch's query blocks travel
// through a ring of kQuerySlots pinned + device slots, one event per slot: a call waits only for the scan that used
// its slot kQuerySlots launches ago (long done), not for the stream -- back-to-back queries leave no gap on the GPU.
// Round 5: a single query of up to kSlideQueryArgSubs sub-fingerprints travels in the kernel's argument segment (no copy
// node), the result words are cleared by the previous scan's last workgroup (no memset node), and up to four queries of
// ONE length share a pass over the corpus (eight in the systolic scan of short queries).
constexpr uint32_t kQuerySlots = 8;
constexpr uint32_t kScanOutWords = 16;      // per slot: 8 running maxima, the ticket, padding

// every scan that used the ring (or, uniform corpus, the staging pair) is done
OSStatus wait_scans(const LBAudioDetectiveCorpus* c) {
    for (const Event& e : c->query_ev) {
        OSStatus st = e.wait();
        if (st != noErr) return st;
    }
    return noErr;
}

SlideCorpusStats ragged_stats(const LBAudioDetectiveCorpus* c) {
    SlideCorpusStats s;
    s.len_hist = &c->len_hist; s.n_pos = c->n_pos; s.ne_max = c->ne_max; s.variant = c->variant; s.subfp_len = c->subfp_len;
    return s;
}

// ONE launch, as `choice` (sliding_choose) has decided it: choice.n_take queries of nq sub-fingerprints, their keys to
// keys + pos[i].  Their blocks (sliding_block_words(nq) words each, one after the other) come either from the host -- h_blocks:
// staged through the launch's ring slot, or sent in the kernel's arguments -- or are on the device already -- d_blocks: what a
// builder of k_query.hip wrote; nothing is staged then.  Either way the launch owns a ring slot's result words and leaves its
// event behind.  What belongs to the corpus is managed here: the ring, the result words, the plan cache and the events.
OSStatus launch_ragged_blocks(LBAudioDetectiveCorpus* c, uint32_t nq, const SlideChoice& choice, const uint32_t* h_blocks,
                              const uint32_t* d_blocks, const uint32_t* pos, uint32_t range, uint64_t index_base, float* d_scores,
                              unsigned long long* keys, hipStream_t stream) {
    if (choice.n_take == 0) return kLBAudioDetectiveArgumentInvalid;
    const size_t all_words = sliding_block_words(nq) * choice.n_take;
    const size_t slot_words = (all_words + 63) & ~(size_t)63;
    if (h_blocks && c->query_slot_words < slot_words) {   // (re)size the ring: everything that used it must be done
        OSStatus st = wait_scans(c);
        if (st != noErr) return st;
        c->query_slot_words = 0;                          // (a failed resize leaves no ring, not a ring of the old size)
        st = c->query.reserve(slot_words * kQuerySlots);
        if (st != noErr) return st;
        c->query_slot_words = slot_words;
    }
    if (!c->d_scan_out) {
        OSStatus st = c->d_scan_out.reserve((size_t)kQuerySlots * kScanOutWords);
        if (st != noErr) return st;
        c->scan_out_dirty = true;
    }
    if (c->scan_out_dirty) {
        // the result words must be zero between scans: the scans themselves leave them so, but a launch that failed may not
        // have -- nothing is trusted after one: everything that may still touch the words finishes, then they are cleared
        (void)wait_scans(c);
        // on the scan's own stream and awaited: the scan may run on a non-blocking stream, which a null-stream memset does
        // not order itself against (round-5 advice)
        LBAD_HIP(hipMemsetAsync(c->d_scan_out, 0, (size_t)kQuerySlots * kScanOutWords * 8, stream));
        LBAD_HIP(hipStreamSynchronize(stream));
        c->scan_out_dirty = false;
    }
    const uint32_t slot = (uint32_t)(c->query_seq++ % kQuerySlots);
    OSStatus st = c->query_ev[slot].wait_or_create();
    if (st != noErr) return st;
    SlideScan scan;
    scan.d_queries = d_blocks;
    if (h_blocks) {
        uint32_t* h_slot = c->query.host + (size_t)slot * c->query_slot_words;
        uint32_t* d_slot = c->query.dev + (size_t)slot * c->query_slot_words;
        std::memcpy(h_slot, h_blocks, all_words * sizeof(uint32_t));
        if (!choice.q_in_args) LBAD_HIP(hipMemcpyAsync(d_slot, h_slot, all_words * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
        scan.d_queries = choice.q_in_args ? nullptr : d_slot;
        scan.h_query = choice.q_in_args ? h_slot : nullptr;
    }
    if (d_scores) LBAD_HIP(hipMemsetAsync(d_scores, 0, c->count * sizeof(float), stream));
    // the plan of this query length: kept while the length and the entries stay (queries of one length are the rule).  Only
    // the task kernel reads it: a batch of short queries on compare_short_multi_kernel leaves the plan alone
    if (choice.reads_plan && (c->plan_nq != nq || c->plan_count != c->count || c->plan_grid != choice.shape.grid || c->plan_bmin != choice.b_min)) {
        // scans on other streams may still read the old plan: every scan leaves its slot's event behind, and a slot is
        // reused only after its event -- the eight events cover everything that can still be running
        st = wait_scans(c);
        if (st == noErr) st = c->plan_built.create();
        if (st != noErr) return st;
        c->plan_nq = 0;
        LBAD_HIP(launch_sliding_plan(c->d_off, c->count, nq, choice.b_min, choice.shape, c->d_plan, stream));
        st = c->plan_built.record(stream);
        if (st != noErr) return st;
        c->plan_stream = stream;
        c->plan_nq = nq; c->plan_count = c->count; c->plan_grid = choice.shape.grid; c->plan_bmin = choice.b_min;
    } else if (c->plan_built && c->plan_stream != stream) {
        LBAD_HIP(hipStreamWaitEvent(stream, c->plan_built, 0));
    }
    scan.d_acc = c->d_scan_out + (size_t)slot * kScanOutWords;
    scan.d_ticket = reinterpret_cast<unsigned int*>(scan.d_acc + 8);
    scan.d_keys = keys;
    for (uint32_t i = 0; i < 8; ++i) scan.key_pos[i] = i < choice.n_take ? pos[i] : 0u;
    SlideCorpus src;
    src.recs = c->d_recs; src.n_pos = c->n_pos; src.off = c->d_off; src.n_entries = c->count;
    src.zero_rec = (uint32_t)(c->rec_capacity + kRecordSlack / 2); src.subfp_len = c->subfp_len; src.plan = c->d_plan;
    SlideCall call;
    call.n_query = nq; call.range = range; call.index_base = index_base;
    call.d_score_bits = reinterpret_cast<unsigned int*>(d_scores);
    call.bound_pruning = c->bound_pruning; call.prune_from = c->prune_from; call.stream = stream;
    {
        const hipError_t launched = launch_compare_sliding(src, choice, scan, call);
        if (launched != hipSuccess) c->scan_out_dirty = true;
        LBAD_HIP(launched);
    }
    // behind the SCAN, not just the copy: the slot's device half and its result words are the kernel's, and the launch
    // that reuses the slot eight launches later may arrive on another stream
    return c->query_ev[slot].record(stream);
}

// Where the blocks of one launch come from: the g queries idx[0..g) (positions in the caller's order, all of `per`
// sub-fingerprints) as host blocks to stage or as blocks that are on the device already -- exactly one of the two is set
using RaggedBlocks = std::function<void(const uint32_t* idx, uint32_t g, uint32_t per, const uint32_t*& h_blocks, const uint32_t*& d_blocks)>;

// n queries against the ragged corpus, query i of lengths[i] sub-fingerprints, key i to keys[i] (d_scores: n == 1).  Queries of
// one length share launches: grouped by length, chunked by what sliding_choose lets a launch take; the keys are zeroed once up
// front when some launch of the call maxes its keys in place.
OSStatus run_ragged(LBAudioDetectiveCorpus* c, const std::vector<uint32_t>& lengths, bool host_blocks, const RaggedBlocks& blocks,
                    uint32_t range, uint64_t index_base, float* d_scores, unsigned long long* keys, hipStream_t stream) {
    const uint32_t n = (uint32_t)lengths.size();
    if (c->count == 0) {                                   // nothing to scan: every key is "no match"
        LBAD_HIP(hipMemsetAsync(keys, 0, (size_t)n * sizeof(unsigned long long), stream));
        return noErr;
    }
    std::vector<uint32_t> order(n);
    for (uint32_t i = 0; i < n; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return lengths[x] < lengths[y]; });
    struct Launch {
        uint32_t at;
        SlideChoice choice;
    };
    std::vector<Launch> launches;
    const SlideCorpusStats stats = ragged_stats(c);
    const uint32_t cus = (uint32_t)device_cu_count();
    bool zero_keys = false;
    for (uint32_t at = 0; at < n;) {
        SlideGroup group;
        group.n_query = lengths[order[at]]; group.range = range; group.scores = d_scores != nullptr; group.host_blocks = host_blocks;
        while (at + group.n_left < n && lengths[order[at + group.n_left]] == group.n_query) ++group.n_left;
        while (group.n_left) {
            const SlideChoice choice = sliding_choose(stats, group, cus);
            if (choice.n_take == 0) return kLBAudioDetectiveArgumentInvalid;
            zero_keys = zero_keys || choice.maxes_keys;
            launches.push_back({at, choice});
            at += choice.n_take;
            group.n_left -= choice.n_take;
        }
    }
    if (zero_keys) LBAD_HIP(hipMemsetAsync(keys, 0, (size_t)n * sizeof(unsigned long long), stream));
    for (const Launch& l : launches) {
        const uint32_t* h_blocks = nullptr;
        const uint32_t* d_blocks = nullptr;
        blocks(order.data() + l.at, l.choice.n_take, lengths[order[l.at]], h_blocks, d_blocks);
        OSStatus st = launch_ragged_blocks(c, lengths[order[l.at]], l.choice, h_blocks, d_blocks, order.data() + l.at, range, index_base,
                                           d_scores, keys, stream);
        if (st != noErr) return st;
    }
    return noErr;
}

// n queries against the ragged corpus, key i to keys[i]
OSStatus run_queries_ragged(LBAudioDetectiveCorpus* c, const LBAudioDetectiveFingerprintRef* qs, uint32_t n, uint32_t range,
                            uint64_t index_base, float* d_scores, unsigned long long* keys, hipStream_t stream) {
    std::vector<uint32_t> lengths(n), block, all;
    for (uint32_t i = 0; i < n; ++i) lengths[i] = qs[i]->count;
    auto from_handles = [&](const uint32_t* idx, uint32_t g, uint32_t per, const uint32_t*& h, const uint32_t*&) {
        all.clear();
        for (uint32_t i = 0; i < g; ++i) {
            build_sliding_query(qs[idx[i]]->data.data(), per, c->subfp_len, range, block);
            all.insert(all.end(), block.begin(), block.end());
        }
        h = all.data();
    };
    return run_ragged(c, lengths, true, from_handles, range, index_base, d_scores, keys, stream);
}

OSStatus run_query_ragged(LBAudioDetectiveCorpus* c, const LBAudioDetectiveFingerprint* q, uint32_t range,
                          uint64_t index_base, float* d_scores, unsigned long long* key_dst, hipStream_t stream) {
    LBAudioDetectiveFingerprintRef one = const_cast<LBAudioDetectiveFingerprint*>(q);
    return run_queries_ragged(c, &one, 1, range, index_base, d_scores, key_dst, stream);
}

// stage the query on the device and launch the scan; key_dst is a device pointer
OSStatus run_query_impl(LBAudioDetectiveCorpus* c, const LBAudioDetectiveFingerprint* q, uint32_t range,
                   uint64_t index_base, float* d_scores, unsigned long long* key_dst, hipStream_t stream) {
    if (!c || !q || !key_dst) return kLBAudioDetectiveArgumentInvalid;
    if (q->length != c->subfp_len || q->count == 0) return kLBAudioDetectiveArgumentInvalid;
    if (!c->ragged && (size_t)q->count * kPackedWords * 4 > 48 * 1024) return kLBAudioDetectiveArgumentInvalid;
    if (range == 0) range = c->subfp_len;  // LBAudioDetective.m:443-445
    if (c->ragged) return run_query_ragged(c, q, range, index_base, d_scores, key_dst, stream);
    std::vector<uint32_t> slots;
    pack_fingerprint(q, slots);
    bool fast = planes_fast_supported(c->subfp_len, c->n_sub, q->count);
    if (c->variant == 1) fast = false;
    if (c->variant == 2 && !fast) return kLBAudioDetectiveArgumentInvalid;
    LBAD_HIP(hipMemsetAsync(key_dst, 0, sizeof(unsigned long long), stream));
    if (fast) {
        // the specialised scan takes its 300-byte query block as a kernel argument: nothing to stage
        std::vector<uint32_t> block;
        build_plane_query(slots.data(), c->n_sub, range, block);
        LBAD_HIP(launch_compare_planes_fast(c->d_planes, c->capacity, c->count, c->n_sub, block.data(), index_base,
                                            d_scores, key_dst, stream));
        return noErr;
    }
    // the staging block and its device copy are reused (and regrown) by every query: wait for the previous one's SCAN
    // (whatever stream it ran on; slot 0 of the ragged ring's events serves this path, a corpus is either ragged or not)
    OSStatus st = c->query_ev[0].wait_or_create();
    if (st == noErr) st = c->query.reserve(slots.size());
    if (st != noErr) return st;
    std::memcpy(c->query.host, slots.data(), slots.size() * sizeof(uint32_t));
    LBAD_HIP(hipMemcpyAsync(c->query.dev, c->query.host, slots.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    LBAD_HIP(launch_compare_planes_generic(c->d_planes, c->capacity, c->count, c->n_sub, c->subfp_len, c->query.dev,
                                           q->count, range, index_base, d_scores, key_dst, stream));
    return c->query_ev[0].record(stream);
}

// LBAudioDetectiveCorpusQuery on the specialised scan: one launch, the result arrives in pinned memory
OSStatus query_fast_impl(LBAudioDetectiveCorpus* c, const LBAudioDetectiveFingerprint* q, uint32_t range, unsigned long long* key) {
    if (!c->h_out) {
        // built in locals and committed only when everything exists: a failure leaves the corpus as it was
        DeviceBuffer<unsigned long long> d_fast;
        PinnedBuffer<unsigned long long> h_out;
        unsigned long long* h_out_dev = nullptr;
        OSStatus st = c->stream ? noErr : kLBAudioDetectiveDeviceError;     // created with the corpus
        if (st == noErr) st = d_fast.reserve(kScanSlots + 1);
        // on the query's own stream: hipMemset returns before the fill is done and the null stream does not order a
        // non-blocking one, so a fill there could land among the first scan's ticket adds (no last workgroup, no answer)
        if (st == noErr) st = hip_status(hipMemsetAsync(d_fast, 0, (kScanSlots + 1) * sizeof(unsigned long long), c->stream), "memset", __LINE__);
        if (st == noErr) st = h_out.reserve(2, hipHostMallocMapped | hipHostMallocCoherent);
        if (st == noErr) {
            h_out[0] = h_out[1] = 0;
            st = hip_status(hipHostGetDevicePointer(reinterpret_cast<void**>(&h_out_dev), h_out, 0), "device pointer", __LINE__);
        }
        if (st != noErr || !h_out_dev) return st != noErr ? st : kLBAudioDetectiveDeviceError;
        c->d_ticket = reinterpret_cast<unsigned int*>(d_fast + kScanSlots);
        c->d_fast_key = std::move(d_fast);
        c->h_out_dev = h_out_dev;
        c->h_out = std::move(h_out);
    }
    if (range == 0) range = c->subfp_len;
    std::vector<uint32_t> slots, block;
    pack_fingerprint(q, slots);
    build_plane_query(slots.data(), c->n_sub, range, block);
    const unsigned long long seq = ++c->seq;
    LBAD_HIP(launch_compare_planes_fast(c->d_planes, c->capacity, c->count, c->n_sub, block.data(), 0, nullptr,
                                        c->d_fast_key, c->stream, c->d_ticket, c->h_out_dev, seq));
    volatile unsigned long long* out = c->h_out.get();
    const auto t0 = std::chrono::steady_clock::now();
    for (uint64_t spins = 1; out[1] != seq; ++spins) {
        if ((spins & 0xFFFFF) == 0) {                       // every million polls: is the stream still alive?
            const hipError_t e = hipStreamQuery(c->stream);
            if (e == hipSuccess) {                          // the kernel is done: its words are on their way or lost
                LBAD_HIP(hipStreamSynchronize(c->stream));
                if (out[1] != seq) return kLBAudioDetectiveDeviceError;
            } else if (e != hipErrorNotReady) {
                return hip_status(e, "corpus query", __LINE__);
            } else if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(30)) {
                fprintf(stderr, "lbaudiodetective: corpus scan not finished after 30 s\n");   // a hung kernel must not hang the host
                return kLBAudioDetectiveDeviceError;
            }
        }
#if defined(__x86_64__)
        __builtin_ia32_pause();
#endif
    }
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    *key = out[0];
    return noErr;
}

OSStatus query_fast(LBAudioDetectiveCorpus* c, const LBAudioDetectiveFingerprint* q, uint32_t range, unsigned long long* key) {
    LBAD_GUARD_BEGIN
    return query_fast_impl(c, q, range, key);
    LBAD_GUARD_END
}

}  // namespace

// ---- the scans the top-K, threshold and packed queries run (api_select.cpp; internal.hpp declares them) ----
// n queries of `per` sub-fingerprints whose blocks a builder wrote to d_blocks, key i to keys[i] (d_scores: n == 1)
OSStatus run_built_ragged(LBAudioDetectiveCorpus* c, const uint32_t* d_blocks, uint32_t n, uint32_t per, uint32_t range,
                          uint64_t index_base, float* d_scores, unsigned long long* keys, hipStream_t stream) {
    // (one length: the order is the caller's, a launch's blocks lie one after the other)
    auto built = [&](const uint32_t* idx, uint32_t, uint32_t, const uint32_t*&, const uint32_t*& d) {
        d = d_blocks + (size_t)idx[0] * sliding_block_words(per);
    };
    return run_ragged(c, std::vector<uint32_t>(n, per), false, built, range, index_base, d_scores, keys, stream);
}

// (host allocations -- the packed query, its constant block -- can fail: nothing may unwind through the C boundary)
OSStatus run_query(LBAudioDetectiveCorpus* c, const LBAudioDetectiveFingerprint* q, uint32_t range, uint64_t index_base,
                   float* d_scores, unsigned long long* key_dst, hipStream_t stream) {
    LBAD_GUARD_BEGIN
    return run_query_impl(c, q, range, index_base, d_scores, key_dst, stream);
    LBAD_GUARD_END
}

}  // namespace lbad

extern "C" {

LBAudioDetectiveCorpusRef LBAudioDetectiveCorpusNew(UInt32 inSubfingerprintLength, UInt32 inSubfingerprintsPerEntry,
                                                    UInt64 inCapacity) {
    if (inCapacity == 0 || inCapacity > 0xFFFFFFFFull) return NULL;  // the key carries a 32-bit index
    if (!lbad::planes_supported(inSubfingerprintLength, inSubfingerprintsPerEntry)) return NULL;
    if (!lbad::device_ready()) {
        fprintf(stderr, "lbaudiodetective: no HIP device, cannot create a corpus\n");
        return NULL;
    }
    LBAudioDetectiveCorpus* c = new LBAudioDetectiveCorpus();
    c->subfp_len = inSubfingerprintLength;
    c->n_sub = inSubfingerprintsPerEntry;
    c->capacity = inCapacity;
    c->n_planes = lbad::planes_per_entry(inSubfingerprintLength, inSubfingerprintsPerEntry);
    // the polled query's own stream exists from the start, so that every append can order it behind itself
    if (c->d_planes.reserve((size_t)c->n_planes * inCapacity) != noErr || c->d_key.reserve(2) != noErr ||
        lbad::hip_status(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking), "stream", __LINE__) != noErr ||
        c->d_shard_keys.reserve(LBAD_SHARD_KEYS) != noErr || c->h_shard_keys.reserve(LBAD_SHARD_KEYS) != noErr) {
        LBAudioDetectiveCorpusDispose(c);
        return NULL;
    }
    return c;
}

LBAudioDetectiveCorpusRef LBAudioDetectiveCorpusNewRagged(UInt32 inSubfingerprintLength, UInt64 inEntryCapacity,
                                                          UInt64 inSubfingerprintCapacity) {
    if (inEntryCapacity == 0 || inEntryCapacity > lbad::kMaxRaggedEntries) return NULL;   // the key carries a 32-bit index (and the scan's claim cursor a little slack)
    if (inSubfingerprintCapacity < inEntryCapacity || inSubfingerprintCapacity > lbad::kMaxRaggedRecords) return NULL;
    if (!lbad::sliding_supported(inSubfingerprintLength)) return NULL;
    if (!lbad::device_ready()) {
        fprintf(stderr, "lbaudiodetective: no HIP device, cannot create a corpus\n");
        return NULL;
    }
    LBAudioDetectiveCorpus* c = new (std::nothrow) LBAudioDetectiveCorpus();
    if (!c) return NULL;
    c->ragged = true;
    c->subfp_len = inSubfingerprintLength;
    c->capacity = inEntryCapacity;
    c->rec_capacity = inSubfingerprintCapacity;
    try {
        c->h_off.assign(1, 0u);
    } catch (const std::bad_alloc&) {
        delete c;
        return NULL;
    }
    // kRecordSlack zero records behind the capacity: the scan reads up to three records past an entry's end (offsets
    // that do not exist, never used) and takes its all-zero record from there
    if (c->d_recs.reserve(2 * ((size_t)inSubfingerprintCapacity + lbad::kRecordSlack)) != noErr ||
        lbad::hip_status(hipMemset(c->d_recs + 2 * (size_t)inSubfingerprintCapacity, 0, (size_t)lbad::kRecordSlack * 32), "corpus slack", __LINE__) != noErr ||
        c->d_off.reserve((size_t)inEntryCapacity + 1) != noErr ||
        lbad::hip_status(hipMemset(c->d_off, 0, 4), "offsets", __LINE__) != noErr ||
        c->d_key.reserve(2) != noErr || c->d_plan.reserve(lbad::sliding_plan_words(inEntryCapacity)) != noErr ||
        c->d_shard_keys.reserve(LBAD_SHARD_KEYS) != noErr || c->h_shard_keys.reserve(LBAD_SHARD_KEYS) != noErr) {
        LBAudioDetectiveCorpusDispose(c);
        return NULL;
    }
    return c;
}

UInt64 LBAudioDetectiveCorpusGetSubfingerprintTotal(LBAudioDetectiveCorpusRef c) {
    if (!c) return 0;
    return c->ragged ? c->n_pos : c->count * c->n_sub;
}

OSStatus LBAudioDetectiveCorpusAppendRaggedPackedDevice(LBAudioDetectiveCorpusRef c, const void* inPacked,
                                                        const UInt32* inCounts, UInt64 inNumberOfEntries, void* inStream) {
    if (!c || !c->ragged || (inNumberOfEntries && (!inPacked || !inCounts))) return kLBAudioDetectiveArgumentInvalid;
    if (inNumberOfEntries == 0) return noErr;
    if (c->count + inNumberOfEntries > c->capacity) return kLBAudioDetectiveArgumentInvalid;
    LBAD_GUARD_BEGIN
    uint64_t total = 0;
    uint32_t longest = c->ne_max;
    for (UInt64 e = 0; e < inNumberOfEntries; ++e) {
        if (inCounts[e] == 0) return kLBAudioDetectiveArgumentInvalid;   // an entry has at least one sub-fingerprint
        total += inCounts[e];
        if (inCounts[e] > longest) longest = inCounts[e];
    }
    if (c->n_pos + total > c->rec_capacity) return kLBAudioDetectiveArgumentInvalid;
    const size_t at = c->h_off.size() - 1;            // == c->count
    c->h_off.resize(at + inNumberOfEntries + 1);
    for (UInt64 e = 0; e < inNumberOfEntries; ++e) c->h_off[at + e + 1] = c->h_off[at + e] + inCounts[e];
    hipStream_t stream = static_cast<hipStream_t>(inStream);
    OSStatus st = lbad::hip_status(hipMemcpyAsync(c->d_off + at, c->h_off.data() + at, (inNumberOfEntries + 1) * 4,
                                                  hipMemcpyHostToDevice, stream), "offsets H2D", __LINE__);
    if (st == noErr)
        st = lbad::hip_status(lbad::launch_pack_records(static_cast<const uint32_t*>(inPacked), total, c->d_off + at,
                                                        inNumberOfEntries, (uint32_t)c->count, c->d_recs, stream),
                              "pack records", __LINE__);
    if (st == noErr) {
        try {
            for (UInt64 e = 0; e < inNumberOfEntries; ++e) ++c->len_hist[inCounts[e]];
        } catch (const std::bad_alloc&) {
            // the entries up to e are counted: rebuild the histogram from the offsets that stay
            c->h_off.resize(at + 1);
            c->len_hist.clear();
            for (size_t k = 0; k + 1 < c->h_off.size(); ++k) ++c->len_hist[c->h_off[k + 1] - c->h_off[k]];
            return kLBAudioDetectiveMemFull;
        }
    }
    if (st != noErr) {
        c->h_off.resize(at + 1);
        return st;
    }
    c->count += inNumberOfEntries;
    c->n_pos += total;
    c->ne_max = longest;
    return noErr;
    LBAD_GUARD_END
}

// Everything that may still touch the corpus' memory is awaited first -- the plan, the scans, the top-K, alignment and packed
// scratch, the joins that scanned it or took their rows from it (join_ev, with the join scratch), the gathers (gather_ev), the
// id calls (ids_ev), the polled query's stream --
// and nothing else: NOT append_event or shard_stale_event (the latter may sit behind a collective that never ends).  The
// members then release what they own.
void LBAudioDetectiveCorpusDispose(LBAudioDetectiveCorpusRef c) {
    if (!c) return;
    (void)c->plan_built.wait();
    for (const lbad::Event& e : c->query_ev) (void)e.wait();
    (void)c->topk_ev.wait();
    (void)c->align_ev.wait();
    (void)c->pq_ev.wait();
    (void)c->join_ev.wait();
    (void)c->gather_ev.wait();
    (void)c->ids_ev.wait();
    if (c->stream) { (void)hipStreamSynchronize(c->stream); (void)hipStreamDestroy(c->stream); }
    delete c;
}

UInt64 LBAudioDetectiveCorpusGetCount(LBAudioDetectiveCorpusRef c) { return c ? c->count : 0; }
unsigned long long* LBAudioDetectiveCorpusShardKeysDevice(LBAudioDetectiveCorpusRef c) { return c ? c->d_shard_keys : NULL; }
unsigned long long* LBAudioDetectiveCorpusShardKeysHost(LBAudioDetectiveCorpusRef c) { return c ? c->h_shard_keys : NULL; }

UInt32 LBAudioDetectiveCorpusGetEntryStrideBytes(LBAudioDetectiveCorpusRef c) {
    if (!c) return 0;
    return c->ragged ? 32u : c->n_planes * 16u;   // ragged: bytes per sub-fingerprint record
}

OSStatus LBAudioDetectiveCorpusSetKernelVariant(LBAudioDetectiveCorpusRef c, UInt32 inVariant) {
    if (!c || inVariant > 4 || (inVariant > 2 && !c->ragged)) return kLBAudioDetectiveArgumentInvalid;
    c->variant = inVariant;
    return noErr;
}

OSStatus LBAudioDetectiveCorpusAppendPackedDevice(LBAudioDetectiveCorpusRef c, const void* inPacked,
                                                  UInt64 inNumberOfEntries, void* inStream) {
    if (!c || c->ragged || (!inPacked && inNumberOfEntries)) return kLBAudioDetectiveArgumentInvalid;
    if (c->count + inNumberOfEntries > c->capacity) return kLBAudioDetectiveArgumentInvalid;
    LBAD_HIP(lbad::launch_pack_planes(static_cast<const uint32_t*>(inPacked), inNumberOfEntries, c->n_sub, c->subfp_len,
                                      c->d_planes, c->capacity, c->count, static_cast<hipStream_t>(inStream)));
    // the polled query runs on the corpus's own stream: it waits for this event instead of keeping the caller's
    // stream handle (which may be gone by then); appends on several streams each leave their event behind
    OSStatus st = c->append_event.create();
    if (st == noErr) st = c->append_event.record(static_cast<hipStream_t>(inStream));
    if (st != noErr) return st;
    if (c->stream) LBAD_HIP(hipStreamWaitEvent(c->stream, c->append_event, 0));
    c->appended = true;
    c->count += inNumberOfEntries;
    return noErr;
}

OSStatus LBAudioDetectiveCorpusAppendFingerprint(LBAudioDetectiveCorpusRef c, LBAudioDetectiveFingerprintRef fp) {
    LBAD_GUARD_BEGIN
    if (!c || !fp || fp->length != c->subfp_len) return kLBAudioDetectiveArgumentInvalid;
    if (c->ragged ? fp->count == 0 : fp->count != c->n_sub) return kLBAudioDetectiveArgumentInvalid;
    std::vector<uint32_t> slots;
    lbad::pack_fingerprint(fp, slots);
    lbad::DeviceBuffer<uint32_t> d;
    OSStatus st = d.reserve(slots.size());
    if (st == noErr) st = lbad::hip_status(hipMemcpy(d, slots.data(), slots.size() * 4, hipMemcpyHostToDevice), "copy", __LINE__);
    const UInt32 n = fp->count;
    if (st == noErr) st = c->ragged ? LBAudioDetectiveCorpusAppendRaggedPackedDevice(c, d, &n, 1, NULL)
                                    : LBAudioDetectiveCorpusAppendPackedDevice(c, d, 1, NULL);
    if (st == noErr) st = lbad::hip_status(hipStreamSynchronize(nullptr), "sync", __LINE__);
    return st;
    LBAD_GUARD_END
}

void LBAudioDetectiveCorpusDecodeKey(UInt64 inKey, SInt64* outIndex, Float32* outScore) {
    const uint32_t bits = (uint32_t)(inKey >> 32);
    float score;
    std::memcpy(&score, &bits, 4);
    if (outScore) *outScore = score;
    // strict '<' against an initial 0.0 (LBAudioDetectiveTests.m:60,80): a best score of 0 selects nothing
    if (outIndex) *outIndex = (inKey == 0 || !(score > 0.0f)) ? -1 : (SInt64)(0xFFFFFFFFu - (uint32_t)inKey);
}

OSStatus LBAudioDetectiveCorpusQueryKeyDevice(LBAudioDetectiveCorpusRef c, LBAudioDetectiveFingerprintRef inQuery,
                                              UInt32 inRange, UInt64 inIndexBase, void* outKey, void* inStream) {
    if (c && inIndexBase + c->count > 0x100000000ull) return kLBAudioDetectiveArgumentInvalid;
    return lbad::run_query(c, inQuery, inRange, inIndexBase, nullptr, static_cast<unsigned long long*>(outKey),
                           static_cast<hipStream_t>(inStream));
}

OSStatus LBAudioDetectiveCorpusScoresDevice(LBAudioDetectiveCorpusRef c, LBAudioDetectiveFingerprintRef inQuery,
                                            UInt32 inRange, Float32* outScores, void* inStream) {
    if (!c || !outScores) return kLBAudioDetectiveArgumentInvalid;
    return lbad::run_query(c, inQuery, inRange, 0, outScores, c->d_key, static_cast<hipStream_t>(inStream));
}

// Several queries in one pass over the corpus.  outKeys is a device pointer to inCount 64-bit keys.
OSStatus LBAudioDetectiveCorpusQueryBatchKeysDevice(LBAudioDetectiveCorpusRef c, const LBAudioDetectiveFingerprintRef* inQueries,
                                                    UInt32 inCount, UInt32 inRange, UInt64 inIndexBase, void* outKeys,
                                                    void* inStream) {
    LBAD_GUARD_BEGIN
    if (!c || !inQueries || !outKeys || inCount == 0) return kLBAudioDetectiveArgumentInvalid;
    if (inIndexBase + c->count > 0x100000000ull) return kLBAudioDetectiveArgumentInvalid;
    hipStream_t stream = static_cast<hipStream_t>(inStream);
    unsigned long long* keys = static_cast<unsigned long long*>(outKeys);
    bool all_fast = c->variant != 1;
    for (UInt32 i = 0; i < inCount && all_fast; ++i)
        all_fast = inQueries[i] && lbad::planes_fast_supported(c->subfp_len, c->n_sub, inQueries[i]->count) &&
                   inQueries[i]->length == c->subfp_len;
    if (c->ragged) {   // queries of one length share their passes over the records (sliding.cpp)
        for (UInt32 i = 0; i < inCount; ++i)
            if (!inQueries[i] || inQueries[i]->length != c->subfp_len || inQueries[i]->count == 0) return kLBAudioDetectiveArgumentInvalid;
        return lbad::run_queries_ragged(c, inQueries, inCount, inRange ? inRange : c->subfp_len, inIndexBase, nullptr, keys, stream);
    }
    if (!all_fast) {   // shapes without the specialised scan: one pass per query
        for (UInt32 i = 0; i < inCount; ++i) {
            OSStatus st = lbad::run_query(c, inQueries[i], inRange, inIndexBase, nullptr, keys + i, stream);
            if (st != noErr) return st;
        }
        return noErr;
    }
    const uint32_t range = inRange ? inRange : c->subfp_len;
    const uint32_t kw = lbad::plane_query_words();
    const size_t words = (size_t)inCount * kw;
    // the staging pair is shared with the single-query generic scan, which may still be running on ANOTHER stream:
    // its event (slot 0) orders every reuse, this path's too (round-3 advice)
    OSStatus st = c->query_ev[0].wait_or_create();
    if (st == noErr) st = c->query.reserve(words);
    if (st != noErr) return st;
    LBAD_HIP(hipStreamSynchronize(stream));   // the pinned staging block is reused by every call
    std::memset(c->query.host, 0, words * sizeof(uint32_t));
    std::vector<uint32_t> slots, block;
    for (UInt32 i = 0; i < inCount; ++i) {
        lbad::pack_fingerprint(inQueries[i], slots);
        lbad::build_plane_query(slots.data(), c->n_sub, range, block);
        std::memcpy(c->query.host + (size_t)i * kw, block.data(), block.size() * sizeof(uint32_t));
    }
    LBAD_HIP(hipMemcpyAsync(c->query.dev, c->query.host, words * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    LBAD_HIP(hipMemsetAsync(keys, 0, (size_t)inCount * sizeof(unsigned long long), stream));
    LBAD_HIP(lbad::launch_compare_planes_batch(c->d_planes, c->capacity, c->count, c->n_sub, c->query.dev, inCount,
                                               inIndexBase, keys, stream));
    return c->query_ev[0].record(stream);
    LBAD_GUARD_END
}

OSStatus LBAudioDetectiveCorpusQueryBatch(LBAudioDetectiveCorpusRef c, const LBAudioDetectiveFingerprintRef* inQueries,
                                          UInt32 inCount, UInt32 inRange, SInt64* outIndices, Float32* outScores) {
    LBAD_GUARD_BEGIN
    if (!c || inCount == 0) return kLBAudioDetectiveArgumentInvalid;
    std::vector<unsigned long long> keys(inCount);
    lbad::DeviceBuffer<unsigned long long> d_keys;
    OSStatus st = d_keys.reserve(inCount);
    if (st == noErr) st = LBAudioDetectiveCorpusQueryBatchKeysDevice(c, inQueries, inCount, inRange, 0, d_keys, NULL);
    if (st == noErr)
        st = lbad::hip_status(hipMemcpy(keys.data(), d_keys, keys.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost),
                              "copy keys", __LINE__);
    if (st != noErr) return st;
    for (UInt32 i = 0; i < inCount; ++i)
        LBAudioDetectiveCorpusDecodeKey(keys[i], outIndices ? outIndices + i : NULL, outScores ? outScores + i : NULL);
    return noErr;
    LBAD_GUARD_END
}

// ---- corpus join: the entries of `q` as queries against `c`, every pair at or above the threshold as CSR (k_join.hip) --------
// (kJoinScratchDefault: internal.hpp, shared with api_occurrences.cpp)
namespace lbad {
namespace {

// what needs neither handle nor device
bool join_args_ok(uint64_t first, uint64_t count, float threshold, uint64_t capacity, uint64_t index_base) {
    return std::isfinite(threshold) && threshold > 0.0f && count != 0 && count <= 0xFFFFFFFFull && first <= 0xFFFFFFFFull &&
           capacity != 0 && capacity <= 0x80000000ull && index_base <= 0x100000000ull;
}

// what the handles decide, before anything is reserved or launched: two uniform corpora of one shape, and that shape the
// specialised scan's -- or, for the ragged join, two ragged corpora of one sub-fingerprint length with no entry above the cap
// (ne_max: the host knows it); the rows and the indices in range; rows per chunk under the scratch limit (at most `count`)
OSStatus join_plan(const LBAudioDetectiveCorpus* c, const LBAudioDetectiveCorpus* q, uint64_t first, uint64_t count,
                   uint64_t index_base, bool ragged, uint64_t* out_chunk) {
    if (ragged) {
        if (!c->ragged || !q->ragged || c->subfp_len != q->subfp_len || c->ne_max > LBAD_JOIN_RAGGED_MAX_SUBFINGERPRINTS ||
            q->ne_max > LBAD_JOIN_RAGGED_MAX_SUBFINGERPRINTS)
            return kLBAudioDetectiveArgumentInvalid;
    } else if (c->ragged || q->ragged || c->subfp_len != q->subfp_len || c->n_sub != q->n_sub ||
               !planes_fast_supported(c->subfp_len, c->n_sub, c->n_sub)) {
        return kLBAudioDetectiveArgumentInvalid;
    }
    if (first + count > q->count || index_base + c->count > 0x100000000ull) return kLBAudioDetectiveArgumentInvalid;
    const uint64_t limit = c->join_scratch_limit ? c->join_scratch_limit : kJoinScratchDefault;
    const uint64_t chunk = ragged ? join_ragged_chunk_rows(c->count, limit) : join_chunk_rows(c->count, limit);
    if (chunk == 0) return kLBAudioDetectiveArgumentInvalid;          // the limit holds no row tile of this corpus
    *out_chunk = chunk < count ? chunk : count;
    return noErr;
}

// (ragged: the join of two ragged corpora, k_join_ragged.hip; lags: its optional lag slots, NULL for the uniform join)
OSStatus join_keys_impl(LBAudioDetectiveCorpus* c, LBAudioDetectiveCorpus* q, uint64_t first, uint64_t count, uint32_t range,
                        float threshold, uint32_t skip, uint64_t capacity, uint64_t index_base, bool ragged, unsigned long long* keys,
                        int32_t* lags, unsigned long long* offsets, hipStream_t stream) {
    if (!c || !q || !keys || !offsets || !join_args_ok(first, count, threshold, capacity, index_base)) return kLBAudioDetectiveArgumentInvalid;
    if (!device_ready()) return kLBAudioDetectiveDeviceUnavailable;
    uint64_t chunk = 0;
    OSStatus st = join_plan(c, q, first, count, index_base, ragged, &chunk);
    if (st != noErr) return st;
    if (range == 0) range = c->subfp_len;
    st = c->join_ev.wait_or_create();                                 // (the scratch is the previous call's until then)
    if (st == noErr && q != c) st = q->join_ev.create();
    if (st != noErr) return st;
    // the rows' corpus keeps ONE event for every join that reads it: this stream goes behind the join recorded there last, so
    // that the record below is behind all of them and a Dispose of `q` awaits them all
    if (q != c) LBAD_HIP(hipStreamWaitEvent(stream, q->join_ev, 0));
    // both corpora's latest appends, awaited on the device
    if (c->append_event.ev) LBAD_HIP(hipStreamWaitEvent(stream, c->append_event, 0));
    if (q != c && q->append_event.ev) LBAD_HIP(hipStreamWaitEvent(stream, q->append_event, 0));
    LBAD_HIP(hipMemsetAsync(keys, 0, (size_t)capacity * sizeof(unsigned long long), stream));
    if (lags) LBAD_HIP(hipMemsetAsync(lags, 0, (size_t)capacity * sizeof(int32_t), stream));
    if (c->count == 0) {
        LBAD_HIP(hipMemsetAsync(offsets, 0, (size_t)(count + 1) * sizeof(unsigned long long), stream));
    } else if (ragged) {
        st = c->d_join_scratch.reserve(join_ragged_scratch_bytes(c->count, chunk));
        if (st != noErr) return st;
        JoinRaggedCall call;
        call.d_recs = c->d_recs; call.d_off = c->d_off; call.n_entries = c->count;
        call.d_qrecs = q->d_recs; call.d_qoff = q->d_off; call.q_ne_max = q->ne_max;
        call.subfp_len = c->subfp_len; call.range = range; call.threshold = threshold; call.skip = skip != 0;
        call.capacity = capacity; call.index_base = index_base; call.d_keys = keys; call.d_lags = lags; call.stream = stream;
        hipError_t e = hipSuccess;
        for (uint64_t r0 = 0; r0 < count && e == hipSuccess; r0 += chunk) {
            const uint32_t rows = (uint32_t)(count - r0 < chunk ? count - r0 : chunk);
            e = launch_join_ragged_chunk(call, c->d_join_scratch, (uint32_t)chunk, first + r0, rows, r0 == 0 ? 1u : 0u, offsets + r0);
        }
        st = hip_status(e, "ragged join", __LINE__);
    } else {
        st = c->d_join_scratch.reserve(join_scratch_bytes(c->count, chunk));
        if (st != noErr) return st;
        JoinCall call;
        call.d_planes = c->d_planes; call.stride = c->capacity; call.n_entries = c->count;
        call.d_qplanes = q->d_planes; call.qstride = q->capacity;
        call.n_sub = c->n_sub; call.range = range; call.threshold = threshold; call.skip = skip != 0;
        call.capacity = capacity; call.index_base = index_base; call.d_keys = keys; call.stream = stream;
        hipError_t e = hipSuccess;
        for (uint64_t r0 = 0; r0 < count && e == hipSuccess; r0 += chunk) {
            const uint32_t rows = (uint32_t)(count - r0 < chunk ? count - r0 : chunk);
            e = launch_join_chunk(call, c->d_join_scratch, (uint32_t)chunk, first + r0, rows, r0 == 0 ? 1u : 0u, offsets + r0);
        }
        st = hip_status(e, "join", __LINE__);
    }
    // behind whatever was launched, also after a failure: the scratch and both corpora's planes are in use until then
    const OSStatus rec = c->join_ev.record(stream);
    const OSStatus rec2 = q != c ? q->join_ev.record(stream) : noErr;
    return st != noErr ? st : (rec != noErr ? rec : rec2);
}

// host-returning form: keys and offsets -- the count + 1 offsets ride as keys behind the capacity slots -- and the ragged join's
// lags, where they are wanted, as the 32-bit values in ONE block of the corpus' key buffer on the null stream (key_block_*), one
// read-back, then decoded
OSStatus join_host_impl(LBAudioDetectiveCorpus* c, LBAudioDetectiveCorpus* q, uint64_t first, uint64_t count, uint32_t range,
                        float threshold, uint32_t skip, uint64_t capacity, bool ragged, SInt64* out_rows, SInt64* out_idx,
                        Float32* out_scores, SInt32* out_lags, UInt64* out_total) {
    if (!c || !q || !out_rows || !out_idx || !out_scores || !out_total || !join_args_ok(first, count, threshold, capacity, 0))
        return kLBAudioDetectiveArgumentInvalid;
    if (!device_ready()) return kLBAudioDetectiveDeviceUnavailable;
    uint64_t chunk = 0;
    OSStatus st = join_plan(c, q, first, count, 0, ragged, &chunk);   // (a refused call reserves nothing)
    if (st != noErr) return st;
    KeyBlock b;
    st = key_block_reserve(c, (size_t)capacity + count + 1, out_lags ? (size_t)capacity : 0, &b);
    if (st != noErr) return st;
    st = join_keys_impl(c, q, first, count, range, threshold, skip, capacity, 0, ragged, b.d_keys, reinterpret_cast<int32_t*>(b.d_words),
                        b.d_keys + capacity, nullptr);
    if (st != noErr) return key_block_failed(st);
    std::vector<unsigned long long> host;
    st = key_block_read(b, b.n_keys, &host);
    if (st != noErr) return st;
    const unsigned long long* off = host.data() + capacity;
    const int32_t* lags = reinterpret_cast<const int32_t*>(off + count + 1);
    uint64_t row = 0;
    for (uint64_t at = 0; at < capacity; ++at) {
        if (out_lags) out_lags[at] = at < off[count] ? lags[at] : 0;
        if (at >= off[count]) {
            out_rows[at] = -1; out_idx[at] = -1; out_scores[at] = 0.0f;
            continue;
        }
        while (off[row + 1] <= at) ++row;          // (at < the total: a row with this slot exists)
        LBAudioDetectiveCorpusDecodeKey(host[at], out_idx + at, out_scores + at);
        out_rows[at] = (SInt64)(first + row);
    }
    *out_total = off[count];
    return noErr;
}
}  // namespace
}  // namespace lbad

extern "C" {

OSStatus LBAudioDetectiveCorpusJoinThresholdKeysDevice(LBAudioDetectiveCorpusRef inCorpus, LBAudioDetectiveCorpusRef inQueries,
                                                       UInt64 inFirstQuery, UInt64 inQueryCount, UInt32 inRange, Float32 inThreshold,
                                                       UInt32 inSkipSameIndex, UInt64 inCapacity, UInt64 inIndexBase, void* outKeys,
                                                       void* outOffsets, void* inStream) {
    LBAD_GUARD_BEGIN
    return lbad::join_keys_impl(inCorpus, inQueries, inFirstQuery, inQueryCount, inRange, inThreshold, inSkipSameIndex, inCapacity,
                                inIndexBase, false, static_cast<unsigned long long*>(outKeys), nullptr,
                                static_cast<unsigned long long*>(outOffsets), static_cast<hipStream_t>(inStream));
    LBAD_GUARD_END
}

OSStatus LBAudioDetectiveCorpusJoinRaggedThresholdKeysDevice(LBAudioDetectiveCorpusRef inCorpus, LBAudioDetectiveCorpusRef inQueries,
                                                             UInt64 inFirstQuery, UInt64 inQueryCount, UInt32 inRange,
                                                             Float32 inThreshold, UInt32 inSkipSameIndex, UInt64 inCapacity,
                                                             UInt64 inIndexBase, void* outKeys, void* outLags, void* outOffsets,
                                                             void* inStream) {
    LBAD_GUARD_BEGIN
    return lbad::join_keys_impl(inCorpus, inQueries, inFirstQuery, inQueryCount, inRange, inThreshold, inSkipSameIndex, inCapacity,
                                inIndexBase, true, static_cast<unsigned long long*>(outKeys), static_cast<int32_t*>(outLags),
                                static_cast<unsigned long long*>(outOffsets), static_cast<hipStream_t>(inStream));
    LBAD_GUARD_END
}

OSStatus LBAudioDetectiveCorpusJoinRaggedThreshold(LBAudioDetectiveCorpusRef inCorpus, LBAudioDetectiveCorpusRef inQueries,
                                                   UInt64 inFirstQuery, UInt64 inQueryCount, UInt32 inRange, Float32 inThreshold,
                                                   UInt32 inSkipSameIndex, UInt64 inCapacity, SInt64* outQueryIndices,
                                                   SInt64* outEntryIndices, Float32* outScores, SInt32* outLags, UInt64* outTotal) {
    LBAD_GUARD_BEGIN
    return lbad::join_host_impl(inCorpus, inQueries, inFirstQuery, inQueryCount, inRange, inThreshold, inSkipSameIndex, inCapacity,
                                true, outQueryIndices, outEntryIndices, outScores, outLags, outTotal);
    LBAD_GUARD_END
}

OSStatus LBAudioDetectiveCorpusJoinThreshold(LBAudioDetectiveCorpusRef inCorpus, LBAudioDetectiveCorpusRef inQueries, UInt64 inFirstQuery,
                                             UInt64 inQueryCount, UInt32 inRange, Float32 inThreshold, UInt32 inSkipSameIndex,
                                             UInt64 inCapacity, SInt64* outQueryIndices, SInt64* outEntryIndices, Float32* outScores,
                                             UInt64* outTotal) {
    LBAD_GUARD_BEGIN
    return lbad::join_host_impl(inCorpus, inQueries, inFirstQuery, inQueryCount, inRange, inThreshold, inSkipSameIndex, inCapacity,
                                false, outQueryIndices, outEntryIndices, outScores, nullptr, outTotal);
    LBAD_GUARD_END
}

OSStatus LBAudioDetectiveCorpusSetJoinScratchLimit(LBAudioDetectiveCorpusRef inCorpus, UInt64 inBytes) {
    if (!inCorpus) return kLBAudioDetectiveArgumentInvalid;
    inCorpus->join_scratch_limit = inBytes;
    // a block above the new limit goes, once the call that uses it is done
    const uint64_t limit = inBytes ? inBytes : lbad::kJoinScratchDefault;
    if (inCorpus->d_join_scratch.capacity() > limit) {
        OSStatus st = inCorpus->join_ev.wait();
        if (st != noErr) return st;
        inCorpus->d_join_scratch.reset();
    }
    return noErr;
}

// Debug / tests: the blocks a builder makes of inCount x inPer sub-fingerprints -- from packed rows on the device (the kernels
// of k_query.hip) or from Booleans on the host (the builders behind the handle-taking calls) -- copied to a host buffer
OSStatus LBAudioDetectiveDebugQueryBlocks(UInt32 inKind, const void* inPackedQueries, const Boolean* inBooleans, UInt32 inCount,
                                          UInt32 inPer, UInt32 inSubfingerprintLength, UInt32 inRange, UInt32* outWords,
                                          UInt64 inCapacity, UInt64* outCount) {
    LBAD_GUARD_BEGIN
    const uint32_t L = inSubfingerprintLength;
    if (inKind > 3 || (!inPackedQueries) == (!inBooleans) || inCount == 0 || inPer == 0 || !outCount || L == 0 ||
        (uint64_t)inCount * inPer > 0xFFFFFFFFull)
        return kLBAudioDetectiveArgumentInvalid;
    if (inKind == 0 ? !lbad::planes_fast_supported(L, inPer, inPer) : (inKind == 3 ? L > 32u * lbad::kPackedWords : !lbad::sliding_supported(L)))
        return kLBAudioDetectiveArgumentInvalid;
    const uint32_t range = inRange ? inRange : L;
    const size_t per_query = inKind == 0 ? lbad::plane_query_words() : (inKind == 1 ? lbad::sliding_block_words(inPer) : (size_t)inPer * lbad::kPackedWords);
    const size_t words = per_query * inCount;
    *outCount = words;
    if (!outWords || inCapacity < words) return kLBAudioDetectiveArgumentInvalid;
    if (inBooleans) {
        std::vector<uint32_t> slots, block;
        LBAudioDetectiveFingerprint fp;
        fp.length = L;
        fp.count = inPer;
        for (UInt32 q = 0; q < inCount; ++q) {
            const Boolean* b = inBooleans + (size_t)q * inPer * L;
            uint32_t* o = outWords + (size_t)q * per_query;
            std::memset(o, 0, per_query * sizeof(uint32_t));
            if (inKind == 1) {
                lbad::build_sliding_query(b, inPer, L, range, block);
                std::memcpy(o, block.data(), per_query * sizeof(uint32_t));
                continue;
            }
            fp.data.assign(b, b + (size_t)inPer * L);
            block.clear();
            if (inKind == 0) {
                lbad::pack_fingerprint(&fp, slots);
                lbad::build_plane_query(slots.data(), inPer, range, block);
            } else {
                lbad::build_align_query(&fp, inKind == 2, block);
            }
            std::memcpy(o, block.data(), block.size() * sizeof(uint32_t));
        }
        return noErr;
    }
    if (!lbad::device_ready()) return kLBAudioDetectiveDeviceUnavailable;
    lbad::DeviceBuffer<uint32_t> d;
    OSStatus st = d.reserve(words);
    if (st != noErr) return st;
    const uint32_t* rows = static_cast<const uint32_t*>(inPackedQueries);
    hipError_t e = inKind == 0   ? lbad::launch_build_plane_queries(rows, inCount, inPer, range, d, nullptr)
                   : inKind == 1 ? lbad::launch_build_sliding_queries(rows, inCount, inPer, L, range, d, nullptr)
                                 : lbad::launch_build_query_rows(rows, inCount, inPer, L, inKind == 2, d, nullptr, nullptr);
    if (e == hipSuccess) e = hipMemcpy(outWords, d, words * sizeof(uint32_t), hipMemcpyDeviceToHost);
    return lbad::hip_status(e, "query blocks", __LINE__);
    LBAD_GUARD_END
}

// Debug / tests: the decision of one ragged launch (sliding_choose) as words; no device is touched
OSStatus LBAudioDetectiveDebugSlidingChoice(const UInt32* inEntryLengths, const UInt64* inEntryCounts, UInt32 inLengthCount,
                                            UInt64 inRecordCount, UInt32 inLongestEntry, UInt32 inKernelVariant,
                                            UInt32 inSubfingerprintLength, UInt32 inQueryLength, UInt32 inQueriesLeft, UInt32 inRange,
                                            UInt32 inScores, UInt32 inHostBlocks, UInt32 inComputeUnits, UInt32* outWords,
                                            UInt32 inCapacity) {
    LBAD_GUARD_BEGIN
    if (!outWords || inCapacity < 21 || inQueryLength == 0 || inQueriesLeft == 0 || inComputeUnits == 0 ||
        (inLengthCount && (!inEntryLengths || !inEntryCounts)) || !lbad::sliding_supported(inSubfingerprintLength))
        return kLBAudioDetectiveArgumentInvalid;
    std::map<uint32_t, uint64_t> hist;
    for (UInt32 i = 0; i < inLengthCount; ++i) hist[inEntryLengths[i]] += inEntryCounts[i];
    lbad::SlideCorpusStats stats;
    stats.len_hist = &hist; stats.n_pos = inRecordCount; stats.ne_max = inLongestEntry; stats.variant = inKernelVariant;
    stats.subfp_len = inSubfingerprintLength;
    lbad::SlideGroup group;
    group.n_query = inQueryLength; group.n_left = inQueriesLeft; group.range = inRange ? inRange : inSubfingerprintLength;
    group.scores = inScores != 0; group.host_blocks = inHostBlocks != 0;
    lbad::sliding_choice_words(lbad::sliding_choose(stats, group, inComputeUnits), inQueryLength, outWords);
    return noErr;
    LBAD_GUARD_END
}

}  // extern "C"

// ---- corpus file: header + the planes of the stored entries, plane-major ----------------------------
namespace {
struct CorpusFileHeader {
    char magic[8];            // "LBADCRP1"
    uint32_t subfp_len, n_sub, n_planes, reserved;
    uint64_t count;
};
}  // namespace

// ragged corpus file: header, the entries' sub-fingerprint counts, the records
namespace {
struct RaggedFileHeader {
    char magic[8];            // "LBADCRP3" (round-4 record layout, sliding_common.hpp); "LBADCRP2" files (round 3) still load
    uint32_t subfp_len, reserved;
    uint64_t count, n_pos;
};

OSStatus save_ragged(LBAudioDetectiveCorpus* c, FILE* f) {
    RaggedFileHeader h;
    std::memcpy(h.magic, "LBADCRP3", 8);
    h.subfp_len = c->subfp_len; h.reserved = 0; h.count = c->count; h.n_pos = c->n_pos;
    if (std::fwrite(&h, sizeof(h), 1, f) != 1) return kLBAudioDetectiveDeviceError;
    std::vector<uint32_t> counts(c->count);
    for (uint64_t e = 0; e < c->count; ++e) counts[e] = c->h_off[e + 1] - c->h_off[e];
    if (c->count && std::fwrite(counts.data(), 4, c->count, f) != c->count) return kLBAudioDetectiveDeviceError;
    const size_t piece = 1u << 20;                        // records per staging piece (32 MiB)
    std::vector<uint4> host(2 * (c->n_pos < piece ? (size_t)c->n_pos : piece));
    for (uint64_t at = 0; at < c->n_pos; at += piece) {
        const size_t n = (size_t)(c->n_pos - at < piece ? c->n_pos - at : piece);
        OSStatus st = lbad::hip_status(hipMemcpy(host.data(), c->d_recs + 2 * at, n * 32, hipMemcpyDeviceToHost),
                                       "corpus records D2H", __LINE__);
        if (st != noErr) return st;
        if (std::fwrite(host.data(), 32, n, f) != n) return kLBAudioDetectiveDeviceError;
    }
    return lbad::ids_save_trailer(c, f);                  // (a corpus without ids: nothing)
}

LBAudioDetectiveCorpusRef load_ragged(FILE* f, long file_size, uint64_t capacity) {
    RaggedFileHeader h;
    if (file_size < (long)sizeof(h) || std::fread(&h, sizeof(h), 1, f) != 1) return NULL;
    const bool old_layout = std::memcmp(h.magic, "LBADCRP2", 8) == 0;
    // untrusted header: the file must really hold what it announces before anything is allocated from it
    if (!lbad::sliding_supported(h.subfp_len) || h.count > lbad::kMaxRaggedEntries || h.n_pos > lbad::kMaxRaggedRecords || h.n_pos < h.count)
        return NULL;
    if ((uint64_t)(file_size - (long)sizeof(h)) < h.count * 4 + h.n_pos * 32) return NULL;
    std::vector<uint32_t> counts;
    try { counts.resize(h.count); } catch (const std::bad_alloc&) { return NULL; }
    if (h.count && std::fread(counts.data(), 4, h.count, f) != h.count) return NULL;
    uint64_t total = 0;
    for (uint64_t e = 0; e < h.count; ++e) {
        if (counts[e] == 0) return NULL;
        total += counts[e];
    }
    if (total != h.n_pos) return NULL;
    uint64_t cap = capacity > h.count ? capacity : (h.count ? h.count : 1);
    if (cap > lbad::kMaxRaggedEntries) cap = lbad::kMaxRaggedEntries;           // (NewRagged's own limits: a large request is clamped, not refused)
    // room for records in proportion to the entry capacity
    uint64_t rec_cap = h.count ? (uint64_t)(((unsigned __int128)h.n_pos * cap + h.count - 1) / h.count) : cap * 64;
    if (rec_cap < cap) rec_cap = cap;
    if (rec_cap > lbad::kMaxRaggedRecords) rec_cap = lbad::kMaxRaggedRecords;
    LBAudioDetectiveCorpusRef c = LBAudioDetectiveCorpusNewRagged(h.subfp_len, cap, rec_cap);
    if (!c) return NULL;
    bool ok = true;
    const size_t piece = 1u << 20;
    uint4* host = static_cast<uint4*>(std::malloc(32 * (h.n_pos < piece ? (size_t)(h.n_pos ? h.n_pos : 1) : piece)));
    if (!host) ok = false;
    for (uint64_t at = 0; ok && at < h.n_pos; at += piece) {
        const size_t n = (size_t)(h.n_pos - at < piece ? h.n_pos - at : piece);
        ok = std::fread(host, 32, n, f) == n &&
             lbad::hip_status(hipMemcpy(c->d_recs + 2 * at, host, n * 32, hipMemcpyHostToDevice), "corpus records H2D",
                              __LINE__) == noErr;
    }
    std::free(host);
    if (ok) {
        try {
            c->h_off.resize(h.count + 1);
        } catch (const std::bad_alloc&) { ok = false; }
    }
    if (ok) {
        c->h_off[0] = 0;
        try {
            for (uint64_t e = 0; e < h.count; ++e) {
                c->h_off[e + 1] = c->h_off[e] + counts[e];
                if (counts[e] > c->ne_max) c->ne_max = counts[e];
                ++c->len_hist[counts[e]];
            }
        } catch (const std::bad_alloc&) { ok = false; }
    }
    if (ok)
        ok = lbad::hip_status(hipMemcpy(c->d_off, c->h_off.data(), (h.count + 1) * 4, hipMemcpyHostToDevice),
                              "corpus offsets H2D", __LINE__) == noErr;
    // The records of a file are data, not structure: every place a record has inside its entry comes from the counts
    // validated above (the scan reads d_off, nothing else), and what a record carries besides its 200 Booleans -- the
    // table row of its `possible`, reserved bits, pairs beyond the length -- is recomputed / cleared here, so a crafted
    // file cannot steer the scan (round-3 advice: the old records carried their own index fields)
    if (ok)
        ok = lbad::hip_status(lbad::launch_restamp_records(c->d_recs, c->d_off, h.count, h.n_pos, h.subfp_len, old_layout, nullptr),
                              "restamp records", __LINE__) == noErr &&
             lbad::hip_status(hipStreamSynchronize(nullptr), "restamp records", __LINE__) == noErr;
    if (ok) ok = lbad::ids_load_trailer(c, f, h.count);      // (f stands behind the records)
    if (!ok) {
        LBAudioDetectiveCorpusDispose(c);
        return NULL;
    }
    c->count = h.count;
    c->n_pos = h.n_pos;
    return c;
}
}  // namespace

OSStatus LBAudioDetectiveCorpusSave(LBAudioDetectiveCorpusRef c, const char* inPath) {
    if (!c || !inPath) return kLBAudioDetectiveArgumentInvalid;
    FILE* f = std::fopen(inPath, "wb");
    if (!f) return -43;
    if (c->ragged) {
        OSStatus rst = kLBAudioDetectiveMemFull;
        try { rst = save_ragged(c, f); } catch (const std::bad_alloc&) {}
        std::fclose(f);
        return rst;
    }
    CorpusFileHeader h;
    std::memcpy(h.magic, "LBADCRP1", 8);
    h.subfp_len = c->subfp_len; h.n_sub = c->n_sub; h.n_planes = c->n_planes; h.reserved = 0; h.count = c->count;
    OSStatus st = std::fwrite(&h, sizeof(h), 1, f) == 1 ? noErr : kLBAudioDetectiveDeviceError;
    std::vector<uint4> host;
    try {
        host.resize(c->count);
    } catch (const std::bad_alloc&) {
        std::fclose(f);
        return kLBAudioDetectiveMemFull;
    }
    for (uint32_t p = 0; p < c->n_planes && st == noErr && c->count; ++p) {
        st = lbad::hip_status(hipMemcpy(host.data(), c->d_planes + (size_t)p * c->capacity, c->count * sizeof(uint4),
                                        hipMemcpyDeviceToHost), "corpus plane D2H", __LINE__);
        if (st == noErr && std::fwrite(host.data(), sizeof(uint4), c->count, f) != c->count) st = kLBAudioDetectiveDeviceError;
    }
    if (st == noErr) {
        st = kLBAudioDetectiveMemFull;
        try { st = lbad::ids_save_trailer(c, f); } catch (const std::bad_alloc&) {}      // (a corpus without ids: nothing)
    }
    std::fclose(f);
    return st;
}

LBAudioDetectiveCorpusRef LBAudioDetectiveCorpusLoad(const char* inPath, UInt64 inCapacity) {
    if (!inPath) return NULL;
    FILE* f = std::fopen(inPath, "rb");
    if (!f) return NULL;
    CorpusFileHeader h;
    LBAudioDetectiveCorpusRef c = NULL;
    // the header is untrusted: the shape must be one the device path supports and the file must really hold
    // count * n_planes planes before anything is allocated from it
    std::fseek(f, 0, SEEK_END);
    const long file_size = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    char magic[8] = {0};
    if (file_size >= 8 && std::fread(magic, 8, 1, f) == 1 &&
        (std::memcmp(magic, "LBADCRP3", 8) == 0 || std::memcmp(magic, "LBADCRP2", 8) == 0)) {
        std::fseek(f, 0, SEEK_SET);
        c = load_ragged(f, file_size, inCapacity);
        std::fclose(f);
        return c;
    }
    std::fseek(f, 0, SEEK_SET);
    bool ok = file_size >= (long)sizeof(h) && std::fread(&h, sizeof(h), 1, f) == 1 &&
              std::memcmp(h.magic, "LBADCRP1", 8) == 0 && h.subfp_len > 0 &&
              h.subfp_len <= LBAD_MAX_SUBFINGERPRINT_LENGTH && h.n_sub > 0 &&
              lbad::planes_supported(h.subfp_len, h.n_sub) && h.n_planes == lbad::planes_per_entry(h.subfp_len, h.n_sub) &&
              h.count <= 0xFFFFFFFFull &&
              (uint64_t)(file_size - (long)sizeof(h)) / sizeof(uint4) / (h.n_planes ? h.n_planes : 1) >= h.count;
    if (ok) {
        const uint64_t cap = inCapacity > h.count ? inCapacity : (h.count ? h.count : 1);
        c = LBAudioDetectiveCorpusNew(h.subfp_len, h.n_sub, cap);
    }
    if (c && h.count) {
        // staged in bounded pieces, not one count-sized vector
        const size_t piece = 1u << 20;
        uint4* host = static_cast<uint4*>(std::malloc(sizeof(uint4) * (h.count < piece ? (size_t)h.count : piece)));
        if (!host) ok = false;
        for (uint32_t p = 0; ok && p < h.n_planes; ++p) {
            for (uint64_t at = 0; ok && at < h.count; at += piece) {
                const size_t n = (size_t)(h.count - at < piece ? h.count - at : piece);
                ok = std::fread(host, sizeof(uint4), n, f) == n &&
                     lbad::hip_status(hipMemcpy(c->d_planes + (size_t)p * c->capacity + at, host, n * sizeof(uint4),
                                                hipMemcpyHostToDevice), "corpus plane H2D", __LINE__) == noErr;
            }
        }
        std::free(host);
        if (!ok) {
            LBAudioDetectiveCorpusDispose(c);
            c = NULL;
        }
    }
    // f stands behind the planes (an empty corpus: behind the header)
    if (c && !lbad::ids_load_trailer(c, f, h.count)) {
        LBAudioDetectiveCorpusDispose(c);
        c = NULL;
    }
    if (c) c->count = h.count;
    std::fclose(f);
    return c;
}

OSStatus LBAudioDetectiveCorpusQuery(LBAudioDetectiveCorpusRef c, LBAudioDetectiveFingerprintRef inQuery, UInt32 inRange,
                                     SInt64* outIndex, Float32* outScore) {
    if (!c) return kLBAudioDetectiveArgumentInvalid;
    unsigned long long key = 0;
    if (inQuery && c->count > 0 && c->variant != 1 && inQuery->length == c->subfp_len &&
        lbad::planes_fast_supported(c->subfp_len, c->n_sub, inQuery->count)) {
        c->appended = false;                                // every append made the query stream wait for it
        OSStatus st = lbad::query_fast(c, inQuery, inRange, &key);
        if (st != noErr) return st;
        LBAudioDetectiveCorpusDecodeKey(key, outIndex, outScore);
        return noErr;
    }
    OSStatus st = lbad::run_query(c, inQuery, inRange, 0, nullptr, c->d_key, nullptr);
    if (st != noErr) return st;
    LBAD_HIP(hipMemcpy(&key, c->d_key, sizeof(key), hipMemcpyDeviceToHost));
    LBAudioDetectiveCorpusDecodeKey(key, outIndex, outScore);
    return noErr;
}

OSStatus LBAudioDetectiveCorpusSetBoundPruning(LBAudioDetectiveCorpusRef c, UInt32 inEnabled) {
    if (!c) return kLBAudioDetectiveArgumentInvalid;
    c->bound_pruning = inEnabled != 0;
    return noErr;
}

OSStatus LBAudioDetectiveCorpusSetBoundPruningThreshold(LBAudioDetectiveCorpusRef c, Float32 inScore) {
    if (!c || !(inScore > 0.0f) || !(inScore <= 1.0f)) return kLBAudioDetectiveArgumentInvalid;
    c->prune_from = inScore;
    return noErr;
}

Float32 LBAudioDetectiveCorpusGetBoundPruningThreshold(LBAudioDetectiveCorpusRef c) { return c ? c->prune_from : 0.0f; }

}  // extern "C"
