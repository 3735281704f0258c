// api_select.cpp -- top-K and threshold queries of the corpus, and the packed queries: exact per-entry scores (the unchanged
// scans' scores path, api_corpus.cpp), then a selection over the score rows (k_topk.hip, k_threshold.hip).  The queries come as
// handles or as packed sub-fingerprints on the device (the builders of k_query.hip); one runner each, one selection loop.
#include "internal.hpp"

#include <cmath>
#include <cstring>
#include <functional>

namespace lbad {
namespace {

// one query's per-entry scores (count floats) to d_scores and the scan's own key word to d_key, on the call's stream
using ScoreScan = std::function<OSStatus(uint32_t q, float* d_scores, unsigned long long* d_key)>;

// What follows a group's score rows: the k best entries of every row (k_topk.hip) or, by_threshold, every entry at or above
// `threshold`, up to `capacity` per row, and the rows' counts (k_threshold.hip).  Row q's keys go to keys + q * slots().
struct Selection {
    bool by_threshold = false;
    uint32_t k = 0;
    float threshold = 0.0f;
    uint64_t capacity = 0;
    uint64_t index_base = 0;
    unsigned long long* keys = nullptr;      // device, n x slots()
    unsigned long long* counts = nullptr;    // device, n (threshold only)
    int32_t* lags = nullptr;                 // device, n x slots(): the packed forms', optional
    uint64_t slots() const { return by_threshold ? capacity : k; }
};

// the selection's words for `rows` score rows of `count` entries, and the selection of the g rows at d_scores for the queries
// from q0 on -- the corpus calls' and, over a caller's scores, the ...KeysFromScoresDevice calls'
size_t selection_scratch_bytes(const Selection& sel, uint64_t count, uint32_t rows) {
    return sel.by_threshold ? threshold_scratch_bytes(count, rows) : topk_scratch_bytes(rows);
}
hipError_t launch_selection(const Selection& sel, const float* d_scores, uint64_t count, uint32_t q0, uint32_t g, void* d_scratch,
                            hipStream_t stream) {
    unsigned long long* keys = sel.keys + (size_t)q0 * sel.slots();
    if (sel.by_threshold)
        return launch_threshold_keys(d_scores, count, g, sel.threshold, sel.capacity, sel.index_base, d_scratch, keys, sel.counts + q0, stream);
    return launch_topk_keys(d_scores, count, g, sel.k, sel.index_base, d_scratch, keys, stream);
}

// score rows, the selection's own scratch and the scans' key words for a call of n queries (allocated exactly: the score rows
// are the size of the corpus).  The caller holds topk_ev: the previous call's scans and selection may still read / write the
// scratch, on whatever stream it ran.
OSStatus reserve_selection(LBAudioDetectiveCorpus* c, const Selection& sel, uint32_t n) {
    const uint32_t rows = n < kQueryBatchMax ? n : kQueryBatchMax;
    OSStatus st = c->d_topk_scores.reserve((size_t)rows * c->count);
    if (st == noErr) st = (sel.by_threshold ? c->d_threshold_scratch : c->d_topk_scratch).reserve(selection_scratch_bytes(sel, c->count, rows));
    if (st == noErr) st = c->d_topk_scan_keys.reserve(kQueryBatchMax);
    return st;
}

// zero keys, zero counts and zero lags: the answer of an empty corpus
OSStatus select_nothing(const Selection& sel, uint32_t n, hipStream_t stream) {
    LBAD_HIP(hipMemsetAsync(sel.keys, 0, (size_t)n * sel.slots() * sizeof(unsigned long long), stream));
    if (sel.counts) LBAD_HIP(hipMemsetAsync(sel.counts, 0, (size_t)n * sizeof(unsigned long long), stream));
    if (sel.lags) LBAD_HIP(hipMemsetAsync(sel.lags, 0, (size_t)n * sel.slots() * sizeof(int32_t), stream));
    return noErr;
}

// The score rows of one group of g <= kQueryBatchMax staged queries (q0 the group's first) to d_topk_scores, row i at i * count:
// d_qblocks given (the batch scan's blocks of ALL the call's queries, on the device): ONE pass of the batch scan; otherwise
// scan_one per query.
OSStatus scan_group_scores(LBAudioDetectiveCorpus* c, uint32_t q0, uint32_t g, hipStream_t stream, const uint32_t* d_qblocks,
                           const ScoreScan& scan_one) {
    if (d_qblocks) {
        LBAD_HIP(launch_compare_planes_batch_scores(c->d_planes, c->capacity, c->count, c->n_sub,
                                                    d_qblocks + (size_t)q0 * plane_query_words(), g, c->d_topk_scores, stream));
        return noErr;
    }
    for (uint32_t i = 0; i < g; ++i) {
        OSStatus st = scan_one(q0 + i, c->d_topk_scores + (size_t)i * c->count, c->d_topk_scan_keys + i);
        if (st != noErr) return st;
    }
    return noErr;
}

// The scans and the selection of n staged queries: groups of up to kQueryBatchMax queries write their score rows
// (scan_group_scores), then one selection over the group's rows.
OSStatus scan_select(LBAudioDetectiveCorpus* c, uint32_t n, const Selection& sel, hipStream_t stream, const uint32_t* d_qblocks,
                     const ScoreScan& scan_one) {
    for (uint32_t q0 = 0; q0 < n; q0 += kQueryBatchMax) {
        const uint32_t g = n - q0 < kQueryBatchMax ? n - q0 : kQueryBatchMax;
        OSStatus st = scan_group_scores(c, q0, g, stream, d_qblocks, scan_one);
        if (st != noErr) return st;
        LBAD_HIP(launch_selection(sel, c->d_topk_scores, c->count, q0, g, sel.by_threshold ? c->d_threshold_scratch : c->d_topk_scratch, stream));
    }
    return noErr;
}

// the batch scan's blocks of n queries (uniform corpus, the specialised shape) through the pinned staging copy to the device,
// every group's at once: the copy is asynchronous on `stream`
OSStatus stage_plane_queries(LBAudioDetectiveCorpus* c, const LBAudioDetectiveFingerprintRef* qs, uint32_t n, uint32_t range,
                             hipStream_t stream) {
    const uint32_t kw = plane_query_words();
    const size_t bytes = (size_t)n * kw * sizeof(uint32_t);
    OSStatus st = c->topk_q.reserve((size_t)n * kw);
    if (st != noErr) return st;
    std::memset(c->topk_q.host, 0, bytes);
    std::vector<uint32_t> slots, block;
    for (uint32_t i = 0; i < n; ++i) {
        pack_fingerprint(qs[i], slots);
        build_plane_query(slots.data(), c->n_sub, range, block);
        std::memcpy(c->topk_q.host + (size_t)i * kw, block.data(), block.size() * sizeof(uint32_t));
    }
    LBAD_HIP(hipMemcpyAsync(c->topk_q.dev, c->topk_q.host, bytes, hipMemcpyHostToDevice, stream));
    return noErr;
}

// The runner of n queries given as handles (checked by the caller): staged from the handles (uniform corpus, the specialised
// shape: the batch scan's blocks; otherwise each scores scan stages its own), then scan_select.  topk_ev is awaited before the
// scratch is touched and recorded behind whatever was launched, also after a failure: the scratch is in use until then.
OSStatus select_handles(LBAudioDetectiveCorpus* c, const LBAudioDetectiveFingerprintRef* qs, uint32_t n, uint32_t range,
                        const Selection& sel, hipStream_t stream) {
    if (range == 0) range = c->subfp_len;   // LBAudioDetective.m:443-445
    bool batch_scan = !c->ragged && c->variant != 1;
    for (uint32_t i = 0; i < n && batch_scan; ++i) batch_scan = planes_fast_supported(c->subfp_len, c->n_sub, qs[i]->count);
    PassGuard scratch(&c->topk_ev);
    OSStatus st = scratch.wait();
    if (st != noErr) return st;
    if (c->count == 0) return scratch.finish(stream, select_nothing(sel, n, stream));
    st = reserve_selection(c, sel, n);
    if (st == noErr && batch_scan) st = stage_plane_queries(c, qs, n, range, stream);
    if (st == noErr)
        st = scan_select(c, n, sel, stream, batch_scan ? c->topk_q.dev.get() : nullptr,
                         [&](uint32_t q, float* d_scores, unsigned long long* d_key) {
                             return run_query(c, qs[q], range, 0, d_scores, d_key, stream);
                         });
    return scratch.finish(stream, st);
}

// ---- packed queries: the blocks come from the builders of k_query.hip instead of the handles' Booleans ---------------------
struct BuiltQueries {
    const uint32_t* scan = nullptr;      // ragged: sliding blocks; uniform: plane blocks (fast) or the rows cleared from the length on
    bool fast = false;
    const uint2* desc = nullptr;         // with lags: launch_align_keys' table and words
    const uint32_t* words = nullptr;
};

// n queries of `per` packed sub-fingerprints at d_rows (device) -> their blocks in the corpus' scratch, on `stream`.  The caller
// holds pq_ev (awaited on the host, as the top-K scratch's is) and records it behind its last kernel.
OSStatus build_packed(LBAudioDetectiveCorpus* c, const uint32_t* d_rows, uint32_t n, uint32_t per, uint32_t range, bool lags,
                      hipStream_t stream, BuiltQueries& out) {
    if ((uint64_t)n * per > 0xFFFFFFFFull) return kLBAudioDetectiveArgumentInvalid;      // (the tables count sub-fingerprints in 32 bits)
    if (lags && (per > 0x7FFFFFFFu || (c->ragged && c->ne_max > 0x7FFFFFFFu))) return kLBAudioDetectiveArgumentInvalid;   // (a lag is a signed 32-bit offset)
    out.fast = !c->ragged && c->variant != 1 && planes_fast_supported(c->subfp_len, c->n_sub, per);
    if (!c->ragged) {
        if (c->variant == 2 && !out.fast) return kLBAudioDetectiveArgumentInvalid;
        if (!out.fast && (size_t)per * kPackedWords * 4 > 48 * 1024) return kLBAudioDetectiveArgumentInvalid;     // (the generic scan keeps the query in LDS)
    }
    const size_t row_words = (size_t)n * per * kPackedWords;
    const size_t scan_words = c->ragged ? (size_t)n * sliding_block_words(per) : (out.fast ? (size_t)n * plane_query_words() : row_words);
    const bool rows_serve_both = !c->ragged && !out.fast;         // the generic scan and the uniform alignment read the same words
    // (every part starts on a 256-byte boundary, as the staging slots of the handle path do)
    const size_t desc_words = lags ? (((size_t)2 * n + 63) & ~(size_t)63) : 0;
    const size_t align_words = lags && !rows_serve_both ? ((row_words + 63) & ~(size_t)63) : 0;
    OSStatus st = c->d_pq.reserve(desc_words + align_words + scan_words);
    if (st != noErr) return st;
    uint2* desc = lags ? reinterpret_cast<uint2*>(c->d_pq.get()) : nullptr;
    uint32_t* words = c->d_pq + desc_words;
    uint32_t* scan = words + align_words;
    if (c->ragged) {
        LBAD_HIP(launch_build_sliding_queries(d_rows, n, per, c->subfp_len, range, scan, stream));
        if (lags) LBAD_HIP(launch_build_query_rows(d_rows, n, per, c->subfp_len, true, words, desc, stream));
    } else if (out.fast) {
        LBAD_HIP(launch_build_plane_queries(d_rows, n, c->n_sub, range, scan, stream));
        if (lags) LBAD_HIP(launch_build_query_rows(d_rows, n, per, c->subfp_len, false, words, desc, stream));
    } else {
        LBAD_HIP(launch_build_query_rows(d_rows, n, per, c->subfp_len, false, scan, desc, stream));
        words = scan;
    }
    out.scan = scan;
    out.desc = desc;
    out.words = lags ? words : nullptr;
    return noErr;
}

// one built query's scan with per-entry scores (top-K) or without (d_scores null; uniform generic shapes, top-1)
OSStatus scan_built_one(LBAudioDetectiveCorpus* c, const BuiltQueries& b, uint32_t q, uint32_t per, uint32_t range, uint64_t index_base,
                        float* d_scores, unsigned long long* d_key, hipStream_t stream) {
    if (c->ragged)
        return run_built_ragged(c, b.scan + (size_t)q * sliding_block_words(per), 1, per, range, index_base, d_scores, d_key, stream);
    LBAD_HIP(hipMemsetAsync(d_key, 0, sizeof(unsigned long long), stream));
    LBAD_HIP(launch_compare_planes_generic(c->d_planes, c->capacity, c->count, c->n_sub, c->subfp_len, b.scan + (size_t)q * per * kPackedWords,
                                           per, range, index_base, d_scores, d_key, stream));
    return noErr;
}

// The runner of n packed queries (checked by the caller): the builders' blocks (build_packed), the same scans and selection,
// and, lags wanted, the alignment of the selected keys (a threshold's capacity <= 2^31 slots: it fits the alignment's 32-bit k).
// Two guards, each event where it is due: topk_ev behind the selection and in FRONT of the alignment -- a following call on
// another stream needs the score rows and the selection's words, and must not wait for the lags as well -- and pq_ev behind
// the last kernel that reads d_pq.  Both also behind what a failed call did launch.
OSStatus select_packed(LBAudioDetectiveCorpus* c, const uint32_t* d_rows, uint32_t n, uint32_t per, uint32_t range, const Selection& sel,
                       hipStream_t stream) {
    if (range == 0) range = c->subfp_len;
    PassGuard scratch(&c->topk_ev), built(&c->pq_ev);
    OSStatus st = scratch.wait();
    if (st == noErr) st = built.wait();
    if (st != noErr) return st;
    BuiltQueries b;
    st = build_packed(c, d_rows, n, per, range, sel.lags != nullptr, stream, b);
    if (st == noErr) st = c->count == 0 ? select_nothing(sel, n, stream) : reserve_selection(c, sel, n);
    if (st == noErr && c->count != 0)
        st = scan_select(c, n, sel, stream, b.fast ? b.scan : nullptr, [&](uint32_t q, float* d_scores, unsigned long long* d_key) {
            return scan_built_one(c, b, q, per, range, 0, d_scores, d_key, stream);
        });
    st = scratch.finish(stream, st);
    if (st == noErr && sel.lags && c->count != 0)
        st = align_keys_built(c, b.desc, b.words, n, per, range, (uint32_t)sel.slots(), sel.keys, sel.index_base, sel.lags, stream);
    return built.finish(stream, st);
}

// packed top-1: no score rows and no selection, the scans write the keys themselves; only d_pq is held
OSStatus packed_keys_impl(LBAudioDetectiveCorpus* c, const uint32_t* d_rows, uint32_t n, uint32_t per, uint32_t range,
                          uint64_t index_base, unsigned long long* keys, hipStream_t stream) {
    if (!c || !d_rows || !keys || n == 0 || per == 0) return kLBAudioDetectiveArgumentInvalid;
    if (index_base + c->count > 0x100000000ull) return kLBAudioDetectiveArgumentInvalid;
    if (!device_ready()) return kLBAudioDetectiveDeviceUnavailable;
    if (range == 0) range = c->subfp_len;   // LBAudioDetective.m:443-445
    PassGuard built(&c->pq_ev);
    OSStatus st = built.wait();
    if (st != noErr) return st;
    BuiltQueries b;
    st = build_packed(c, d_rows, n, per, range, false, stream, b);
    if (st != noErr) return built.finish(stream, st);
    if (c->ragged) {
        st = run_built_ragged(c, b.scan, n, per, range, index_base, nullptr, keys, stream);
    } else if (b.fast) {
        // the batch scan even for one query: it equals the single-query scan bit for bit
        st = hip_status(hipMemsetAsync(keys, 0, (size_t)n * sizeof(unsigned long long), stream), "keys", __LINE__);
        if (st == noErr)
            st = hip_status(launch_compare_planes_batch(c->d_planes, c->capacity, c->count, c->n_sub, b.scan, n, index_base, keys, stream),
                            "batch scan", __LINE__);
    } else {
        for (uint32_t q = 0; q < n && st == noErr; ++q) st = scan_built_one(c, b, q, per, range, index_base, nullptr, keys + q, stream);
    }
    return built.finish(stream, st);
}

// ---- the entry points' argument checks, each in its own order, in front of the runners -------------------------------------
OSStatus topk_keys_impl(LBAudioDetectiveCorpus* c, const LBAudioDetectiveFingerprintRef* qs, uint32_t n, uint32_t range, uint32_t k,
                        uint64_t index_base, unsigned long long* keys, hipStream_t stream) {
    if (!c || !qs || !keys || n == 0 || k == 0 || k > kTopKMax) return kLBAudioDetectiveArgumentInvalid;
    if (index_base + c->count > 0x100000000ull) return kLBAudioDetectiveArgumentInvalid;
    for (uint32_t i = 0; i < n; ++i)
        if (!qs[i] || qs[i]->length != c->subfp_len || qs[i]->count == 0) return kLBAudioDetectiveArgumentInvalid;
    Selection sel;
    sel.k = k; sel.index_base = index_base; sel.keys = keys;
    return select_handles(c, qs, n, range, sel, stream);
}

// what needs neither corpus nor device: a finite threshold above 0, at least one slot per row, n x capacity <= 2^31 slots
bool threshold_args_ok(uint32_t n, float threshold, uint64_t capacity) {
    return n != 0 && std::isfinite(threshold) && threshold > 0.0f && capacity != 0 && capacity <= 0x80000000ull &&
           (uint64_t)n * capacity <= 0x80000000ull;
}

Selection threshold_selection(float threshold, uint64_t capacity, uint64_t index_base, unsigned long long* keys,
                              unsigned long long* counts, int32_t* lags) {
    Selection sel;
    sel.by_threshold = true; sel.threshold = threshold; sel.capacity = capacity; sel.index_base = index_base;
    sel.keys = keys; sel.counts = counts; sel.lags = lags;
    return sel;
}

// The selection alone over a caller's rows of `count` scores, at most rows_max per launch, on a scratch of its own (not counted
// among a corpus' bytes for long: the stream is awaited and the scratch freed on return)
OSStatus keys_from_scores(const float* d_scores, uint64_t count, uint32_t n_rows, uint32_t rows_max, const Selection& sel, hipStream_t stream) {
    const uint32_t rows = n_rows < rows_max ? n_rows : rows_max;
    DeviceBuffer<void> scratch;
    OSStatus st = scratch.reserve(selection_scratch_bytes(sel, count, rows));
    if (st != noErr) return st;
    const char* what = sel.by_threshold ? "threshold selection" : "top-K selection";
    for (uint32_t r0 = 0; r0 < n_rows && st == noErr; r0 += rows)
        st = hip_status(launch_selection(sel, d_scores + (size_t)r0 * count, count, r0, n_rows - r0 < rows ? n_rows - r0 : rows, scratch, stream),
                        what, __LINE__);
    const OSStatus done = hip_status(hipStreamSynchronize(stream), what, __LINE__);
    return st != noErr ? st : done;
}

// (the threshold calls refuse bad scalars and NULL outputs before they look at the device, and the device before the corpus)
OSStatus threshold_keys_impl(LBAudioDetectiveCorpus* c, const LBAudioDetectiveFingerprintRef* qs, uint32_t n, uint32_t range,
                             float threshold, uint64_t capacity, uint64_t index_base, unsigned long long* keys,
                             unsigned long long* counts, hipStream_t stream) {
    if (!qs || !keys || !counts || !threshold_args_ok(n, threshold, capacity)) return kLBAudioDetectiveArgumentInvalid;
    for (uint32_t i = 0; i < n; ++i)
        if (!qs[i] || qs[i]->count == 0) return kLBAudioDetectiveArgumentInvalid;
    if (!device_ready()) return kLBAudioDetectiveDeviceUnavailable;
    if (!c || index_base + c->count > 0x100000000ull) return kLBAudioDetectiveArgumentInvalid;
    for (uint32_t i = 0; i < n; ++i)
        if (qs[i]->length != c->subfp_len) return kLBAudioDetectiveArgumentInvalid;
    return select_handles(c, qs, n, range, threshold_selection(threshold, capacity, index_base, keys, counts, nullptr), stream);
}

// ---- host-returning forms: the call's results in ONE block of the corpus' key buffer on the null stream (key_block_*), one
// read-back, then decoded -------------------------------------------------------------------------------------------------
OSStatus topk_host_impl(LBAudioDetectiveCorpus* c, const LBAudioDetectiveFingerprintRef* qs, uint32_t n, uint32_t range, uint32_t k,
                        SInt64* out_idx, Float32* out_scores, UInt32* out_counts) {
    if (!c || !qs || n == 0 || k == 0 || k > kTopKMax || !out_idx || !out_scores || !out_counts) return kLBAudioDetectiveArgumentInvalid;
    KeyBlock b;
    OSStatus st = key_block_reserve(c, (size_t)n * k, 0, &b);
    if (st != noErr) return st;
    st = topk_keys_impl(c, qs, n, range, k, 0, b.d_keys, nullptr);
    if (st != noErr) return key_block_failed(st);
    std::vector<unsigned long long> keys;
    st = key_block_read(b, b.n_keys, &keys);
    if (st != noErr) return st;
    for (uint32_t q = 0; q < n; ++q) {
        UInt32 got = 0;
        for (uint32_t i = 0; i < k; ++i) {
            LBAudioDetectiveCorpusDecodeKey(keys[(size_t)q * k + i], out_idx + (size_t)q * k + i, out_scores + (size_t)q * k + i);
            if (out_idx[(size_t)q * k + i] >= 0) ++got;
        }
        out_counts[q] = got;
    }
    return noErr;
}

// the n 64-bit counts ride as keys behind the n x capacity slots, the lags (want_lags) are the block's 32-bit values.  A list
// that was cut (count > capacity) is no error.
OSStatus threshold_host_impl(LBAudioDetectiveCorpus* c, const LBAudioDetectiveFingerprintRef* qs, uint32_t n, uint32_t range,
                             float threshold, uint64_t capacity, SInt64* out_idx, Float32* out_scores, SInt32* out_lags, bool want_lags,
                             UInt64* out_counts) {
    if (!qs || !out_idx || !out_scores || !out_counts || (want_lags && !out_lags) || !threshold_args_ok(n, threshold, capacity))
        return kLBAudioDetectiveArgumentInvalid;
    for (uint32_t i = 0; i < n; ++i)
        if (!qs[i] || qs[i]->count == 0 || (want_lags && qs[i]->count > 0x7FFFFFFFu)) return kLBAudioDetectiveArgumentInvalid;
    if (!device_ready()) return kLBAudioDetectiveDeviceUnavailable;
    if (!c) return kLBAudioDetectiveArgumentInvalid;
    const size_t slots = (size_t)n * capacity;
    KeyBlock b;
    OSStatus st = key_block_reserve(c, slots + n, want_lags ? slots : 0, &b);
    if (st != noErr) return st;
    st = threshold_keys_impl(c, qs, n, range, threshold, capacity, 0, b.d_keys, b.d_keys + slots, nullptr);
    if (st == noErr && want_lags && c->count != 0)
        st = align_keys_handles(c, qs, n, range, (uint32_t)capacity, b.d_keys, 0, reinterpret_cast<int32_t*>(b.d_words), nullptr);
    if (st != noErr) return key_block_failed(st);
    std::vector<unsigned long long> host;
    st = key_block_read(b, b.n_keys, &host);
    if (st != noErr) return st;
    const int32_t* lags = reinterpret_cast<const int32_t*>(host.data() + b.n_keys);
    for (size_t at = 0; at < slots; ++at) {
        LBAudioDetectiveCorpusDecodeKey(host[at], out_idx + at, out_scores + at);
        if (want_lags) out_lags[at] = out_idx[at] >= 0 && c->count != 0 ? lags[at] : 0;
    }
    for (uint32_t q = 0; q < n; ++q) out_counts[q] = host[slots + q];
    return noErr;
}

}  // namespace
}  // namespace lbad

extern "C" {

OSStatus LBAudioDetectiveCorpusQueryBatchThresholdKeysDevice(LBAudioDetectiveCorpusRef c, const LBAudioDetectiveFingerprintRef* inQueries,
                                                             UInt32 inCount, UInt32 inRange, Float32 inThreshold, UInt64 inCapacity,
                                                             UInt64 inIndexBase, void* outKeys, void* outCounts, void* inStream) {
    LBAD_GUARD_BEGIN
    return lbad::threshold_keys_impl(c, inQueries, inCount, inRange, inThreshold, inCapacity, inIndexBase,
                                     static_cast<unsigned long long*>(outKeys), static_cast<unsigned long long*>(outCounts),
                                     static_cast<hipStream_t>(inStream));
    LBAD_GUARD_END
}

OSStatus LBAudioDetectiveCorpusQueryBatchThreshold(LBAudioDetectiveCorpusRef c, const LBAudioDetectiveFingerprintRef* inQueries,
                                                   UInt32 inCount, UInt32 inRange, Float32 inThreshold, UInt64 inCapacity,
                                                   SInt64* outIndices, Float32* outScores, UInt64* outCounts) {
    LBAD_GUARD_BEGIN
    return lbad::threshold_host_impl(c, inQueries, inCount, inRange, inThreshold, inCapacity, outIndices, outScores, nullptr, false,
                                     outCounts);
    LBAD_GUARD_END
}

OSStatus LBAudioDetectiveCorpusQueryBatchThresholdAligned(LBAudioDetectiveCorpusRef c, const LBAudioDetectiveFingerprintRef* inQueries,
                                                          UInt32 inCount, UInt32 inRange, Float32 inThreshold, UInt64 inCapacity,
                                                          SInt64* outIndices, Float32* outScores, SInt32* outLags, UInt64* outCounts) {
    LBAD_GUARD_BEGIN
    return lbad::threshold_host_impl(c, inQueries, inCount, inRange, inThreshold, inCapacity, outIndices, outScores, outLags, true,
                                     outCounts);
    LBAD_GUARD_END
}

OSStatus LBAudioDetectiveCorpusQueryThreshold(LBAudioDetectiveCorpusRef c, LBAudioDetectiveFingerprintRef inQuery, UInt32 inRange,
                                              Float32 inThreshold, UInt64 inCapacity, SInt64* outIndices, Float32* outScores,
                                              UInt64* outCount) {
    LBAD_GUARD_BEGIN
    if (!inQuery) return kLBAudioDetectiveArgumentInvalid;
    return lbad::threshold_host_impl(c, &inQuery, 1, inRange, inThreshold, inCapacity, outIndices, outScores, nullptr, false, outCount);
    LBAD_GUARD_END
}

OSStatus LBAudioDetectiveCorpusQueryPackedThresholdKeysDevice(LBAudioDetectiveCorpusRef c, const void* inPackedQueries, UInt32 inCount,
                                                              UInt32 inSubfingerprintsPerQuery, UInt32 inRange, Float32 inThreshold,
                                                              UInt64 inCapacity, UInt64 inIndexBase, void* outKeys, void* outCounts,
                                                              void* outLags, void* inStream) {
    LBAD_GUARD_BEGIN
    if (!inPackedQueries || !outKeys || !outCounts || inSubfingerprintsPerQuery == 0 || !lbad::threshold_args_ok(inCount, inThreshold, inCapacity))
        return kLBAudioDetectiveArgumentInvalid;
    if (!lbad::device_ready()) return kLBAudioDetectiveDeviceUnavailable;
    if (!c || inIndexBase + c->count > 0x100000000ull) return kLBAudioDetectiveArgumentInvalid;
    return lbad::select_packed(c, static_cast<const uint32_t*>(inPackedQueries), inCount, inSubfingerprintsPerQuery, inRange,
                               lbad::threshold_selection(inThreshold, inCapacity, inIndexBase, static_cast<unsigned long long*>(outKeys),
                                                         static_cast<unsigned long long*>(outCounts), static_cast<int32_t*>(outLags)),
                               static_cast<hipStream_t>(inStream));
    LBAD_GUARD_END
}

OSStatus LBAudioDetectiveThresholdKeysFromScoresDevice(const Float32* inScores, UInt64 inCount, UInt32 inRows, Float32 inThreshold,
                                                       UInt64 inCapacity, UInt64 inIndexBase, void* outKeys, void* outCounts,
                                                       void* inStream) {
    LBAD_GUARD_BEGIN
    if (!inScores || !outKeys || !outCounts || !lbad::threshold_args_ok(inRows, inThreshold, inCapacity))
        return kLBAudioDetectiveArgumentInvalid;
    if (inCount > 0x100000000ull || inIndexBase + inCount > 0x100000000ull) return kLBAudioDetectiveArgumentInvalid;
    if (!lbad::device_ready()) return kLBAudioDetectiveDeviceUnavailable;
    return lbad::keys_from_scores(inScores, inCount, inRows, lbad::kThresholdRowsMax,
                                  lbad::threshold_selection(inThreshold, inCapacity, inIndexBase, static_cast<unsigned long long*>(outKeys),
                                                            static_cast<unsigned long long*>(outCounts), nullptr),
                                  static_cast<hipStream_t>(inStream));
    LBAD_GUARD_END
}

OSStatus LBAudioDetectiveCorpusQueryBatchTopKKeysDevice(LBAudioDetectiveCorpusRef c, const LBAudioDetectiveFingerprintRef* inQueries,
                                                        UInt32 inCount, UInt32 inRange, UInt32 inK, UInt64 inIndexBase,
                                                        void* outKeys, void* inStream) {
    LBAD_GUARD_BEGIN
    return lbad::topk_keys_impl(c, inQueries, inCount, inRange, inK, inIndexBase, static_cast<unsigned long long*>(outKeys),
                                static_cast<hipStream_t>(inStream));
    LBAD_GUARD_END
}

OSStatus LBAudioDetectiveCorpusQueryBatchTopK(LBAudioDetectiveCorpusRef c, const LBAudioDetectiveFingerprintRef* inQueries,
                                              UInt32 inCount, UInt32 inRange, UInt32 inK, SInt64* outIndices, Float32* outScores,
                                              UInt32* outCounts) {
    LBAD_GUARD_BEGIN
    return lbad::topk_host_impl(c, inQueries, inCount, inRange, inK, outIndices, outScores, outCounts);
    LBAD_GUARD_END
}

OSStatus LBAudioDetectiveCorpusQueryTopK(LBAudioDetectiveCorpusRef c, LBAudioDetectiveFingerprintRef inQuery, UInt32 inRange,
                                         UInt32 inK, SInt64* outIndices, Float32* outScores, UInt32* outCount) {
    LBAD_GUARD_BEGIN
    if (!inQuery) return kLBAudioDetectiveArgumentInvalid;
    return lbad::topk_host_impl(c, &inQuery, 1, inRange, inK, outIndices, outScores, outCount);
    LBAD_GUARD_END
}

OSStatus LBAudioDetectiveCorpusQueryPackedKeysDevice(LBAudioDetectiveCorpusRef c, const void* inPackedQueries, UInt32 inCount,
                                                     UInt32 inSubfingerprintsPerQuery, UInt32 inRange, UInt64 inIndexBase, void* outKeys,
                                                     void* inStream) {
    LBAD_GUARD_BEGIN
    return lbad::packed_keys_impl(c, static_cast<const uint32_t*>(inPackedQueries), inCount, inSubfingerprintsPerQuery, inRange,
                                  inIndexBase, static_cast<unsigned long long*>(outKeys), static_cast<hipStream_t>(inStream));
    LBAD_GUARD_END
}

OSStatus LBAudioDetectiveCorpusQueryPackedTopKKeysDevice(LBAudioDetectiveCorpusRef c, const void* inPackedQueries, UInt32 inCount,
                                                         UInt32 inSubfingerprintsPerQuery, UInt32 inRange, UInt32 inK,
                                                         UInt64 inIndexBase, void* outKeys, void* outLags, void* inStream) {
    LBAD_GUARD_BEGIN
    if (!c || !inPackedQueries || !outKeys || inCount == 0 || inSubfingerprintsPerQuery == 0 || inK == 0 || inK > lbad::kTopKMax)
        return kLBAudioDetectiveArgumentInvalid;
    if (inIndexBase + c->count > 0x100000000ull) return kLBAudioDetectiveArgumentInvalid;
    if (!lbad::device_ready()) return kLBAudioDetectiveDeviceUnavailable;
    lbad::Selection sel;
    sel.k = inK; sel.index_base = inIndexBase; sel.keys = static_cast<unsigned long long*>(outKeys); sel.lags = static_cast<int32_t*>(outLags);
    return lbad::select_packed(c, static_cast<const uint32_t*>(inPackedQueries), inCount, inSubfingerprintsPerQuery, inRange, sel,
                               static_cast<hipStream_t>(inStream));
    LBAD_GUARD_END
}

OSStatus LBAudioDetectiveTopKKeysFromScoresDevice(const Float32* inScores, UInt64 inCount, UInt32 inRows, UInt32 inK,
                                                  UInt64 inIndexBase, void* outKeys, void* inStream) {
    LBAD_GUARD_BEGIN
    if (!inScores || !outKeys || inRows == 0 || inK == 0 || inK > lbad::kTopKMax) return kLBAudioDetectiveArgumentInvalid;
    if (inCount > 0x100000000ull || inIndexBase + inCount > 0x100000000ull) return kLBAudioDetectiveArgumentInvalid;
    lbad::Selection sel;
    sel.k = inK; sel.index_base = inIndexBase; sel.keys = static_cast<unsigned long long*>(outKeys);
    return lbad::keys_from_scores(inScores, inCount, inRows, 64, sel, static_cast<hipStream_t>(inStream));   // (64 rows bound the scratch: about 11 MiB)
    LBAD_GUARD_END
}

}  // extern "C"
