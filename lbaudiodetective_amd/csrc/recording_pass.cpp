// recording_pass.cpp -- the host side that the three families of the occurrences pass share (api_occurrences.cpp,
// api_recording.cpp, api_timeline.cpp): the plan of a call, the staging of its query, the events that keep one call's scratch
// from the next call on another stream, the host path of the list forms that return rows of keys (api_occurrences_batch.cpp,
// api_occurrences_tail.cpp), and the key block of the host-returning forms.  internal.hpp states each piece.
#include "internal.hpp"

#include <cmath>
#include <cstring>

namespace lbad {

OSStatus pass_plan(const LBAudioDetectiveCorpus* c, const PassQuery& q, uint64_t index_base, const PassFamily& fam, PassPlan* plan) {
    const uint32_t n_query = q.fp ? q.fp->count : q.per;
    if (!c->ragged || (q.fp ? q.fp->length : c->subfp_len) != c->subfp_len || n_query == 0 || n_query > 0x7FFFFFFFu ||
        c->ne_max > LBAD_OCCURRENCES_MAX_ENTRY_SUBFINGERPRINTS || index_base + c->count > 0x100000000ull)
        return kLBAudioDetectiveArgumentInvalid;
    *plan = PassPlan();
    OcPassCall& call = plan->call;
    call.d_recs = c->d_recs; call.d_off = c->d_off; call.ne_max = c->ne_max; call.subfp_len = c->subfp_len;
    call.range = q.range ? q.range : c->subfp_len; call.n_query = n_query; call.tiles = 1;
    if (c->count == 0) return noErr;
    call.ne_min = c->len_hist.begin()->first;
    call.tiles = fam.tiles(n_query, call.ne_min, c->ne_max);
    const uint64_t limit = c->join_scratch_limit ? c->join_scratch_limit : kJoinScratchDefault;
    const uint64_t chunk = fam.chunk_entries(call.tiles, limit), block = fam.block_entries();
    if (chunk == 0) return kLBAudioDetectiveArgumentInvalid;          // the limit holds no block of entries at this query length
    plan->chunk = chunk < c->count ? chunk : (c->count + block - 1) / block * block;
    plan->any = call.ne_min <= n_query;
    return noErr;
}

PassGuard::PassGuard(LBAudioDetectiveCorpus* c, const PassQuery& q, bool topk) {
    ev[0] = &c->join_ev;
    ev[1] = q.fp ? &c->align_ev : &c->pq_ev;
    ev[2] = topk ? &c->topk_ev : nullptr;
}

OSStatus PassGuard::wait() {
    OSStatus st = noErr;
    for (Event* e : ev)
        if (e && st == noErr) st = e->wait_or_create();
    return st;
}

OSStatus PassGuard::finish(hipStream_t stream, OSStatus st) {
    for (Event* e : ev) {
        const OSStatus rec = e ? e->record(stream) : noErr;
        if (st == noErr) st = rec;
    }
    return st;
}

OSStatus pass_stage_query(LBAudioDetectiveCorpus* c, const PassQuery& q, hipStream_t stream, OcPassCall* call) {
    OSStatus st;
    if (q.fp) {
        std::vector<uint32_t> words;
        build_align_query(q.fp, true, words);
        st = c->align_q.reserve(words.size());
        if (st != noErr) return st;
        std::memcpy(c->align_q.host, words.data(), words.size() * sizeof(uint32_t));
        call->d_qwords = c->align_q.dev;
        st = hip_status(hipMemcpyAsync(c->align_q.dev, c->align_q.host, words.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream),
                        "query words", __LINE__);
    } else {
        st = c->d_pq.reserve((size_t)q.per * kPackedWords);
        if (st != noErr) return st;
        call->d_qwords = c->d_pq;
        st = hip_status(launch_build_query_rows(q.d_rows, 1, q.per, c->subfp_len, true, c->d_pq, nullptr, stream), "query words", __LINE__);
    }
    call->stream = stream;
    if (st == noErr && c->append_event.ev) LBAD_HIP(hipStreamWaitEvent(stream, c->append_event, 0));
    return st;
}

bool key_rows_args_ok(const void* c, const void* d_rows, const void* keys, const void* counts, uint32_t recordings, uint32_t per,
                      float threshold, uint64_t capacity, uint64_t index_base) {
    return c && d_rows && keys && counts && recordings != 0 && per != 0 && (uint64_t)recordings * per <= 0x7FFFFFFFull &&
           std::isfinite(threshold) && threshold > 0.0f && capacity != 0 && capacity <= 0x80000000ull &&
           (uint64_t)recordings * capacity <= 0x80000000ull && index_base <= 0x100000000ull;
}

OSStatus zero_key_rows(uint32_t recordings, uint64_t slots, unsigned long long* keys, int32_t* lags, unsigned long long* counts,
                       hipStream_t stream) {
    const size_t n = (size_t)recordings * slots;
    LBAD_HIP(hipMemsetAsync(keys, 0, n * sizeof(unsigned long long), stream));
    if (lags) LBAD_HIP(hipMemsetAsync(lags, 0, n * sizeof(int32_t), stream));
    if (counts) LBAD_HIP(hipMemsetAsync(counts, 0, (size_t)recordings * sizeof(unsigned long long), stream));
    return noErr;
}

namespace {

// everything behind the wait, on the call's stream
OSStatus key_rows_launch(LBAudioDetectiveCorpus* c, const KeyRowsPasses& passes, OccurrencesCall call, const KeyRows& rows,
                         const KeyRowsChunk& chunk) {
    const uint32_t per = call.n_query;
    if (c->append_event.ev) LBAD_HIP(hipStreamWaitEvent(call.stream, c->append_event, 0));
    OSStatus st = zero_key_rows(rows.recordings, call.capacity, rows.keys, rows.lags, nullptr, call.stream);
    if (st != noErr) return st;
    for (uint32_t r0 = 0; r0 < rows.recordings; r0 += passes.recordings_per_pass) {
        const uint32_t n = rows.recordings - r0 < passes.recordings_per_pass ? rows.recordings - r0 : passes.recordings_per_pass;
        LBAD_HIP(launch_build_query_rows(rows.d_rows + (size_t)r0 * per * kPackedWords, n, per, c->subfp_len, true, c->d_pq, nullptr,
                                         call.stream));
        call.d_keys = rows.keys + (size_t)r0 * call.capacity;
        call.d_lags = rows.lags ? rows.lags + (size_t)r0 * call.capacity : nullptr;
        LBAD_HIP(pass_chunks(c->count, passes.entries_per_chunk, [&](uint64_t e0, uint64_t m) {
            return chunk(call, r0, n, e0, m, e0 == 0 ? 1u : 0u, rows.counts + r0);
        }));
        // a pass of one recording: the running total behind the last chunk is the recording's count
        if (passes.recordings_per_pass == 1)
            LBAD_HIP(hipMemcpyAsync(rows.counts + r0, c->d_join_scratch.get(), sizeof(unsigned long long), hipMemcpyDeviceToDevice,
                                    call.stream));
    }
    return noErr;
}

}  // namespace

OSStatus key_rows_call(LBAudioDetectiveCorpus* c, const PassQuery& q, const PassPlan& single, const KeyRowsPasses& passes, uint64_t tiles,
                       const KeyRows& rows, const KeyRowsChunk& chunk) {
    PassGuard guard(c, q, false);
    OSStatus st = guard.wait();                            // (the scratch and the staged rows are the previous call's until then)
    if (st == noErr) st = c->d_join_scratch.reserve(passes.scratch_bytes);
    if (st == noErr) st = c->d_pq.reserve((size_t)passes.recordings_per_pass * q.per * kPackedWords);
    if (st != noErr) return st;
    OccurrencesCall call;
    static_cast<OcPassCall&>(call) = single.call;
    call.tiles = tiles; call.stream = rows.stream;
    call.d_qwords = c->d_pq;
    call.threshold = rows.threshold; call.peaks = rows.peaks; call.capacity = rows.capacity; call.index_base = rows.index_base;
    return guard.finish(rows.stream, key_rows_launch(c, passes, call, rows, chunk));
}

OSStatus key_block_reserve(LBAudioDetectiveCorpus* c, size_t n_keys, size_t n_words, KeyBlock* b) {
    OSStatus st = c->topk_ev.wait();
    if (st == noErr) st = c->d_topk_keys.reserve(n_keys + (n_words + 1) / 2);
    if (st != noErr) return st;
    b->d_keys = c->d_topk_keys;
    b->d_words = n_words ? reinterpret_cast<uint32_t*>(b->d_keys + n_keys) : nullptr;
    b->n_keys = n_keys;
    b->n_words = n_words;
    return noErr;
}

OSStatus key_block_read(const KeyBlock& b, size_t m, std::vector<unsigned long long>* host) {
    // (the whole block holds n_words values, which need not be n_keys: counts or offsets may ride among the keys)
    host->assign(m + ((m == b.n_keys ? b.n_words : (b.d_words ? m : 0)) + 1) / 2, 0ull);
    if (m == b.n_keys) {
        LBAD_HIP(hipMemcpy(host->data(), b.d_keys, host->size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    } else if (m) {
        LBAD_HIP(hipMemcpy(host->data(), b.d_keys, m * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        if (b.d_words) LBAD_HIP(hipMemcpy(host->data() + m, b.d_words, m * sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    return noErr;
}

OSStatus key_block_failed(OSStatus st) {
    (void)hipStreamSynchronize(nullptr);
    return st;
}

}  // namespace lbad
