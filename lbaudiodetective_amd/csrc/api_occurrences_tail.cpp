// api_occurrences_tail.cpp -- the tail occurrences (k_occurrences_tail.hip): the batch occurrences' rows (api_occurrences_batch.cpp)
// with only the cells a push has completed -- per recording those whose entry ends inside its newest sub-fingerprints, their number
// read on the device.  The plan is occurrences_tail_plan's, here and in the debug symbol; the corpus' checks, the events, the staging
// buffer and the scratch are the batch call's (recording_pass.cpp), which stays as it is.
// The peaks form (k_occurrences_tail_peaks.hip) is the same path: its bound is 62, its plan occurrences_tail_plan's at the bound + 2
// (tail_plan below, for the call and the debug symbol alike), and its chunks go to launch_occurrences_tail_peaks_chunk.
#include "internal.hpp"

#include <cmath>

namespace lbad {
namespace {

// a cell of this call is one offset of an entry not longer than the recording: ONE tile, whatever the lengths
uint64_t tail_tiles(uint32_t, uint32_t, uint32_t) { return 1; }
const PassFamily kFamily = {tail_tiles, occurrences_chunk_entries, occurrences_block_entries};

// which list: every cell a push completed, or the peaks among the cells it completed one sub-fingerprint ago (and, final, the newest)
struct TailForm {
    bool peaks = false;
    bool final = false;
    uint32_t bound() const { return peaks ? LBAD_OCCURRENCES_TAIL_PEAKS_MAX_NEW : LBAD_OCCURRENCES_TAIL_MAX_NEW; }
};

// THE plan of either form: the peaks form's recordings take two more lanes, the cells that only supply a neighbour's value
bool tail_plan(const TailForm& form, uint32_t recordings, uint32_t per, uint32_t ne_min, uint32_t ne_max, uint64_t entries, uint32_t max_new,
               uint64_t limit_bytes, OccurrencesTailPlan* plan) {
    return occurrences_tail_plan(recordings, per, ne_min, ne_max, entries, form.peaks ? max_new + 2u : max_new, limit_bytes, plan);
}

// what needs neither handle nor device: the batch call's checks, the new counts and their bound
bool tail_args_ok(const TailForm& form, const void* c, const void* d_rows, const void* d_new, const void* keys, const void* counts,
                  uint32_t recordings, uint32_t per, uint32_t max_new, float threshold, uint64_t capacity, uint64_t index_base) {
    return c && d_rows && d_new && (reinterpret_cast<uintptr_t>(d_new) & 3u) == 0 && keys && counts && max_new != 0 &&
           max_new <= form.bound() && recordings != 0 && per != 0 && (uint64_t)recordings * per <= 0x7FFFFFFFull &&
           std::isfinite(threshold) && threshold > 0.0f && capacity != 0 && capacity <= 0x80000000ull &&
           (uint64_t)recordings * capacity <= 0x80000000ull && index_base <= 0x100000000ull;
}

OSStatus zero_outputs(uint32_t recordings, uint64_t capacity, unsigned long long* keys, int32_t* lags, unsigned long long* counts,
                      hipStream_t stream) {
    const size_t slots = (size_t)recordings * capacity;
    LBAD_HIP(hipMemsetAsync(keys, 0, slots * sizeof(unsigned long long), stream));
    if (lags) LBAD_HIP(hipMemsetAsync(lags, 0, slots * sizeof(int32_t), stream));
    if (counts) LBAD_HIP(hipMemsetAsync(counts, 0, (size_t)recordings * sizeof(unsigned long long), stream));
    return noErr;
}

// everything behind the wait, on the call's stream: the zeros, then pass by pass the recordings' rows and the compaction -- one
// chunk of the whole corpus for several recordings, entry chunks and the carried total for one
OSStatus tail_launch(LBAudioDetectiveCorpus* c, const TailForm& form, const OccurrencesTailPlan& plan, OccurrencesCall call, const uint32_t* d_rows,
                     const uint32_t* d_new, uint32_t max_new, uint32_t recordings, unsigned long long* keys, int32_t* lags,
                     unsigned long long* counts) {
    const uint32_t per = call.n_query;
    if (c->append_event.ev) LBAD_HIP(hipStreamWaitEvent(call.stream, c->append_event, 0));
    OSStatus st = zero_outputs(recordings, call.capacity, keys, lags, nullptr, call.stream);
    if (st != noErr) return st;
    for (uint32_t r0 = 0; r0 < recordings; r0 += plan.recordings_per_pass) {
        const uint32_t n = recordings - r0 < plan.recordings_per_pass ? recordings - r0 : plan.recordings_per_pass;
        LBAD_HIP(launch_build_query_rows(d_rows + (size_t)r0 * per * kPackedWords, n, per, c->subfp_len, true, c->d_pq, nullptr, call.stream));
        call.d_keys = keys + (size_t)r0 * call.capacity;
        call.d_lags = lags ? lags + (size_t)r0 * call.capacity : nullptr;
        LBAD_HIP(pass_chunks(c->count, plan.entries_per_chunk, [&](uint64_t e0, uint64_t m) {
            if (form.peaks)
                return launch_occurrences_tail_peaks_chunk(call, plan, n, d_new + r0, max_new, form.final, c->d_join_scratch, e0, m,
                                                           e0 == 0 ? 1u : 0u, counts + r0);
            return launch_occurrences_tail_chunk(call, plan, n, d_new + r0, max_new, c->d_join_scratch, e0, m, e0 == 0 ? 1u : 0u, counts + r0);
        }));
        // a pass of one recording: the running total behind the last chunk is the recording's count
        if (plan.recordings_per_pass == 1)
            LBAD_HIP(hipMemcpyAsync(counts + r0, c->d_join_scratch.get(), sizeof(unsigned long long), hipMemcpyDeviceToDevice, call.stream));
    }
    return noErr;
}

OSStatus tail_impl(const TailForm& form, LBAudioDetectiveCorpus* c, const uint32_t* d_rows, uint32_t recordings, uint32_t per, const uint32_t* d_new,
                   uint32_t max_new, uint32_t range, float threshold, uint64_t capacity, uint64_t index_base, unsigned long long* keys,
                   int32_t* lags, unsigned long long* counts, hipStream_t stream) {
    if (!tail_args_ok(form, c, d_rows, d_new, keys, counts, recordings, per, max_new, threshold, capacity, index_base))
        return kLBAudioDetectiveArgumentInvalid;
    if (!device_ready()) return kLBAudioDetectiveDeviceUnavailable;
    // what the corpus decides (pass_plan's checks, the batch call's), before anything is reserved or launched
    PassQuery pq;
    pq.d_rows = d_rows; pq.per = per; pq.range = range;
    PassPlan single;
    OSStatus st = pass_plan(c, pq, index_base, kFamily, &single);
    if (st != noErr) return st;
    OccurrencesTailPlan plan;
    if (!tail_plan(form, recordings, per, single.call.ne_min, c->ne_max, c->count, max_new, c->join_scratch_limit, &plan))
        return kLBAudioDetectiveArgumentInvalid;
    // nothing to compare, or no entry with a complete position inside the recordings: zeros
    if (c->count == 0 || !single.any) return zero_outputs(recordings, capacity, keys, lags, counts, stream);
    PassGuard guard(c, pq, false);
    st = guard.wait();                                     // (the scratch and the staged rows are the previous call's until then)
    if (st == noErr) st = c->d_join_scratch.reserve(plan.scratch_bytes);
    if (st == noErr) st = c->d_pq.reserve((size_t)plan.recordings_per_pass * per * kPackedWords);
    if (st != noErr) return st;
    OccurrencesCall call;
    static_cast<OcPassCall&>(call) = single.call;
    call.tiles = 1; call.stream = stream;
    call.d_qwords = c->d_pq;
    call.threshold = threshold; call.peaks = false; call.capacity = capacity; call.index_base = index_base;
    return guard.finish(stream, tail_launch(c, form, plan, call, d_rows, d_new, max_new, recordings, keys, lags, counts));
}

OSStatus tail_debug_plan(const TailForm& form, UInt32 inRecordings, UInt32 inSubfingerprints, UInt32 inShortestEntry, UInt32 inLongestEntry,
                         UInt64 inEntries, UInt32 inMaxNew, UInt64 inScratchLimit, UInt32* outLanes, UInt32* outRecordingsPerWorkgroup,
                         UInt32* outWindowRecords, UInt64* outLdsBytes, UInt32* outRecordingsPerPass, UInt64* outEntriesPerChunk,
                         UInt64* outScratchBytes) {
    if (!outLanes || !outRecordingsPerWorkgroup || !outWindowRecords || !outLdsBytes || !outRecordingsPerPass || !outEntriesPerChunk ||
        !outScratchBytes || inRecordings == 0 || inSubfingerprints == 0 || (uint64_t)inRecordings * inSubfingerprints > 0x7FFFFFFFull ||
        inShortestEntry > inLongestEntry || inLongestEntry > LBAD_OCCURRENCES_MAX_ENTRY_SUBFINGERPRINTS ||
        (inEntries != 0 && inShortestEntry == 0) || inEntries > 0x100000000ull || inMaxNew == 0 || inMaxNew > form.bound())
        return kLBAudioDetectiveArgumentInvalid;
    OccurrencesTailPlan plan;
    if (!tail_plan(form, inRecordings, inSubfingerprints, inShortestEntry, inLongestEntry, inEntries, inMaxNew, inScratchLimit, &plan))
        return kLBAudioDetectiveArgumentInvalid;
    *outLanes = plan.lanes;
    *outRecordingsPerWorkgroup = plan.recordings_per_workgroup;
    *outWindowRecords = plan.window_records;
    *outLdsBytes = plan.lds_bytes;
    *outRecordingsPerPass = plan.recordings_per_pass;
    *outEntriesPerChunk = plan.entries_per_chunk;
    *outScratchBytes = plan.scratch_bytes;
    return noErr;
}

}  // namespace
}  // namespace lbad

extern "C" {

OSStatus LBAudioDetectiveCorpusQueryPackedOccurrencesTailBatchKeysDevice(LBAudioDetectiveCorpusRef c, const void* inPackedQueries,
                                                                         UInt32 inRecordings, UInt32 inSubfingerprints,
                                                                         const void* inNewCounts, UInt32 inMaxNew, UInt32 inRange,
                                                                         Float32 inThreshold, UInt64 inCapacity, UInt64 inIndexBase,
                                                                         void* outKeys, void* outLags, void* outCounts, void* inStream) {
    LBAD_GUARD_BEGIN
    return lbad::tail_impl(lbad::TailForm(), c, static_cast<const uint32_t*>(inPackedQueries), inRecordings, inSubfingerprints,
                           static_cast<const uint32_t*>(inNewCounts), inMaxNew, inRange, inThreshold, inCapacity, inIndexBase,
                           static_cast<unsigned long long*>(outKeys), static_cast<int32_t*>(outLags),
                           static_cast<unsigned long long*>(outCounts), static_cast<hipStream_t>(inStream));
    LBAD_GUARD_END
}

OSStatus LBAudioDetectiveDebugOccurrencesTailPlan(UInt32 inRecordings, UInt32 inSubfingerprints, UInt32 inShortestEntry, UInt32 inLongestEntry,
                                                  UInt64 inEntries, UInt32 inMaxNew, UInt64 inScratchLimit, UInt32* outLanes,
                                                  UInt32* outRecordingsPerWorkgroup, UInt32* outWindowRecords, UInt64* outLdsBytes,
                                                  UInt32* outRecordingsPerPass, UInt64* outEntriesPerChunk, UInt64* outScratchBytes) {
    return lbad::tail_debug_plan(lbad::TailForm(), inRecordings, inSubfingerprints, inShortestEntry, inLongestEntry, inEntries, inMaxNew,
                                 inScratchLimit, outLanes, outRecordingsPerWorkgroup, outWindowRecords, outLdsBytes, outRecordingsPerPass,
                                 outEntriesPerChunk, outScratchBytes);
}

OSStatus LBAudioDetectiveCorpusQueryPackedOccurrencesTailPeaksBatchKeysDevice(LBAudioDetectiveCorpusRef c, const void* inPackedQueries,
                                                                              UInt32 inRecordings, UInt32 inSubfingerprints,
                                                                              const void* inNewCounts, UInt32 inMaxNew, UInt32 inFinal,
                                                                              UInt32 inRange, Float32 inThreshold, UInt64 inCapacity,
                                                                              UInt64 inIndexBase, void* outKeys, void* outLags,
                                                                              void* outCounts, void* inStream) {
    LBAD_GUARD_BEGIN
    lbad::TailForm form;
    form.peaks = true;
    form.final = inFinal != 0;
    return lbad::tail_impl(form, c, static_cast<const uint32_t*>(inPackedQueries), inRecordings, inSubfingerprints,
                           static_cast<const uint32_t*>(inNewCounts), inMaxNew, inRange, inThreshold, inCapacity, inIndexBase,
                           static_cast<unsigned long long*>(outKeys), static_cast<int32_t*>(outLags),
                           static_cast<unsigned long long*>(outCounts), static_cast<hipStream_t>(inStream));
    LBAD_GUARD_END
}

OSStatus LBAudioDetectiveDebugOccurrencesTailPeaksPlan(UInt32 inRecordings, UInt32 inSubfingerprints, UInt32 inShortestEntry,
                                                       UInt32 inLongestEntry, UInt64 inEntries, UInt32 inMaxNew, UInt64 inScratchLimit,
                                                       UInt32* outLanes, UInt32* outRecordingsPerWorkgroup, UInt32* outWindowRecords,
                                                       UInt64* outLdsBytes, UInt32* outRecordingsPerPass, UInt64* outEntriesPerChunk,
                                                       UInt64* outScratchBytes) {
    lbad::TailForm form;
    form.peaks = true;
    return lbad::tail_debug_plan(form, inRecordings, inSubfingerprints, inShortestEntry, inLongestEntry, inEntries, inMaxNew, inScratchLimit,
                                 outLanes, outRecordingsPerWorkgroup, outWindowRecords, outLdsBytes, outRecordingsPerPass,
                                 outEntriesPerChunk, outScratchBytes);
}

}  // extern "C"
