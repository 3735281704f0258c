// api_occurrences_tail.cpp -- the tail occurrences (k_occurrences_tail.hip): the batch occurrences' rows (api_occurrences_batch.cpp)
// with only the cells a push has completed -- per recording those whose entry ends inside its newest sub-fingerprints, their number
// read on the device.  The plan is occurrences_tail_plan's, here and in the debug symbol; the corpus' checks, the events, the staging
// buffer and the scratch are the batch call's (recording_pass.cpp), which stays as it is.
// The argument checks, the zeros and the pass loop are recording_pass.cpp's for every list of key rows (key_rows_call).
// The peaks form (the kernels' PEAKS instances) is the same path: its bound is 62, its plan occurrences_tail_plan's at the bound + 2
// (tail_plan below, for the call and the debug symbol alike), and TailForm goes with every chunk to launch_occurrences_tail_chunk.
#include "internal.hpp"

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
    return key_rows_args_ok(c, d_rows, keys, counts, recordings, per, threshold, capacity, index_base) && d_new &&
           (reinterpret_cast<uintptr_t>(d_new) & 3u) == 0 && max_new != 0 && max_new <= form.bound();
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
    if (c->count == 0 || !single.any) return zero_key_rows(recordings, capacity, keys, lags, counts, stream);
    KeyRows rows;
    rows.d_rows = d_rows; rows.recordings = recordings; rows.threshold = threshold; rows.capacity = capacity; rows.index_base = index_base;
    rows.keys = keys; rows.lags = lags; rows.counts = counts; rows.stream = stream;
    const KeyRowsPasses passes = {plan.recordings_per_pass, plan.entries_per_chunk, plan.scratch_bytes};
    return key_rows_call(c, pq, single, passes, 1, rows,
                         [&](const OccurrencesCall& call, uint32_t r0, uint32_t n, uint64_t e0, uint64_t m, uint32_t first,
                             unsigned long long* d_counts) {
                             return launch_occurrences_tail_chunk(call, plan, n, d_new + r0, max_new, form.peaks, form.final, c->d_join_scratch,
                                                                  e0, m, first, d_counts);
                         });
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
