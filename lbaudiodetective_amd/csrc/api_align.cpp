// api_align.cpp -- where corpus matches align: the best sliding offset of a (query, entry) pair (k_align.hip), behind the
// top-1 and top-K queries, on keys the caller holds, and as the whole score profile of one pair.
#include "internal.hpp"

#include <cstring>

namespace lbad {
namespace {

// (every entry point first waits for align_ev: the previous alignment's kernels may still read / write the scratch, on
// whatever stream they ran)

AlignSource source(const LBAudioDetectiveCorpus* c, uint32_t range) {
    AlignSource s;
    s.ragged = c->ragged;
    s.recs = c->d_recs;
    s.off = c->d_off;
    s.planes = c->d_planes;
    s.stride = c->capacity;
    s.count = c->count;
    s.n_sub = c->n_sub;
    s.subfp_len = c->subfp_len;
    s.range = range ? range : c->subfp_len;    // LBAudioDetective.m:443-445
    return s;
}

// n1 - n2 + 1 of a query of nq sub-fingerprints against the longest / shortest entry: a bound over every pair
uint64_t max_offsets(const LBAudioDetectiveCorpus* c, uint64_t nq) {
    uint64_t lo = c->n_sub, hi = c->n_sub;
    if (c->ragged) {
        if (c->len_hist.empty()) return 1;
        lo = c->len_hist.begin()->first;
        hi = c->len_hist.rbegin()->first;
    }
    const uint64_t a = hi > nq ? hi - nq : 0, b = nq > lo ? nq - lo : 0;
    return (a > b ? a : b) + 1;
}

// the checks that need no device: handles, counts, pointers
bool queries_ok(const LBAudioDetectiveFingerprintRef* qs, uint32_t n) {
    if (!qs || n == 0) return false;
    for (uint32_t i = 0; i < n; ++i)
        if (!qs[i] || qs[i]->count == 0 || qs[i]->count > 0x7FFFFFFFu) return false;    // (a lag is a signed 32-bit offset)
    return true;
}

// ... and those that need the corpus
bool corpus_ok(const LBAudioDetectiveCorpus* c, const LBAudioDetectiveFingerprintRef* qs, uint32_t n) {
    if (!c || (c->ragged && c->ne_max > 0x7FFFFFFFu)) return false;
    for (uint32_t i = 0; i < n; ++i)
        if (qs[i]->length != c->subfp_len) return false;
    return true;
}

// the queries' words and their table to the device on `stream`: n (first sub-fingerprint, count) pairs, padded to 32 bytes,
// then the build_align_query blocks
OSStatus stage_queries(LBAudioDetectiveCorpus* c, const LBAudioDetectiveFingerprintRef* qs, uint32_t n, const uint2** d_desc,
                       const uint32_t** d_words, hipStream_t stream) {
    const size_t desc_words = ((size_t)2 * n + 7) & ~(size_t)7;
    std::vector<uint32_t> all(desc_words, 0u);
    uint64_t first = 0;
    for (uint32_t i = 0; i < n; ++i) {
        all[2 * i] = (uint32_t)first;
        all[2 * i + 1] = qs[i]->count;
        first += qs[i]->count;
    }
    if (first > 0xFFFFFFFFull) return kLBAudioDetectiveArgumentInvalid;
    for (uint32_t i = 0; i < n; ++i) build_align_query(qs[i], c->ragged, all);
    const size_t bytes = all.size() * sizeof(uint32_t);
    OSStatus st = c->align_q.reserve(all.size());
    if (st != noErr) return st;
    std::memcpy(c->align_q.host, all.data(), bytes);
    LBAD_HIP(hipMemcpyAsync(c->align_q.dev, c->align_q.host, bytes, hipMemcpyHostToDevice, stream));
    *d_desc = reinterpret_cast<const uint2*>(c->align_q.dev.get());
    *d_words = c->align_q.dev + desc_words;
    return noErr;
}

// the launch alone: queries whose words and table are on the device, max_off a bound of n1 - n2 + 1 over the pairs
OSStatus align_launch(LBAudioDetectiveCorpus* c, const uint2* d_desc, const uint32_t* d_words, uint32_t n, uint64_t max_off, uint32_t range,
                      uint32_t k, const unsigned long long* keys, uint64_t index_base, int32_t* lags, float* scores, hipStream_t stream) {
    const uint64_t pairs = (uint64_t)n * k;
    if (align_parts(pairs, max_off) > 1) {
        OSStatus st = c->d_align_best.reserve(pairs);
        if (st != noErr) return st;
    }
    LBAD_HIP(launch_align_keys(source(c, range), d_words, d_desc, n, k, keys, index_base, max_off, c->d_align_best, lags, scores, stream));
    return noErr;
}

// lags (and scores) of n x k keys on `stream`; the caller has waited for align_ev and records it afterwards
OSStatus align_keys_impl(LBAudioDetectiveCorpus* c, const LBAudioDetectiveFingerprintRef* qs, uint32_t n, uint32_t range, uint32_t k,
                         const unsigned long long* keys, uint64_t index_base, int32_t* lags, float* scores, hipStream_t stream) {
    const uint2* d_desc = nullptr;
    const uint32_t* d_words = nullptr;
    OSStatus st = stage_queries(c, qs, n, &d_desc, &d_words, stream);
    if (st != noErr) return st;
    uint64_t max_off = 1;
    for (uint32_t i = 0; i < n; ++i) {
        const uint64_t m = max_offsets(c, qs[i]->count);
        max_off = m > max_off ? m : max_off;
    }
    return align_launch(c, d_desc, d_words, n, max_off, range, k, keys, index_base, lags, scores, stream);
}

}  // namespace

OSStatus align_keys_built(LBAudioDetectiveCorpus* c, const uint2* d_desc, const uint32_t* d_words, uint32_t n, uint32_t per,
                          uint32_t range, uint32_t k, const unsigned long long* keys, uint64_t index_base, int32_t* lags,
                          hipStream_t stream) {
    if (!c || per == 0 || per > 0x7FFFFFFFu || (c->ragged && c->ne_max > 0x7FFFFFFFu)) return kLBAudioDetectiveArgumentInvalid;
    OSStatus st = c->align_ev.wait_or_create();       // (the per-pair maxima of a split launch are the previous alignment's until then)
    if (st == noErr) st = align_launch(c, d_desc, d_words, n, max_offsets(c, per), range, k, keys, index_base, lags, nullptr, stream);
    if (st != noErr) return st;
    return c->align_ev.record(stream);
}

// the same for queries given as handles (any k: the threshold queries align as many slots as a row has)
OSStatus align_keys_handles(LBAudioDetectiveCorpus* c, const LBAudioDetectiveFingerprintRef* qs, uint32_t n, uint32_t range, uint32_t k,
                            const unsigned long long* keys, uint64_t index_base, int32_t* lags, hipStream_t stream) {
    if (!queries_ok(qs, n) || k == 0 || !keys || !lags || !corpus_ok(c, qs, n)) return kLBAudioDetectiveArgumentInvalid;
    OSStatus st = c->align_ev.wait_or_create();
    if (st == noErr) st = align_keys_impl(c, qs, n, range, k, keys, index_base, lags, nullptr, stream);
    if (st != noErr) return st;
    return c->align_ev.record(stream);
}

}  // namespace lbad

extern "C" {

OSStatus LBAudioDetectiveCorpusAlignKeysDevice(LBAudioDetectiveCorpusRef c, const LBAudioDetectiveFingerprintRef* inQueries,
                                               UInt32 inCount, UInt32 inRange, UInt32 inK, const void* inKeys, UInt64 inIndexBase,
                                               void* outLags, void* outScores, void* inStream) {
    LBAD_GUARD_BEGIN
    if (!lbad::queries_ok(inQueries, inCount) || inK == 0 || inK > lbad::kTopKMax || !inKeys || !outLags)
        return kLBAudioDetectiveArgumentInvalid;
    if (!lbad::device_ready()) return kLBAudioDetectiveDeviceUnavailable;
    if (!lbad::corpus_ok(c, inQueries, inCount) || inIndexBase + c->count > 0x100000000ull) return kLBAudioDetectiveArgumentInvalid;
    hipStream_t stream = static_cast<hipStream_t>(inStream);
    OSStatus st = c->align_ev.wait_or_create();
    if (st == noErr)
        st = lbad::align_keys_impl(c, inQueries, inCount, inRange, inK, static_cast<const unsigned long long*>(inKeys), inIndexBase,
                                   static_cast<int32_t*>(outLags), static_cast<float*>(outScores), stream);
    if (st != noErr) return st;
    return c->align_ev.record(stream);
    LBAD_GUARD_END
}

OSStatus LBAudioDetectiveCorpusQueryBatchTopKAligned(LBAudioDetectiveCorpusRef c, const LBAudioDetectiveFingerprintRef* inQueries,
                                                     UInt32 inCount, UInt32 inRange, UInt32 inK, SInt64* outIndices,
                                                     Float32* outScores, SInt32* outLags, UInt32* outCounts) {
    LBAD_GUARD_BEGIN
    if (!lbad::queries_ok(inQueries, inCount) || inK == 0 || inK > lbad::kTopKMax || !outIndices || !outScores || !outLags ||
        !outCounts)
        return kLBAudioDetectiveArgumentInvalid;
    if (!lbad::device_ready()) return kLBAudioDetectiveDeviceUnavailable;
    if (!lbad::corpus_ok(c, inQueries, inCount)) return kLBAudioDetectiveArgumentInvalid;
    OSStatus st = c->align_ev.wait_or_create();
    if (st != noErr) return st;
    // keys, then lags, in one block: one read-back
    const size_t words = (size_t)inCount * inK;
    const size_t bytes = words * (sizeof(unsigned long long) + sizeof(int32_t));
    st = c->d_align_out.reserve(bytes);
    if (st != noErr) return st;
    unsigned long long* d_keys = static_cast<unsigned long long*>(c->d_align_out.get());
    int32_t* d_lags = reinterpret_cast<int32_t*>(d_keys + words);
    st = LBAudioDetectiveCorpusQueryBatchTopKKeysDevice(c, inQueries, inCount, inRange, inK, 0, d_keys, NULL);
    if (st == noErr) st = lbad::align_keys_impl(c, inQueries, inCount, inRange, inK, d_keys, 0, d_lags, nullptr, nullptr);
    if (st != noErr) return st;
    st = c->align_ev.record(nullptr);
    if (st != noErr) return st;
    std::vector<unsigned char> host(bytes);
    LBAD_HIP(hipMemcpy(host.data(), d_keys, bytes, hipMemcpyDeviceToHost));
    const unsigned long long* keys = reinterpret_cast<const unsigned long long*>(host.data());
    const int32_t* lags = reinterpret_cast<const int32_t*>(host.data() + words * sizeof(unsigned long long));
    for (UInt32 q = 0; q < inCount; ++q) {
        UInt32 got = 0;
        for (UInt32 i = 0; i < inK; ++i) {
            const size_t at = (size_t)q * inK + i;
            LBAudioDetectiveCorpusDecodeKey(keys[at], outIndices + at, outScores + at);
            outLags[at] = outIndices[at] >= 0 ? lags[at] : 0;
            if (outIndices[at] >= 0) ++got;
        }
        outCounts[q] = got;
    }
    return noErr;
    LBAD_GUARD_END
}

OSStatus LBAudioDetectiveCorpusQueryAligned(LBAudioDetectiveCorpusRef c, LBAudioDetectiveFingerprintRef inQuery, UInt32 inRange,
                                            SInt64* outIndex, Float32* outScore, SInt32* outLag) {
    LBAD_GUARD_BEGIN
    if (!lbad::queries_ok(&inQuery, 1) || !outIndex || !outScore || !outLag) return kLBAudioDetectiveArgumentInvalid;
    if (!lbad::device_ready()) return kLBAudioDetectiveDeviceUnavailable;
    if (!lbad::corpus_ok(c, &inQuery, 1)) return kLBAudioDetectiveArgumentInvalid;
    OSStatus st = c->align_ev.wait_or_create();
    if (st == noErr) st = c->d_align_out.reserve(16);
    if (st != noErr) return st;
    // the top-1 scan's key (LBAudioDetectiveCorpusQuery's, which the polled form returns as well), then its pair aligned
    unsigned long long* d_key = static_cast<unsigned long long*>(c->d_align_out.get());
    int32_t* d_lag = reinterpret_cast<int32_t*>(d_key + 1);
    st = LBAudioDetectiveCorpusQueryKeyDevice(c, inQuery, inRange, 0, d_key, NULL);
    if (st == noErr) st = lbad::align_keys_impl(c, &inQuery, 1, inRange, 1, d_key, 0, d_lag, nullptr, nullptr);
    if (st != noErr) return st;
    st = c->align_ev.record(nullptr);
    if (st != noErr) return st;
    unsigned long long out[2] = {0ull, 0ull};
    LBAD_HIP(hipMemcpy(out, d_key, 16, hipMemcpyDeviceToHost));
    LBAudioDetectiveCorpusDecodeKey(out[0], outIndex, outScore);
    int32_t lag;
    std::memcpy(&lag, &out[1], sizeof(lag));
    *outLag = *outIndex >= 0 ? lag : 0;
    return noErr;
    LBAD_GUARD_END
}

OSStatus LBAudioDetectiveCorpusMatchProfile(LBAudioDetectiveCorpusRef c, LBAudioDetectiveFingerprintRef inQuery, UInt32 inRange,
                                            UInt64 inEntry, Float32* outScores, UInt64 inCapacity, UInt64* outCount,
                                            SInt32* outFirstLag) {
    LBAD_GUARD_BEGIN
    if (!lbad::queries_ok(&inQuery, 1) || !outCount || !outFirstLag || (!outScores && inCapacity)) return kLBAudioDetectiveArgumentInvalid;
    if (!lbad::device_ready()) return kLBAudioDetectiveDeviceUnavailable;
    if (!lbad::corpus_ok(c, &inQuery, 1) || inEntry >= c->count) return kLBAudioDetectiveArgumentInvalid;
    const uint64_t ne = c->ragged ? c->h_off[inEntry + 1] - c->h_off[inEntry] : c->n_sub;
    const uint64_t nq = inQuery->count;
    const uint64_t n_off = (ne > nq ? ne - nq : nq - ne) + 1;
    *outCount = n_off;
    *outFirstLag = 0;
    if (inCapacity < n_off || !outScores) return kLBAudioDetectiveArgumentInvalid;
    OSStatus st = c->align_ev.wait_or_create();
    if (st == noErr) st = c->d_align_out.reserve(n_off * sizeof(float));
    const uint2* d_desc = nullptr;
    const uint32_t* d_words = nullptr;
    if (st == noErr) st = lbad::stage_queries(c, &inQuery, 1, &d_desc, &d_words, nullptr);
    if (st != noErr) return st;
    float* d_out = static_cast<float*>(c->d_align_out.get());
    LBAD_HIP(lbad::launch_align_profile(lbad::source(c, inRange), d_words, inQuery->count, inEntry, n_off, d_out, nullptr));
    st = c->align_ev.record(nullptr);
    if (st != noErr) return st;
    LBAD_HIP(hipMemcpy(outScores, d_out, n_off * sizeof(float), hipMemcpyDeviceToHost));
    return noErr;
    LBAD_GUARD_END
}

}  // extern "C"
