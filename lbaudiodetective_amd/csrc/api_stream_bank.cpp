// api_stream_bank.cpp -- the stream bank: the live counterpart of LBAudioDetectiveFingerprintClipsDevice.
// A bank owns the carried partial frames of N channels and each channel's H most recent sub-fingerprints in HBM.  A push takes
// one ragged block of new samples, fingerprints every frame that became complete -- all channels in one launch chain: stage
// (k_stream_bank.hip), lbad::fingerprint_clips_device on the staged one-frame clips, commit -- and leaves the results in the
// packed layout every ...Packed...Device query reads.  The sample counts come from the host, so the host plans a push alone and
// mirrors carried lengths, totals and carried-buffer sides: PushDevice and WindowDevice read nothing back.
#include "internal.hpp"

#include <cstring>

struct LBAudioDetectiveStreamBank {
    LBAudioDetective* det = nullptr;
    uint32_t n = 0, history = 0, frames_per_pass = 0;
    uint32_t window = 0, stride = 0, bands = 0, subfp_len = 0, hop = 0;
    // `mutex` serialises the host side of every call.  A call on another stream than its predecessor first waits, on the device,
    // for `done` -- the predecessor's last launch (the detective's StreamOrder does the same for its own scratch).
    std::mutex mutex;
    bool broken = false;                         // a HIP call failed behind a push's first launch: the device state is unknown
    // the host mirror
    std::vector<uint32_t> pending;               // samples carried
    std::vector<uint64_t> totals;                // sub-fingerprints since creation / the last reset
    std::vector<uint8_t> side;                   // which carried buffer holds them
    lbad::DeviceBuffer<float> d_carry;           // BankDev::carry
    lbad::DeviceBuffer<uint32_t> d_ring;         // BankDev::ring
    lbad::DeviceBuffer<float> d_clips;           // the staged frames of a pass: at most frames_per_pass x (window + hop)
    lbad::DeviceBuffer<uint32_t> d_new;          // a push's packed sub-fingerprints, all passes
    lbad::DeviceBuffer<float> d_fresh;           // the host form's samples
    lbad::Event fresh_ev;                        // ... behind their copy
    // the upload tables: the pinned half is rewritten only after the event behind its previous copy
    lbad::StagingPair<lbad::BankRow> rows;
    lbad::Event rows_ev;
    lbad::StagingPair<uint2> list;
    lbad::Event list_ev;
    lbad::Event done;
    hipStream_t done_stream = nullptr;
    bool done_valid = false;
};

namespace lbad {
namespace {

constexpr uint32_t kBankMaxChannels = 1u << 24;
constexpr uint32_t kBankMaxHistory = 1u << 20;
constexpr uint64_t kBankMaxFrames = 0x7FFFFFFFull;       // frames of one push
constexpr uint64_t kBankMaxWindowRows = 0x80000000ull;   // sub-fingerprints of one window call

// the plan of one channel: frames that p carried and n new samples complete, what is carried on, what the ring keeps
struct ChannelPlan {
    uint64_t ready = 0;
    uint32_t p_after = 0, kept = 0;
};
ChannelPlan plan_channel(uint32_t window, uint32_t stride, uint32_t history, uint32_t p, uint32_t n) {
    ChannelPlan c;
    const uint64_t have = (uint64_t)p + n, hop = (uint64_t)kRowsPerFrame * stride;
    c.ready = subfingerprint_count(have, window, stride);
    c.p_after = (uint32_t)(have - c.ready * hop);        // < window + hop
    c.kept = (uint32_t)(c.ready < history ? c.ready : history);
    return c;
}

bool settings_ok(uint32_t window, uint32_t stride) {
    return window >= kMinWindow && window <= kMaxWindow && (window & (window - 1)) == 0 && stride != 0 &&
           stride <= 0xFFFFFFFFu / kRowsPerFrame - kMaxWindow;
}

BankDev bank_dev(const LBAudioDetectiveStreamBank* b) {
    BankDev d;
    d.carry = b->d_carry; d.carry_stride = (uint64_t)b->window + b->hop; d.n_channels = b->n;
    d.ring = b->d_ring; d.history = b->history; d.window = b->window; d.hop = b->hop;
    return d;
}

// a call's stream goes behind the previous call's last launch where the two differ
OSStatus order_begin(LBAudioDetectiveStreamBank* b, hipStream_t stream) {
    if (b->done_valid && b->done_stream != stream) LBAD_HIP(hipStreamWaitEvent(stream, b->done, 0));
    return noErr;
}
OSStatus order_end(LBAudioDetectiveStreamBank* b, hipStream_t stream) {
    const OSStatus st = b->done.record(stream);
    b->done_valid = st == noErr;
    b->done_stream = stream;
    return st;
}

// the bank's settings are still the detective's, and its plan stands (the detective's lock is held here and ONLY here: it is free
// again when fingerprint_clips_device, which takes it itself, is called)
OSStatus settings_unchanged(LBAudioDetectiveStreamBank* b) {
    LBAudioDetective* d = b->det;
    LBAD_LOCK(d);
    if (d->window != b->window || d->stride != b->stride || d->bands != b->bands || d->subfp_len != b->subfp_len)
        return kLBAudioDetectiveArgumentInvalid;
    return ensure_plan(d);
}

// Everything of a push behind its argument checks that need no handle.  host: the samples are host memory.
OSStatus push_impl(LBAudioDetectiveStreamBank* b, const Float32* samples, bool host, const UInt32* counts, UInt32* out_counts,
                   void* out_packed, UInt64 capacity, UInt64* out_total, hipStream_t stream) {
    std::lock_guard<std::mutex> lock(b->mutex);
    if (b->broken) return kLBAudioDetectiveDeviceError;
    OSStatus st = settings_unchanged(b);
    if (st != noErr) return st;
    // the plan: one row per channel with new samples
    std::vector<BankRow> rows;
    std::vector<ChannelPlan> plans;
    uint64_t n_samples = 0, total = 0;
    for (uint32_t c = 0; c < b->n; ++c) {
        if (counts[c] == 0) continue;
        const ChannelPlan cp = plan_channel(b->window, b->stride, b->history, b->pending[c], counts[c]);
        BankRow r;
        std::memset(&r, 0, sizeof(r));
        r.fresh_at = n_samples;
        r.p = b->pending[c]; r.n = counts[c]; r.ready = (uint32_t)cp.ready;
        r.first = (uint32_t)total;
        r.ring_at = (uint32_t)(b->totals[c] % b->history);
        r.channel = c; r.side = b->side[c];
        n_samples += counts[c];
        total += cp.ready;
        if (total > kBankMaxFrames) return kLBAudioDetectiveArgumentInvalid;
        rows.push_back(r);
        plans.push_back(cp);
    }
    if (n_samples != 0 && !samples) return kLBAudioDetectiveArgumentInvalid;
    if (out_packed && capacity < total) return kLBAudioDetectiveArgumentInvalid;
    auto report = [&]() {
        if (out_counts) {
            for (uint32_t c = 0; c < b->n; ++c) out_counts[c] = 0;
            for (size_t i = 0; i < rows.size(); ++i) out_counts[rows[i].channel] = rows[i].ready;
        }
        if (out_total) *out_total = total;
    };
    if (rows.empty()) {
        report();
        return noErr;
    }
    // memory, before anything is launched: a failure here changes nothing
    const uint64_t clip = (uint64_t)b->window + b->hop;
    const uint64_t pass = total < b->frames_per_pass ? total : b->frames_per_pass;
    st = b->rows_ev.wait_or_create();
    if (st == noErr) st = b->rows.reserve(rows.size());
    if (st == noErr) st = b->d_new.reserve((size_t)total * kPackedWords);
    if (st == noErr) st = b->d_clips.reserve((size_t)(pass * clip));
    if (st == noErr && host) st = b->fresh_ev.create();
    if (st == noErr && host) st = b->d_fresh.reserve((size_t)n_samples);
    if (st == noErr) st = b->done.create();
    if (st != noErr) return st;
    // the launch chain: any failure from here on leaves the device state unknown
    const BankDev dev = bank_dev(b);
    auto chain = [&]() -> OSStatus {
        OSStatus s = order_begin(b, stream);
        if (s != noErr) return s;
        std::memcpy(b->rows.host.get(), rows.data(), rows.size() * sizeof(BankRow));
        LBAD_HIP(hipMemcpyAsync(b->rows.dev, b->rows.host, rows.size() * sizeof(BankRow), hipMemcpyHostToDevice, stream));
        s = b->rows_ev.record(stream);
        if (s != noErr) return s;
        const float* d_fresh = samples;
        if (host) {
            LBAD_HIP(hipMemcpyAsync(b->d_fresh, samples, (size_t)n_samples * sizeof(float), hipMemcpyHostToDevice, stream));
            s = b->fresh_ev.record(stream);
            if (s != noErr) return s;
            d_fresh = b->d_fresh;
        }
        for (uint64_t g0 = 0; g0 < total; g0 += pass) {
            const uint32_t nf = (uint32_t)(total - g0 < pass ? total - g0 : pass);
            LBAD_HIP(launch_bank_stage(dev, b->rows.dev, (uint32_t)rows.size(), d_fresh, (uint32_t)g0, nf, b->d_clips, stream));
            s = fingerprint_clips_device(b->det, b->d_clips, 0, nf, clip, b->d_new + g0 * kPackedWords, nullptr, nullptr, stream);
            if (s != noErr) return s;
        }
        LBAD_HIP(launch_bank_commit(dev, b->rows.dev, (uint32_t)rows.size(), d_fresh, b->d_new, (uint32_t)total, out_packed, stream));
        return noErr;
    };
    st = chain();
    const OSStatus rec = order_end(b, stream);
    if (st == noErr) st = rec;
    if (st == noErr && host) st = b->fresh_ev.wait();    // the caller's samples have left its memory
    if (st != noErr) {
        b->broken = true;
        return st;
    }
    for (size_t i = 0; i < rows.size(); ++i) {
        const uint32_t c = rows[i].channel;
        b->pending[c] = plans[i].p_after;
        b->totals[c] += plans[i].ready;
        if (plans[i].ready) b->side[c] ^= 1u;
    }
    report();
    return noErr;
}

OSStatus push_checked(LBAudioDetectiveStreamBank* b, const Float32* samples, bool host, const UInt32* counts, UInt32* out_counts,
                      void* out_packed, UInt64 capacity, UInt64* out_total, void* stream) {
    if (!b || !counts || (reinterpret_cast<uintptr_t>(samples) & 3u) != 0 || (reinterpret_cast<uintptr_t>(out_packed) & 15u) != 0)
        return kLBAudioDetectiveArgumentInvalid;
    if (!device_ready()) return kLBAudioDetectiveDeviceUnavailable;
    return push_impl(b, samples, host, counts, out_counts, out_packed, capacity, out_total, static_cast<hipStream_t>(stream));
}

OSStatus window_impl(LBAudioDetectiveStreamBank* b, const UInt32* channels, uint32_t n_list, uint32_t q, void* out, hipStream_t stream) {
    std::lock_guard<std::mutex> lock(b->mutex);
    if (b->broken) return kLBAudioDetectiveDeviceError;
    if (q > b->history || (uint64_t)n_list * q > kBankMaxWindowRows) return kLBAudioDetectiveArgumentInvalid;
    for (uint32_t j = 0; j < n_list; ++j)
        if (channels[j] >= b->n || b->totals[channels[j]] < q) return kLBAudioDetectiveArgumentInvalid;
    if (n_list == 0) return noErr;
    OSStatus st = b->list_ev.wait_or_create();
    if (st == noErr) st = b->list.reserve(n_list);
    if (st == noErr) st = b->done.create();
    if (st != noErr) return st;
    uint2* h = b->list.host;
    for (uint32_t j = 0; j < n_list; ++j) h[j] = make_uint2(channels[j], (uint32_t)((b->totals[channels[j]] - q) % b->history));
    auto chain = [&]() -> OSStatus {
        OSStatus s = order_begin(b, stream);
        if (s != noErr) return s;
        LBAD_HIP(hipMemcpyAsync(b->list.dev, b->list.host, (size_t)n_list * sizeof(uint2), hipMemcpyHostToDevice, stream));
        s = b->list_ev.record(stream);
        if (s != noErr) return s;
        LBAD_HIP(launch_bank_window(bank_dev(b), b->list.dev, n_list, q, out, stream));
        return noErr;
    };
    st = chain();
    const OSStatus rec = order_end(b, stream);
    if (st == noErr) st = rec;
    if (st != noErr) b->broken = true;
    return st;
}

}  // namespace
}  // namespace lbad

extern "C" {

LBAudioDetectiveStreamBankRef LBAudioDetectiveStreamBankNew(LBAudioDetectiveRef inDetective, UInt32 inNumberOfChannels,
                                                            UInt32 inHistorySubfingerprints, UInt32 inFramesPerPass) {
    try {
        if (!inDetective || inNumberOfChannels == 0 || inNumberOfChannels > lbad::kBankMaxChannels || inHistorySubfingerprints == 0 ||
            inHistorySubfingerprints > lbad::kBankMaxHistory)
            return NULL;
        if (!lbad::device_ready()) return NULL;
        LBAudioDetectiveStreamBank* b = new LBAudioDetectiveStreamBank();
        b->det = inDetective;
        b->n = inNumberOfChannels;
        b->history = inHistorySubfingerprints;
        b->frames_per_pass = inFramesPerPass ? inFramesPerPass : inNumberOfChannels;
        bool ok;
        {
            LBAudioDetective* d = inDetective;
            LBAD_LOCK(d);
            b->window = d->window; b->stride = d->stride; b->bands = d->bands; b->subfp_len = d->subfp_len;
            ok = lbad::settings_ok(b->window, b->stride) && lbad::ensure_plan(d) == noErr;
        }
        if (ok) {
            b->hop = lbad::kRowsPerFrame * b->stride;
            b->pending.assign(b->n, 0);
            b->totals.assign(b->n, 0);
            b->side.assign(b->n, 0);
            ok = b->d_carry.reserve((size_t)2 * b->n * ((size_t)b->window + b->hop)) == noErr &&
                 b->d_ring.reserve((size_t)b->n * b->history * lbad::kPackedWords) == noErr;
        }
        if (!ok) {
            delete b;
            return NULL;
        }
        return b;
    } catch (const std::exception&) {
        return NULL;
    }
}

void LBAudioDetectiveStreamBankDispose(LBAudioDetectiveStreamBankRef inBank) {
    if (!inBank) return;
    // whatever was launched has left the bank's memory before it goes
    (void)inBank->done.wait();
    (void)inBank->rows_ev.wait();
    (void)inBank->list_ev.wait();
    (void)inBank->fresh_ev.wait();
    delete inBank;
}

OSStatus LBAudioDetectiveStreamBankPushDevice(LBAudioDetectiveStreamBankRef inBank, const Float32* inSamples,
                                              const UInt32* inSampleCounts, UInt32* outNewCounts, void* outNewPacked,
                                              UInt64 inNewCapacity, UInt64* outNewTotal, void* inStream) {
    LBAD_GUARD_BEGIN
    return lbad::push_checked(inBank, inSamples, false, inSampleCounts, outNewCounts, outNewPacked, inNewCapacity, outNewTotal, inStream);
    LBAD_GUARD_END
}

OSStatus LBAudioDetectiveStreamBankPush(LBAudioDetectiveStreamBankRef inBank, const Float32* inSamples,
                                        const UInt32* inSampleCounts, UInt32* outNewCounts, void* outNewPacked,
                                        UInt64 inNewCapacity, UInt64* outNewTotal, void* inStream) {
    LBAD_GUARD_BEGIN
    return lbad::push_checked(inBank, inSamples, true, inSampleCounts, outNewCounts, outNewPacked, inNewCapacity, outNewTotal, inStream);
    LBAD_GUARD_END
}

OSStatus LBAudioDetectiveStreamBankGetCounts(LBAudioDetectiveStreamBankRef inBank, UInt64* outTotals, UInt32* outPendingSamples) {
    LBAD_GUARD_BEGIN
    if (!inBank || (!outTotals && !outPendingSamples)) return kLBAudioDetectiveArgumentInvalid;
    if (!lbad::device_ready()) return kLBAudioDetectiveDeviceUnavailable;
    std::lock_guard<std::mutex> lock(inBank->mutex);
    for (uint32_t c = 0; c < inBank->n; ++c) {
        if (outTotals) outTotals[c] = inBank->totals[c];
        if (outPendingSamples) outPendingSamples[c] = inBank->pending[c];
    }
    return noErr;
    LBAD_GUARD_END
}

OSStatus LBAudioDetectiveStreamBankWindowDevice(LBAudioDetectiveStreamBankRef inBank, const UInt32* inChannels,
                                                UInt32 inNumberOfChannels, UInt32 inSubfingerprints, void* outPacked, void* inStream) {
    LBAD_GUARD_BEGIN
    if (!inBank || (inNumberOfChannels && !inChannels) || !outPacked || inSubfingerprints == 0 ||
        (reinterpret_cast<uintptr_t>(outPacked) & 15u) != 0)
        return kLBAudioDetectiveArgumentInvalid;
    if (!lbad::device_ready()) return kLBAudioDetectiveDeviceUnavailable;
    return lbad::window_impl(inBank, inChannels, inNumberOfChannels, inSubfingerprints, outPacked, static_cast<hipStream_t>(inStream));
    LBAD_GUARD_END
}

LBAudioDetectiveFingerprintRef LBAudioDetectiveStreamBankCopyFingerprint(LBAudioDetectiveStreamBankRef inBank, UInt32 inChannel) {
    try {
        if (!inBank || !lbad::device_ready()) return NULL;
        LBAudioDetectiveStreamBank* b = inBank;
        std::lock_guard<std::mutex> lock(b->mutex);
        if (b->broken || inChannel >= b->n) return NULL;
        const uint64_t total = b->totals[inChannel];
        const uint32_t count = (uint32_t)(total < b->history ? total : b->history);
        std::vector<uint32_t> words((size_t)b->history * lbad::kPackedWords);
        if (count) {
            if (b->done.wait() != noErr) return NULL;
            if (hipMemcpy(words.data(), b->d_ring + (size_t)inChannel * b->history * lbad::kPackedWords, words.size() * sizeof(uint32_t),
                          hipMemcpyDeviceToHost) != hipSuccess)
                return NULL;
        }
        LBAudioDetectiveFingerprint* fp = new LBAudioDetectiveFingerprint();
        fp->length = b->subfp_len;
        fp->count = count;
        try {
            fp->data.assign((size_t)count * b->subfp_len, 0);
        } catch (const std::bad_alloc&) {
            delete fp;
            return NULL;
        }
        for (uint32_t s = 0; s < count; ++s) {
            const uint64_t slot = (total - count + s) % b->history;
            LBAudioDetectiveUnpackSubfingerprint(words.data() + (size_t)slot * lbad::kPackedWords, b->subfp_len,
                                                 fp->data.data() + (size_t)s * b->subfp_len);
        }
        return fp;
    } catch (const std::exception&) {
        return NULL;
    }
}

OSStatus LBAudioDetectiveStreamBankResetChannels(LBAudioDetectiveStreamBankRef inBank, const UInt32* inChannels, UInt32 inNumberOfChannels) {
    LBAD_GUARD_BEGIN
    if (!inBank || (inNumberOfChannels && !inChannels)) return kLBAudioDetectiveArgumentInvalid;
    if (!lbad::device_ready()) return kLBAudioDetectiveDeviceUnavailable;
    std::lock_guard<std::mutex> lock(inBank->mutex);
    if (inBank->broken) return kLBAudioDetectiveDeviceError;
    for (uint32_t j = 0; j < inNumberOfChannels; ++j)
        if (inChannels[j] >= inBank->n) return kLBAudioDetectiveArgumentInvalid;
    // the mirror alone: with a total of 0 nothing of the ring is in reach, and with nothing carried no sample is
    for (uint32_t j = 0; j < inNumberOfChannels; ++j) {
        inBank->pending[inChannels[j]] = 0;
        inBank->totals[inChannels[j]] = 0;
    }
    return noErr;
    LBAD_GUARD_END
}

OSStatus LBAudioDetectiveDebugStreamBankPlan(UInt32 inWindowSize, UInt32 inAnalysisStride, UInt32 inHistorySubfingerprints,
                                             UInt32 inNumberOfChannels, const UInt32* inPending, const UInt32* inSampleCounts,
                                             UInt32* outReady, UInt32* outPendingAfter, UInt32* outKept) {
    LBAD_GUARD_BEGIN
    if (!lbad::settings_ok(inWindowSize, inAnalysisStride) || inHistorySubfingerprints == 0 || inNumberOfChannels == 0 || !inPending ||
        !inSampleCounts || !outReady || !outPendingAfter || !outKept)
        return kLBAudioDetectiveArgumentInvalid;
    const uint64_t clip = (uint64_t)inWindowSize + (uint64_t)lbad::kRowsPerFrame * inAnalysisStride;
    for (uint32_t c = 0; c < inNumberOfChannels; ++c)
        if (inPending[c] >= clip) return kLBAudioDetectiveArgumentInvalid;          // no channel ever carries a whole frame
    for (uint32_t c = 0; c < inNumberOfChannels; ++c) {
        const lbad::ChannelPlan cp = lbad::plan_channel(inWindowSize, inAnalysisStride, inHistorySubfingerprints, inPending[c], inSampleCounts[c]);
        outReady[c] = (uint32_t)cp.ready;
        outPendingAfter[c] = cp.p_after;
        outKept[c] = cp.kept;
    }
    return noErr;
    LBAD_GUARD_END
}

}  // extern "C"
