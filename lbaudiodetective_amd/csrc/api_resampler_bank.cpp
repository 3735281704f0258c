// api_resampler_bank.cpp -- the resampler bank: the streaming form of the file front end's sample-rate converter for many live
// channels.  A bank owns each channel's filter history in HBM and a device copy of its rate pair's PhaseTable.  A
// push takes one ragged block of new samples and emits every output whose last possible tap has arrived -- all channels in two
// launches: convert, commit (k_resample_bank.hip) -- in the layout LBAudioDetectiveStreamBankPushDevice reads.  The sample counts
// come from the host, so the host plans a call alone and mirrors input totals, output totals and carried-buffer sides: nothing is
// read back.
#include "internal.hpp"
#include "audiofile.hpp"

#include <cmath>
#include <cstring>

struct LBAudioDetectiveResamplerBank {
    double rate_in = 0.0, rate_out = 0.0;
    uint32_t mode = 0, n = 0, run = 0;
    const lbad::PhaseTable* ph = nullptr;        // process-lifetime storage (audiofile.cpp)
    // `mutex` serialises the host side of every call.  A call on another stream than its predecessor first waits, on the device,
    // for `done` -- the predecessor's last launch.
    std::mutex mutex;
    bool broken = false;                         // a HIP call failed behind a call's first launch: the device state is unknown
    // the host mirror
    std::vector<uint64_t> in_total, out_total;   // samples received / emitted since the channel (re)started
    std::vector<uint8_t> side;                   // which carried buffer holds x[c0, L)
    lbad::DeviceBuffer<float> d_carry;           // ResamplerBankDev::carry
    lbad::DeviceBuffer<int32_t> d_first;         // the PhaseTable on the device
    lbad::DeviceBuffer<uint32_t> d_count;
    lbad::DeviceBuffer<double> d_wsum, d_w;
    lbad::DeviceBuffer<unsigned char> d_fresh;   // the host form's samples
    lbad::Event fresh_ev;                        // ... behind their copy
    // the upload table: the pinned half is rewritten only after the event behind its previous copy
    lbad::StagingPair<lbad::ResamplerRow> rows;
    lbad::Event rows_ev;
    lbad::Event done;
    hipStream_t done_stream = nullptr;
    bool done_valid = false;
};

namespace lbad {
namespace {

constexpr uint32_t kRsBankMaxChannels = 1u << 24;
constexpr uint64_t kRsBankMaxOutputs = 0x7FFFFFFFull;    // outputs of one call

// the rate pair's phase table, or nullptr for a pair the bank does not take
const PhaseTable* bank_phases(double rate_in, double rate_out, uint32_t mode) {
    if (mode > 1 || !(rate_in > 0.0) || !(rate_out > 0.0) || rate_in == rate_out) return nullptr;
    ResamplePlan rp;
    if (!resample_plan(1, rate_in, rate_out, mode, rp) || rp.copy || !rp.phases) return nullptr;
    const PhaseTable* ph = rp.phases;
    if (ph->m_span == 0 || ph->m_span > kResamplerBankMaxSpan) return nullptr;
    return ph;
}

// outputs of a run: the most (<= 256) whose input range, at most floor((run - 1) p / q) + 1 + span samples, can be staged
uint32_t bank_run(const PhaseTable* ph) {
    const uint64_t more = (uint64_t)(kResamplerBankStageMax - ph->m_span - 1) * ph->q / ph->p;
    return (uint32_t)(more + 1 < kResamplerBankMaxRun ? more + 1 : kResamplerBankMaxRun);
}

// Outputs n and n + q share their weights, so a lane that takes several of them loads each weight once -- but positions inside a
// period fill the lanes of a run only where q is large: below two runs a unit is a run of consecutive outputs (integer ratios
// have q = 1, and lanes of one phase share their loads anyway).  LBAD_RSBANK_CONSECUTIVE: that form for every pair (DESIGN.md
// 4.4p measures both).
uint64_t bank_period(const PhaseTable* ph, uint32_t run) {
#if defined(LBAD_RSBANK_CONSECUTIVE)
    return kResamplerBankNoPeriod;
#else
    return ph->q >= 2ull * run ? ph->q : kResamplerBankNoPeriod;
#endif
}

long tap_high(const PhaseTable* ph) { return (long)ph->m_min + (long)ph->m_span - 1; }

// outputs whose every possible tap index is below L: the n with (n p) div q + m_hi < L
uint64_t emitted(const PhaseTable* ph, uint64_t L) {
    const long m_hi = tap_high(ph);
    if (m_hi >= 0 && L <= (uint64_t)m_hi) return 0;
    const unsigned __int128 num = (unsigned __int128)(uint64_t)((long)L - m_hi) * ph->q;
    const unsigned __int128 e = (num + ph->p - 1) / ph->p;
    return e > 0xFFFFFFFFFFFFFFFFull ? 0xFFFFFFFFFFFFFFFFull : (uint64_t)e;
}

// signal index of the first sample a channel with E outputs emitted still needs: max(0, ip(E) + m_lo), at most L
uint64_t carried_from(const PhaseTable* ph, uint64_t E, uint64_t L) {
    const unsigned __int128 ip = (unsigned __int128)E * ph->p / ph->q;
    const __int128 c = (__int128)ip + ph->m_min;
    if (c <= 0) return 0;
    return c < (__int128)L ? (uint64_t)c : L;
}

// the plan of one channel: from L samples received, E = emitted(L) emitted and n new ones
struct ChannelPlan {
    uint64_t end = 0, e_after = 0, c0 = 0, c1 = 0;
    bool ok = false;
};
ChannelPlan plan_channel(const PhaseTable* ph, double rate_in, double rate_out, uint32_t mode, uint64_t L, uint64_t E, uint32_t n,
                         bool finish) {
    ChannelPlan c;
    c.end = L + n;
    if (c.end < L) return c;
    c.e_after = emitted(ph, c.end);
    if (finish) {
        ResamplePlan rp;
        if (!resample_plan(c.end, rate_in, rate_out, mode, rp)) return c;
        if (rp.n_out > c.e_after) c.e_after = rp.n_out;     // (n_out >= emitted always: m_hi q / p > 1)
    }
    if (c.e_after < E) return c;
    if (c.e_after - E > kRsBankMaxOutputs) return c;
    if (c.e_after > 0x7FFFFFFFFFFFFFFFull / ph->p) return c;    // n p stays inside 63 bits for every output of the channel
    c.c0 = carried_from(ph, E, L);
    c.c1 = finish ? c.end : carried_from(ph, c.e_after, c.end);
    c.ok = true;
    return c;
}

ResamplerBankDev bank_dev(const LBAudioDetectiveResamplerBank* b) {
    ResamplerBankDev d;
    d.carry = b->d_carry; d.carry_stride = ((uint64_t)b->ph->m_span + 3) & ~3ull; d.n_channels = b->n;
    d.p = b->ph->p; d.q = b->ph->q; d.m_min = b->ph->m_min; d.m_span = b->ph->m_span;
    d.first = b->d_first; d.count = b->d_count; d.wsum = b->d_wsum; d.w = b->d_w;
    d.run = b->run; d.period = bank_period(b->ph, b->run);
    return d;
}

// a call's stream goes behind the previous call's last launch where the two differ
OSStatus order_begin(LBAudioDetectiveResamplerBank* b, hipStream_t stream) {
    if (b->done_valid && b->done_stream != stream) LBAD_HIP(hipStreamWaitEvent(stream, b->done, 0));
    return noErr;
}
OSStatus order_end(LBAudioDetectiveResamplerBank* b, hipStream_t stream) {
    const OSStatus st = b->done.record(stream);
    b->done_valid = st == noErr;
    b->done_stream = stream;
    return st;
}

// Everything of a push or a finish behind the argument checks that need no handle.  counts: one per channel (a finish: null, and
// `listed` marks its channels); host: the samples are host memory.
OSStatus emit_impl(LBAudioDetectiveResamplerBank* b, const void* samples, uint32_t format, bool host, const UInt32* counts,
                   const std::vector<uint8_t>* listed, UInt32* out_counts, Float32* out, UInt64 capacity, UInt64* out_total,
                   hipStream_t stream) {
    const bool finish = listed != nullptr;
    if (b->broken) return kLBAudioDetectiveDeviceError;
    const PhaseTable* ph = b->ph;
    // the plan: one row per channel with new samples / being finished
    std::vector<ResamplerRow> rows;
    std::vector<ChannelPlan> plans;
    uint64_t n_samples = 0, total = 0, units = 0;
    for (uint32_t c = 0; c < b->n; ++c) {
        const uint32_t n = finish ? 0u : counts[c];
        if (finish ? !(*listed)[c] : n == 0) continue;
        const uint64_t L = b->in_total[c], E = b->out_total[c];
        const ChannelPlan cp = plan_channel(ph, b->rate_in, b->rate_out, b->mode, L, E, n, finish);
        if (!cp.ok) return kLBAudioDetectiveArgumentInvalid;
        ResamplerRow r;
        std::memset(&r, 0, sizeof(r));
        r.fresh_at = n_samples;
        r.L = L; r.end = cp.end;
        r.out_first = E;
        r.ip0 = E * ph->p / ph->q;               // (E p < 2^63: the channel's earlier calls checked it)
        r.r0 = (uint32_t)(E * ph->p % ph->q);
        r.out_at = total;
        r.c0 = cp.c0; r.c1 = cp.c1;
        r.n = n; r.emit = (uint32_t)(cp.e_after - E);
        r.first_unit = (uint32_t)units;
        r.channel = c; r.side = b->side[c];
        n_samples += n;
        total += r.emit;
        units += resampler_bank_units(r.emit, bank_period(ph, b->run), b->run);
        if (total > kRsBankMaxOutputs) return kLBAudioDetectiveArgumentInvalid;
        rows.push_back(r);
        plans.push_back(cp);
    }
    if (n_samples != 0 && !samples) return kLBAudioDetectiveArgumentInvalid;
    if (total != 0 && !out) return kLBAudioDetectiveArgumentInvalid;
    if (capacity < total) return kLBAudioDetectiveArgumentInvalid;
    auto report = [&]() {
        if (out_counts) {
            for (uint32_t c = 0; c < b->n; ++c) out_counts[c] = 0;
            for (size_t i = 0; i < rows.size(); ++i) out_counts[rows[i].channel] = rows[i].emit;
        }
        if (out_total) *out_total = total;
    };
    auto commit_mirror = [&]() {
        for (size_t i = 0; i < rows.size(); ++i) {
            const uint32_t c = rows[i].channel;
            if (finish) {
                b->in_total[c] = 0;
                b->out_total[c] = 0;
            } else {
                b->in_total[c] = plans[i].end;
                b->out_total[c] = plans[i].e_after;
                if (rows[i].emit) b->side[c] ^= 1u;
            }
        }
    };
    if (rows.empty() || (finish && total == 0)) {            // (a finish that emits nothing launches nothing)
        commit_mirror();
        report();
        return noErr;
    }
    // memory, before anything is launched: a failure here changes nothing
    const size_t elem = format ? sizeof(int16_t) : sizeof(float);
    OSStatus st = b->rows_ev.wait_or_create();
    if (st == noErr) st = b->rows.reserve(rows.size());
    if (st == noErr && host) st = b->fresh_ev.create();
    if (st == noErr && host) st = b->d_fresh.reserve((size_t)n_samples * elem);
    if (st == noErr) st = b->done.create();
    if (st == noErr) st = order_begin(b, stream);            // (a wait, nothing of this call's: a failure still changes nothing)
    if (st != noErr) return st;
    // the launch chain: any failure from here on leaves the device state unknown
    const ResamplerBankDev dev = bank_dev(b);
    auto chain = [&]() -> OSStatus {
        OSStatus s;
        std::memcpy(b->rows.host.get(), rows.data(), rows.size() * sizeof(ResamplerRow));
        LBAD_HIP(hipMemcpyAsync(b->rows.dev, b->rows.host, rows.size() * sizeof(ResamplerRow), hipMemcpyHostToDevice, stream));
        s = b->rows_ev.record(stream);
        if (s != noErr) return s;
        const void* d_fresh = samples;
        if (host && n_samples) {
            LBAD_HIP(hipMemcpyAsync(b->d_fresh, samples, (size_t)n_samples * elem, hipMemcpyHostToDevice, stream));
            s = b->fresh_ev.record(stream);
            if (s != noErr) return s;
            d_fresh = b->d_fresh;
        }
        LBAD_HIP(launch_resampler_bank_convert(dev, b->rows.dev, (uint32_t)rows.size(), d_fresh, format, (uint32_t)units, out, stream));
        if (!finish) LBAD_HIP(launch_resampler_bank_commit(dev, b->rows.dev, (uint32_t)rows.size(), d_fresh, format, stream));
        return noErr;
    };
    st = chain();
    const OSStatus rec = order_end(b, stream);
    if (st == noErr) st = rec;
    if (st == noErr && host && n_samples) st = b->fresh_ev.wait();   // the caller's samples have left its memory
    if (st != noErr) {
        b->broken = true;
        return st;
    }
    commit_mirror();
    report();
    return noErr;
}

OSStatus push_checked(LBAudioDetectiveResamplerBank* b, const void* samples, UInt32 format, bool host, const UInt32* counts,
                      UInt32* out_counts, Float32* out, UInt64 capacity, UInt64* out_total, void* stream) {
    if (!b || !counts || format > 1u || (reinterpret_cast<uintptr_t>(samples) & (format ? 1u : 3u)) != 0 ||
        (reinterpret_cast<uintptr_t>(out) & 3u) != 0)
        return kLBAudioDetectiveArgumentInvalid;
    if (!device_ready()) return kLBAudioDetectiveDeviceUnavailable;
    std::lock_guard<std::mutex> lock(b->mutex);
    return emit_impl(b, samples, format, host, counts, nullptr, out_counts, out, capacity, out_total, static_cast<hipStream_t>(stream));
}

}  // namespace
}  // namespace lbad

extern "C" {

LBAudioDetectiveResamplerBankRef LBAudioDetectiveResamplerBankNew(Float64 inInputSampleRate, Float64 inOutputSampleRate,
                                                                  UInt32 inResamplerMode, UInt32 inNumberOfChannels) {
    try {
        if (inNumberOfChannels == 0 || inNumberOfChannels > lbad::kRsBankMaxChannels) return NULL;
        const lbad::PhaseTable* ph = lbad::bank_phases(inInputSampleRate, inOutputSampleRate, inResamplerMode);
        if (!ph) return NULL;
        if (!lbad::device_ready()) return NULL;
        LBAudioDetectiveResamplerBank* b = new LBAudioDetectiveResamplerBank();
        b->rate_in = inInputSampleRate; b->rate_out = inOutputSampleRate;
        b->mode = inResamplerMode;
        b->n = inNumberOfChannels;
        b->ph = ph;
        b->run = lbad::bank_run(ph);
        b->in_total.assign(b->n, 0);
        b->out_total.assign(b->n, 0);
        b->side.assign(b->n, 0);
        const size_t q = (size_t)ph->q, stride = ((size_t)ph->m_span + 3) & ~(size_t)3;
        // (synchronous copies: the tables are in place when New returns, whatever stream the first push runs on)
        const bool ok = b->d_carry.reserve((size_t)2 * b->n * stride) == noErr && b->d_first.reserve(q) == noErr &&
                        b->d_count.reserve(q) == noErr && b->d_wsum.reserve(q) == noErr && b->d_w.reserve(ph->w.size()) == noErr &&
                        hipMemcpy(b->d_first, ph->first.data(), q * sizeof(int32_t), hipMemcpyHostToDevice) == hipSuccess &&
                        hipMemcpy(b->d_count, ph->count.data(), q * sizeof(uint32_t), hipMemcpyHostToDevice) == hipSuccess &&
                        hipMemcpy(b->d_wsum, ph->wsum.data(), q * sizeof(double), hipMemcpyHostToDevice) == hipSuccess &&
                        hipMemcpy(b->d_w, ph->w.data(), ph->w.size() * sizeof(double), hipMemcpyHostToDevice) == hipSuccess;
        if (!ok) {
            delete b;
            return NULL;
        }
        return b;
    } catch (const std::exception&) {
        return NULL;
    }
}

void LBAudioDetectiveResamplerBankDispose(LBAudioDetectiveResamplerBankRef inBank) {
    if (!inBank) return;
    // whatever was launched has left the bank's memory before it goes
    (void)inBank->done.wait();
    (void)inBank->rows_ev.wait();
    (void)inBank->fresh_ev.wait();
    delete inBank;
}

OSStatus LBAudioDetectiveResamplerBankPushDevice(LBAudioDetectiveResamplerBankRef inBank, const void* inSamples, UInt32 inSampleFormat,
                                                 const UInt32* inSampleCounts, UInt32* outNewCounts, Float32* outSamples,
                                                 UInt64 inCapacity, UInt64* outNewTotal, void* inStream) {
    LBAD_GUARD_BEGIN
    return lbad::push_checked(inBank, inSamples, inSampleFormat, false, inSampleCounts, outNewCounts, outSamples, inCapacity, outNewTotal,
                              inStream);
    LBAD_GUARD_END
}

OSStatus LBAudioDetectiveResamplerBankPush(LBAudioDetectiveResamplerBankRef inBank, const void* inSamples, UInt32 inSampleFormat,
                                           const UInt32* inSampleCounts, UInt32* outNewCounts, Float32* outSamples,
                                           UInt64 inCapacity, UInt64* outNewTotal, void* inStream) {
    LBAD_GUARD_BEGIN
    return lbad::push_checked(inBank, inSamples, inSampleFormat, true, inSampleCounts, outNewCounts, outSamples, inCapacity, outNewTotal,
                              inStream);
    LBAD_GUARD_END
}

OSStatus LBAudioDetectiveResamplerBankFinishChannels(LBAudioDetectiveResamplerBankRef inBank, const UInt32* inChannels, UInt32 inNumberOfChannels,
                                                     UInt32* outNewCounts, Float32* outSamples, UInt64 inCapacity, UInt64* outNewTotal, void* inStream) {
    LBAD_GUARD_BEGIN
    if (!inBank || (inNumberOfChannels && !inChannels) || (reinterpret_cast<uintptr_t>(outSamples) & 3u) != 0)
        return kLBAudioDetectiveArgumentInvalid;
    if (!lbad::device_ready()) return kLBAudioDetectiveDeviceUnavailable;
    std::lock_guard<std::mutex> lock(inBank->mutex);
    std::vector<uint8_t> listed(inBank->n, 0);
    for (uint32_t j = 0; j < inNumberOfChannels; ++j) {
        if (inChannels[j] >= inBank->n || listed[inChannels[j]]) return kLBAudioDetectiveArgumentInvalid;
        listed[inChannels[j]] = 1;
    }
    return lbad::emit_impl(inBank, nullptr, 0, false, nullptr, &listed, outNewCounts, outSamples, inCapacity, outNewTotal,
                           static_cast<hipStream_t>(inStream));
    LBAD_GUARD_END
}

OSStatus LBAudioDetectiveResamplerBankGetCounts(LBAudioDetectiveResamplerBankRef inBank, UInt64* outInputTotals, UInt64* outOutputTotals) {
    LBAD_GUARD_BEGIN
    if (!inBank || (!outInputTotals && !outOutputTotals)) return kLBAudioDetectiveArgumentInvalid;
    if (!lbad::device_ready()) return kLBAudioDetectiveDeviceUnavailable;
    std::lock_guard<std::mutex> lock(inBank->mutex);
    for (uint32_t c = 0; c < inBank->n; ++c) {
        if (outInputTotals) outInputTotals[c] = inBank->in_total[c];
        if (outOutputTotals) outOutputTotals[c] = inBank->out_total[c];
    }
    return noErr;
    LBAD_GUARD_END
}

OSStatus LBAudioDetectiveResamplerBankResetChannels(LBAudioDetectiveResamplerBankRef inBank, const UInt32* inChannels, UInt32 inNumberOfChannels) {
    LBAD_GUARD_BEGIN
    if (!inBank || (inNumberOfChannels && !inChannels)) return kLBAudioDetectiveArgumentInvalid;
    if (!lbad::device_ready()) return kLBAudioDetectiveDeviceUnavailable;
    std::lock_guard<std::mutex> lock(inBank->mutex);
    if (inBank->broken) return kLBAudioDetectiveDeviceError;
    for (uint32_t j = 0; j < inNumberOfChannels; ++j)
        if (inChannels[j] >= inBank->n) return kLBAudioDetectiveArgumentInvalid;
    // the mirror alone: with L = 0 nothing carried is in reach, and taps at negative indices are never read
    for (uint32_t j = 0; j < inNumberOfChannels; ++j) {
        inBank->in_total[inChannels[j]] = 0;
        inBank->out_total[inChannels[j]] = 0;
    }
    return noErr;
    LBAD_GUARD_END
}

OSStatus LBAudioDetectiveDebugResamplerBankPlan(Float64 inInputSampleRate, Float64 inOutputSampleRate, UInt32 inResamplerMode,
                                                UInt32 inNumberOfChannels, const UInt64* inInputTotals, const UInt64* inOutputTotals,
                                                const UInt32* inSampleCounts, UInt32 inFinish, UInt32* outNew, UInt32* outCarried,
                                                SInt32* outTapLow, SInt32* outTapHigh) {
    LBAD_GUARD_BEGIN
    if (inNumberOfChannels == 0 || !inInputTotals || !inOutputTotals || !inSampleCounts || !outNew || !outCarried)
        return kLBAudioDetectiveArgumentInvalid;
    const lbad::PhaseTable* ph = lbad::bank_phases(inInputSampleRate, inOutputSampleRate, inResamplerMode);
    if (!ph) return kLBAudioDetectiveArgumentInvalid;
    std::vector<lbad::ChannelPlan> plans(inNumberOfChannels);
    for (uint32_t c = 0; c < inNumberOfChannels; ++c) {
        if (inOutputTotals[c] != lbad::emitted(ph, inInputTotals[c])) return kLBAudioDetectiveArgumentInvalid;
        plans[c] = lbad::plan_channel(ph, inInputSampleRate, inOutputSampleRate, inResamplerMode, inInputTotals[c], inOutputTotals[c],
                                      inSampleCounts[c], inFinish != 0);
        if (!plans[c].ok) return kLBAudioDetectiveArgumentInvalid;
    }
    for (uint32_t c = 0; c < inNumberOfChannels; ++c) {
        outNew[c] = (uint32_t)(plans[c].e_after - inOutputTotals[c]);
        outCarried[c] = (uint32_t)(plans[c].end - plans[c].c1);
    }
    if (outTapLow) *outTapLow = ph->m_min;
    if (outTapHigh) *outTapHigh = (SInt32)lbad::tap_high(ph);
    return noErr;
    LBAD_GUARD_END
}

}  // extern "C"
