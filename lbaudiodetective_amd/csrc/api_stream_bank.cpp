// api_stream_bank.cpp -- the stream bank: the live counterpart of LBAudioDetectiveFingerprintClipsDevice.
// A bank owns the carried partial frames of N channels and each channel's H most recent sub-fingerprints in HBM.  A push takes
// one ragged block of new samples, fingerprints every frame that became complete -- all channels in one launch chain: stage
// (k_stream_bank.hip), lbad::fingerprint_clips_device on the staged one-frame clips, commit -- and leaves the results in the
// packed layout every ...Packed...Device query reads.  The sample counts come from the host, so the host plans a push alone and
// mirrors carried lengths, totals and carried-buffer sides: PushDevice and WindowDevice read nothing back.
// A PHASED bank (LBAudioDetectiveStreamBankNewPhased) keeps a ring of each channel's last 128 frame rows as
// well and fingerprints every frame a push completes at any of P frame phases, from one transform of the channel's windows
// (push_phased_impl); the other calls are the same code on N x P virtual channels.
#include "internal.hpp"

#include <cstring>

struct LBAudioDetectiveStreamBank {
    LBAudioDetective* det = nullptr;
    uint32_t n = 0, history = 0, frames_per_pass = 0;
    // a phased bank (LBAudioDetectiveStreamBankNewPhased): nv = n * phases virtual channels, v = c * phases + p.
    // totals and the sub-fingerprint rings are per VIRTUAL channel, the carried samples per real channel; nv == n otherwise
    bool phased = false;
    uint32_t phases = 1, nv = 0;
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
    // phased: per real channel the samples and the frame rows since creation / the last reset, the ring of its last 128 rows,
    // the push's new rows, and the push's tables (sample rows, ring rows, sub-fingerprint rows, frame list) in one upload
    std::vector<uint64_t> samples_total, rows_done;
    uint64_t work_windows = 0, work_frames = 0;
    lbad::DeviceBuffer<float> d_row_ring;        // [n][128][bands]
    lbad::DeviceBuffer<float> d_new_rows;        // [new rows of a push][bands]
    lbad::StagingPair<uint4> tables;
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

// ---- the phased bank's push --------------------------------------------------------------------------
// A channel's windows are transformed in GROUPS of kBankGroup consecutive rows, a group as soon as its last window is there:
// every frame start and end, at every phase, is a multiple of 128 / 32 = 4 rows, so a frame's rows are complete exactly when
// its last group is, no window is ever transformed twice, and what is transformed does not depend on the number of phases.
// The carried samples start at the first window that is not transformed yet (fewer than window + 3 strides).
constexpr uint32_t kBankGroup = 4;
constexpr uint64_t kBankStageFloats = 64ull << 20;       // staged samples of one stage-1 pass at most (256 MiB)

OSStatus push_phased_impl(LBAudioDetectiveStreamBank* b, const Float32* samples, bool host, const UInt32* counts, UInt32* out_counts,
                          void* out_packed, UInt64 capacity, UInt64* out_total, hipStream_t stream) {
    std::lock_guard<std::mutex> lock(b->mutex);
    if (b->broken) return kLBAudioDetectiveDeviceError;
    // the detective's lock for the whole call: its plan's tables are read by the launches below
    LBAudioDetective* d = b->det;
    LBAD_LOCK(d);
    if (d->window != b->window || d->stride != b->stride || d->bands != b->bands || d->subfp_len != b->subfp_len)
        return kLBAudioDetectiveArgumentInvalid;
    OSStatus st = ensure_plan(d);
    if (st != noErr) return st;
    const Plan& plan = d->plan;
    const bool select32 = d->variant != 1 && haar_select32_supported(plan);
    if (!select32 && d->variant == 2) return kLBAudioDetectiveArgumentInvalid;
    const uint32_t W = b->window, S = b->stride, P = b->phases, h = kRowsPerFrame / P;
    const uint32_t group_hop = kBankGroup * S, clip = W + (kBankGroup - 1) * S;
    // the plan: per channel with new samples a sample row (BankRow with groups where the unphased bank has frames) and, where it
    // transforms windows, a ring row; per virtual channel with new frames a sub-fingerprint row; per new frame a list entry
    std::vector<BankRow> rows, vrows;
    std::vector<PhasedRow> prows;
    std::vector<HopFrame> list;
    uint64_t n_samples = 0, groups_total = 0, total = 0;
    for (uint32_t c = 0; c < b->n; ++c) {
        if (counts[c] == 0) continue;
        const uint64_t have = (uint64_t)b->pending[c] + counts[c];
        const uint64_t groups = have >= W ? ((have - W) / S + 1) / kBankGroup : 0;
        const uint64_t first_new = b->rows_done[c], new_row0 = groups_total * kBankGroup, n_new = groups * kBankGroup;
        BankRow r;
        std::memset(&r, 0, sizeof(r));
        r.fresh_at = n_samples;
        r.p = b->pending[c]; r.n = counts[c]; r.ready = (uint32_t)groups;
        r.first = (uint32_t)groups_total;
        r.channel = c; r.side = b->side[c];
        rows.push_back(r);
        if (n_new) {
            PhasedRow pr;
            std::memset(&pr, 0, sizeof(pr));
            pr.new_row0 = new_row0; pr.n_new = (uint32_t)n_new; pr.ring_at = (uint32_t)(first_new % kRowsPerFrame); pr.channel = c;
            prows.push_back(pr);
        }
        const uint64_t n_after = b->samples_total[c] + counts[c];
        for (uint32_t p = 0; p < P; ++p) {
            const size_t v = (size_t)c * P + p;
            const uint64_t count = subfingerprint_count_at_phase(n_after, W, S, P, p), was = b->totals[v];
            if (count == was) continue;
            if (total + (count - was) > kBankMaxFrames) return kLBAudioDetectiveArgumentInvalid;
            BankRow vr;
            std::memset(&vr, 0, sizeof(vr));
            vr.ready = (uint32_t)(count - was);
            vr.first = (uint32_t)total;
            vr.ring_at = (uint32_t)(was % b->history);
            vr.channel = (uint32_t)v;
            vrows.push_back(vr);
            for (uint64_t j = was; j < count; ++j) {
                const uint64_t at = (uint64_t)p * h + (uint64_t)kRowsPerFrame * j;     // the frame's first row
                const uint64_t old = first_new > at ? first_new - at : 0;              // its rows of earlier pushes: in the ring
                if (old > kRowsPerFrame || at + kRowsPerFrame > first_new + n_new) return kLBAudioDetectiveDeviceError;   // (never: see above)
                HopFrame f;
                std::memset(&f, 0, sizeof(f));
                f.a_row0 = (uint64_t)c * kRowsPerFrame;
                f.a_first = (uint32_t)(at % kRowsPerFrame);
                f.split = (uint32_t)old;
                f.b_row0 = new_row0 + (at + old - first_new);
                list.push_back(f);
            }
            total += count - was;
        }
        n_samples += counts[c];
        groups_total += groups;
        if (groups_total > kBankMaxFrames / kBankGroup) return kLBAudioDetectiveArgumentInvalid;
    }
    if (n_samples != 0 && !samples) return kLBAudioDetectiveArgumentInvalid;
    if (out_packed && capacity < total) return kLBAudioDetectiveArgumentInvalid;
    auto report = [&]() {
        if (out_counts) {
            for (uint32_t v = 0; v < b->nv; ++v) out_counts[v] = 0;
            for (const BankRow& vr : vrows) out_counts[vr.channel] = vr.ready;
        }
        if (out_total) *out_total = total;
    };
    if (rows.empty()) {
        report();
        return noErr;
    }
    // memory, before anything is launched: a failure here changes nothing
    uint64_t pass_groups = (uint64_t)b->frames_per_pass * (kRowsPerFrame / kBankGroup);
    if (pass_groups > kBankStageFloats / clip) pass_groups = kBankStageFloats / clip;
    if (pass_groups == 0) pass_groups = 1;
    if (pass_groups > groups_total) pass_groups = groups_total;
    const uint64_t pass_frames = total < b->frames_per_pass ? total : b->frames_per_pass;
    // the tables, each from a 16-byte boundary: sample rows, sub-fingerprint rows, ring rows, frame list
    const size_t at_vrows = rows.size() * sizeof(BankRow), at_prows = at_vrows + vrows.size() * sizeof(BankRow);
    const size_t at_list = at_prows + prows.size() * sizeof(PhasedRow), table_bytes = at_list + list.size() * sizeof(HopFrame);
    st = b->rows_ev.wait_or_create();
    if (st == noErr) st = b->tables.reserve(table_bytes / sizeof(uint4));
    if (st == noErr) st = b->d_new.reserve((size_t)total * kPackedWords);
    if (st == noErr) st = b->d_clips.reserve((size_t)(pass_groups * clip));
    if (st == noErr) st = b->d_new_rows.reserve((size_t)(groups_total * kBankGroup * b->bands));
    if (st == noErr && host) st = b->fresh_ev.create();
    if (st == noErr && host) st = b->d_fresh.reserve((size_t)n_samples);
    if (st == noErr) st = b->done.create();
    if (st != noErr) return st;
    // the launch chain: any failure from here on leaves the device state unknown
    BankDev dev = bank_dev(b);
    BankDev dev_groups = dev;            // the stage and carry kernels take a group for a frame: W + 3 S samples, 4 S apart
    dev_groups.hop = group_hop;
    dev_groups.window = clip - group_hop;
    auto chain = [&]() -> OSStatus {
        OSStatus s = order_begin(b, stream);
        if (s != noErr) return s;
        char* th = reinterpret_cast<char*>(b->tables.host.get());
        const char* td = reinterpret_cast<const char*>(b->tables.dev.get());
        std::memcpy(th, rows.data(), rows.size() * sizeof(BankRow));
        if (!vrows.empty()) std::memcpy(th + at_vrows, vrows.data(), vrows.size() * sizeof(BankRow));
        if (!prows.empty()) std::memcpy(th + at_prows, prows.data(), prows.size() * sizeof(PhasedRow));
        if (!list.empty()) std::memcpy(th + at_list, list.data(), list.size() * sizeof(HopFrame));
        LBAD_HIP(hipMemcpyAsync(b->tables.dev, b->tables.host, table_bytes, hipMemcpyHostToDevice, stream));
        s = b->rows_ev.record(stream);
        if (s != noErr) return s;
        const BankRow* d_rows = reinterpret_cast<const BankRow*>(td);
        const BankRow* d_vrows = reinterpret_cast<const BankRow*>(td + at_vrows);
        const PhasedRow* d_prows = reinterpret_cast<const PhasedRow*>(td + at_prows);
        const HopFrame* d_list = reinterpret_cast<const HopFrame*>(td + at_list);
        const float* d_fresh = samples;
        if (host) {
            LBAD_HIP(hipMemcpyAsync(b->d_fresh, samples, (size_t)n_samples * sizeof(float), hipMemcpyHostToDevice, stream));
            s = b->fresh_ev.record(stream);
            if (s != noErr) return s;
            d_fresh = b->d_fresh;
        }
        // stage 1: every new group once, into the push's block of new rows (full rows: the window-oriented generic kernel)
        for (uint64_t g0 = 0; g0 < groups_total; g0 += pass_groups) {
            const uint32_t ng = (uint32_t)(groups_total - g0 < pass_groups ? groups_total - g0 : pass_groups);
            LBAD_HIP(launch_bank_stage(dev_groups, d_rows, (uint32_t)rows.size(), d_fresh, (uint32_t)g0, ng, b->d_clips, stream));
            LBAD_HIP(launch_fft_bands_windows(plan, b->d_clips, 0, ng, clip, kBankGroup, b->d_new_rows + g0 * kBankGroup * b->bands, stream));
        }
        // stage 2 at a row hop: every frame the push completes, from the ring and the new rows
        for (uint64_t f0 = 0; f0 < total; f0 += pass_frames) {
            StageHop hop;
            hop.list = d_list + f0;
            hop.n_list = (uint32_t)(total - f0 < pass_frames ? total - f0 : pass_frames);
            hop.tail = b->d_new_rows;
            uint32_t* out = b->d_new + f0 * kPackedWords;
            LBAD_HIP(select32 ? launch_haar_select32_hop(plan, b->d_row_ring, hop, 0, out, stream)
                              : launch_haar_select_hop(plan, b->d_row_ring, hop, 0, out, stream));
        }
        LBAD_HIP(launch_bank_commit_rows(dev, d_vrows, (uint32_t)vrows.size(), b->d_new, (uint32_t)total, out_packed, stream));
        LBAD_HIP(launch_bank_row_ring(b->d_row_ring, b->bands, d_prows, (uint32_t)prows.size(), b->d_new_rows, stream));
        LBAD_HIP(launch_bank_commit_carry(dev_groups, d_rows, (uint32_t)rows.size(), d_fresh, stream));
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
    for (const BankRow& r : rows) {
        const uint32_t c = r.channel;
        b->pending[c] = (uint32_t)((uint64_t)r.p + r.n - (uint64_t)r.ready * group_hop);
        b->samples_total[c] += r.n;
        b->rows_done[c] += (uint64_t)r.ready * kBankGroup;
        if (r.ready) b->side[c] ^= 1u;
    }
    for (const BankRow& vr : vrows) b->totals[vr.channel] += vr.ready;
    b->work_windows += groups_total * kBankGroup;
    b->work_frames += total;
    report();
    return noErr;
}

// Everything of a push behind its argument checks that need no handle.  host: the samples are host memory.
OSStatus push_impl(LBAudioDetectiveStreamBank* b, const Float32* samples, bool host, const UInt32* counts, UInt32* out_counts,
                   void* out_packed, UInt64 capacity, UInt64* out_total, hipStream_t stream) {
    if (b->phased) return push_phased_impl(b, samples, host, counts, out_counts, out_packed, capacity, out_total, stream);
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
        if (channels[j] >= b->nv || b->totals[channels[j]] < q) return kLBAudioDetectiveArgumentInvalid;
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

// phases == 0: the unphased bank
static LBAudioDetectiveStreamBankRef bank_new(LBAudioDetectiveRef inDetective, UInt32 inNumberOfChannels, UInt32 inHistorySubfingerprints,
                                              UInt32 inFramesPerPass, UInt32 inPhases) {
    try {
        const bool phased = inPhases != 0;
        const uint32_t phases = phased ? inPhases : 1;
        if (!inDetective || inNumberOfChannels == 0 || inNumberOfChannels > lbad::kBankMaxChannels / phases || inHistorySubfingerprints == 0 ||
            inHistorySubfingerprints > lbad::kBankMaxHistory)
            return NULL;
        if (!lbad::device_ready()) return NULL;
        LBAudioDetectiveStreamBank* b = new LBAudioDetectiveStreamBank();
        b->det = inDetective;
        b->n = inNumberOfChannels;
        b->phased = phased;
        b->phases = phases;
        b->nv = inNumberOfChannels * phases;
        b->history = inHistorySubfingerprints;
        b->frames_per_pass = inFramesPerPass ? inFramesPerPass : b->nv;
        bool ok;
        {
            LBAudioDetective* d = inDetective;
            LBAD_LOCK(d);
            b->window = d->window; b->stride = d->stride; b->bands = d->bands; b->subfp_len = d->subfp_len;
            ok = lbad::settings_ok(b->window, b->stride) && lbad::ensure_plan(d) == noErr;
            // the phased bank stages groups of windows that overlap: no stride beyond the window
            if (phased && b->stride > b->window) ok = false;
        }
        if (ok) {
            b->hop = lbad::kRowsPerFrame * b->stride;
            b->pending.assign(b->n, 0);
            b->totals.assign(b->nv, 0);
            b->side.assign(b->n, 0);
            ok = b->d_carry.reserve((size_t)2 * b->n * ((size_t)b->window + b->hop)) == noErr &&
                 b->d_ring.reserve((size_t)b->nv * b->history * lbad::kPackedWords) == noErr;
            if (ok && phased) {
                b->samples_total.assign(b->n, 0);
                b->rows_done.assign(b->n, 0);
                ok = b->d_row_ring.reserve((size_t)b->n * lbad::kRowsPerFrame * b->bands) == noErr;
            }
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

LBAudioDetectiveStreamBankRef LBAudioDetectiveStreamBankNew(LBAudioDetectiveRef inDetective, UInt32 inNumberOfChannels,
                                                            UInt32 inHistorySubfingerprints, UInt32 inFramesPerPass) {
    return bank_new(inDetective, inNumberOfChannels, inHistorySubfingerprints, inFramesPerPass, 0);
}

LBAudioDetectiveStreamBankRef LBAudioDetectiveStreamBankNewPhased(LBAudioDetectiveRef inDetective, UInt32 inNumberOfChannels,
                                                                  UInt32 inHistorySubfingerprints, UInt32 inFramesPerPass, UInt32 inPhases) {
    if (!lbad::valid_phases(inPhases)) return NULL;
    return bank_new(inDetective, inNumberOfChannels, inHistorySubfingerprints, inFramesPerPass, inPhases);
}

UInt32 LBAudioDetectiveStreamBankGetPhases(LBAudioDetectiveStreamBankRef inBank) { return inBank ? inBank->phases : 0; }

OSStatus LBAudioDetectiveStreamBankGetWork(LBAudioDetectiveStreamBankRef inBank, UInt64* outWindowsTransformed, UInt64* outFramesSelected) {
    LBAD_GUARD_BEGIN
    if (!inBank || !inBank->phased || (!outWindowsTransformed && !outFramesSelected)) return kLBAudioDetectiveArgumentInvalid;
    std::lock_guard<std::mutex> lock(inBank->mutex);
    if (outWindowsTransformed) *outWindowsTransformed = inBank->work_windows;
    if (outFramesSelected) *outFramesSelected = inBank->work_frames;
    return noErr;
    LBAD_GUARD_END
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
    for (uint32_t v = 0; outTotals && v < inBank->nv; ++v) outTotals[v] = inBank->totals[v];
    for (uint32_t c = 0; outPendingSamples && c < inBank->n; ++c) outPendingSamples[c] = inBank->pending[c];
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
        if (b->broken || inChannel >= b->nv) return NULL;
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
        const uint32_t c = inChannels[j];
        inBank->pending[c] = 0;
        for (uint32_t p = 0; p < inBank->phases; ++p) inBank->totals[(size_t)c * inBank->phases + p] = 0;
        if (inBank->phased) inBank->samples_total[c] = inBank->rows_done[c] = 0;     // (no row of the ring is in reach either)
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
