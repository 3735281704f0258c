// internal.hpp -- shared declarations of the HIP library (not installed; the ABI is include/lbaudiodetective.h)
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <functional>
#include <new>
#include <stdexcept>
#include <map>
#include <mutex>
#include <vector>

#include "../../include/lbaudiodetective.h"
#include "buffers.hpp"   // hip_status / LBAD_HIP and the owning types

namespace lbad {

constexpr uint32_t kRowsPerFrame = 128;  // LBAudioDetective.m:25
constexpr uint32_t kPackedWords = LBAD_PACKED_WORDS;
constexpr uint32_t kMaxBands = 64;
constexpr uint32_t kSparseFrameDwMax = 128 * 17;       // the largest compact frame (Plan::Sparse): 128 rows of at most 16 + 1 stored bands
constexpr uint32_t kMinWindow = 16;
constexpr uint32_t kMaxWindow = 8192;

// Host allocations sized by caller or file data (decoded audio, resampler output, zero padding) can fail:
// nothing may unwind through the C boundary.  memFullErr is MacErrors.h's -108.
#define LBAD_GUARD_BEGIN try {
#define LBAD_GUARD_END                                                    \
    }                                                                     \
    catch (const std::bad_alloc&) { return kLBAudioDetectiveMemFull; }    \
    catch (const std::exception&) { return kLBAudioDetectiveArgumentInvalid; }

bool device_ready();
// Per-device facts and one-time set-up, keyed by the CURRENT device (a process may use several).
constexpr int kMaxDevices = 64;
int current_device();                       // hipGetDevice, -1 on failure
int device_cu_count();                      // CUs of the current device (256 when the query fails)
// One slot per device: returns true when `value` differs from what was recorded for the current device
// (and records it) -- "has this function's attribute / table been set up on this device for this size?"
struct PerDevice {
    size_t seen[kMaxDevices] = {};
    bool changed(size_t value) {
        const int d = current_device();
        if (d < 0 || d >= kMaxDevices) return true;
        if (seen[d] == value) return false;
        seen[d] = value;
        return true;
    }
};

// The grid of a launch whose workgroups carry state in LDS from one work item to the next (w += gridDim.x): the work, at most
// the launcher's own ceiling, at most the tests' ceiling where one is set (LBAudioDetectiveDebugSetGridCeiling; 0: none) --
// never 0 for work > 0.  Results do not depend on the grid; a launch that really strides (a grid below its work) is counted.
// The plain grid-stride launches (x += gridDim.x * threads, nothing carried) take their grids from here as well, so that the
// tests' ceiling reaches their second trips: the stream and resampler banks, the duplicate groups' init, hook and flatten
// (k_groups.hip), the gather's copy launches (k_gather.hip), the top-K selection's histogram and gather passes (k_topk.hip,
// grid.x only) and every launch of the entry ids (k_ids.hip).  The corpus scans of k_compare.hip keep their own caps: the 10 M-entry tests cross them by shape.
inline std::atomic<uint32_t> g_grid_ceiling{0};
inline std::atomic<uint64_t> g_strided_launches{0};
inline uint32_t strided_grid(uint64_t work, uint32_t built_in_ceiling) {
    uint64_t grid = work < built_in_ceiling ? work : built_in_ceiling;
    const uint32_t tests = g_grid_ceiling.load(std::memory_order_relaxed);
    if (tests != 0 && grid > tests) grid = tests;
    if (grid == 0 && work > 0) grid = 1;
    if (grid < work) g_strided_launches.fetch_add(1, std::memory_order_relaxed);
    return (uint32_t)grid;
}

// ---- per-configuration device plan ---------------------------------------------------------
struct BandTable {
    std::vector<uint32_t> indices;  // bands + 1
    std::vector<uint32_t> lo, hi;   // bin bounds per band
    uint32_t kmin = 0, kmax = 0;    // union of [lo, hi) over non-empty bands (kmin == kmax: nothing read)
    // Where a window's power terms lie in LDS (k_rows_full.hip, k_rows_stream2.hip): band b's terms in bin order from word
    // term_at[b], the bands one after the other with a gap in front of a band where its first term would share a bank
    // (word mod 32) with an earlier band's -- the lanes that add the bands' terms side by side then never meet on a bank.
    // term_end: first word behind the last band.  ordered == false (a table whose bands overlap or are not in bin order;
    // make_band_table never makes one): terms by bin number, term_at[b] = lo[b] - kmin.
    std::vector<uint32_t> term_at;
    uint32_t term_end = 0;
    bool ordered = true;
    // 2048-sample windows on k_rows_full.hip: bit (q * 16 + u) * 2 + half is set when NO lane's bin of that place in the split
    // pass (k_rows_full.hip: slot_work) is read by a band -- the kernel has an instance that leaves the default table's out
    uint64_t unread_terms16 = 0;
};

// host-side, double precision; mirrors LBAudioDetective.m:361-371,382-383
void make_band_table(double sample_rate, uint32_t window, uint32_t bands, BandTable& out);
// bin bounds of every band when ComputeFrequencies is handed n_frames != window (a short read, :281,382-383);
// reads stay inside the window-sized buffer
void make_band_bounds(double sample_rate, uint32_t window, uint32_t n_frames, const BandTable& table, uint32_t* lo,
                      uint32_t* hi);
// master twiddle table exp(-2 pi i k / W), k in [0, W/2)
void make_twiddles(uint32_t W, std::vector<float>& re, std::vector<float>& im);

struct Plan {
    double sample_rate = 0;
    uint32_t window = 0, stride = 0, bands = 0, subfp_len = 0;
    uint32_t log2w = 0;
    uint32_t keep = 0;  // wavelets whose sign pair survives the truncation to subfp_len Booleans
    BandTable table;
    // device copies
    DeviceBuffer<float> d_tw;     // [W/2] re then [W/2] im
    DeviceBuffer<uint32_t> d_bands;  // [bands] lo, [bands] hi, [bands] divisor as float bits, ... (api_detective.cpp: eight rows + 1 word, then RN(1 / divisor) and "short division proven" from word 9 * bands)
    DeviceBuffer<float> d_bin_const; // per-bin twiddles of the pruned kernel (only when pruned_ok)
    bool pruned_ok = false;
    bool lanes_ok = false;        // ... and its band-sums-in-lanes form (rows_lanes_supported: the default 44.1 kHz table)
    bool full_ok = false;         // k_rows_full.hip applies
    bool stream_ok = false;       // k_rows_stream.hip applies (also uses d_claim)
    bool stream2_ok = false;      // k_rows_stream2.hip applies (preferred over k_rows_full.hip when the clip length is even)
    DeviceBuffer<uint32_t> d_claim;  // its per-XCD claim counters (8 words)
    // Structurally empty bands (round 4): a band whose bin range is empty is +0.0 in every window (17 of the 32
    // bands at 44.1 kHz / 1024).  `sparse.ok`: 32 bands and at most ONE live band among the left sixteen -- stage 1 then
    // writes compact frames (128 rows of the `n_stored` bands that can be non-zero: the live ones of the right sixteen in
    // ascending order, then the left half's one live band)
    // and stage 2 runs its sparse form (k_haar_select32.hip): one thread per row, and only the columns of the row
    // transform that can be non-zero go through the column transform and the select.
    struct Sparse {
        bool ok = false;
        uint32_t left = 32;            // the live band of the left half (32: none)
        uint32_t n_cols = 0;           // columns of the row transform's output that can be non-zero ...
        uint8_t cols[32] = {};         // ... in ascending ordered position
        uint32_t n_stored = 0;         // bands a compact frame's row holds
        uint8_t stored[17] = {};       // ... which ones, by position in the row
        uint8_t pos_right[16];         // position of band 16 + j in the row (0xFF: structurally empty, not stored)
        uint8_t pos_left = 0xFF;       // position of the left half's live band
        uint32_t frame_dw() const { return 128u * n_stored; }
    } sparse;
    // measurement knobs of the generic stage-1 kernel (LBAudioDetectiveSetKernelTuning): waves per workgroup
    // (0 = automatic) and whether the per-lane twiddle cache is used
    uint32_t tune_waves = 0;
    bool tune_cache = true;
    bool valid = false;
};

// End-of-file treatment of upstream's file loop for one file inside a float32 clip: the file's windows start at
// row `row_begin` / sample `pcm_begin` of the clip; windows from `first_short` on (counted from the file's first
// window) belong to reads that cannot be met in full.
struct FileDesc;
struct FileTail {
    uint32_t mode = 0;          // 1: nothing read -> all-zero rows; 2: partial reads over the stale spectrum; 3: mode 1 for a
                                //    whole batch in one launch (d_files / n_files / max_rows below, one FileTail in all)
    const FileDesc* d_files = nullptr;
    uint32_t n_files = 0;
    uint64_t max_rows = 0;
    uint64_t first_short = 0;   // first such window of the file
    uint64_t n_client = 0;      // samples the file really has at the processing rate
    const uint32_t* d_tbl = nullptr;   // mode 2: per window [n_read, lo[bands], hi[bands]] on the device
    uint64_t row_begin = 0;     // first row of the file inside the clip
    uint64_t rows = 0;          // rows of the file (0: all rows of the clip)
    uint64_t pcm_begin = 0;     // first sample of the file inside the clip
};

// ---- kernel launchers (k_*.hip) -------------------------------------------------------------
// windows -> frame rows.  frames: [n_clips * frames_per_clip][128][bands]
// fmt: 0 float32, 1 int16, 2 int32 samples
hipError_t launch_fft_bands(const Plan& plan, const void* d_pcm, uint32_t fmt, uint64_t n_clips,
                            uint64_t samples_per_clip, uint32_t frames_per_clip, float* d_frames, hipStream_t stream);
hipError_t launch_fft_bands_windows(const Plan& plan, const void* d_pcm, uint32_t fmt, uint64_t n_clips, uint64_t samples_per_clip,
                                    uint32_t windows_per_clip, float* d_frames, hipStream_t stream);
// frame rows -> packed sub-fingerprints.  d_haar (optional) receives the decomposed frames.
hipError_t launch_haar_select(const Plan& plan, float* d_frames, uint64_t n_frames, uint32_t* d_packed,
                              float* d_haar_out, hipStream_t stream);
// specialised stage 1 (k_rows_pruned.hip): 1024-sample windows whose bands read only bins 0..21
bool rows_pruned_supported(const Plan& plan);
void rows_pruned_constants(std::vector<float>& out);
// compact: rows of 16 floats (plan.sparse), else rows of 32
hipError_t launch_rows_pruned(const Plan& plan, const float* d_bin_const, const void* d_pcm, uint32_t fmt,
                              uint64_t n_clips, uint64_t samples_per_clip, uint32_t frames_per_clip, float* d_frames,
                              hipStream_t stream, bool compact = false, uint32_t band_form = 0);
// its second kernel, frame_rows_lanes_kernel: every band's bins in one lane, band sums in registers.  Applies where
// rows_pruned_supported holds and the plan's non-empty bands are exactly the compiled table's (44.1 kHz / 1024 / 32 bands);
// band_form of launch_rows_pruned: 0 takes it where it applies, 1 never, 2 takes it or fails.  rows_lanes_table appends its
// per-task rows to the band table (nothing for another table).
bool rows_lanes_supported(const Plan& plan);
void rows_lanes_table(const Plan& plan, std::vector<uint32_t>& band_tbl);

// specialised stage 1 without pruning (k_rows_full.hip): 1024- and 2048-sample windows, any band table
bool rows_full_supported(const Plan& plan);
bool rows_full_supported_fmt(const Plan& plan, uint32_t fmt);   // strides other than 64: float32 input only
hipError_t launch_rows_full(const Plan& plan, const void* d_pcm, uint32_t fmt, uint64_t n_clips,
                            uint64_t samples_per_clip, uint32_t frames_per_clip, float* d_frames, hipStream_t stream);

// specialised stage 1 for 4096-sample windows (k_rows_stream.hip): a wave walks the windows of a frame and keeps
// the sub-transforms consecutive windows share.  Needs an even samples_per_clip (aligned sample pairs).
bool rows_stream_supported(const Plan& plan);
hipError_t launch_rows_stream(const Plan& plan, const void* d_pcm, uint32_t fmt, uint64_t n_clips,
                              uint64_t samples_per_clip, uint32_t frames_per_clip, float* d_frames, hipStream_t stream);

// the same plan for 2048-sample windows (k_rows_stream2.hip; the reference's default configuration)
bool rows_stream2_supported(const Plan& plan);
hipError_t launch_rows_stream2(const Plan& plan, const void* d_pcm, uint32_t fmt, uint64_t n_clips,
                               uint64_t samples_per_clip, uint32_t frames_per_clip, float* d_frames, hipStream_t stream);

// specialised stage 2 (k_haar_select32.hip): 128 x 32 frames, keep <= 128
bool haar_select32_supported(const Plan& plan);
// compact: d_frames holds plan.sparse's rows of 16 floats (the sparse form; d_haar_out must be zeroed by the caller)
hipError_t launch_haar_select32(const Plan& plan, const float* d_frames, uint64_t n_frames, uint32_t* d_packed,
                                float* d_haar_out, hipStream_t stream, bool compact = false);
void plan_sparse(Plan& plan);    // fills plan.sparse from plan.table

// ---- stage 2 at a row hop (frame phases) ------------------------------------------------------------
// The hop forms of stage 2 read a frame's 128 rows from TWO row runs: rows [0, split) at run A's rows
// a_row0 + ((a_first + r) & mask), rows [split, 128) at run B's rows b_row0 + (r - split).  Two ways to say which:
//
// batch (list == null): P phases of a clip; frame j of phase p is the 128 rows from row p * hop + 128 j of the clip's row run.
//   The run's first 128 * count0 rows are what stage 1 wrote for the clip (A = d_frames, clip * 128 * count0 rows in); the rows
//   behind them, which only a phase's last frame reads, are in B = `tail`: per clip ONE frame of rows, the run's rows
//   tail_row0 .. tail_row0 + 127 (tail_row0 <= 128 * count0: a straddling frame reads from both).  Phases 0 .. full_phases - 1
//   have count0 frames, the others count0 - 1; the output is [clip][phase][count0] slots, zero at and behind a phase's count.
// list (the phased stream bank): workgroup g takes list[g]; A = d_frames is the channels' row rings (128 rows each, row number
//   t of a channel at t mod 128: mask 127), B = `tail` the rows the push has just transformed; output slot g.
struct HopFrame {
    uint64_t a_row0, b_row0;
    uint32_t a_first, split;            // split <= 128
    uint32_t pad[2];
};
static_assert(sizeof(HopFrame) == 32, "HopFrame is uploaded as it is");
struct StageHop {
    const float* tail = nullptr;
    uint32_t phases = 1, hop = kRowsPerFrame;
    uint32_t count0 = 0, full_phases = 1;
    uint32_t tail_row0 = 0;
    const HopFrame* list = nullptr;
    uint32_t n_list = 0;
};
inline bool stage_hop_valid(const StageHop& h) {
    if (h.list) return h.n_list <= 0x7fffffffu;
    const uint64_t last = (uint64_t)(h.full_phases - 1) * h.hop + (uint64_t)kRowsPerFrame * h.count0;   // behind the last row any frame reads
    return h.phases >= 1 && h.phases <= 32 && (h.phases & (h.phases - 1)) == 0 && h.hop * h.phases == kRowsPerFrame && h.count0 >= 1 &&
           h.count0 <= 0xFFFFFFFFu / kRowsPerFrame - 1 && h.full_phases >= 1 && h.full_phases <= h.phases &&
           (h.tail ? (uint64_t)h.tail_row0 <= (uint64_t)kRowsPerFrame * h.count0 && last <= (uint64_t)h.tail_row0 + kRowsPerFrame
                   : h.full_phases == 1);
}
inline uint64_t stage_hop_frames(const StageHop& h, uint64_t n_clips) { return h.list ? h.n_list : n_clips * h.phases * h.count0; }
#if defined(__HIPCC__)
struct HopSource {
    uint64_t a_row0, b_row0;
    uint32_t a_first, split, mask;
    bool empty;                         // a slot at or behind its phase's count: zeros
};
// what workgroup `slot` reads (workgroup-uniform)
__device__ __forceinline__ HopSource hop_source(const StageHop& h, uint32_t slot) {
    HopSource s;
    if (h.list) {
        const HopFrame f = h.list[slot];
        s.a_row0 = f.a_row0; s.b_row0 = f.b_row0; s.a_first = f.a_first; s.split = f.split;
        s.mask = kRowsPerFrame - 1;
        s.empty = false;
        return s;
    }
    const uint32_t j = slot % h.count0, cp = slot / h.count0;
    const uint32_t phase = cp % h.phases, clip = cp / h.phases;
    const uint32_t first = phase * h.hop + kRowsPerFrame * j, main_rows = kRowsPerFrame * h.count0;
    s.empty = j >= h.count0 - (phase < h.full_phases ? 0u : 1u);
    s.a_row0 = (uint64_t)clip * main_rows;
    s.a_first = first;
    s.mask = 0xFFFFFFFFu;
    s.split = first < main_rows ? main_rows - first : 0u;      // (>= 128: the whole frame is in A)
    s.b_row0 = (uint64_t)clip * kRowsPerFrame + (main_rows - h.tail_row0);
    return s;
}
// row `row` of the frame; rows of row_dw floats
__device__ __forceinline__ const float* hop_row(const float* run_a, const float* run_b, const HopSource& s, uint32_t row, uint32_t row_dw) {
    return row < s.split ? run_a + (s.a_row0 + ((s.a_first + row) & s.mask)) * row_dw : run_b + (s.b_row0 + (row - s.split)) * row_dw;
}
#endif
hipError_t launch_haar_select32_hop(const Plan& plan, const float* d_frames, const StageHop& hop, uint64_t n_clips, uint32_t* d_packed,
                                    hipStream_t stream, bool compact = false);
hipError_t launch_haar_select_hop(const Plan& plan, const float* d_frames, const StageHop& hop, uint64_t n_clips, uint32_t* d_packed,
                                  hipStream_t stream);

// ---- stage 1: ONE decision per call (api_detective.cpp: stage1_choose), and per kernel file ONE function that names the
// template instance -- each launcher dispatches on what its function returns and LBAudioDetectiveDebugStage1Choice reports the
// same value, so the report cannot drift from the launch.  None of them touches a device.
enum class Stage1Family : uint32_t { Generic = 0, Pruned = 1, Stream2 = 2, Full = 3, Stream = 4 };
// fft_bands_kernel<log2w, wpb, cached> (k_fft_bands.hip)
struct FftBandsInstance {
    uint32_t log2w = 0, wpb = 0;
    bool cached = false;
};
FftBandsInstance fft_bands_instance(const Plan& plan);
// rows_full_kernel<log2l, fmt, s64, lean ? the default table's unread terms : 0> (k_rows_full.hip).  ok == false: integer
// input at a stride other than 64 (rows_full_supported_fmt), the launch fails
struct RowsFullInstance {
    uint32_t log2l = 0, fmt = 0;
    bool s64 = false, lean = false, ok = false;
};
RowsFullInstance rows_full_instance(const Plan& plan, uint32_t fmt);
// rows_stream2_kernel<fmt, qlo, qhi> (k_rows_stream2.hip)
struct RowsStream2Instance {
    uint32_t fmt = 0, qlo = 0, qhi = 0;
};
RowsStream2Instance rows_stream2_instance(const Plan& plan, uint32_t fmt);
// what the decision looks at beside the plan
struct Stage1Call {
    uint32_t variant = 0, fmt = 0;
    uint64_t n_clips = 0, spc = 0;
    uint32_t ptr_mod8 = 0;          // the clip pointer's address modulo 8
    bool raw_tap = false, tail = false;
};
struct Stage1Choice {
    OSStatus status = noErr;        // what the call returns as far as the choice decides it
    bool launches = false;          // false: the status is an error, or there is no clip or no whole frame
    uint64_t per = 0;               // frames per clip
    Stage1Family family = Stage1Family::Generic;
    FftBandsInstance generic;       // the family's instance (the others stay zero)
    RowsFullInstance full;
    RowsStream2Instance stream2;
    bool compact = false;           // rows of plan.sparse's stored bands between the stages
    bool stage2_select32 = false;   // k_haar_select32.hip (its sparse form when compact), else k_haar_select.hip
};
Stage1Choice stage1_choose(const Plan& plan, const Stage1Call& call);
constexpr uint32_t kStage1ChoiceWords = 12;
void stage1_choice_words(const Stage1Choice& ch, const Stage1Call& call, const Plan& plan, uint32_t* out12);   // LBAudioDetectiveDebugStage1Choice's words
// the host half of a plan: everything stage1_choose reads (table, sparse form, which specialised kernels apply), no device
OSStatus plan_host(Plan& p, double rate, uint32_t window, uint32_t stride, uint32_t bands, uint32_t subfp_len);

// end-of-file chain of upstream's file loop, tail mode "stale" (k_file_tail.hip); d_tbl: per window
// [n_read, lo[bands], hi[bands]]
hipError_t launch_empty_rows(const Plan& p, float* d_rows, uint64_t n_rows, hipStream_t stream);
hipError_t launch_file_tail(const Plan& plan, const float* d_pcm, uint64_t n_client, uint32_t hop, uint64_t first_short,
                            uint32_t n_tail, const uint32_t* d_tbl, float* d_frames, hipStream_t stream);

// generic matrix ops behind the Frame API
// one file of a batch for the table-driven kernels (k_decode.hip, k_resample.hip, k_file_tail.hip)
struct FileDesc {
    uint32_t kind, channels, bits, flags;      // AudioPayload::Kind; flags: 1 float samples, 2 little endian
    uint64_t bytes_off, total_frames;          // payload inside the batch's byte block; frames it decodes to
    uint64_t dec_off, first, n_in;             // decoded samples inside the batch's block; first / count that are valid
    uint64_t out_off, n_write;                 // the file's slot in the clip; samples to write there
    uint32_t mode, copy;                       // converter model; 1: rates equal, copy
    double ratio, scale, half;                 // ResamplePlan
    uint64_t row_begin, rows, first_short;     // the file's rows in the clip; first window whose read is short
    // rational position (audiofile.hpp, PhaseTable): q != 0, the phases' weights on the device
    uint64_t ph_p, ph_q;
    int32_t ph_m_min;
    uint32_t ph_m_span;
    const int32_t* ph_first;
    const uint32_t* ph_count;
    const double* ph_wsum;
    const double* ph_w;
};
struct PhaseTable;
// the device copy of a phase table, made on first use and kept by the detective
struct DevPhase {
    const PhaseTable* host = nullptr;
    DeviceBuffer<int32_t> first;
    DeviceBuffer<uint32_t> count;
    DeviceBuffer<double> wsum, w;
};
OSStatus device_phase(struct ::LBAudioDetective* d, const PhaseTable* host, hipStream_t stream, FileDesc& f);
hipError_t launch_decode_batch(const FileDesc* d_files, uint32_t n_files, uint64_t max_units, const uint8_t* d_bytes,
                               float* d_decoded, hipStream_t stream);
hipError_t launch_resample_batch(const FileDesc* d_files, uint32_t n_files, uint64_t max_out, const float* d_decoded, int res,
                                 const double* d_table, uint64_t table_n, float* d_pcm, hipStream_t stream);
hipError_t launch_empty_rows_batch(const Plan& p, const FileDesc* d_files, uint32_t n_files, uint64_t max_rows, float* d_frames,
                                   hipStream_t stream);
hipError_t launch_haar2d_generic(float* d_m, float* d_tmp, uint32_t rows, uint32_t cols, hipStream_t stream);
hipError_t launch_extract_generic(const float* d_m, uint32_t n, uint32_t n_wavelets, uint8_t* d_out,
                                  hipStream_t stream);

// compare
// slot layout: entries[e][s][8 words]; writes per-entry score (optional) and atomically maxes the key
hipError_t launch_compare_slots(const uint32_t* d_entries, uint64_t n_entries, uint32_t n_sub, uint32_t subfp_len,
                                const uint32_t* d_query, uint32_t n_query, uint32_t range, uint64_t index_base,
                                float* d_scores, unsigned long long* d_key, hipStream_t stream);
// one fingerprint against one (slot layout, a = the side with at least as many sub-fingerprints): the score's
// float bits are atomicMax-ed into *d_out_bits (zeroed by the caller)
hipError_t launch_compare_pair(const uint32_t* d_a, uint32_t n1, const uint32_t* d_b, uint32_t n2, uint32_t subfp_len,
                               uint32_t range, unsigned int* d_out_bits, hipStream_t stream);
// plane layout (tight bitstream, 16-byte planes); supported shapes only
bool planes_supported(uint32_t subfp_len, uint32_t n_sub);
uint32_t planes_per_entry(uint32_t subfp_len, uint32_t n_sub);
hipError_t launch_pack_planes(const uint32_t* d_slots, uint64_t n_entries, uint32_t n_sub, uint32_t subfp_len,
                              uint4* d_planes, uint64_t plane_stride, uint64_t first, hipStream_t stream);
hipError_t launch_compare_planes_generic(const uint4* d_planes, uint64_t plane_stride, uint64_t n_entries,
                                         uint32_t n_sub, uint32_t subfp_len, const uint32_t* d_query,
                                         uint32_t n_query, uint32_t range, uint64_t index_base, float* d_scores,
                                         unsigned long long* d_key, hipStream_t stream);
// specialised scan (200-Boolean sub-fingerprints, query and entries of equal count <= 8)
bool planes_fast_supported(uint32_t subfp_len, uint32_t n_sub, uint32_t n_query);
uint32_t planes_fast_const_words(uint32_t n_sub);
void build_plane_query(const uint32_t* q_slots, uint32_t n_sub, uint32_t range, std::vector<uint32_t>& out);
// d_ticket / host_out_dev / seq: optional tail for the host-synchronous query: d_key is then an array of
// kScanSlots per-workgroup slots, the last workgroup reduces them and hands the key to pinned host memory;
// pass nullptr to get the plain device-key behaviour
constexpr uint32_t kScanSlots = 512;
hipError_t launch_compare_planes_fast(const uint4* d_planes, uint64_t plane_stride, uint64_t n_entries,
                                      uint32_t n_sub, const uint32_t* d_qc, uint64_t index_base, float* d_scores,
                                      unsigned long long* d_key, hipStream_t stream, unsigned int* d_ticket = nullptr,
                                      unsigned long long* host_out_dev = nullptr, unsigned long long seq = 0);
uint32_t plane_query_words();
hipError_t launch_compare_planes_batch(const uint4* d_planes, uint64_t plane_stride, uint64_t n_entries, uint32_t n_sub,
                                       const uint32_t* d_qblocks, uint32_t n_queries, uint64_t index_base,
                                       unsigned long long* d_keys, hipStream_t stream);
void pack_fingerprint(const struct ::LBAudioDetectiveFingerprint* fp, std::vector<uint32_t>& out);
// the batch scan's scores-writing form: d_scores receives n_queries rows of n_entries scores (row q at d_scores + q * n_entries)
hipError_t launch_compare_planes_batch_scores(const uint4* d_planes, uint64_t plane_stride, uint64_t n_entries, uint32_t n_sub,
                                              const uint32_t* d_qblocks, uint32_t n_queries, float* d_scores, hipStream_t stream);
constexpr uint32_t kQueryBatchMax = 8;   // queries per pass of the batch scan (k_compare.hip: kQueryBatch)

// top-K selection (k_topk.hip): per row of n scores (row r at d_scores + r * n) the k <= kTopKMax largest keys
// (score bits << 32) | (0xFFFFFFFF - (index_base + e)) of the entries whose score is > 0 (NaN never), descending, 0-padded,
// to d_keys + r * k.  d_scratch: topk_scratch_bytes(rows) bytes, initialised by the sequence itself; a fixed sequence of
// launches on `stream`, no host round trip.  index_base + n <= 2^32.
constexpr uint32_t kTopKMax = LBAD_TOPK_MAX;
size_t topk_scratch_bytes(uint32_t rows);
hipError_t launch_topk_keys(const float* d_scores, uint64_t n, uint32_t rows, uint32_t k, uint64_t index_base, void* d_scratch,
                            unsigned long long* d_keys, hipStream_t stream);

// threshold selection (k_threshold.hip): per row of n scores (row r at d_scores + r * n, 4-byte aligned) the keys of the entries
// whose score is >= threshold (a float compare; threshold > 0), in ascending entry index, the first min(count, capacity) of them
// to d_keys + r * capacity, zero keys behind them, and the true count to d_counts[r].  d_scratch: threshold_scratch_bytes(n,
// rows) bytes, written before they are read; a memset and three launches on `stream`, no host round trip.  rows <=
// kThresholdRowsMax, index_base + n <= 2^32.
constexpr uint32_t kThresholdRowsMax = kQueryBatchMax;
size_t threshold_scratch_bytes(uint64_t n, uint32_t rows);
hipError_t launch_threshold_keys(const float* d_scores, uint64_t n, uint32_t rows, float threshold, uint64_t capacity,
                                 uint64_t index_base, void* d_scratch, unsigned long long* d_keys, unsigned long long* d_counts,
                                 hipStream_t stream);

// corpus join (k_join.hip): every pair (row of `queries`, entry of the scanned corpus; two uniform corpora of ONE specialised
// shape) whose score -- the row as the query of the specialised scan -- is >= threshold, as CSR: the keys in (row, entry)
// order to d_keys where their position is below the capacity, the offsets of the rows to the caller's offsets.  The call's
// constants:
struct JoinCall {
    const uint4* d_planes = nullptr;     // the scanned corpus: planes, plane stride (its capacity), entries
    uint64_t stride = 0, n_entries = 0;
    const uint4* d_qplanes = nullptr;    // the rows' corpus
    uint64_t qstride = 0;
    uint32_t n_sub = 0, range = 0;
    float threshold = 0.0f;
    bool skip = false;                   // leave out the pair whose row index equals the entry's index
    uint64_t capacity = 0, index_base = 0;
    unsigned long long* d_keys = nullptr;    // `capacity` slots, zeroed by the caller
    hipStream_t stream = nullptr;
};
// scratch of a chunk of `rows` rows against n_entries entries, and the rows a chunk may have under a limit (a whole number of
// row tiles; 0: the limit is too small for one tile)
size_t join_scratch_bytes(uint64_t n_entries, uint64_t rows);
uint64_t join_chunk_rows(uint64_t n_entries, uint64_t limit_bytes);
// one chunk: `rows` rows from row `first_row` of the rows' corpus; out_offsets: the caller's offsets AT the chunk's first row
// (rows + 1 words are written: the last is the running total).  d_scratch: join_scratch_bytes(n_entries, chunk_rows_max) bytes,
// the SAME block and chunk_rows_max for every chunk of a call -- its first words carry the total from chunk to chunk;
// first_chunk starts it at 0.  Five launches on the call's stream, nothing visits the host.
hipError_t launch_join_chunk(const JoinCall& call, void* d_scratch, uint32_t chunk_rows_max, uint64_t first_row, uint32_t rows,
                             uint32_t first_chunk, unsigned long long* out_offsets);
// the two scans between a join's count and scatter kernels: counts[row][entry tile] -> tile_at (offsets inside the row), row_base
// and the caller's offsets on top of *state (the total carried between chunks); shared with k_join_ragged.hip
void launch_join_scans(const uint32_t* counts, uint64_t etiles, uint32_t rows, uint32_t* tile_at, unsigned long long* row_base,
                       unsigned long long* state, uint32_t first_chunk, unsigned long long* out_offsets, hipStream_t stream);

// ragged corpus join (k_join_ragged.hip): the same CSR for two RAGGED corpora of one sub-fingerprint length; the score of a pair
// is the ragged scan's (the shorter slides along the longer), and each match's signed lag goes to d_lags where that is given.
struct JoinRaggedCall {
    const uint4* d_recs = nullptr;       // the scanned corpus: records, record positions, entries
    const uint32_t* d_off = nullptr;
    uint64_t n_entries = 0;
    const uint4* d_qrecs = nullptr;      // the rows' corpus
    const uint32_t* d_qoff = nullptr;
    uint32_t q_ne_max = 0;               // its longest entry (<= LBAD_JOIN_RAGGED_MAX_SUBFINGERPRINTS, as the scanned corpus')
    uint32_t subfp_len = 0, range = 0;
    float threshold = 0.0f;
    bool skip = false;
    uint64_t capacity = 0, index_base = 0;
    unsigned long long* d_keys = nullptr;    // `capacity` slots, zeroed by the caller
    int32_t* d_lags = nullptr;               // optional: `capacity` slots, zeroed by the caller
    hipStream_t stream = nullptr;
};
// as join_scratch_bytes / join_chunk_rows / launch_join_chunk (four launches: no row blocks are built)
size_t join_ragged_scratch_bytes(uint64_t n_entries, uint64_t rows);
uint64_t join_ragged_chunk_rows(uint64_t n_entries, uint64_t limit_bytes);
hipError_t launch_join_ragged_chunk(const JoinRaggedCall& call, void* d_scratch, uint32_t chunk_rows_max, uint64_t first_row,
                                    uint32_t rows, uint32_t first_chunk, unsigned long long* out_offsets);

// what a call of the occurrences pass is, whichever family folds its cells (k_occurrences.hip, k_recording.hip, k_timeline.hip)
struct OcPassCall {
    const uint4* d_recs = nullptr;       // the corpus: records, record positions
    const uint32_t* d_off = nullptr;
    uint32_t ne_min = 0, ne_max = 0;     // its shortest and longest entry (ne_max <= LBAD_OCCURRENCES_MAX_ENTRY_SUBFINGERPRINTS)
    uint32_t subfp_len = 0, range = 0;
    const uint32_t* d_qwords = nullptr;  // the query as build_align_query's ragged form, 16-byte aligned, on the device
    uint32_t n_query = 0;
    uint64_t tiles = 0;                  // tiles per entry, the family's bound over every pair of the call (stated at its struct)
    hipStream_t stream = nullptr;
};

// occurrences (k_occurrences.hip): every cell (entry, sliding offset) of ONE query against a ragged corpus whose quotient q_o --
// LBAudioDetectiveCorpusMatchProfile's value -- is >= threshold (with `peaks`: and a local peak of its profile), in (entry,
// offset) order: keys and, where given, signed lags to the slots below the capacity.
struct OccurrencesCall : OcPassCall {    // tiles: occurrences_tiles(n_query, ne_min, ne_max)
    float threshold = 0.0f;
    bool peaks = false;
    uint64_t capacity = 0, index_base = 0;
    unsigned long long* d_keys = nullptr;    // `capacity` slots, zeroed by the caller
    int32_t* d_lags = nullptr;               // optional: `capacity` slots, zeroed by the caller
};
uint32_t occurrences_block_entries();    // entries a chunk is a whole number of
// tiles per entry: a bound over every pair of the call
uint64_t occurrences_tiles(uint32_t n_query, uint32_t ne_min, uint32_t ne_max);
// scratch of a chunk of `entries` entries, the entries a chunk may have under a limit (0: the limit is too small for one block of
// entries), and the LDS of a workgroup
size_t occurrences_scratch_bytes(uint64_t entries, uint64_t tiles);
uint64_t occurrences_chunk_entries(uint64_t tiles, uint64_t limit_bytes);
size_t occurrences_lds_bytes(uint32_t n_query, uint32_t ne_max);
// one chunk: `entries` entries from `first_entry`.  d_scratch: occurrences_scratch_bytes(chunk_entries_max, tiles) bytes, the SAME
// block and chunk_entries_max for every chunk of a call -- its first word carries the total from chunk to chunk (first_chunk
// starts it at 0) and holds the call's total behind the last chunk.  Four launches on the call's stream, nothing visits the host.
hipError_t launch_occurrences_chunk(const OccurrencesCall& call, void* d_scratch, uint64_t chunk_entries_max, uint64_t first_entry,
                                    uint64_t entries, uint32_t first_chunk);
constexpr uint64_t kJoinScratchDefault = 256ull << 20;   // LBAudioDetectiveCorpusSetJoinScratchLimit's 0

// recording scores (k_recording.hip): the occurrences pass' cells of ONE query against a ragged corpus folded per entry to the
// largest cell -- the ragged scan's score, bit for bit -- and the lowest offset that reaches it as the signed lag.
struct RecordingCall : OcPassCall {      // tiles: occurrences_tiles(n_query, ne_min, ne_max)
    float* d_scores = nullptr;           // one per entry of the CORPUS (a chunk writes its own entries')
    int32_t* d_lags = nullptr;           // optional: likewise
};
// scratch of a chunk of `entries` entries (one 64-bit partial per entry and tile) and the entries a chunk may have under a limit
// (a whole number of occurrences_block_entries(); 0: the limit is too small for one block)
size_t recording_scratch_bytes(uint64_t entries, uint64_t tiles);
uint64_t recording_chunk_entries(uint64_t tiles, uint64_t limit_bytes);
// one chunk: `entries` entries from `first_entry`, every word of d_scratch written before it is read.  Two launches on the call's
// stream, nothing visits the host.
hipError_t launch_recording_chunk(const RecordingCall& call, void* d_scratch, uint64_t first_entry, uint64_t entries);
// d_lags[slot] = d_entry_lags[entry that d_keys[slot] names], 0 for a zero key; n <= 2^31 slots, index_base + count <= 2^32
hipError_t launch_recording_lag_gather(const unsigned long long* d_keys, uint64_t n, uint64_t index_base, uint64_t count,
                                       const int32_t* d_entry_lags, int32_t* d_lags, hipStream_t stream);

// recording timeline (k_timeline.hip): the occurrences pass' cells of ONE query against a ragged corpus folded per OFFSET of the
// query over the entries not longer than it: the largest key  q_o bits << 32 | 0xFFFFFFFF - (index base + entry)  of the cells
// at or above the threshold, 0 where there is none.
struct TimelineCall : OcPassCall {       // tiles: timeline_tiles(n_query, ne_min); ne_min <= n_query
    float threshold = 0.0f;
    uint64_t index_base = 0;
    unsigned long long* d_keys = nullptr;    // n_query words, zeroed by the caller in front of the first chunk
};
uint32_t timeline_block_entries();       // entries a chunk is a whole number of
// tiles of 126 offsets that hold every offset an entry not longer than the query can start at
uint64_t timeline_tiles(uint32_t n_query, uint32_t ne_min);
// scratch of a chunk of `entries` entries (one 64-bit partial per block of timeline_block_entries() entries and offset of a tile)
// and the entries a chunk may have under a limit (a whole number of blocks; 0: the limit is too small for one)
size_t timeline_scratch_bytes(uint64_t entries, uint64_t tiles);
uint64_t timeline_chunk_entries(uint64_t tiles, uint64_t limit_bytes);
// one chunk: `entries` entries from `first_entry` folded into d_keys, every word of d_scratch written before it is read.  Two or
// three launches on the call's stream, nothing visits the host.
hipError_t launch_timeline_chunk(const TimelineCall& call, void* d_scratch, uint64_t first_entry, uint64_t entries);
// d_lengths[o] = sub-fingerprints of the entry d_keys[o] names, 0 for a zero key; n < 2^31 offsets, index_base + count <= 2^32
hipError_t launch_timeline_lengths(const unsigned long long* d_keys, uint32_t n, uint64_t index_base, uint64_t count,
                                   const uint32_t* d_off, uint32_t* d_lengths, hipStream_t stream);

// batch recording timeline (k_timeline_batch.hip): the timeline above for `recordings` recordings of n_query sub-fingerprints each,
// one after the other in d_qwords and in d_keys.  A call runs in passes over recordings and, within a pass, in chunks over entries.
constexpr uint32_t kTimelineBatchFormShared = 0;   // form S: the single call's mapping, the recording one more coordinate of a unit
constexpr uint32_t kTimelineBatchFormWave = 1;     // form W: a window per wave, for recordings of fewer than four tiles
struct TimelineBatchPlan {
    uint32_t form = kTimelineBatchFormShared;
    uint64_t tiles = 0;                  // timeline_tiles(n_query, ne_min), per recording
    uint32_t recordings_per_pass = 0;
    uint64_t entries_per_chunk = 0;      // a multiple of timeline_block_entries(), or the corpus rounded up to one (0: empty corpus)
    uint64_t scratch_bytes = 0;          // recordings_per_pass x timeline_scratch_bytes(entries_per_chunk, tiles)
    uint64_t lds_bytes = 0;              // of a workgroup of the form's maxima kernel
};
// THE plan of a call, the debug symbol's and the real call's: several recordings a pass when one recording's whole-corpus partials
// fit the limit (0: kJoinScratchDefault), else one recording a pass with the single call's entry chunks; recordings x entries x
// tiles of a pass within the pair loop's 32-bit indices.  Form W exactly when tiles < 4 and four windows of 126 + 2 + ne_max
// records with the table fit the LDS budget (and the tests do not force form S).  false: the limit holds no block of entries of
// one recording.  With one recording: the single call's tiles, chunk and scratch.
bool timeline_batch_plan(uint32_t recordings, uint32_t per, uint32_t ne_min, uint32_t ne_max, uint64_t entries, uint64_t limit_bytes,
                         bool force_shared, TimelineBatchPlan* plan);
// one chunk of one pass: `recordings` recordings from call.d_qwords / call.d_keys on, `entries` entries from `first_entry`, folded
// into the keys; d_scratch: plan.scratch_bytes, every word written before it is read.  Two or three launches on the call's stream.
hipError_t launch_timeline_batch_chunk(const TimelineCall& call, const TimelineBatchPlan& plan, uint32_t recordings, void* d_scratch,
                                       uint64_t first_entry, uint64_t entries);

// batch recording scores (k_recording_batch.hip): the recording scores above for `recordings` recordings of n_query sub-fingerprints
// each, one after the other in d_qwords; scores and lags as rows of `pitch` words, one per recording.  A call runs in passes over
// recordings and, within a pass, in chunks over entries.
constexpr uint32_t kRecordingBatchFormShared = 0;  // form S: the single call's mapping, the recording one more coordinate of a unit
constexpr uint32_t kRecordingBatchFormWave = 1;    // form W: a window per wave, for recordings of fewer than four tiles
struct RecordingBatchPlan {
    uint32_t form = kRecordingBatchFormShared;
    uint64_t tiles = 0;                  // occurrences_tiles(n_query, ne_min, ne_max), per recording
    uint32_t recordings_per_pass = 0;
    uint64_t entries_per_chunk = 0;      // a multiple of occurrences_block_entries(), or the corpus rounded up to one (0: empty corpus)
    uint64_t scratch_bytes = 0;          // recordings_per_pass x recording_scratch_bytes(entries_per_chunk, tiles)
    uint64_t lds_bytes = 0;              // of a workgroup of the form's maxima kernel
};
// THE plan of a call, the debug symbol's and the real call's: several recordings a pass when one recording's whole-corpus partials
// fit the limit (0: kJoinScratchDefault) -- the smallest of the recordings, limit / those partials, kOcMaxItems / (entries x
// tiles), 65 535 and, for the key form, the rows of a score and a lag per entry that fit the same limit (at least one) -- else one
// recording a pass with the single call's entry chunks.  Form W exactly when tiles < 4 and four windows of 126 + 2 + ne_max records
// with the table fit the LDS budget (and the tests do not force form S).  false: the limit holds no block of entries of one
// recording.  With one recording: the single call's tiles, chunk and scratch.
bool recording_batch_plan(uint32_t recordings, uint32_t per, uint32_t ne_min, uint32_t ne_max, uint64_t entries, uint64_t limit_bytes,
                          bool key_form, bool force_shared, RecordingBatchPlan* plan);
// one chunk of one pass: `recordings` recordings from call.d_qwords on, `entries` entries from `first_entry`; call.d_scores (and
// d_lags, optional) are row 0 of the pass, rows `pitch` words apart.  d_scratch: plan.scratch_bytes, every word written before it
// is read.  Two launches on the call's stream.
hipError_t launch_recording_batch_chunk(const RecordingCall& call, const RecordingBatchPlan& plan, uint32_t recordings, uint64_t pitch,
                                        void* d_scratch, uint64_t first_entry, uint64_t entries);
// d_lags[r][slot] = d_entry_lags[r][entry that d_keys[r][slot] names] over rows x k slots (rows of `count` entry lags), 0 for a zero
// key; rows x k <= 2^31, index_base + count <= 2^32
hipError_t launch_recording_batch_lag_gather(const unsigned long long* d_keys, uint32_t rows, uint32_t k, uint64_t index_base, uint64_t count,
                                             const int32_t* d_entry_lags, int32_t* d_lags, hipStream_t stream);

// batch occurrences (k_occurrences_batch.hip): the occurrences above for `recordings` recordings of n_query sub-fingerprints each,
// one after the other in d_qwords; keys and lags as rows of `capacity` slots, one per recording, and a count per recording.  A call
// runs in passes over recordings and, within a pass of ONE recording, in chunks over entries.
constexpr uint32_t kOccurrencesBatchFormShared = 0;    // form S: the single call's unit, the recording one more coordinate
constexpr uint32_t kOccurrencesBatchFormWave = 1;      // form W: a window per wave, for recordings of fewer than four tiles
struct OccurrencesBatchPlan {
    uint32_t form = kOccurrencesBatchFormShared;
    uint64_t tiles = 0;                  // occurrences_tiles(n_query, ne_min, ne_max), per recording
    uint32_t recordings_per_pass = 0;
    uint64_t entries_per_chunk = 0;      // a multiple of occurrences_block_entries(), or the corpus rounded up to one (0: empty corpus)
    uint64_t scratch_bytes = 0;          // recordings_per_pass x occurrences_scratch_bytes(entries_per_chunk, tiles)
    uint64_t lds_bytes = 0;              // of a workgroup of the form's count and scatter kernels
};
// THE plan of a call, the debug symbol's and the real call's: several recordings a pass when one recording's scratch for the whole
// corpus fits the limit (0: kJoinScratchDefault) -- the smallest of the recordings, limit / that scratch, kOcMaxItems / (entries x
// tiles) and 65 535 -- else one recording a pass with the single call's entry chunks and its carried total.  Form W exactly when
// tiles < 4 and four windows of 126 + 2 + ne_max records with the table fit the LDS budget (and the tests do not force form S).
// false: the limit holds no block of entries of one recording.  With one recording: the single call's tiles, chunk and scratch.
bool occurrences_batch_plan(uint32_t recordings, uint32_t per, uint32_t ne_min, uint32_t ne_max, uint64_t entries, uint64_t limit_bytes,
                            bool force_shared, OccurrencesBatchPlan* plan);
// one chunk of one pass: `recordings` recordings from call.d_qwords on, `entries` entries from `first_entry`; call.d_keys (and
// d_lags, optional) are row 0 of the pass, rows call.capacity slots apart, zeroed by the caller.  A pass of more than one recording
// is ONE chunk of the whole corpus (first_chunk 1) and writes its recordings' counts to d_counts; a pass of one recording
// (plan.recordings_per_pass == 1) carries its total in the first word of d_scratch as launch_occurrences_chunk does, for the
// caller to copy.  d_scratch: plan.scratch_bytes, the SAME block for every chunk of a pass.  Four or five launches on the call's
// stream, nothing visits the host.
hipError_t launch_occurrences_batch_chunk(const OccurrencesCall& call, const OccurrencesBatchPlan& plan, uint32_t recordings,
                                          void* d_scratch, uint64_t first_entry, uint64_t entries, uint32_t first_chunk,
                                          unsigned long long* d_counts);
// d_counts[r] = d_offsets[(r + 1) x stride] - d_offsets[r x stride] for the recordings of a pass: the scans' offsets, `stride` rows
// a recording (k_occurrences_batch.hip's totals kernel, for the batch and the tail lists)
hipError_t launch_occurrences_totals(const unsigned long long* d_offsets, uint32_t recordings, uint32_t stride, unsigned long long* d_counts,
                                     hipStream_t stream);
// tail occurrences (k_occurrences_tail.hip): the batch occurrences' rows with only the cells whose entry ends inside a recording's
// newest d_r = min(new count on the device, max_new, n_query) sub-fingerprints, for the entries not longer than the recording; no
// peak rule.  A call runs in passes over recordings and, within a pass of ONE recording, in chunks over entries.
struct OccurrencesTailPlan {
    uint32_t lanes = 0;                  // D: the next power of two >= max_new, the lanes of a recording
    uint32_t recordings_per_workgroup = 0;   // 256 / D, fewer where that many sub-windows do not fit the LDS (at least 1)
    uint32_t window_records = 0;         // a recording's sub-window: min(n_query, min(ne_max, n_query) + D - 1)
    uint64_t lds_bytes = 0;              // recordings_per_workgroup x window_records x 36 + the table
    uint32_t recordings_per_pass = 0;
    uint64_t entries_per_chunk = 0;      // a multiple of occurrences_block_entries(), or the corpus rounded up to one (0: empty corpus)
    uint64_t scratch_bytes = 0;          // recordings_per_pass x occurrences_scratch_bytes(entries_per_chunk, 1)
};
// the four fields a workgroup's shape is (plan.cpp): what the launch holds the plan against
void occurrences_tail_shape(uint32_t per, uint32_t ne_max, uint32_t max_new, OccurrencesTailPlan* plan);
// THE plan of a call, the debug symbol's and the real call's (plan.cpp): the shape above; several recordings a pass when one
// recording's scratch for the whole corpus (the occurrences' formula with ONE tile) fits the limit (0: kJoinScratchDefault) -- the
// smallest of the recordings, limit / that scratch, kOcMaxItems / entries and 65 535 -- else one recording a pass in entry chunks
// with the carried total.  false: the limit holds no block of entries of one recording.  1 <= max_new <= 64.
bool occurrences_tail_plan(uint32_t recordings, uint32_t per, uint32_t ne_min, uint32_t ne_max, uint64_t entries, uint32_t max_new,
                           uint64_t limit_bytes, OccurrencesTailPlan* plan);
// one chunk of one pass: `recordings` recordings from call.d_qwords on with their new counts from d_new_counts on, `entries` entries
// from `first_entry`; call.tiles == 1, call.peaks unused; keys, lags, counts, scratch and chunks as launch_occurrences_batch_chunk.
// `peaks`: the list under the peak rule -- per recording the cells whose entry ends inside the d_r sub-fingerprints in FRONT of the
// newest one, with `final` the newest cell too, that are local peaks of the window's profile (k_occurrences.hip's rule); `plan` is
// then occurrences_tail_plan's at max_new + 2 (a recording's lanes hold the two neighbour cells), 1 <= max_new <= 62.
// Four or five launches on the call's stream, nothing visits the host.
hipError_t launch_occurrences_tail_chunk(const OccurrencesCall& call, const OccurrencesTailPlan& plan, uint32_t recordings,
                                         const uint32_t* d_new_counts, uint32_t max_new, bool peaks, bool final, void* d_scratch,
                                         uint64_t first_entry, uint64_t entries, uint32_t first_chunk, unsigned long long* d_counts);
// recording tail (k_recording_tail.hip): the tail occurrences' cells folded per (recording, entry) to the best of them -- score =
// max(+0, the largest q_o of the pair's tail cells), lag = -(the lowest tail offset that reaches it), +0 and 0 where the pair has no
// tail cell -- as rows of `pitch` words, one per recording.  A fixed output shape: no counts, no scans, no scatter, and a pass
// takes ALL entries in one launch.
struct RecordingTailPlan {
    uint32_t lanes = 0;                  // occurrences_tail_shape's four, unchanged
    uint32_t recordings_per_workgroup = 0;
    uint32_t window_records = 0;
    uint64_t lds_bytes = 0;
    uint32_t recordings_per_pass = 0;
    uint64_t scratch_bytes = 0;          // key forms: recordings_per_pass x entries x 8, a score and a lag row per recording; else 0
};
// THE plan of a call, the debug symbol's and the real calls' (plan.cpp): the tail occurrences' shape; the recordings of a pass are
// the smallest of the recordings, 65 535, what keeps the units (blocks of entries x recordings) within 32 bits and, for the key
// forms, max(1, limit / (entries x 8)) (0: kJoinScratchDefault) -- the score and lag rows the selection reads, as
// recording_batch_plan's key form has them.  An empty corpus: all recordings, no scratch.  1 <= max_new <= 64.
void recording_tail_plan(uint32_t recordings, uint32_t per, uint32_t ne_max, uint64_t entries, uint32_t max_new, uint64_t limit_bytes,
                         bool key_form, RecordingTailPlan* plan);
// one pass: `recordings` recordings from call.d_qwords on with their new counts from d_new_counts on, every entry of the corpus;
// call.d_scores (and d_lags, optional) are row 0 of the pass, rows `pitch` words apart, every word of `entries` per row written.
// call.tiles == 1.  One launch on the call's stream, no scratch.
hipError_t launch_recording_tail(const RecordingCall& call, const RecordingTailPlan& plan, uint32_t recordings, const uint32_t* d_new_counts,
                                 uint32_t max_new, uint64_t entries, uint64_t pitch);
// timeline tail (k_timeline_tail.hip): the tail occurrences' cells at or above a threshold folded per (recording, OFFSET) to the
// largest key  q_o bits << 32 | 0xFFFFFFFF - (index base + entry)  -- the batch timeline's key of that cell -- and merged by
// unsigned maximum with the previous timeline shifted left by the recording's new count.  A cell of an entry of n_j sub-fingerprints
// at offset o lies at slot (n_query - o) - shortest entry of a recording's STRIP of `strip_width` 64-bit accumulators.
struct TimelineTailPlan {
    uint32_t lanes = 0;                  // occurrences_tail_shape's lanes and sub-window
    uint32_t recordings_per_workgroup = 0;   // 256 / D, fewer where that many sub-windows AND strips do not fit the LDS (at least 1)
    uint32_t window_records = 0;
    uint32_t strip_width = 0;            // min(ne_max, n_query) - ne_min + D; 0: no entry takes part
    uint64_t lds_bytes = 0;              // windows + table, rounded up to 8 bytes, + recordings_per_workgroup x strip_width x 8
    uint32_t recordings_per_pass = 0;
    uint64_t scratch_bytes = 0;          // recordings_per_pass x strip_width x 8: the pass' strips
};
// the five fields a workgroup's shape is (plan.cpp): what the launch holds the plan against
void timeline_tail_shape(uint32_t per, uint32_t ne_min, uint32_t ne_max, uint32_t max_new, TimelineTailPlan* plan);
// THE plan of a call, the debug symbol's and the real call's (plan.cpp): the shape above; the recordings of a pass are the smallest
// of the recordings, 65 535, what keeps the units (blocks of entries x recordings) within 32 bits, and limit / (strip_width x 8)
// (0: kJoinScratchDefault).  The strips do not grow with the entries, so a pass takes ALL entries in one launch.  false: the limit
// holds no strip of one recording.  An empty corpus or ne_min > per: no strip, all recordings, no scratch.  1 <= max_new <= 64.
bool timeline_tail_plan(uint32_t recordings, uint32_t per, uint32_t ne_min, uint32_t ne_max, uint64_t entries, uint32_t max_new,
                        uint64_t limit_bytes, TimelineTailPlan* plan);
// one pass' cells: `recordings` recordings from call.d_qwords on with their new counts from d_new_counts on, every entry of the
// corpus, into d_strips [recordings][plan.strip_width], ZEROED by the caller, with atomic maxima.  call.tiles == 1, call.ne_min <=
// call.n_query.  One launch on the call's stream.
hipError_t launch_timeline_tail_cells(const TimelineCall& call, const TimelineTailPlan& plan, uint32_t recordings,
                                      const uint32_t* d_new_counts, uint32_t max_new, uint64_t entries, unsigned long long* d_strips);
// one pass' rows: keys[r][o] = max(strip of r at (per - o) - ne_min (0 outside it, or with d_strips == nullptr), d_prev[r][o +
// min(new count, per)] (0 beyond the row, or with d_prev == nullptr)), and where wanted the lengths of the entries the keys name
// (0 for a zero key or an index outside the corpus).  Every word of `recordings` rows written.  One launch.
hipError_t launch_timeline_tail_finish(const unsigned long long* d_strips, uint32_t strip_width, uint32_t ne_min, uint32_t recordings,
                                       uint32_t per, const uint32_t* d_new_counts, const unsigned long long* d_prev, uint64_t index_base,
                                       uint64_t count, const uint32_t* d_off, unsigned long long* d_keys, uint32_t* d_lengths,
                                       hipStream_t stream);

// threshold selection over ANY number of rows (k_occurrences_batch.hip): launch_threshold_keys' results -- per row of n scores the
// keys of the entries whose score is >= threshold in ascending entry index, the first min(count, capacity) of them to d_keys + r *
// capacity, the true count to d_counts[r] -- through the joins' scans with a row per recording.  The caller has zeroed the keys.
// d_scratch: threshold_batch_scratch_bytes(n, rows) bytes, written before they are read; four launches, whatever the rows.
// rows <= 65 535, rows x capacity <= 2^31, index_base + n <= 2^32.
size_t threshold_batch_scratch_bytes(uint64_t entries, uint32_t rows);
hipError_t launch_threshold_batch_keys(const float* d_scores, uint64_t n, uint32_t rows, float threshold, uint64_t capacity,
                                       uint64_t index_base, void* d_scratch, unsigned long long* d_keys, unsigned long long* d_counts,
                                       hipStream_t stream);

// recording segments (k_segments.hip): per recording the non-overlapping spans of a timeline's winners -- d_keys and d_lengths as
// the timeline calls write them, [recordings][per], per <= LBAD_SEGMENTS_MAX_SUBFINGERPRINTS, both products with `recordings`
// below 2^31 -- greedy in descending key order (ties to the lower offset), in start order to the rows of `capacity` slots of
// d_starts / d_out_keys / d_out_lengths (may be null), zeros behind them, the true count to d_counts.  The outputs overlap no
// input.  One launch, no scratch; segments_lds_bytes: the dynamic LDS of a workgroup (0 for a length outside the cap).
size_t segments_lds_bytes(uint32_t per);
hipError_t launch_timeline_segments(const unsigned long long* d_keys, const uint32_t* d_lengths, uint32_t recordings, uint32_t per,
                                    uint32_t capacity, uint32_t* d_starts, unsigned long long* d_out_keys, uint32_t* d_out_lengths,
                                    uint32_t* d_counts, hipStream_t stream);

// occurrence segments (k_occurrence_segments.hip): per recording the non-overlapping spans over ALL cells of an occurrences row --
// d_keys / d_lags / d_lengths [recordings][cap_in] (the lengths of the entries the keys name), the first min(d_counts[r], cap_in)
// slots of a row (all of them with d_counts null), cap_in <= LBAD_OCCURRENCE_SEGMENTS_MAX_CANDIDATES, per <=
// LBAD_SEGMENTS_MAX_SUBFINGERPRINTS, the three products with `recordings` below 2^31 -- greedy in descending key order (ties to
// the lower start, then the lower slot), in start order to the rows of `cap_out` slots of d_starts / d_out_keys / d_out_lags /
// d_out_lengths (the last two may be null), zeros behind them, the true count to d_out_counts.  The outputs overlap no input.  One
// launch, no scratch; occurrence_segments_lds_bytes: the dynamic LDS of a workgroup (0 for a shape outside the caps).
size_t occurrence_segments_lds_bytes(uint32_t cap_in, uint32_t per);
hipError_t launch_occurrence_segments(const unsigned long long* d_keys, const int32_t* d_lags, const uint32_t* d_lengths,
                                      const unsigned long long* d_counts, uint32_t recordings, uint32_t cap_in, uint32_t per,
                                      uint32_t cap_out, uint32_t* d_starts, unsigned long long* d_out_keys, int32_t* d_out_lags,
                                      uint32_t* d_out_lengths, uint32_t* d_out_counts, hipStream_t stream);
// launch_timeline_lengths for a uniform corpus, which keeps no offsets: n_sub for every key that names one of its `count` entries
hipError_t launch_entry_lengths_uniform(const unsigned long long* d_keys, uint32_t n, uint64_t index_base, uint64_t count, uint32_t n_sub,
                                        uint32_t* d_lengths, hipStream_t stream);

// The host side the three families above share (recording_pass.cpp; DESIGN.md 4.4n states the protocol).
// The query of a call: a handle (staged through the alignment's pair, under its event) or packed sub-fingerprints on the device
// (through the builder of k_query.hip, under the packed calls' event), and the range it is compared over (0: the whole length)
struct PassQuery {
    const struct ::LBAudioDetectiveFingerprint* fp = nullptr;
    const uint32_t* d_rows = nullptr;
    uint32_t per = 0;
    uint32_t range = 0;
};
// a family as the plan sees it: its tiles (ne_max may go unused), the entries of a chunk under a limit, the entries a chunk is
// a whole number of
struct PassFamily {
    uint64_t (*tiles)(uint32_t n_query, uint32_t ne_min, uint32_t ne_max);
    uint64_t (*chunk_entries)(uint64_t tiles, uint64_t limit_bytes);
    uint32_t (*block_entries)();
};
struct PassPlan {
    OcPassCall call;                     // the shared fields of the family's call, all but the query's words and the stream
    uint64_t chunk = 0;                  // entries per chunk: the scratch limit's, or the whole corpus rounded up to a block
    bool any = false;                    // an entry takes part: the shortest is not longer than the query
};
// What the corpus decides, before anything is reserved or launched: a ragged corpus of the query's sub-fingerprint length with no
// entry above the cap (ne_max: the host knows it), the indices in range, a scratch limit that holds a block of entries.  An
// empty corpus gives tiles 1, chunk 0.
OSStatus pass_plan(const struct ::LBAudioDetectiveCorpus* c, const PassQuery& q, uint64_t index_base, const PassFamily& fam, PassPlan* plan);
// The events a call takes: join_ev (the partials), the query's (align_ev or pq_ev: the staged words) and, with `topk`, topk_ev
// (the score row and the selection's words).  wait() before the scratch is touched; then every way out goes through finish(),
// which records them all on the stream behind whatever was launched, also after a failure -- the scratch and the staged words
// are in use until then -- and gives the call's status, else the first record's that failed.  The top-K and threshold queries
// (api_select.cpp) name their events themselves: one guard per point of the stream at which an event is due.
struct PassGuard {
    Event* ev[3] = {nullptr, nullptr, nullptr};
    PassGuard(struct ::LBAudioDetectiveCorpus* c, const PassQuery& q, bool topk);
    explicit PassGuard(Event* e0, Event* e1 = nullptr, Event* e2 = nullptr) : ev{e0, e1, e2} {}
    OSStatus wait();
    OSStatus finish(hipStream_t stream, OSStatus st);
};
// the query's words onto the device on `stream` (call->d_qwords, call->stream), and behind them the corpus' latest append awaited
// on the stream.  The caller holds the query's event.
OSStatus pass_stage_query(struct ::LBAudioDetectiveCorpus* c, const PassQuery& q, hipStream_t stream, OcPassCall* call);
// the chunks of a corpus of `count` entries in turn, until one fails: launch(first entry, entries)
template <typename Launch>
hipError_t pass_chunks(uint64_t count, uint64_t chunk, Launch launch) {
    hipError_t e = hipSuccess;
    for (uint64_t e0 = 0; e0 < count && e == hipSuccess; e0 += chunk) e = launch(e0, count - e0 < chunk ? count - e0 : chunk);
    return e;
}
// The list forms whose results are rows of keys, one per recording (api_occurrences_batch.cpp's occurrences and both lists of
// api_occurrences_tail.cpp; the key forms of api_recording_tail.cpp take the zeros).  What needs neither handle nor device: the
// blocks, one or more recordings whose sub-fingerprints and slots stay within 32-bit indices, a finite threshold above 0, 1 .. 2^31
// slots per recording, an index base a corpus can lie behind
bool key_rows_args_ok(const void* c, const void* d_rows, const void* keys, const void* counts, uint32_t recordings, uint32_t per,
                      float threshold, uint64_t capacity, uint64_t index_base);
// zero keys and, where given, lags over recordings x slots, and zero counts where given
OSStatus zero_key_rows(uint32_t recordings, uint64_t slots, unsigned long long* keys, int32_t* lags, unsigned long long* counts,
                       hipStream_t stream);
struct KeyRows {
    const uint32_t* d_rows = nullptr;    // the recordings' packed sub-fingerprints, on the device
    uint32_t recordings = 0;
    float threshold = 0.0f;
    bool peaks = false;                  // the call's peaks flag (the tail lists': false, their rule is the kernel instance's)
    uint64_t capacity = 0, index_base = 0;
    unsigned long long* keys = nullptr;  // [recordings][capacity]
    int32_t* lags = nullptr;             // optional: likewise
    unsigned long long* counts = nullptr;    // [recordings]
    hipStream_t stream = nullptr;
};
// the three fields of a family's plan the host path goes by
struct KeyRowsPasses {
    uint32_t recordings_per_pass = 0;
    uint64_t entries_per_chunk = 0;
    uint64_t scratch_bytes = 0;
};
// one chunk of one pass: the family's launch_*_chunk with `call`'s keys and lags at the pass' row 0
using KeyRowsChunk = std::function<hipError_t(const OccurrencesCall& call, uint32_t first_recording, uint32_t recordings, uint64_t first_entry,
                                              uint64_t entries, uint32_t first_chunk, unsigned long long* d_counts)>;
// One call behind its plan and a corpus that is not empty: the events (PassGuard without the top-K's), the scratch and the staging
// buffer reserved, the call filled from the single plan with `tiles`, and on the stream the corpus' latest append awaited, the zero
// keys and lags, then pass by pass the recordings' rows (launch_build_query_rows) and the chunks -- one chunk of the whole corpus
// for several recordings, entry chunks and the carried total, copied to the recording's count, for one.
OSStatus key_rows_call(struct ::LBAudioDetectiveCorpus* c, const PassQuery& q, const PassPlan& single, const KeyRowsPasses& passes,
                       uint64_t tiles, const KeyRows& rows, const KeyRowsChunk& chunk);
// The block of a host-returning form in the corpus' key buffer, for the null stream: n_keys keys and, behind them, n_words 32-bit
// values, once the buffer's previous user (a top-K, threshold or join call) has left it.
struct KeyBlock {
    unsigned long long* d_keys = nullptr;
    uint32_t* d_words = nullptr;         // nullptr: n_words == 0
    size_t n_keys = 0, n_words = 0;
};
OSStatus key_block_reserve(struct ::LBAudioDetectiveCorpus* c, size_t n_keys, size_t n_words, KeyBlock* b);
// the first m keys and, where there are any, m values behind them (host[m] onwards) read back; m == n_keys: the whole block,
// every value of it, in one copy
OSStatus key_block_read(const KeyBlock& b, size_t m, std::vector<unsigned long long>* host);
// after a failure behind the reservation: whatever was launched has left the key buffer before its next user
OSStatus key_block_failed(OSStatus st);

// removal (k_remove.hip): the index of a call -- which entries go and where the others land -- and the moves of a chunk.
// The index block of a corpus of `count` entries (remove_index_layout places it in d_block, 16-byte aligned, `words` words):
// head (entries kept, lowest removed index or 0xFFFFFFFF, two zero words), tiles + 1 tile offsets (kept entries below the
// tile; the last word = the total), the map (new index per entry, 0xFFFFFFFF for a removed one), then the flags and the per-tile
// words.  The host reads the first head_words words, or map_words of them when it wants the map as well: ONE copy.
struct RemoveIndex {
    uint64_t tiles = 0;
    uint32_t *head = nullptr, *tile_offsets = nullptr, *map = nullptr, *flags = nullptr, *tile_counts = nullptr, *tile_first = nullptr;
    uint64_t words = 0, head_words = 0, map_at = 0, map_words = 0;    // map_at: the map's first word inside the block
};
uint32_t remove_tile_entries();          // entries (records of a ragged corpus) per tile: what a chunk is a whole number of
RemoveIndex remove_index_layout(void* d_block, uint64_t count);
// a memset and four launches on `stream`: d_list holds n_list keys (keys: 0xFFFFFFFF - low word = index_base + entry; zero keys
// and keys of other entries are skipped) or n_list 64-bit indices.  1 <= count <= 2^32 - 1.
hipError_t launch_remove_index(const unsigned long long* d_list, uint64_t n_list, bool keys, uint64_t index_base, uint64_t count,
                               const RemoveIndex& ix, hipStream_t stream);
// uniform: the kept entries of [e0, e1), new indices base .. , to d_bounce (plane p at p * bstride; bstride >= entries kept)
hipError_t launch_remove_gather_planes(const uint4* d_planes, uint64_t stride, uint32_t n_planes, const uint32_t* d_map, uint64_t e0,
                                       uint64_t e1, uint32_t base, uint4* d_bounce, uint64_t bstride, hipStream_t stream);
// the first k uint4 of every plane of d_bounce to d_dst + p * stride + base
hipError_t launch_remove_scatter(const uint4* d_bounce, uint64_t bstride, uint32_t n_planes, uint4* d_dst, uint64_t stride, uint64_t base,
                                 uint64_t k, hipStream_t stream);
// ragged: the records [r0, r1) of kept entries, new positions base .. , to d_bounce (`slots` records), their entry-index field
// rewritten; d_new_off: the kept entries' new first records, by NEW index
hipError_t launch_remove_gather_records(const uint4* d_recs, const uint32_t* d_old_off, const uint32_t* d_new_off, const uint32_t* d_map,
                                        uint64_t n_entries, uint64_t r0, uint64_t r1, uint64_t base, uint4* d_bounce, uint64_t slots,
                                        hipStream_t stream);

// gather (k_gather.hip): entries handed back in the packed layout, named by keys.  A corpus as its kernels read it:
struct GatherSource {
    bool ragged = false;
    const uint4* recs = nullptr;        // ragged: the records, the entries' record positions and the longest entry
    const uint32_t* off = nullptr;
    uint32_t ne_max = 0;
    const uint4* planes = nullptr;      // uniform: the planes, plane stride `stride`, planes per entry
    uint64_t stride = 0;
    uint32_t n_planes = 0, n_sub = 0;
    uint64_t count = 0;
    uint32_t subfp_len = 0;
};
uint32_t gather_tile_keys();                     // keys per tile of the lengths and offsets launches
size_t gather_scratch_bytes(uint64_t n_keys);    // one 64-bit sum per tile
// 1 <= n_keys <= 2^31 keys at d_keys (a zero key, or an index outside [index_base, index_base + count): an empty row) -> the
// rows' offsets (n_keys + 1 words, the last one the true total) to d_offsets and the sub-fingerprints at positions below
// `capacity` to d_packed (16-byte aligned; may be null when capacity is 0), 32 bytes each.  d_scratch: gather_scratch_bytes(n_keys)
// bytes, written before they are read.  Three launches and the copy on `stream`, nothing visits the host.
hipError_t launch_gather(const GatherSource& src, const unsigned long long* d_keys, uint64_t n_keys, uint64_t index_base, void* d_scratch,
                         void* d_packed, uint64_t capacity, unsigned long long* d_offsets, hipStream_t stream);

// entry ids (k_ids.hip): the caller's 64-bit ids of the entries, one word per entry (0: no id).
// d_out[i] = the id of the entry key i names, 0 for a zero key or an index outside [index_base, index_base + count); d_ids null (a
// corpus without ids): all zeros.  n <= 2^31 keys, index_base + count <= 2^32.  One launch.
hipError_t launch_ids_from_keys(const unsigned long long* d_keys, uint64_t n, uint64_t index_base, uint64_t count,
                                const unsigned long long* d_ids, unsigned long long* d_out, hipStream_t stream);
// the id index: an open-addressing table of `slots` id words (0: empty) and `slots` index words, slots = ids_index_slots(count) -- a
// power of two >= 2 x count, at least 1024.  The build is an init and an insert launch; afterwards the id of every entry with a
// non-zero id owns one slot whose index word is the LOWEST index with that id.
uint64_t ids_index_slots(uint64_t count);
hipError_t launch_ids_index_build(const unsigned long long* d_ids, uint64_t count, unsigned long long* d_slot_ids,
                                  uint32_t* d_slot_index, uint64_t slots, hipStream_t stream);
// d_out[i] = bits(1.0f) << 32 | 0xFFFFFFFF - (index_base + index) for the lowest index whose id is d_list[i]; a zero key for id 0,
// an id no entry has, or a null table (a corpus without ids).  n <= 2^31.  One launch, the table is only read.
hipError_t launch_keys_from_ids(const unsigned long long* d_list, uint64_t n, uint64_t index_base, uint64_t count,
                                const unsigned long long* d_slot_ids, const uint32_t* d_slot_index, uint64_t slots,
                                unsigned long long* d_out, hipStream_t stream);
// behind a removal's moves: d_map (RemoveIndex::map) takes the ids of the kept entries from `first` (the lowest removed index) on
// to their new indices through d_scratch (count - first words), and the words from `kept` to the old `count` become zero.
// first <= kept < count.  Two launches (one where kept == first).
hipError_t launch_ids_compact(unsigned long long* d_ids, const uint32_t* d_map, uint64_t first, uint64_t kept, uint64_t count,
                              unsigned long long* d_scratch, hipStream_t stream);

// groups (k_groups.hip): the connected components of the graph whose edges are match keys, and the keys of every entry that is
// not its group's first.  1 <= n <= 2^32 vertices, labels as a forest whose parents lie below their vertices (any content is
// legal input without a reset).  Slots: n_slots <= 2^31 keys; their rows by d_offsets (n_rows + 1 words, CSR) or, when it is
// null, by rows of `pitch` slots; a row's entry is first_row + r or, with d_row_keys, the entry key r names.  d_group_count
// (may be null) must hold 0: the flatten launch ADDS the number of roots.  At most three launches on `stream`.
hipError_t launch_group_labels(const unsigned long long* d_keys, uint64_t n_slots, const unsigned long long* d_offsets, uint64_t pitch,
                               uint64_t n_rows, uint64_t first_row, const unsigned long long* d_row_keys, uint64_t index_base, uint64_t n,
                               bool reset, uint32_t* d_labels, unsigned long long* d_group_count, hipStream_t stream);
size_t group_extra_scratch_bytes(uint64_t n);    // one 64-bit count per tile of 1024 vertices and the total behind them
// the keys (score word 1.0f) of the vertices whose label is not their own index, ascending, to the slots below `capacity` of
// d_keys (zeroed by the caller); the true count to the last word of d_scratch (group_extra_scratch_bytes(n) bytes)
hipError_t launch_group_extra_keys(const uint32_t* d_labels, uint64_t n, uint64_t index_base, uint64_t capacity, void* d_scratch,
                                   unsigned long long* d_keys, hipStream_t stream);

// alignment (k_align.hip): the best sliding offset of (query, entry) pairs, after selection.  A corpus as its kernels read it:
struct AlignSource {
    bool ragged = false;
    const uint4* recs = nullptr;        // ragged: the records and the entries' record positions
    const uint32_t* off = nullptr;
    const uint4* planes = nullptr;      // uniform: the planes, plane stride `stride`
    uint64_t stride = 0, count = 0;
    uint32_t n_sub = 0, subfp_len = 0;
    uint32_t range = 0;                 // >= 1 (0 resolved by the caller)
};
// a query's sub-fingerprints as the kernels read them (8 words each), appended to out
void build_align_query(const struct ::LBAudioDetectiveFingerprint* q, bool ragged, std::vector<uint32_t>& out);
// workgroups that share one pair of a keys launch; above 1, d_best must hold pairs words
uint32_t align_parts(uint64_t pairs, uint64_t max_offsets);
// n_queries x k keys (query q's row at d_keys + q * k, index = index_base + entry) -> lags (and, d_scores != null, the recomputed
// scores) in the same places.  d_qwords: build_align_query blocks one after the other; d_qdesc: per query (first
// sub-fingerprint in d_qwords, count).  max_offsets: a bound of n1 - n2 + 1 over the pairs (spreads long pairs).
hipError_t launch_align_keys(const AlignSource& src, const uint32_t* d_qwords, const uint2* d_qdesc, uint32_t n_queries, uint32_t k,
                             const unsigned long long* d_keys, uint64_t index_base, uint64_t max_offsets,
                             unsigned long long* d_best, int32_t* d_lags, float* d_scores, hipStream_t stream);
// every q_o of the pair (query of n_query sub-fingerprints at d_qwords, entry), n_offsets = n1 - n2 + 1 floats to d_out
hipError_t launch_align_profile(const AlignSource& src, const uint32_t* d_qwords, uint32_t n_query, uint64_t entry, uint64_t n_offsets,
                                float* d_out, hipStream_t stream);

// ragged corpus: a stream of 32-byte sub-fingerprint records, entries of any length back to back (sliding_common.hpp has the
// layout).  sliding.cpp: the host side; k_records.hip, k_sliding.hip, k_sliding_short.hip: the kernels
bool sliding_supported(uint32_t subfp_len);
// words of the scan's block of a query of n_query sub-fingerprints: 16 per sub-fingerprint and one zero sub-fingerprint of slack
constexpr size_t sliding_block_words(size_t n_query) { return (n_query + 1u) * 16u; }
// the block of one query from unpacked Booleans (n_query x subfp_len)
void build_sliding_query(const Boolean* bools, uint32_t n_query, uint32_t subfp_len, uint32_t range,
                         std::vector<uint32_t>& out);
uint4 sliding_range_mask(uint32_t subfp_len, uint32_t range);    // pairs inside min(range, length), one bit each
// d_off_new: ABSOLUTE record positions of the n_new new entries (n_new + 1 values, the first one = slot 0's position)
hipError_t launch_pack_records(const uint32_t* d_slots, uint64_t n_new_pos, const uint32_t* d_off_new, uint64_t n_new,
                               uint32_t first_entry, uint4* d_recs, hipStream_t stream);
// records read from a file: derived fields (table row, place inside the entry) recomputed from d_off, reserved bits and
// pairs beyond the length cleared (old_layout: the round-3 "LBADCRP2" record)
hipError_t launch_restamp_records(uint4* d_recs, const uint32_t* d_off, uint64_t n_entries, uint64_t n, uint32_t subfp_len,
                                  bool old_layout, hipStream_t stream);
hipError_t launch_synth_ragged(uint32_t seed, uint64_t first_entry, uint64_t n_entries, const uint32_t* d_off,
                               uint64_t n_pos, uint32_t subfp_len, uint32_t* d_out, hipStream_t stream);

// ---- the scan of a ragged corpus: ONE decision per launch (sliding.cpp: sliding_choose), handed to the launcher ----------------
// shape of a task scan: workgroups (one per CU) and the tasks of either kind each of them owns
struct SlideShape {
    uint32_t grid = 0, chunk_a = 0, chunk_b = 0;
};
// what the decision looks at.  The corpus: its histogram of entry lengths, records stored, longest entry, kernel variant (3
// forces the split of the scan where one exists, 4 forbids it)
struct SlideCorpusStats {
    const std::map<uint32_t, uint64_t>* len_hist = nullptr;
    uint64_t n_pos = 0;
    uint32_t ne_max = 0, variant = 0, subfp_len = 0;
};
// ... and the queries: their length, how many of that length are still to go, the range (>= 1), whether per-entry scores are
// wanted (one query per launch then) and whether the blocks are on the host (a short single query can travel in the kernel's
// arguments) or on the device already
struct SlideGroup {
    uint32_t n_query = 0, n_left = 0, range = 0;
    bool scores = false, host_blocks = false;
};
enum class SlideKernel : uint32_t { Task = 0, Short = 1, ShortMulti = 2 };   // compare_sliding_ / compare_short_ / compare_short_multi_kernel
// One launch of the scan, decided: everything the corpus' side (ring, plan cache, zeroing of keys) and the launcher need.
struct SlideChoice {
    uint32_t n_take = 0;               // queries this launch takes (0: there is no such launch -- a task count beyond 32 bits)
    SlideKernel kernel = SlideKernel::Task;
    // the instance: compare_sliding_kernel<full, false, qlds, n_take, threads>, compare_short_kernel<look <= 6 ? 1 : 4, n_take>,
    // compare_short_multi_kernel<n_take, n_query>
    bool full = false, qlds = false;
    uint32_t threads = 0;
    uint32_t look = 0;                 // Short: records a window reaches back
    // b_min > 0: the scan is SPLIT -- "B" entries (not longer than the query) of fewer sub-fingerprints go through the systolic
    // scan in a second launch, and tasks_b and the plan count only the others
    uint32_t b_min = 0;
    uint64_t tasks_a = 0, tasks_b = 0; // groups of four sliding offsets over the entries longer / not longer than the query
    SlideShape shape;
    bool reads_plan = false;           // only the task kernel walks the plan's runs of entries
    bool q_in_args = false;            // the single query's block travels in the kernel's argument segment, nothing is copied
    bool maxes_keys = false;           // the launch maxes its keys in place: they must be zero in front of it
    // a systolic launch over the same keys follows (the short entries of a split scan, or what compare_short_multi_kernel
    // leaves: the entries not longer than the query)
    bool second = false;
    uint32_t second_look = 0, second_only_upto = 0;
    uint32_t cus = 0;                  // compute units the grids were sized for
};
SlideChoice sliding_choose(const SlideCorpusStats& corpus, const SlideGroup& group, uint32_t cus);
void sliding_choice_words(const SlideChoice& ch, uint32_t n_query, uint32_t* out21);    // LBAudioDetectiveDebugSlidingChoice's words

// The corpus as the scan's kernels read it (cf. AlignSource)
struct SlideCorpus {
    const uint4* recs = nullptr;
    uint64_t n_pos = 0;                // records stored
    const uint32_t* off = nullptr;     // n_entries + 1 record positions
    uint64_t n_entries = 0;
    uint32_t zero_rec = 0;             // index of an all-zero record behind the stored ones
    uint32_t subfp_len = 0;
    const uint32_t* plan = nullptr;    // launch_sliding_plan's output for this query length (read when choice.reads_plan)
};
// The queries of one launch and where their keys go.  d_queries: choice.n_take blocks of sliding_block_words(n_query) words, one
// after the other, on the device; h_query: the same block of a single query on the host when choice.q_in_args (d_queries may
// be null then).  d_acc (8 words) and d_ticket are zero between scans (the scan leaves them so); d_keys receives the results.
struct SlideScan {
    const uint32_t* d_queries = nullptr;
    const uint32_t* h_query = nullptr;
    unsigned long long* d_acc = nullptr;
    unsigned int* d_ticket = nullptr;
    unsigned long long* d_keys = nullptr;
    uint32_t key_pos[8] = {};     // query i's key goes to d_keys[key_pos[i]]
};
// the scalars of a call.  d_score_bits (optional, one query only; n_entries words) must be zero on entry and receives the
// float bits of every entry's match
struct SlideCall {
    uint32_t n_query = 0, range = 0;
    uint64_t index_base = 0;
    unsigned int* d_score_bits = nullptr;
    bool bound_pruning = true;
    float prune_from = 0.7f;
    hipStream_t stream = nullptr;
};
size_t sliding_plan_words(uint64_t capacity);
// the plan of a query length (where every workgroup's run of entries starts) into d_plan
hipError_t launch_sliding_plan(const uint32_t* d_off, uint64_t n_entries, uint32_t n_query, uint32_t b_min, const SlideShape& sh,
                               uint32_t* d_plan, hipStream_t stream);
// performs the launches the choice names
hipError_t launch_compare_sliding(const SlideCorpus& src, const SlideChoice& choice, const SlideScan& scan, const SlideCall& call);
// limits of a ragged corpus (the key carries a 32-bit index, the scan's claim cursor and its record offsets want a little slack)
constexpr uint64_t kMaxRaggedEntries = 0xFFFF0000ull;
constexpr uint64_t kMaxRaggedRecords = 0xFFFFFF00ull;
constexpr uint32_t kRecordSlack = 8;   // records allocated behind a ragged corpus' capacity (zero: over-read + the zero record)

// query blocks built on the device (k_query.hip) from n_queries x per packed sub-fingerprints at d_rows (8 words each, 4-byte
// aligned), bit for bit what the host builders make from the same Booleans; bits at or above the length are ignored.
// plane blocks: plane_query_words() words per query (build_plane_query, zero padded), per == n_sub, length 200
hipError_t launch_build_plane_queries(const uint32_t* d_rows, uint32_t n_queries, uint32_t n_sub, uint32_t range,
                                      uint32_t* d_blocks, hipStream_t stream);
// sliding blocks: sliding_block_words(per) words per query (build_sliding_query's); d_blocks 16-byte aligned
hipError_t launch_build_sliding_queries(const uint32_t* d_rows, uint32_t n_queries, uint32_t per, uint32_t subfp_len, uint32_t range,
                                        uint32_t* d_blocks, hipStream_t stream);
// 8 words per sub-fingerprint to d_words (16-byte aligned): the slot words cleared from the length on (the generic uniform
// scan's query, build_align_query's uniform form), or with `pairs` build_align_query's ragged form; d_desc (optional):
// launch_align_keys' table, query q = (q * per, per)
hipError_t launch_build_query_rows(const uint32_t* d_rows, uint32_t n_queries, uint32_t per, uint32_t subfp_len, bool pairs,
                                   uint32_t* d_words, uint2* d_desc, hipStream_t stream);

// stream bank (k_stream_bank.hip; api_stream_bank.cpp is its host side).  The bank as its kernels read it:
struct BankDev {
    float* carry = nullptr;             // [2 sides][n_channels][carry_stride] carried samples
    uint64_t carry_stride = 0;          // floats per channel and side: window + hop (a multiple of 16)
    uint64_t n_channels = 0;
    uint32_t* ring = nullptr;           // [n_channels][history][8 words] packed sub-fingerprints, number t of a channel at t mod history
    uint32_t history = 0, window = 0, hop = 0;
};
// One channel that received samples in a push (48 bytes; the host plans the push and uploads these, in channel order)
struct BankRow {
    uint64_t fresh_at;                  // its first new sample inside the push's sample block
    uint32_t p, n, ready;               // samples carried, samples new, frames they complete
    uint32_t first;                     // its first frame among the push's frames (channel order, then time)
    uint32_t ring_at;                   // ring slot of that frame: the channel's total mod history
    uint32_t channel, side;             // side: the carried buffer that holds the p samples
    uint32_t pad[3];
};
static_assert(sizeof(BankRow) == 48, "BankRow is uploaded as it is");
// frames [g0, g0 + nf) of the push as one-frame clips of window + hop samples to d_clips (16-byte aligned)
hipError_t launch_bank_stage(const BankDev& b, const BankRow* d_rows, uint32_t n_rows, const float* d_fresh, uint32_t g0, uint32_t nf,
                             float* d_clips, hipStream_t stream);
// behind the last pass: the push's `total` packed sub-fingerprints at d_packed into the rings and (d_out != null, 16-byte aligned)
// the caller's block, then what every row's channel carries on -- into the other side where it completed a frame.  Two launches.
hipError_t launch_bank_commit(const BankDev& b, const BankRow* d_rows, uint32_t n_rows, const float* d_fresh, const uint32_t* d_packed,
                              uint32_t total, void* d_out, hipStream_t stream);
// the two halves of launch_bank_commit alone (the phased bank: its sample rows and its sub-fingerprint rows are two tables)
hipError_t launch_bank_commit_rows(const BankDev& b, const BankRow* d_rows, uint32_t n_rows, const uint32_t* d_packed, uint32_t total,
                                   void* d_out, hipStream_t stream);
hipError_t launch_bank_commit_carry(const BankDev& b, const BankRow* d_rows, uint32_t n_rows, const float* d_fresh, hipStream_t stream);
// the phased bank's row rings (k_stream_bank_phased.hip): per real channel the last 128 rows of `row_dw` floats, row number t of
// a channel at t mod 128.  One PhasedRow per channel that transformed windows in the push: its last min(n_new, 128) new rows
// (d_new_rows + (new_row0 + i) * row_dw) go to their ring slots.
struct PhasedRow {
    uint64_t new_row0;                  // the channel's first new row among the push's new rows
    uint32_t n_new, ring_at;            // new rows; ring slot of the first of them: the channel's row count mod 128
    uint32_t channel;
    uint32_t pad[3];
};
static_assert(sizeof(PhasedRow) == 32, "PhasedRow is uploaded as it is");
hipError_t launch_bank_row_ring(float* d_row_ring, uint32_t row_dw, const PhasedRow* d_rows, uint32_t n_rows, const float* d_new_rows,
                                hipStream_t stream);
// d_list[j] = (channel, ring slot of the oldest of its q rows) -> d_out[j][q][32 bytes] (16-byte aligned); n_list * q <= 2^31
hipError_t launch_bank_window(const BankDev& b, const uint2* d_list, uint64_t n_list, uint32_t q, void* d_out, hipStream_t stream);

// resampler bank (k_resample_bank.hip; api_resampler_bank.cpp is its host side).  The bank as its kernels read it:
constexpr uint32_t kResamplerBankStageMax = 2816;      // samples of a run's staged input range (k_resample.hip's kInMaxR)
constexpr uint32_t kResamplerBankMaxRun = 256;         // outputs of a run: one per lane
constexpr uint64_t kResamplerBankNoPeriod = 0x80000000ull;
constexpr uint32_t kResamplerBankPeriods = 4;          // periods of q outputs a workgroup takes side by side: one weight load for all
constexpr uint32_t kResamplerBankMaxSpan = LBAD_RESAMPLER_BANK_MAX_TAP_SPAN;
static_assert(kResamplerBankMaxSpan < kResamplerBankStageMax, "a run of one output can always be staged");
struct ResamplerBankDev {
    float* carry = nullptr;             // [2 sides][n_channels][carry_stride] carried samples
    uint64_t carry_stride = 0;          // floats per channel and side: the tap span rounded up to a multiple of 4
    uint64_t n_channels = 0;
    uint64_t p = 0, q = 0;              // the rate pair in lowest terms, and its PhaseTable on the device
    int32_t m_min = 0;
    uint32_t m_span = 0;
    const int32_t* first = nullptr;
    const uint32_t* count = nullptr;
    const double* wsum = nullptr;
    const double* w = nullptr;
    uint32_t run = 0;                   // outputs per workgroup: the most (<= 256) whose input range fits kResamplerBankStageMax
    uint64_t period = 0;                // q where a unit takes positions inside the period in several periods (q >= 2 run); else
                                        // kResamplerBankNoPeriod, above any call's outputs: a unit is a run of consecutive outputs
};
// One channel that received samples in a push or is being finished (88 bytes; the host plans the call and uploads these, in
// channel order).  Signal indices count the channel's samples since it (re)started.
struct ResamplerRow {
    uint64_t fresh_at;                  // its first new sample inside the push's sample block
    uint64_t L, end;                    // samples before the push; the in-signal bound L + n (only a finish has taps beyond it)
    uint64_t out_first, ip0;            // its first output of the call and that output's (n p) div q
    uint64_t out_at;                    // where that output goes in the caller's block (channel order, then time)
    uint64_t c0, c1;                    // signal index of the first sample carried before / after the call
    uint32_t r0;                        // the first output's phase (n p) mod q
    uint32_t n, emit;                   // samples new, outputs to emit
    uint32_t first_unit;                // its first unit (a run inside the period x a group of periods) among the call's
    uint32_t channel, side;             // side: the carried buffer that holds x[c0, L)
};
static_assert(sizeof(ResamplerRow) == 88, "ResamplerRow is uploaded as it is");
// format: 0 float32, 1 int16 samples at d_fresh.  n_units: the units of all rows (resampler_bank_units); d_out: the caller's block
// units of a row that emits `emit` outputs: runs inside the period (the row's outputs where they are fewer) x groups of periods;
// period: ResamplerBankDev::period
inline uint64_t resampler_bank_units(uint64_t emit, uint64_t period, uint32_t run) {
    const uint64_t in_period = emit < period ? emit : period, periods = (emit + period - 1) / period;
    return ((in_period + run - 1) / run) * ((periods + kResamplerBankPeriods - 1) / kResamplerBankPeriods);
}
hipError_t launch_resampler_bank_convert(const ResamplerBankDev& b, const ResamplerRow* d_rows, uint32_t n_rows, const void* d_fresh,
                                         uint32_t format, uint32_t n_units, float* d_out, hipStream_t stream);
// behind it: what every row's channel carries on -- into the other side where it emitted an output
hipError_t launch_resampler_bank_commit(const ResamplerBankDev& b, const ResamplerRow* d_rows, uint32_t n_rows, const void* d_fresh,
                                        uint32_t format, hipStream_t stream);

// measurement: ticks of the shader clock and of the constant 100 MHz clock over ~usec microseconds (2 words)
hipError_t launch_clock_probe(uint32_t usec, unsigned long long* d_out, hipStream_t stream);
// synthetic data
hipError_t launch_synth_clips(uint32_t seed, uint64_t first, uint64_t n_clips, uint32_t rate_hz, uint32_t n_samples,
                              uint32_t stereo, float* d_out, hipStream_t stream);
hipError_t launch_synth_corpus(uint32_t seed, uint64_t first, uint64_t n_entries, uint32_t n_sub, uint32_t subfp_len,
                               uint32_t* d_out, hipStream_t stream);

// ---- shared between the api_*.cpp files ------------------------------------------------------------------
uint64_t subfingerprint_count(uint64_t n_samples, uint32_t window, uint32_t stride);
// frame phases (api_detective.cpp): P is a power of two up to 32; the count of phase p is that of the signal without its first p * (128 / P) * stride samples
bool valid_phases(uint32_t phases);
uint64_t subfingerprint_count_at_phase(uint64_t n_samples, uint32_t window, uint32_t stride, uint32_t phases, uint32_t phase);
OSStatus ensure_plan(struct ::LBAudioDetective* d);
// the batch hot path on device memory; tails: end-of-file treatment of files laid out inside ONE float32 clip
OSStatus fingerprint_clips_device(struct ::LBAudioDetective* d, const void* d_pcm, uint32_t fmt, uint64_t n_clips,
                                  uint64_t samples_per_clip, uint32_t* d_packed, float* d_raw, float* d_haar,
                                  hipStream_t stream, const FileTail* tails = nullptr, size_t n_tails = 0);
// api_align.cpp: the lags of n x k keys for n queries of `per` sub-fingerprints each whose alignment words and table a builder
// wrote to the device; waits for / records the alignment scratch's event itself
OSStatus align_keys_built(struct ::LBAudioDetectiveCorpus* c, const uint2* d_desc, const uint32_t* d_words, uint32_t n, uint32_t per,
                          uint32_t range, uint32_t k, const unsigned long long* keys, uint64_t index_base, int32_t* lags,
                          hipStream_t stream);
// ... and for n queries given as handles, staged by the alignment itself
OSStatus align_keys_handles(struct ::LBAudioDetectiveCorpus* c, const ::LBAudioDetectiveFingerprintRef* qs, uint32_t n, uint32_t range,
                            uint32_t k, const unsigned long long* keys, uint64_t index_base, int32_t* lags, hipStream_t stream);
// api_corpus.cpp, the top-1 scans as the top-K and threshold queries (api_select.cpp) run them: one query given as a handle,
// staged and scanned on `stream`, its key to key_dst (device) and, d_scores given, its per-entry scores (count floats) ...
OSStatus run_query(struct ::LBAudioDetectiveCorpus* c, const struct ::LBAudioDetectiveFingerprint* q, uint32_t range, uint64_t index_base,
                   float* d_scores, unsigned long long* key_dst, hipStream_t stream);
// ... and n queries of `per` sub-fingerprints against a ragged corpus whose sliding blocks a builder wrote to d_blocks, key i to
// keys[i] (d_scores: n == 1)
OSStatus run_built_ragged(struct ::LBAudioDetectiveCorpus* c, const uint32_t* d_blocks, uint32_t n, uint32_t per, uint32_t range,
                          uint64_t index_base, float* d_scores, unsigned long long* keys, hipStream_t stream);
::LBAudioDetectiveFingerprintRef fingerprint_from_bools(const struct ::LBAudioDetective* d, const Boolean* bools, uint64_t per);
// the file entry points (api_files.cpp): decode, conversion and the window loop of n files in one launch chain per
// hop value; statuses (optional) receives every file's status
OSStatus process_audio_files(struct ::LBAudioDetective* d, const char* const* paths, size_t n,
                             ::LBAudioDetectiveFingerprintRef* out, OSStatus* statuses);

}  // namespace lbad

// ---- handle layouts ------------------------------------------------------------------------
struct LBAudioDetectiveFingerprint {
    uint32_t length = 0;
    uint32_t count = 0;
    std::vector<Boolean> data;  // count * length
};

struct LBAudioDetectiveFrame {
    uint32_t max_rows = 0;
    uint32_t n_rows = 0;
    uint32_t row_length = 0;
    std::vector<std::vector<Float32>> rows;  // max_rows slots, ragged like the reference
};

struct LBAudioDetective {
    AudioStreamBasicDescription format;
    uint32_t subfp_len;
    uint32_t window;
    uint32_t stride;
    uint32_t bands;
    uint32_t variant = 0;
    uint32_t band_form = 0;   // LBAudioDetectiveSetBandSumForm
    uint32_t tune_waves = 0;  // copied into the plan
    bool tune_cache = true;
    uint32_t hop_mode = 1;   // file entry points: 0 = hop in processing-rate samples, 1 = upstream's file-frame hop
    uint32_t tail_mode = 1;  // hop mode 1, windows past the end of the file: 0 zero-filled, 1 nothing read, 2 stale spectrum
    uint32_t resampler = 0;  // 0 long Kaiser sinc, 1 short sinc, 2 linear interpolation
    lbad::Plan plan;         // lazily rebuilt when the configuration changes
    lbad::DeviceBuffer<float> d_frames;  // frame rows between stage 1 and stage 2
    // bytes of HBM the inter-stage buffer may take.  512 MiB = 32 768 frames per chunk: the configs[1] pass of 500 000
    // frames runs as 16 chunks and is 2.5 % FASTER than as one (20.05 against 20.57 ms; 16 GiB was the default until
    // round 3), below 128 MiB the launches start to cost (tools/exp/scratch_chunks.py)
    uint64_t scratch_limit = 512ull << 20;
    // persistent buffers of the one-off (host in, host out) entry points; they only grow (a quarter more than asked for)
    lbad::DeviceBuffer<void> d_io_pcm;
    lbad::DeviceBuffer<uint32_t> d_io_packed;
    lbad::PinnedBuffer<void> h_io;   // pinned staging for small calls
    hipStream_t io_stream = nullptr;
    // converter state of the file entry points: input / output samples and the two kernel tables, grown on demand
    lbad::DeviceBuffer<uint8_t> d_rs_bytes[2];   // the files' payloads as read; file batches, slot 1: run i + 1's payloads go up while run i is decoded
    hipStream_t up_stream = nullptr;  // the uploads of a file batch (beside io_stream, which runs the kernels)
    hipEvent_t up_done[2] = {nullptr, nullptr};      // behind a run's uploads, on up_stream
    hipEvent_t bytes_free[2] = {nullptr, nullptr};   // behind the decode kernel that read the slot's payloads, on io_stream
    hipEvent_t packed_done[2] = {nullptr, nullptr};  // behind the copy of a group's packed results into the slot's pinned block
    lbad::DeviceBuffer<float> d_rs_in;           // decoded mono samples at the file's rate
    lbad::DeviceBuffer<float> d_rs_out;
    lbad::DeviceBuffer<double> d_rs_table[2];
    std::vector<lbad::DevPhase> d_phases;   // phase tables of the rational rate pairs met so far
    lbad::DeviceBuffer<lbad::FileDesc> d_rs_desc;   // per-file descriptors of a file batch
    lbad::DeviceBuffer<uint32_t> d_rs_tail;      // tail-mode-2 tables of a file batch
    // a file batch goes through in runs, two in flight (api_files.cpp): while the device works on run i the host reads
    // run i + 1 into the other pinned block, and run i's results are unpacked while the device works on run i + 1
    lbad::PinnedBuffer<uint8_t> h_files[2];      // per slot: pinned block a run of files is read into
    lbad::PinnedBuffer<uint32_t> h_packed[2];    // ... and the pinned landing area of a run's packed results
    bool file_pipeline = true;        // LBAudioDetectiveSetFilePipeline(…, 0): one run at a time (measurement)
    // optional per-stage timing (hipEvents on the caller's stream)
    bool timing = false;
    std::vector<hipEvent_t> ev;   // 3 per chunk: start, after stage 1, after stage 2
    size_t ev_used = 0;
    // Concurrent use (round 3).  The claim counters of the plan, the inter-stage rows and the io / converter buffers
    // are ONE set per detective: `mutex` serialises the host side of every entry point, and a batch call that arrives
    // on another stream than its predecessor first waits (on the device, hipStreamWaitEvent) for `done` -- the
    // predecessor's last kernel.  Two threads with two streams therefore get correct results, one after the other;
    // for overlap use one detective per stream.  Nothing is recorded or awaited while the stream is being captured
    // into a graph (a replay is the caller's to order).
    std::recursive_mutex mutex;
    hipEvent_t done = nullptr;
    hipStream_t done_stream = nullptr;
    bool done_valid = false;
};

// first statement of every entry point that touches a detective's state
#define LBAD_LOCK(d) std::unique_lock<std::recursive_mutex> lbad_lock_; if (d) lbad_lock_ = std::unique_lock<std::recursive_mutex>((d)->mutex)

struct LBAudioDetectiveCorpus {
    uint32_t subfp_len = 0;
    uint32_t n_sub = 0;
    uint64_t capacity = 0;
    uint64_t count = 0;
    uint32_t variant = 0;
    // The blocks made with the corpus (planes or records, offsets, plan, keys) keep their addresses for its lifetime.
    lbad::DeviceBuffer<uint4> d_planes;          // plane layout [n_planes][capacity]
    uint32_t n_planes = 0;
    lbad::StagingPair<uint32_t> query;           // query block on the device and the pinned staging copy of it
    lbad::DeviceBuffer<unsigned long long> d_key;
    // host-synchronous query without memset / copy / stream synchronisation (api_corpus.cpp)
    lbad::DeviceBuffer<unsigned long long> d_fast_key;   // zero between queries
    unsigned int* d_ticket = nullptr;            // (inside d_fast_key, behind the scan's slots)
    lbad::PinnedBuffer<unsigned long long> h_out;        // pinned, host-coherent: [0] key, [1] sequence number
    unsigned long long* h_out_dev = nullptr;     // its device address (an alias, like d_ticket)
    unsigned long long seq = 0;
    hipStream_t stream = nullptr;
    bool appended = false;                       // entries were appended since the last polled query
    lbad::Event append_event;                    // recorded behind the latest append on ITS stream
    // ragged form (LBAudioDetectiveCorpusNewRagged): entries of any length as a stream of 32-byte records
    bool ragged = false;
    lbad::DeviceBuffer<uint4> d_recs;            // 2 x uint4 per record
    uint64_t rec_capacity = 0;                   // records
    uint64_t n_pos = 0;                          // records stored
    lbad::DeviceBuffer<uint32_t> d_off;          // capacity + 1 record positions (entry e = [off[e], off[e + 1]))
    std::vector<uint32_t> h_off;                 // count + 1
    uint32_t ne_max = 0;                         // longest entry
    std::map<uint32_t, uint64_t> len_hist;       // entries per length: the scan's task totals for any query length
    // the scan's plan for ONE query length (k_sliding.hip): rebuilt when the length, the entries or the grid change
    lbad::DeviceBuffer<uint32_t> d_plan;
    uint32_t plan_nq = 0, plan_grid = 0, plan_bmin = 0;
    bool bound_pruning = true;     // top-1 scans of a ragged corpus may drop passes that cannot reach the best match so far (exact)
    float prune_from = 0.7f;       // ... once a match of at least this score is known (LBAudioDetectiveCorpusSetBoundPruningThreshold)
    uint64_t plan_count = 0;
    lbad::Event plan_built;                      // behind the plan's kernels, on plan_stream
    hipStream_t plan_stream = nullptr;
    // key block of the sharded query (api_rccl.cpp), made with the corpus so that the collective call never allocates
    lbad::DeviceBuffer<unsigned long long> d_shard_keys;
    lbad::PinnedBuffer<unsigned long long> h_shard_keys;
    // ring of query slots in `query` (ragged scan): slot size in words, one event per slot, queries so far
    size_t query_slot_words = 0;
    lbad::Event query_ev[8];
    // per ring slot: the scan's running maxima (8 words) and its ticket, ZERO between scans -- the scan's last workgroup
    // leaves them so (sliding_common.hpp: ScanOut); 16 words per slot
    lbad::DeviceBuffer<unsigned long long> d_scan_out;
    bool scan_out_dirty = false;                 // a scan's launch failed: clear the words before the next one
    std::mutex shard_lock;                       // the sharded query's key block is one per corpus (api_rccl.cpp)
    bool shard_stale = false;                    // a sharded query timed out: work may still be queued behind the key block
    lbad::Event shard_stale_event;               // ... recorded behind that work when the call gave up (the stream may be gone by the next call)
    uint64_t query_seq = 0;
    // top-K queries (api_select.cpp): score rows (up to kQueryBatchMax x count floats), the selection's scratch, the staged
    // query blocks of the batch scan, the scans' own key words (the top-1 state -- d_key, the polled slots -- stays
    // untouched) and the keys of the host-returning forms.  Grown on demand.  topk_ev covers d_topk_scores, d_topk_scratch,
    // d_threshold_scratch, topk_q, d_topk_scan_keys and d_topk_keys: a call touches them only after it, and records it behind
    // its selection -- the last kernel that reads or writes any of them -- also after a failure, behind whatever was launched.
    // The alignment that a packed call runs behind its selection is NOT under it (align_ev and pq_ev cover what it reads): the
    // next call on another stream waits for the selection, not for the lags.  The recording passes that select (api_recording.cpp)
    // keep their score row and selection words under it too.
    lbad::DeviceBuffer<float> d_topk_scores;
    lbad::DeviceBuffer<void> d_topk_scratch;
    lbad::StagingPair<uint32_t> topk_q;
    lbad::DeviceBuffer<unsigned long long> d_topk_scan_keys;   // kQueryBatchMax words
    lbad::DeviceBuffer<unsigned long long> d_topk_keys;
    lbad::Event topk_ev;
    // threshold queries (api_select.cpp): the tile counts and offsets of the selection of k_threshold.hip.  The score rows, the
    // scans' key words, the staged query blocks, the host forms' key buffer and the event are the top-K calls': one convention
    // for one scratch.
    lbad::DeviceBuffer<void> d_threshold_scratch;
    // alignment (api_align.cpp): the staged query words and their table (device + pinned), the per-pair maxima of a split
    // launch, and the results of the host-returning forms (keys, lags or a profile) on their way back.  Grown on demand; a
    // call reuses them only after align_ev, recorded behind the previous call's last kernel.
    lbad::StagingPair<uint32_t> align_q;
    lbad::DeviceBuffer<unsigned long long> d_align_best;
    lbad::DeviceBuffer<void> d_align_out;
    lbad::Event align_ev;
    // packed queries (the ...QueryPacked...Device calls): what the builders of k_query.hip write -- the scan's blocks, then the
    // alignment's table and words.  Grown on demand.  pq_ev covers d_pq alone: a call touches it only after it, and records it
    // behind the last kernel that reads d_pq (the last scan, or the alignment when lags are wanted), also after a failure.
    lbad::DeviceBuffer<uint32_t> d_pq;
    lbad::Event pq_ev;
    // corpus join (LBAudioDetectiveCorpusJoinThreshold..., k_join.hip), held by the corpus that is scanned: the chunk's row
    // blocks, counts, offsets and the total carried between chunks.  Grown on demand up to the limit (0 = the default); a call
    // reuses it only after join_ev, recorded behind its last kernel.  A corpus that only supplies the rows records its own
    // join_ev too, each join's stream first going behind the record before: Dispose awaits every join that reads the planes.
    lbad::DeviceBuffer<void> d_join_scratch;
    lbad::Event join_ev;
    uint64_t join_scratch_limit = 0;
    // removal (LBAudioDetectiveCorpusRemove..., api_remove.cpp, k_remove.hip): the index block (RemoveIndex) with the staged
    // list of the host form and, ragged, the new offsets behind it; and the bounce buffer the kept planes or records of a chunk
    // pass through, bounded by the limit (0 = the default).  Both grow on demand; a removal is synchronous, nothing of it is in
    // flight when it returns.
    lbad::DeviceBuffer<uint32_t> d_remove_index;
    lbad::DeviceBuffer<unsigned long long> d_remove_list;
    lbad::DeviceBuffer<uint32_t> d_remove_off;
    lbad::DeviceBuffer<uint4> d_remove_bounce;
    uint64_t remove_scratch_limit = 0;
    // gather (LBAudioDetectiveCorpusGather..., api_gather.cpp, k_gather.hip): the tile sums of the offsets' scan.  Grown on demand;
    // a call reuses it only after gather_ev, recorded behind its last kernel.
    lbad::DeviceBuffer<void> d_gather_scratch;
    lbad::Event gather_ev;
    // entry ids (LBAudioDetectiveCorpusSetEntryIds..., api_ids.cpp, k_ids.hip): empty until the first ids are set, then `capacity`
    // words for the corpus' lifetime (0: no id; the words at and above the count are zero).  The id index (slot ids and slot
    // indices, ids_slots of each in use) is built by the first KeysFromIds after anything made it stale and kept until then;
    // d_ids_scratch is the removal's compaction block, h_ids_stage the host form's pinned staging.  ids_ev covers them all: an
    // id call touches them only after it, and records it behind its last launch, also after a failure.
    lbad::DeviceBuffer<unsigned long long> d_ids;
    lbad::DeviceBuffer<unsigned long long> d_ids_slot_ids;
    lbad::DeviceBuffer<uint32_t> d_ids_slot_index;
    uint64_t ids_slots = 0;
    bool ids_index_valid = false;
    lbad::DeviceBuffer<unsigned long long> d_ids_scratch;
    lbad::PinnedBuffer<unsigned long long> h_ids_stage;
    lbad::Event ids_ev;
};

namespace lbad {
// api_ids.cpp, for the corpus file (api_corpus.cpp): the trailer of a corpus with ids behind the payload (nothing for one
// without), and the trailer of a file read back -- false: a trailer that lies about itself, the load fails
OSStatus ids_save_trailer(struct ::LBAudioDetectiveCorpus* c, FILE* f);
bool ids_load_trailer(struct ::LBAudioDetectiveCorpus* c, FILE* f, uint64_t count);
// api_ids.cpp, for the removal (api_remove.cpp): the ids of a corpus that has them move with the entries (map: the call's device
// map; first: the lowest removed index; kept < count entries stay) on `stream`, and the index is stale
OSStatus ids_compact(struct ::LBAudioDetectiveCorpus* c, const uint32_t* d_map, uint64_t first, uint64_t kept, hipStream_t stream);
}  // namespace lbad
