// k_rows_pruned.hip -- specialised stage 1 for 1024-sample windows whose bands read only the
// lowest FFT bins (44.1 kHz / 1024: bins 0..21): windows -> 128 x 32 frame rows.
//
// Same arithmetic as k_fft_bands.hip / oracle rfft_exec (radix-2 DIT, nested-fma butterflies),
// but only the butterflies the 22 consumed bins depend on are executed:
//
//   * 8 lanes own one window.  Lane r holds the 64 complex points z[r + 8m] and runs DIT stages
//     1..5 (two 32-point blocks) entirely in registers with compile-time twiddles.
//   * Stage 6 is pruned to the 43 outputs k64 in [0,21] u [43,63] that feed bins 0..21 and their
//     mirror bins 491..511 (needed by the real-FFT split pass).
//   * Stages 7..9 combine the 8 lanes.  Each needed bin is a 7-butterfly reduction tree over the
//     8 lanes' values of one stage-6 output; the values cross lanes through a per-wave LDS
//     transpose buffer and one lane evaluates both trees of a bin pair (k, 512-k), the split
//     pass, the positive-only normalisation and the power term.
//   * The work unit is a quarter frame (32 windows): its PCM span (31 * 64 + 1024 samples) goes from
//     HBM to LDS once, so the 16x window overlap costs no extra HBM traffic.  Persistent workgroups
//     (two per CU) claim frames from per-XCD counters and refill the span buffer with
//     global_load_lds behind the arithmetic of the current unit (see frame_rows_pruned_kernel).
//
// Executed work, counted in the compiled main loop (one quarter frame per iteration; tests/test_isa_rows_pruned.py
// pins the butterflies): 739 vector instructions per wave on the fast path, 629 of them the packed butterflies
// (498 v_pk_fma_f32, 131 v_pk_add_f32), which is 2321 float operations per lane (an FMA = 2) or 18.6 k per window,
// instead of 25.6 k for the full transform and with every slot of a packed instruction counted; results are
// bit-identical because every surviving butterfly is evaluated exactly as in the full network.  The band means
// divide by a per-band constant: three instructions per quotient behind a guard (const_div.hpp), the IEEE
// sequence only in the waves whose guard trips.
//
// Two kernels share everything up to the split pass.  frame_rows_pruned_kernel adds a band's power terms through LDS (band =
// lane) and takes any table whose bands read bins 0..21; frame_rows_lanes_kernel (further down) is compiled for the default
// 44.1 kHz table, deals the bins out so that every band lies in one lane and adds in registers (tests/test_isa_rows_lanes.py
// pins its loop).  launch_rows_pruned takes the second where rows_lanes_supported holds.
#include "internal.hpp"

#include <cstring>
#include "const_div.hpp"
#include "fft64_lane.hpp"

namespace lbad {
namespace {

constexpr int kW = 1024;
constexpr int kStride = 64;
constexpr int kBands = 32;
constexpr int kBins = 22;           // bins 0..21
constexpr int kRows = 43;           // stage-6 outputs kept per lane
constexpr int kRowsA = 22;          // pass 1: rows 0..21 ("+" side), pass 2: rows 22..42 (mirror side)
constexpr int kRowDw = 20;          // dwords per transpose row: 8 lanes x 8 B, padded 64 -> 80 B
constexpr int kWinDw = 464;         // 22 rows x 20 = 440, padded so that window stride = 16 (mod 32) banks
constexpr int kWaves = 4;
constexpr int kThreads = kWaves * 64;
constexpr int kUnitWindows = 32;    // a workgroup owns a quarter frame: 4 waves x 8 windows
constexpr int kSpan = (kUnitWindows - 1) * kStride + kW;  // 3008 samples
constexpr int kSpanDw = kSpan + 16 * (kSpan >> 6);        // 16-dword skew per 64 samples: 3760
constexpr int kTDw = kWaves * 8 * kWinDw;                 // per wave: 8 windows x one pass of rows
constexpr int kBinConst = 14;       // per-bin twiddle block, see rows_pruned_constants()
constexpr int kConstStride = 20;    // 14 floats per bin padded to 80 B: lanes with different bins hit different banks
constexpr int kConstDw = kBins * kConstStride;
constexpr int kClaimOffset = 312;   // plan.d_bin_const: 308 constants, padding, then 8 claim counters (one per XCD) and the exit ticket
constexpr int kClaimWords = 16;     // counters [0..7], ticket [8], padding
constexpr int kLdsBytes = (kSpanDw + kTDw + kConstDw + 4) * 4;   // 75 856 B: two workgroups per CU
constexpr int kWgPerCu = 2;
static_assert(kWgPerCu * kLdsBytes <= 160 * 1024, "two workgroups must fit one CU's LDS");

using namespace lane64;

// stage-6 outputs: row i < 22 is k64 = i ("+" output of pair j = i); row i >= 22 is k64 = i + 21
// ("-" output of pair j = i - 11)
template <int I>
__device__ __forceinline__ cplx stage6_row(const cplx (&x)[64]) {
    constexpr int j = I < 22 ? I : I - 11;
    constexpr bool plus = I < 22;
    const cplx u = x[j], v = x[j + 32];
    if constexpr (j == 0) {
        return u + v;   // only the "+" output of pair 0 is needed
    } else if constexpr (j == 16) {
        return plus ? fma2(mk(1.0f, -1.0f), v.yx, u) : fma2(mk(-1.0f, 1.0f), v.yx, u);
    } else {
        constexpr float wr = kTw64Re[j], wi = kTw64Im[j];
        if constexpr (plus) return fma2(mk(wr, wr), v, fma2(mk(-wi, wi), v.yx, u));
        else return fma2(mk(-wr, -wr), v, fma2(mk(wi, -wi), v.yx, u));
    }
}

// rows [I, END) of stage 6 -> transpose buffer rows [I - FIRST, ...).  volatile keeps the compiler
// from fusing pairs into ds_write2_b64 / ds_read2_b64, which run at half the rate of the plain
// 64-bit forms on gfx950.
template <int I, int END, int FIRST>
__device__ __forceinline__ void store_rows(const cplx (&x)[64], float* trow) {
    if constexpr (I < END) {
        *(lds_vf32x2*)(trow + (I - FIRST) * kRowDw) = stage6_row<I>(x);
        store_rows<I + 1, END, FIRST>(x, trow);
    }
}

template <int I, int END, int FIRST>
__device__ __forceinline__ void hold_rows(const cplx (&x)[64], cplx (&h)[kRows - kRowsA]) {
    if constexpr (I < END) {
        h[I - FIRST] = stage6_row<I>(x);
        hold_rows<I + 1, END, FIRST>(x, h);
    }
}
template <int I, int N>
__device__ __forceinline__ void store_held(const cplx (&h)[kRows - kRowsA], float* trow) {
    if constexpr (I < N) {
        *(lds_vf32x2*)(trow + I * kRowDw) = h[I];
        store_held<I + 1, N>(h, trow);
    }
}

template <int M>
__device__ __forceinline__ void load_points(cplx (&x)[64], const float* src) {
    if constexpr (M < 64) {
        // register slot I holds point m = brev6(I): sample 2r + 16 m of the window sits
        // (m & 3) * 16 + (m >> 2) * 80 dwords after the lane base.  Loading in slot order lets the
        // first butterflies start while the later points are still in flight.
        constexpr int m = brev6(M);
        x[M] = *(const lds_vf32x2*)(src + (m & 3) * 16 + (m >> 2) * 80);
        load_points<M + 1>(x, src);
    }
}

// 7-butterfly reduction over the 8 lanes' values of one stage-6 row (DIT stages 7, 8, 9).  Operands
// and evaluation are separate so that a pass can have the reads of all its rounds in flight at once.
typedef float f32x4 __attribute__((ext_vector_type(4)));
struct TreeIn {
    f32x4 q0, q1, q2, q3;
};
struct TreeTw {     // twiddles of one tree: W_128^k, W_256^k, W_512^k (or their mirror forms)
    f32x2 t0, t1, t2;
};
// LDS reads after the span prefetch of an iteration are written out: the compiler cannot tell the buffers carved out of the
// one dynamic LDS array apart, so it orders every LDS load of its own behind the outstanding global_load_lds (s_waitcnt
// vmcnt(0) in the middle of the unit), although the prefetch writes the span buffer only.  A read issued here is invisible to
// that bookkeeping and to the compiler's lgkmcnt counting: whoever issues one waits for it with lds_wait before the first use.
// LDS serves a wave's operations in order, so lgkmcnt(N) is enough for a read that at least N later LDS operations follow; the
// "memory" clobbers keep the reads, the waits and the stores around them in program order.
typedef __attribute__((address_space(3))) const float lds_cf32;
__device__ __forceinline__ uint32_t lds_addr(const float* p) { return (uint32_t)(size_t)(lds_cf32*)p; }
template <int BYTES>
__device__ __forceinline__ f32x4 lds_read128(uint32_t addr) {
    f32x4 v;
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(BYTES) : "memory");
    return v;
}
template <int BYTES>
__device__ __forceinline__ float lds_read32(uint32_t addr) {
    float v;
    asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(BYTES) : "memory");
    return v;
}
// the row BYTES behind LDS address `a` (rows a fixed distance apart share one address register)
template <int BYTES = 0>
__device__ __forceinline__ TreeIn tree_load(uint32_t a) {
    TreeIn in;
    in.q0 = lds_read128<BYTES>(a);
    in.q1 = lds_read128<BYTES + 16>(a);
    in.q2 = lds_read128<BYTES + 32>(a);
    in.q3 = lds_read128<BYTES + 48>(a);
    return in;
}
// at most N LDS operations of the wave still outstanding: the operands are defined from here on
template <int N>
__device__ __forceinline__ void lds_wait(TreeIn& in) {
    asm volatile("s_waitcnt lgkmcnt(%4)" : "+v"(in.q0), "+v"(in.q1), "+v"(in.q2), "+v"(in.q3) : "n"(N) : "memory");
}
template <int N>
__device__ __forceinline__ void lds_wait(TreeIn (&in)[3]) {
    asm volatile("s_waitcnt lgkmcnt(%12)"
                 : "+v"(in[0].q0), "+v"(in[0].q1), "+v"(in[0].q2), "+v"(in[0].q3), "+v"(in[1].q0), "+v"(in[1].q1),
                   "+v"(in[1].q2), "+v"(in[1].q3), "+v"(in[2].q0), "+v"(in[2].q1), "+v"(in[2].q2), "+v"(in[2].q3)
                 : "n"(N)
                 : "memory");
}
// pass 1: the mirror-row stores follow the twelve reads, and the counter saturates at 15
constexpr int kPass1Wait = kRows - kRowsA < 15 ? kRows - kRowsA : 15;
__device__ __forceinline__ TreeTw tree_twiddles(const float* tw) {
    TreeTw t;
    t.t0 = *reinterpret_cast<const f32x2*>(tw);
    t.t1 = *reinterpret_cast<const f32x2*>(tw + 2);
    t.t2 = *reinterpret_cast<const f32x2*>(tw + 4);
    return t;
}
__device__ __forceinline__ cplx tree_eval(const TreeIn& in, const TreeTw& t) {
    const cplx x0 = mk(in.q0.x, in.q0.y), x1 = mk(in.q0.z, in.q0.w), x2 = mk(in.q1.x, in.q1.y), x3 = mk(in.q1.z, in.q1.w);
    const cplx x4 = mk(in.q2.x, in.q2.y), x5 = mk(in.q2.z, in.q2.w), x6 = mk(in.q3.x, in.q3.y), x7 = mk(in.q3.z, in.q3.w);
    const cplx y0 = madd(x0, t.t0.x, t.t0.y, x4), y1 = madd(x1, t.t0.x, t.t0.y, x5);
    const cplx y2 = madd(x2, t.t0.x, t.t0.y, x6), y3 = madd(x3, t.t0.x, t.t0.y, x7);
    const cplx z0 = madd(y0, t.t1.x, t.t1.y, y2), z1 = madd(y1, t.t1.x, t.t1.y, y3);
    return madd(z0, t.t2.x, t.t2.y, z1);
}

// per-bin constants (kBinConst floats, padded to kConstStride): [0..5] twiddles of the "+" tree (stages 7, 8,
// 9), [6..11] of the mirror tree, [12..13] split-pass twiddle W_1024^k
//
// The span of the quarter frame starting at sample `first` goes to LDS skewed by 16 dwords per 64
// samples (so that the 4 windows of a 32-lane group hit disjoint bank quarters when the points are read).
// FMT 0 (float32): one global_load_lds_dword per 64 samples -- the data never passes through VGPRs
// and the wave does not wait for it before the head of the next iteration (the LDS reads in between are issued by hand,
// see lds_read128: tests/test_isa_rows_waits.py); FMT 1 / 2 (int16 / 32768, int32 / 2^31) convert in registers.
typedef __attribute__((address_space(1))) const void gvoid_t;
typedef __attribute__((address_space(3))) void lvoid_t;

template <int FMT>
__device__ __forceinline__ void span_to_lds(const void* __restrict__ pcm_raw, uint64_t first, float* span, int wave,
                                            int lane) {
    if constexpr (FMT == 0) {
        // `wave` is wave-uniform (an SGPR): chunk c = wave + 4 i, fully unrolled, LDS base through M0.  The chunks of a
        // wave are 1024 B apart in HBM.  Four of them share one address and differ in the instruction's immediate
        // offset, which the hardware adds on BOTH sides, so the LDS base gives it back; the address itself is a
        // scalar base (the wave's first sample) plus one 32-bit lane offset, so that stepping it is scalar work too.
        // The LDS bases are re-derived from `lbase` at every call (the empty asm hides that they never change):
        // eleven loop-invariant scalars are more than the scalar file has left, they were spilled to vector lanes.
        const uint64_t first_w = first + 64 * wave;
        const uint64_t first_s = ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(first_w >> 32)) << 32) |
                                 (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)first_w);
        const char* src = static_cast<const char*>(pcm_raw) + 4 * first_s;
        const uint32_t lane_off = 4u * (uint32_t)lane;
        uint32_t lbase = (uint32_t)(size_t)(lvoid_t*)(span + 80 * wave);
        int tail_wave = wave;                             // likewise: no 64-bit mask of "wave < 3" kept over the loop
        asm volatile("" : "+s"(lbase), "+s"(tail_wave));
        constexpr int kFull = (kSpan / 64) / kWaves;      // 47 chunks: 11 rounds of 4, then waves 0..2
        static_assert(kFull == 11, "three groups of four loads");
#define LBAD_SPAN_LOAD(I)                                                                                            \
    __builtin_amdgcn_global_load_lds((gvoid_t*)(src + 4 * 64 * kWaves * ((I) & ~3) + lane_off),                      \
                                     (lvoid_t*)(size_t)(lbase + 4 * (80 * kWaves * (I) - 64 * kWaves * ((I) & 3))),  \
                                     4, 4 * 64 * kWaves * ((I) & 3), 0)
        LBAD_SPAN_LOAD(0); LBAD_SPAN_LOAD(1); LBAD_SPAN_LOAD(2); LBAD_SPAN_LOAD(3);
        LBAD_SPAN_LOAD(4); LBAD_SPAN_LOAD(5); LBAD_SPAN_LOAD(6); LBAD_SPAN_LOAD(7);
        LBAD_SPAN_LOAD(8); LBAD_SPAN_LOAD(9); LBAD_SPAN_LOAD(10);
        if (tail_wave < kSpan / 64 - kFull * kWaves) LBAD_SPAN_LOAD(11);
#undef LBAD_SPAN_LOAD
    } else if constexpr (FMT == 1) {
        const int16_t* src = static_cast<const int16_t*>(pcm_raw) + first;
        for (int s = threadIdx.x; s < kSpan; s += kThreads)
            span[s + 16 * (s >> 6)] = (float)src[s] * (1.0f / 32768.0f);
    } else {
        const int32_t* src = static_cast<const int32_t*>(pcm_raw) + first;
        for (int s = threadIdx.x; s < kSpan; s += kThreads)
            span[s + 16 * (s >> 6)] = (float)src[s] * (1.0f / 2147483648.0f);
    }
}

// Persistent workgroups, two per CU.  Every XCD owns a contiguous range of frames; its workgroups take
// the first ones statically and claim the rest, a frame (four quarter frames) at a time, from a per-XCD
// counter (the waves of a workgroup do not land evenly on the SIMDs, so equal static shares finish up
// to 40 % apart).  As soon as every wave holds its points of quarter frame u in registers, the span of
// the next one streams into the same LDS buffer behind the arithmetic; the claim for the frame after
// is in flight for three iterations (a global atomic: nothing waits for it or in front of it before the loop head), and
// the rows of u drain to HBM during u + 1.
// No memset node in front of a launch: every workgroup takes a ticket when it is done with the counters (its last claim
// has returned), and the last one leaves the counters and the ticket at zero for the next launch.  Launches that share
// the counters never overlap: they belong to one plan, whose calls are serialised (StreamOrder orders different
// streams, a captured graph keeps its stream's order).
// The claim goes through a global address-space pointer: an atomic on a generic one is a flat instruction, which may touch LDS,
// and the compiler then drains the span prefetch issued just before it (s_waitcnt vmcnt(0)) in front of the claim.
typedef __attribute__((address_space(1))) uint32_t claim_ctr_t;
__device__ __forceinline__ void claims_done(uint32_t* claim_ctr) {
    __threadfence();
    if (atomicAdd(claim_ctr + 8, 1u) == gridDim.x - 1u) {
        __threadfence();
#pragma unroll
        for (int i = 0; i < 9; ++i) atomicExch(claim_ctr + i, 0u);
        __threadfence();
    }
}

template <int FMT>
__global__ __launch_bounds__(kThreads, kWgPerCu) void frame_rows_pruned_kernel(const void* __restrict__ pcm_raw,
                                                                         uint64_t samples_per_clip,
                                                                         uint32_t frames_per_clip, uint64_t n_units,
                                                                         uint64_t units_per_xcd,
                                                                         const float* __restrict__ bin_const,
                                                                         const uint32_t* __restrict__ band_tbl,
                                                                         uint32_t* __restrict__ claim_ctr,
                                                                         float* __restrict__ frames, uint32_t frame_dw,
                                                                         uint32_t place_tbl) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* span = smem;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    float* tbuf = smem + kSpanDw + wave * (8 * kWinDw);
    float* vbuf = tbuf;                       // power terms reuse the wave's transpose area after the trees
    float* cbuf = smem + kSpanDw + kTDw;
    uint32_t* claim_slot = reinterpret_cast<uint32_t*>(cbuf + kConstDw);

    // Workgroup b runs on XCD b % 8 (observed dispatch order; used for speed only: a workgroup on
    // another XCD would see its own copy of the counter and repeat work, not skip any).  Giving every
    // XCD a contiguous range makes neighbouring quarter frames -- whose PCM spans overlap by a third --
    // share one L2 instead of fetching the overlap from HBM once per XCD.
    const uint32_t wg_per_xcd = gridDim.x >> 3;
    const uint64_t xcd_begin = (uint64_t)(blockIdx.x & 7) * units_per_xcd;     // units_per_xcd is a multiple of 4
    const uint64_t xcd_end = xcd_begin + units_per_xcd < n_units ? xcd_begin + units_per_xcd : n_units;
    uint64_t unit = xcd_begin + 4 * (uint64_t)(blockIdx.x >> 3);
    if (unit >= xcd_end) {
        if (threadIdx.x == 0) claims_done(claim_ctr);
        return;
    }

    auto span_start = [&](uint64_t u) {
        const uint32_t frame = (uint32_t)(u >> 2);          // the launcher keeps unit numbers below 2^31
        const uint32_t clip = frame / frames_per_clip;
        const uint32_t fi = frame - clip * frames_per_clip;
        return (uint64_t)clip * samples_per_clip + (uint64_t)(fi * 128 + (uint32_t)(u & 3) * kUnitWindows) * kStride;
    };
    // the claimer keeps its counter's address in vector registers: the scalar file is full, and as a scalar pair
    // it was spilled to vector lanes and fetched back at every claim
    claim_ctr_t* my_ctr = (claim_ctr_t*)(claim_ctr + (blockIdx.x & 7));
    asm volatile("" : "+v"(my_ctr));
    const bool claimer = threadIdx.x == 0;
    uint32_t claimed = 0;

    span_to_lds<FMT>(pcm_raw, span_start(unit), span, wave, lane);
    for (int i = threadIdx.x; i < kBins * kBinConst; i += kThreads)
        cbuf[(i / kBinConst) * kConstStride + (i % kBinConst)] = bin_const[i];
    const int band = lane & 31;
    const uint32_t b_lo = band_tbl[band], b_hi = band_tbl[kBands + band];
    const float b_div = __uint_as_float(band_tbl[2 * kBands + band]);
    // the band's mean is p / b_div.  b_rcp = RN(1 / b_div); a band whose divisor is proven for the short form of
    // const_div.hpp accepts dividends up to the largest finite float, any other band none (a sum of squares is >= +0,
    // so its bit pattern orders like its value)
    const float b_rcp = __uint_as_float(band_tbl[9 * kBands + band]);
    const int b_fast_hi = band_tbl[10 * kBands + band] ? (int)kBandDivHi : -1;   // compared as bit patterns
    // where the band's mean of row w goes inside a frame of frame_dw floats: w * b_mult + b_off -- rows of 32 bands, or
    // the compact frame of plan.sparse (128 rows of the bands that can be non-zero; b_off = 0xFFFFFFFF: a band that is +0.0
    // in every window and that nobody reads)
    // Two words, unpacked where they are used (the empty asm hides that they never change): with b_lo, b_hi, b_mult and b_off
    // in registers of their own, and what the compiler derived from them ahead of the loop, the kernel took 250 VGPRs, with
    // the packed words 241.  A band reads bins below kBins, a row has at most kBands words.
    const uint32_t b_range = b_lo | (b_hi << 8);
    const uint32_t b_mult0 = band_tbl[place_tbl * kBands + band], b_off0 = band_tbl[(place_tbl + 1) * kBands + band];
    const uint32_t b_place = b_off0 != 0xFFFFFFFFu ? b_mult0 | (b_off0 << 8) : 0xFFFFFFFFu;

    const int w8 = lane >> 3, r = lane & 7;
    const float inv_norm = 1.0f / (float)(kW / 4);
    // bin tasks: the 8 lanes of a window share its 22 bins, lane r taking bins r', r' + 8, r' + 16 (< 22): eight lanes
    // read eight consecutive rows of one window.  r' = r, or r ^ 4 in the windows 1, 2 (mod 4) of the wave (round 5):
    // a ds_read_b128 is served in the lane groups {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}, ... -- lanes 0-3 of window
    // 0, 4-7 of windows 1 and 2, 0-3 of window 3 --, and with r' = r throughout two of the four windows of a group
    // met on the same 16-byte slots (window pitch 116 slots = 4 mod 16, rows 5 slots apart): every tree read took twice
    // its cycles, 18 % of the kernel's LDS-active cycles were conflicts.  With the halves of windows 1 and 2 swapped the
    // sixteen lanes of every group read sixteen different slots (the pitch stays: the 16 contiguous lanes of a
    // ds_write_b64 group want the windows 16 banks apart).
#ifdef LBAD_EXP_TREE_NOSWAP
    const int rr = r;
#else
    const int rr = r ^ ((((w8 + 1) >> 1) & 1) << 2);
#endif
    int tk[3];
#pragma unroll
    for (int rd = 0; rd < 3; ++rd) tk[rd] = rr + 8 * rd < kBins ? rr + 8 * rd : kBins - 1;
    const bool last_valid = rr + 16 < kBins;
    // LDS addresses of the rows a lane's trees read: tasks 0 and 1 are always eight rows apart (rr + 8 < kBins)
    const uint32_t row01 = lds_addr(tbuf + w8 * kWinDw + tk[0] * kRowDw), row2 = lds_addr(tbuf + w8 * kWinDw + tk[2] * kRowDw);
    const uint32_t mrow10 = lds_addr(tbuf + w8 * kWinDw + (21 - tk[1]) * kRowDw), mrow2 = lds_addr(tbuf + w8 * kWinDw + (21 - tk[2]) * kRowDw);

    // a lane serves the same three (window, bin) tasks in every quarter frame: their twiddles stay in registers
    __syncthreads();
    TreeTw twp[3], twm[3];
    f32x2 ws[3];
#pragma unroll
    for (int rd = 0; rd < 3; ++rd) {
        const float* c = cbuf + tk[rd] * kConstStride;
        twp[rd] = tree_twiddles(c);
        twm[rd] = tree_twiddles(c + 6);
        ws[rd] = *reinterpret_cast<const f32x2*>(c + 12);
    }

    float out[4] = {0.0f, 0.0f, 0.0f, 0.0f};   // band means of the previous quarter frame, stored one iteration late
    float* out_ptr = nullptr;
#ifdef LBAD_EXP_TIMELINE
    long long ts[8];
#define STAMP(i) ts[i] = __builtin_readcyclecounter()
#else
#define STAMP(i)
#endif
    auto store_out = [&]() {
        if (!out_ptr) return;
        uint32_t place = b_place;
        asm volatile("" : "+v"(place));
        const uint32_t b_mult = place & 0xFFu;
#pragma unroll
        for (int q = 0; q < 4; ++q) out_ptr[q * 2 * b_mult] = out[q];
    };
    for (;;) {
        STAMP(0);
#ifdef LBAD_EXP_TIMELINE
        const unsigned long long rt0 = __builtin_amdgcn_s_memrealtime();
#endif
        // ---- A: this quarter frame's span has landed (own loads: vmcnt, the other waves': barrier) ----
        __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0)
        const uint32_t quarter = (uint32_t)(unit & 3);
        if (quarter == 3 && claimer) claim_slot[0] = claimed;    // claimed three iterations ago
        __syncthreads();
        STAMP(1);

        // ---- B1: 64 points of this lane; once every wave has its points the span buffer is free -------
        cplx x[64];
        load_points<0>(x, span + 80 * (8 * wave + w8) + 2 * r);
        const uint64_t next = quarter == 3 ? xcd_begin + 4 * ((uint64_t)wg_per_xcd + claim_slot[0]) : unit + 1;
        __syncthreads();
        if (next < xcd_end) span_to_lds<FMT>(pcm_raw, span_start(next), span, wave, lane);
        if (quarter == 0 && claimer) claimed = __hip_atomic_fetch_add(my_ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#ifndef LBAD_EXP_TIMELINE
        store_out();
#endif
        STAMP(2);

        // ---- B2: DIT stages 1..5 in registers ---------------------------------------------------------
        // Issue priority: low while this wave is the arithmetic-heavy one, high for everything else (LDS
        // transposes, point reads, prefetch issue), whose short instructions should not queue behind the
        // co-resident wave's butterflies (17.3 -> 16.9 ms).
        __builtin_amdgcn_s_setprio(0);
        stage_blocks<1, 0>(x);
        stage_blocks<2, 0>(x);
        stage_blocks<3, 0>(x);
        stage_blocks<4, 0>(x);
        stage_blocks<5, 0>(x);
        STAMP(3);
        __builtin_amdgcn_s_setprio(3);

        // ---- B3/B4: stage 6, then the "+" rows through the transpose buffer; the mirror rows wait in
        //      registers (the 64 points are dead from here on, which leaves room to keep every read of a
        //      pass in flight) -----------------------------------------------------------------------------
        store_rows<0, kRowsA, 0>(x, tbuf + w8 * kWinDw + 2 * r);
        cplx held[kRows - kRowsA];
        hold_rows<kRowsA, kRows, kRowsA>(x, held);
        cplx za[3];
        {
            TreeIn in[3];
            in[0] = tree_load(row01);
            in[1] = tree_load<4 * 8 * kRowDw>(row01);
            in[2] = tree_load(row2);
            // ---- pass 2: the mirror rows reuse the same buffer.  LDS executes a wave's operations in
            //      order, so these stores cannot pass the reads above, and they are on their way while
            //      the trees of pass 1 are evaluated. ------------------------------------------------------
            store_held<0, kRows - kRowsA>(held, tbuf + w8 * kWinDw + 2 * r);
            lds_wait<kPass1Wait>(in);
#pragma unroll
            for (int rd = 0; rd < 3; ++rd) za[rd] = tree_eval(in[rd], twp[rd]);
        }
        STAMP(4);
        float pw[3];
        {
            TreeIn in[3];
            // mirror bin 512 - k is stage-6 row 43 - k, i.e. row 21 - k of this pass (bin 0 has no mirror:
            // its lane reads the stale row 21, which keeps the stride, and drops the result)
            in[0] = tree_load<4 * 8 * kRowDw>(mrow10);
            in[1] = tree_load(mrow10);
            in[2] = tree_load(mrow2);
#pragma unroll
            for (int rd = 0; rd < 3; ++rd) {
                const int k = tk[rd];
                if (rd == 0) lds_wait<8>(in[0]);        // four reads per round: two, one, no round behind this one
                else if (rd == 1) lds_wait<4>(in[1]);
                else lds_wait<0>(in[2]);
                const cplx b = tree_eval(in[rd], twm[rd]);
                const cplx a = za[rd];
                float re, im;
                if (k == 0) {
                    const float sm = a.x + a.y, df = a.x - a.y;
                    re = sm + sm;
                    im = df + df;
                } else {
                    const float sr = a.x + b.x, si = a.y - b.y;
                    const float dr = a.x - b.x, di = a.y + b.y;
                    const float wr = ws[rd].x, wi = ws[rd].y;
                    re = __fmaf_rn(wr, di, __fmaf_rn(wi, dr, sr));
                    im = __fmaf_rn(-wr, dr, __fmaf_rn(wi, di, si));
                }
                if (re > 0.0f) re = __fmul_rn(re, inv_norm);
                if (im > 0.0f) im = __fmul_rn(im, inv_norm);
                pw[rd] = __fadd_rn(__fmul_rn(re, re), __fmul_rn(im, im));
            }
        }
        STAMP(5);
        // power terms -> LDS only after every tree of the wave has read its rows
#pragma unroll
        for (int rd = 0; rd < 3; ++rd)
            if (rd < 2 || last_valid) vbuf[w8 * 24 + tk[rd]] = pw[rd];

        // ---- B5: band means, 8 windows x 32 bands per wave.  The four windows a lane serves advance
        //      together: one LDS round trip per bin instead of four. -----------------------------------
        float p[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        const float* vb = vbuf + (lane >> 5) * 24;
        uint32_t range = b_range;
        asm volatile("" : "+v"(range));
        for (uint32_t k = range & 0xFFu, k_end = range >> 8; k < k_end; ++k) {
            float v[4];
            const uint32_t va = lds_addr(vb + k);
            v[0] = lds_read32<0>(va);
            v[1] = lds_read32<4 * 48>(va);
            v[2] = lds_read32<4 * 96>(va);
            v[3] = lds_read32<4 * 144>(va);
            asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]) : : "memory");
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (v[q] == v[q] && fabsf(v[q]) != INFINITY) p[q] = __fadd_rn(p[q], v[q]);
        }
        // row = quarter * 32 + 8 * wave + 2 q + (lane >> 5)
        {
            uint32_t place = b_place;
            asm volatile("" : "+v"(place));
            const uint32_t b_mult = place & 0xFFu, b_off = place >> 8;
            out_ptr = place != 0xFFFFFFFFu
                          ? frames + (unit >> 2) * frame_dw + (quarter * kUnitWindows + 8 * wave + (lane >> 5)) * b_mult + b_off
                          : nullptr;
        }
        // three instructions per quotient where every lane of the wave has a proven divisor and dividends that are +0 or
        // in [kBandDivLo, kBandDivHi]; otherwise (tiny sums, +inf by overflow, other divisors) the wave divides
        DivGuard g;
        g.dividends(p[0], p[1]);
        g.dividends(p[2], p[3]);
        const int p_max = max(max((int)__float_as_uint(p[0]), (int)__float_as_uint(p[1])),
                              max((int)__float_as_uint(p[2]), (int)__float_as_uint(p[3])));
        if (__builtin_expect(__builtin_amdgcn_ballot_w64(g.lo < 2u * kBandDivLo - 1u || p_max > b_fast_hi) == 0, 1)) {
#pragma unroll
            for (int q = 0; q < 4; ++q) out[q] = div_c<true>(p[q], b_div, b_rcp);
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) out[q] = div_c<false>(p[q], b_div, b_rcp);
        }
#ifdef LBAD_EXP_TIMELINE
        STAMP(6);
        if (lane == 0) {
            float* o = frames + ((unit >> 2) * 128 + quarter * kUnitWindows + 8 * wave) * kBands;
            for (int i = 1; i < 7; ++i) o[i - 1] = (float)(ts[i] - ts[i - 1]);
            o[6] = (float)(ts[0] & 0xFFFFFF);
            o[7] = (float)__builtin_amdgcn_s_getreg(((16 - 1) << 11) | 4);
            o[8] = (float)(ts[0] >> 24 & 0xFFFFFF);
            o[9] = (float)(__builtin_amdgcn_s_memrealtime() - rt0);
        }
#endif
        if (next >= xcd_end) break;
        unit = next;
    }
#ifndef LBAD_EXP_TIMELINE
    store_out();
#endif
    if (claimer) claims_done(claim_ctr);
}

// ---- band sums in lanes ---------------------------------------------------------------------------------------------
// The default 44.1 kHz table has 15 live bands over bins 0..21, none wider than three bins, and the eight lanes of a window
// evaluate three bins each: dealt out as below, every band lies wholly inside one lane and its sum is two adds in
// registers.  Lane j of a window takes kLaneBin[j] (the two-bin lanes come last); the stage-6 row of bin k goes to
// transpose position 8 rd + j, where k is lane j's rd-th bin, so that every lane still reads positions j, j + 8, j + 16.
constexpr int kLaneBands = 15;
constexpr int kLaneBandLo[kLaneBands] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 12, 14, 17, 19};
constexpr int kLaneBandHi[kLaneBands] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 12, 14, 17, 19, 22};
constexpr int kLaneBin[8][3] = {{0, 1, 2}, {3, 4, 5}, {6, 7, 8}, {9, 10, 11}, {14, 15, 16}, {19, 20, 21}, {12, 13, -1}, {17, 18, -1}};
constexpr int kLanesFirstRow = 11;  // plan.d_bands: the per-task rows start at word kLanesFirstRow * 32 (rows_lanes_table)

constexpr int lanes_pos(int k) {    // transpose position of bin k
    for (int j = 0; j < 8; ++j)
        for (int rd = 0; rd < 3; ++rd)
            if (kLaneBin[j][rd] == k) return 8 * rd + j;
    return -1;
}
constexpr int lanes_band_of(int k) {
    for (int b = 0; b < kLaneBands; ++b)
        if (k >= kLaneBandLo[b] && k < kLaneBandHi[b]) return b;
    return -1;
}
// bit j: lane j's rd-th bin continues the band of the bin before it (which is then the bin k - 1: sums stay in bin order)
constexpr uint32_t lanes_cont_mask(int rd) {
    uint32_t m = 0;
    for (int j = 0; j < 8; ++j)
        if (kLaneBin[j][rd] >= 0 && kLaneBin[j][rd] == kLaneBin[j][rd - 1] + 1 &&
            lanes_band_of(kLaneBin[j][rd]) == lanes_band_of(kLaneBin[j][rd - 1]))
            m |= 1u << j;
    return m;
}
// the bins at positions 8 rd + j, j = 0..7, five bits each
constexpr uint64_t lanes_bin_pack(int rd) {
    uint64_t v = 0;
    for (int j = 0; j < 8; ++j) v |= (uint64_t)(kLaneBin[j][rd] >= 0 ? kLaneBin[j][rd] : 0) << (5 * j);
    return v;
}
constexpr bool lanes_table_ok() {
    for (int k = 0; k < kBins; ++k)
        if (lanes_pos(k) < 0 || lanes_pos(k) >= kBins || lanes_band_of(k) < 0) return false;
    for (int b = 0; b < kLaneBands; ++b) {      // a band's bins: one lane, consecutive tasks
        for (int k = kLaneBandLo[b] + 1; k < kLaneBandHi[b]; ++k)
            if (lanes_pos(k) != lanes_pos(k - 1) + 8) return false;
    }
    return lanes_pos(kBins - 1) == kBins - 1;   // what the tasks without a bin read
}
static_assert(lanes_table_ok(), "every bin has one position below 22 and every band lies in one lane, in bin order");

template <int I, int END>
__device__ __forceinline__ void store_rows_lanes(const cplx (&x)[64], float* trow) {
    if constexpr (I < END) {
        *(lds_vf32x2*)(trow + lanes_pos(I) * kRowDw) = stage6_row<I>(x);
        store_rows_lanes<I + 1, END>(x, trow);
    }
}
// held row I is the mirror of bin 21 - I: it goes where the bin's "+" row was
template <int I, int N>
__device__ __forceinline__ void store_held_lanes(const cplx (&h)[kRows - kRowsA], float* trow) {
    if constexpr (I < N) {
        *(lds_vf32x2*)(trow + lanes_pos(kBins - 1 - I) * kRowDw) = h[I];
        store_held_lanes<I + 1, N>(h, trow);
    }
}

// frame_rows_pruned_kernel up to and including the split pass; then a lane adds its own power terms.
//   t_i: the power term of the lane's i-th bin, +0.0 where it is NaN or +inf (the filter of k_fft_bands.hip; a term is a sum
//   of two squares, so -inf does not occur);  s0 = t0, s1 = (cont1 ? s0 : +0.0) + t1, s2 = (cont2 ? s1 : +0.0) + t2.
// This is the oracle's `p = 0; p += term` in bin order, bit for bit: a term is a sum of two squares, hence >= +0.0 and never
// -0.0, so 0 + t = t, p + 0 = p, and a skipped term equals an added +0.0.  A sum that ends a band is divided and stored; the
// per-task divisor, RN(1 / divisor), "proven" flag and the band's place in a row come from the plan (rows_lanes_table), a task
// that ends no band has the place 0xFFFFFFFF, divisor 1, and stores nothing.  The guard of const_div.hpp looks at all three
// sums of every lane (more than the stored ones: never less safe).  With full rows (the tap) the lanes also store the +0.0
// of the structurally empty bands, dealt out by the same table; compact rows have no such band.
template <int FMT>
__global__ __launch_bounds__(kThreads, kWgPerCu) void frame_rows_lanes_kernel(const void* __restrict__ pcm_raw,
                                                                        uint64_t samples_per_clip,
                                                                        uint32_t frames_per_clip, uint64_t n_units,
                                                                        uint64_t units_per_xcd,
                                                                        const float* __restrict__ bin_const,
                                                                        const uint32_t* __restrict__ band_tbl,
                                                                        uint32_t* __restrict__ claim_ctr,
                                                                        float* __restrict__ frames, uint32_t frame_dw,
                                                                        uint32_t row_dw, uint32_t place_row) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* span = smem;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    float* tbuf = smem + kSpanDw + wave * (8 * kWinDw);
    float* cbuf = smem + kSpanDw + kTDw;
    static_assert((kSpanDw + kTDw + kConstDw) % 2 == 0, "the slot behind the constants is 8-byte aligned");
    typedef __attribute__((address_space(3))) volatile uint64_t lds_vu64;
    lds_vu64* next_slot = (lds_vu64*)(cbuf + kConstDw);

    const uint32_t wg_per_xcd = gridDim.x >> 3;
    const uint64_t xcd_begin = (uint64_t)(blockIdx.x & 7) * units_per_xcd;     // units_per_xcd is a multiple of 4
    const uint64_t xcd_end = xcd_begin + units_per_xcd < n_units ? xcd_begin + units_per_xcd : n_units;
    uint64_t unit = xcd_begin + 4 * (uint64_t)(blockIdx.x >> 3);
    if (unit >= xcd_end) {
        if (threadIdx.x == 0) claims_done(claim_ctr);
        return;
    }

    auto span_start = [&](uint64_t u) {
        const uint32_t frame = (uint32_t)(u >> 2);          // the launcher keeps unit numbers below 2^31
        const uint32_t clip = frame / frames_per_clip;
        const uint32_t fi = frame - clip * frames_per_clip;
        return (uint64_t)clip * samples_per_clip + (uint64_t)(fi * 128 + (uint32_t)(u & 3) * kUnitWindows) * kStride;
    };
    claim_ctr_t* my_ctr = (claim_ctr_t*)(claim_ctr + (blockIdx.x & 7));
    asm volatile("" : "+v"(my_ctr));
    const bool claimer = threadIdx.x == 0;
    uint32_t claimed = 0;
    // the unit of claim 0, one scalar pair over the loop (the empty asm keeps it from being taken apart into two again)
    uint64_t claim_base = xcd_begin + 4 * (uint64_t)wg_per_xcd;
    asm volatile("" : "+s"(claim_base));

    span_to_lds<FMT>(pcm_raw, span_start(unit), span, wave, lane);
    // block p of the constants holds those of the bin at position p: a lane then picks the blocks j, j + 8, j + 16 as it picks the
    // rows, and both the fill and the picks touch LDS exactly as in frame_rows_pruned_kernel (a task without a bin evaluates bin
    // 21, whose row it reads)
    for (int i = threadIdx.x; i < kBins * kBinConst; i += kThreads) {
        const int p = i / kBinConst;
        constexpr uint64_t kBin0 = lanes_bin_pack(0), kBin1 = lanes_bin_pack(1), kBin2 = lanes_bin_pack(2);
        const int k = (int)(((p < 8 ? kBin0 : p < 16 ? kBin1 : kBin2) >> (5 * (p & 7))) & 31u);
        cbuf[p * kConstStride + (i % kBinConst)] = bin_const[k * kBinConst + (i % kBinConst)];
    }

    const int w8 = lane >> 3, r = lane & 7;
    const float inv_norm = 1.0f / (float)(kW / 4);
    // rr: the lane's place j among the eight of its window (the swap of round 5 stays, see frame_rows_pruned_kernel)
    const int rr = r ^ ((((w8 + 1) >> 1) & 1) << 2);
    int tk[3];      // transpose positions read, as before: j, j + 8, j + 16 (clamped to a valid row)
#pragma unroll
    for (int rd = 0; rd < 3; ++rd) tk[rd] = rr + 8 * rd < kBins ? rr + 8 * rd : kBins - 1;
    // LDS addresses of the rows a lane's trees read: tasks 0 and 1 are always eight rows apart (rr + 8 < kBins)
    const uint32_t row01 = lds_addr(tbuf + w8 * kWinDw + tk[0] * kRowDw), row2 = lds_addr(tbuf + w8 * kWinDw + tk[2] * kRowDw);

    // per-task constants: divisor, RN(1 / divisor), place in a row; one "proven" word per lane
    const uint32_t* task_tbl = band_tbl + kLanesFirstRow * kBands;
    float t_div[3], t_rcp[3];
    uint32_t t_off = 0, z_off = 0;      // three places of a row, eight bits each (0xFF: none): band means, empty bands
    bool proven = true;
#pragma unroll
    for (int rd = 0; rd < 3; ++rd) {
        t_div[rd] = __uint_as_float(task_tbl[8 * rd + rr]);
        t_rcp[rd] = __uint_as_float(task_tbl[kBands + 8 * rd + rr]);
        proven = proven && task_tbl[2 * kBands + 8 * rd + rr] != 0u;
        t_off |= (task_tbl[place_row * kBands + 8 * rd + rr] & 0xFFu) << (8 * rd);
        z_off |= (task_tbl[5 * kBands + 8 * rd + rr] & 0xFFu) << (8 * rd);
    }
    const int t_fast_hi = proven ? (int)kBandDivHi : -1;   // compared as bit patterns
    constexpr uint32_t kCont1 = lanes_cont_mask(1), kCont2 = lanes_cont_mask(2);
    const uint32_t m_cont1 = (kCont1 >> rr) & 1u ? 0xFFFFFFFFu : 0u;
    const uint32_t m_cont2 = (kCont2 >> rr) & 1u ? 0xFFFFFFFFu : 0u;
    const bool is_dc = rr == 0;                   // the lane whose first bin is bin 0

    __syncthreads();
    TreeTw twp[3], twm[3];
    f32x2 ws[3];
#pragma unroll
    for (int rd = 0; rd < 3; ++rd) {
        const float* c = cbuf + tk[rd] * kConstStride;
        twp[rd] = tree_twiddles(c);
        twm[rd] = tree_twiddles(c + 6);
        ws[rd] = *reinterpret_cast<const f32x2*>(c + 12);
    }

    float out[3] = {0.0f, 0.0f, 0.0f};   // band means of the previous quarter frame, stored one iteration late
    float* out_row = nullptr;
#ifdef LBAD_EXP_TIMELINE
    long long ts[8];
#define STAMP(i) ts[i] = __builtin_readcyclecounter()
#else
#define STAMP(i)
#endif
    // the places are unpacked at every store (the empty asm hides that they never change): six loop-invariant lane masks are
    // more than the scalar file has left, they were spilled to vector lanes
    auto store_out = [&]() {
        if (!out_row) return;
        uint32_t places = t_off;
        asm volatile("" : "+v"(places));
#pragma unroll
        for (int rd = 0; rd < 3; ++rd) {
            const uint32_t o = (places >> (8 * rd)) & 0xFFu;
            if (o != 0xFFu) out_row[o] = out[rd];
        }
        uint32_t layout = place_row;                // (likewise: no 64-bit mask of "full rows" kept over the loop)
        asm volatile("" : "+s"(layout));
        if (layout == 3u) {                         // full rows
            places = z_off;
            asm volatile("" : "+v"(places));
#pragma unroll
            for (int rd = 0; rd < 3; ++rd) {
                const uint32_t o = (places >> (8 * rd)) & 0xFFu;
                if (o != 0xFFu) out_row[o] = 0.0f;
            }
        }
    };
    for (;;) {
        STAMP(0);
#ifdef LBAD_EXP_TIMELINE
        const unsigned long long rt0 = __builtin_amdgcn_s_memrealtime();
#endif
        // ---- A: this quarter frame's span has landed (own loads: vmcnt, the other waves': barrier) ----
        __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0)
        const uint32_t quarter = (uint32_t)(unit & 3);
        // (claimed three iterations ago; the slot holds the unit the claim stands for, 64 bits as every unit number)
        if (quarter == 3 && claimer) *next_slot = claim_base + 4 * (uint64_t)claimed;
        __syncthreads();
        STAMP(1);

        // ---- B1: 64 points of this lane; once every wave has its points the span buffer is free -------
        cplx x[64];
        load_points<0>(x, span + 80 * (8 * wave + w8) + 2 * r);
        const uint64_t next = quarter == 3 ? *next_slot : unit + 1;
        __syncthreads();
        if (next < xcd_end) span_to_lds<FMT>(pcm_raw, span_start(next), span, wave, lane);
        if (quarter == 0 && claimer) claimed = __hip_atomic_fetch_add(my_ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#ifndef LBAD_EXP_TIMELINE
        store_out();
#endif
        STAMP(2);

        // ---- B2: DIT stages 1..5 in registers ---------------------------------------------------------
        __builtin_amdgcn_s_setprio(0);
        stage_blocks<1, 0>(x);
        stage_blocks<2, 0>(x);
        stage_blocks<3, 0>(x);
        stage_blocks<4, 0>(x);
        stage_blocks<5, 0>(x);
        STAMP(3);
        __builtin_amdgcn_s_setprio(3);

        // ---- B3/B4: stage 6, the "+" rows to their positions; the mirror rows wait in registers ------
        store_rows_lanes<0, kRowsA>(x, tbuf + w8 * kWinDw + 2 * r);
        cplx held[kRows - kRowsA];
        hold_rows<kRowsA, kRows, kRowsA>(x, held);
        cplx za[3];
        {
            TreeIn in[3];
            in[0] = tree_load(row01);
            in[1] = tree_load<4 * 8 * kRowDw>(row01);
            in[2] = tree_load(row2);
            // pass 2: the mirror row of a bin takes the bin's position (bin 0 has none: its position keeps the stale "+" row,
            // whose tree is dropped below)
            store_held_lanes<0, kRows - kRowsA>(held, tbuf + w8 * kWinDw + 2 * r);
            lds_wait<kPass1Wait>(in);
#pragma unroll
            for (int rd = 0; rd < 3; ++rd) za[rd] = tree_eval(in[rd], twp[rd]);
        }
        STAMP(4);
        float pw[3];
        {
            TreeIn in[3];
            in[0] = tree_load(row01);
            in[1] = tree_load<4 * 8 * kRowDw>(row01);
            in[2] = tree_load(row2);
#pragma unroll
            for (int rd = 0; rd < 3; ++rd) {
                if (rd == 0) lds_wait<8>(in[0]);        // four reads per round: two, one, no round behind this one
                else if (rd == 1) lds_wait<4>(in[1]);
                else lds_wait<0>(in[2]);
                const cplx b = tree_eval(in[rd], twm[rd]);
                const cplx a = za[rd];
                float re, im;
                if (rd == 0 && is_dc) {
                    const float sm = a.x + a.y, df = a.x - a.y;
                    re = sm + sm;
                    im = df + df;
                } else {
                    const float sr = a.x + b.x, si = a.y - b.y;
                    const float dr = a.x - b.x, di = a.y + b.y;
                    const float wr = ws[rd].x, wi = ws[rd].y;
                    re = __fmaf_rn(wr, di, __fmaf_rn(wi, dr, sr));
                    im = __fmaf_rn(-wr, dr, __fmaf_rn(wi, di, si));
                }
                if (re > 0.0f) re = __fmul_rn(re, inv_norm);
                if (im > 0.0f) im = __fmul_rn(im, inv_norm);
                pw[rd] = __fadd_rn(__fmul_rn(re, re), __fmul_rn(im, im));
            }
        }
        STAMP(5);

        // ---- B5: band sums in registers, in bin order ------------------------------------------------------------------
        float s[3];
#pragma unroll
        for (int rd = 0; rd < 3; ++rd) s[rd] = pw[rd] < INFINITY ? pw[rd] : 0.0f;     // NaN and +inf are skipped
        s[1] = __fadd_rn(__uint_as_float(__float_as_uint(s[0]) & m_cont1), s[1]);
        s[2] = __fadd_rn(__uint_as_float(__float_as_uint(s[1]) & m_cont2), s[2]);
        DivGuard g;
        g.dividends(s[0], s[1]);
        g.dividends(s[2], s[2]);
        const int s_max = max(max((int)__float_as_uint(s[0]), (int)__float_as_uint(s[1])), (int)__float_as_uint(s[2]));
        if (__builtin_expect(__builtin_amdgcn_ballot_w64(g.lo < 2u * kBandDivLo - 1u || s_max > t_fast_hi) == 0, 1)) {
#pragma unroll
            for (int rd = 0; rd < 3; ++rd) out[rd] = div_c<true>(s[rd], t_div[rd], t_rcp[rd]);
        } else {
#pragma unroll
            for (int rd = 0; rd < 3; ++rd) out[rd] = div_c<false>(s[rd], t_div[rd], t_rcp[rd]);
        }
        // row = quarter * 32 + 8 * wave + window of the wave
        out_row = frames + (unit >> 2) * frame_dw + (quarter * kUnitWindows + 8 * wave + w8) * row_dw;
#ifdef LBAD_EXP_TIMELINE
        asm volatile("" ::"v"(out[0]), "v"(out[1]), "v"(out[2]));   // nothing stores the means in this build: keep their work
        STAMP(6);
        if (lane == 0) {
            float* o = frames + ((unit >> 2) * 128 + quarter * kUnitWindows + 8 * wave) * kBands;
            for (int i = 1; i < 7; ++i) o[i - 1] = (float)(ts[i] - ts[i - 1]);
            o[6] = (float)(ts[0] & 0xFFFFFF);
            o[7] = (float)__builtin_amdgcn_s_getreg(((16 - 1) << 11) | 4);
            o[8] = (float)(ts[0] >> 24 & 0xFFFFFF);
            o[9] = (float)(__builtin_amdgcn_s_memrealtime() - rt0);
        }
#endif
        if (next >= xcd_end) break;
        unit = next;
    }
#ifndef LBAD_EXP_TIMELINE
    store_out();
#endif
    if (claimer) claims_done(claim_ctr);
}
#undef STAMP

}  // namespace

bool rows_pruned_supported(const Plan& p) {
    if (p.window != (uint32_t)kW || p.stride != (uint32_t)kStride || p.bands != (uint32_t)kBands) return false;
    if (p.table.kmax > (uint32_t)kBins) return false;
    // the compile-time W_64 table must be bit-identical to the run-time master table
    std::vector<float> re, im;
    make_twiddles(kW, re, im);
    for (int t = 0; t < 32; ++t)
        if (re[16 * t] != kTw64Re[t] || im[16 * t] != kTw64Im[t]) return false;
    return true;
}

// per-bin twiddle block (see kBinConst)
void rows_pruned_constants(std::vector<float>& out) {
    std::vector<float> re, im;
    make_twiddles(kW, re, im);
    out.assign((size_t)kClaimOffset + kClaimWords, 0.0f);   // constants, padding, claim counters and ticket (zero between launches)
    for (int k = 0; k < kBins; ++k) {
        float* c = &out[(size_t)k * kBinConst];
        // "+" tree of Z[k]: W_128^k, W_256^k, W_512^k
        c[0] = re[8 * k]; c[1] = im[8 * k];
        c[2] = re[4 * k]; c[3] = im[4 * k];
        c[4] = re[2 * k]; c[5] = im[2 * k];
        if (k > 0) {
            // mirror tree of Z[512 - k]: exponents 128 - k, 256 - k, 512 - k all lie in the upper half of
            // their stage, i.e. the "u - w v" output: w' = -W^(e - m/2)
            c[6] = -re[8 * (64 - k)];   c[7] = -im[8 * (64 - k)];
            c[8] = -re[4 * (128 - k)];  c[9] = -im[4 * (128 - k)];
            c[10] = -re[2 * (256 - k)]; c[11] = -im[2 * (256 - k)];
            c[12] = re[k]; c[13] = im[k];   // W_1024^k of the split pass
        }
    }
}

// the band table's part of rows_lanes_supported: 32 bands whose non-empty ones are exactly the compiled table's, and empty
// bands whose mean is +0.0 (a zero divisor would make it NaN)
static bool lanes_bands_match(const Plan& p) {
    if (p.window != (uint32_t)kW || p.bands != (uint32_t)kBands || p.table.lo.size() != (size_t)kBands ||
        p.table.indices.size() != (size_t)kBands + 1)
        return false;
    int n = 0;
    for (int b = 0; b < kBands; ++b) {
        if (p.table.lo[b] >= p.table.hi[b]) {
            if (p.table.indices[b + 1] == p.table.indices[b]) return false;
            continue;
        }
        if (n == kLaneBands || p.table.lo[b] != (uint32_t)kLaneBandLo[n] || p.table.hi[b] != (uint32_t)kLaneBandHi[n]) return false;
        ++n;
    }
    return n == kLaneBands;
}

bool rows_lanes_supported(const Plan& p) { return rows_pruned_supported(p) && lanes_bands_match(p); }

// Six rows of 32 words behind the eleven of the band table, indexed by task 8 rd + j (lane j's rd-th bin): the divisor of the
// bin's band, RN(1 / divisor), whether the short division is proven for it, the band's word inside a full row and inside a
// compact row of plan.sparse (0xFFFFFFFF: the task does not end a band, or the band is not stored), and, by the same index, the
// words of a full row that belong to structurally empty bands (0xFFFFFFFF: none), which the lanes set to +0.0.
void rows_lanes_table(const Plan& p, std::vector<uint32_t>& tbl) {
    if (!lanes_bands_match(p)) return;
    tbl.resize((size_t)(kLanesFirstRow + 6) * kBands, 0u);
    uint32_t* t = &tbl[(size_t)kLanesFirstRow * kBands];
    const float one = 1.0f;
    for (int i = 0; i < kBands; ++i) {
        std::memcpy(&t[i], &one, 4);
        std::memcpy(&t[kBands + i], &one, 4);
        t[2 * kBands + i] = 1u;
        t[3 * kBands + i] = t[4 * kBands + i] = t[5 * kBands + i] = 0xFFFFFFFFu;
    }
    int empty = 0;
    for (uint32_t b = 0; b < (uint32_t)kBands; ++b) {
        if (p.table.lo[b] >= p.table.hi[b]) {           // dealt out over the 24 task slots: 17 empty bands at most three a lane
            if (empty < 24) t[5 * kBands + empty] = b;
            ++empty;
            continue;
        }
        const float div = (float)(p.table.indices[b + 1] - p.table.indices[b]);
        const float rcp = 1.0f / div;
        for (uint32_t k = p.table.lo[b]; k < p.table.hi[b]; ++k) {
            const int at = lanes_pos((int)k);
            std::memcpy(&t[at], &div, 4);
            std::memcpy(&t[kBands + at], &rcp, 4);
            t[2 * kBands + at] = band_div_proven(div) ? 1u : 0u;
            if (k + 1 != p.table.hi[b]) continue;       // the band's last bin: its task holds the whole sum
            t[3 * kBands + at] = b;
            if (p.sparse.ok) {
                const uint32_t pos = b >= 16 ? p.sparse.pos_right[b - 16] : (b == p.sparse.left ? p.sparse.pos_left : 0xFFu);
                if (pos != 0xFFu) t[4 * kBands + at] = pos;
            }
        }
    }
}

template <int FMT>
static hipError_t launch_rows_fmt(const Plan& plan, const float* d_bin_const, const void* d_pcm, uint64_t n_frames,
                                  uint64_t samples_per_clip, uint32_t frames_per_clip, float* d_frames,
                                  hipStream_t stream, bool compact, bool lanes) {
    static PerDevice attr, attr_lanes;
    if (!lanes && attr.changed(kLdsBytes)) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(frame_rows_pruned_kernel<FMT>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes);
        if (e != hipSuccess) return e;
    }
    if (lanes && attr_lanes.changed(kLdsBytes)) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(frame_rows_lanes_kernel<FMT>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes);
        if (e != hipSuccess) return e;
    }
    // work is claimed by frames: every XCD's range is a whole number of frames
    const uint64_t n_units = n_frames * 4, units_per_xcd = 4 * ((n_frames + 7) / 8);
    const int n_cu = device_cu_count();
    // every CU holds kWgPerCu persistent workgroups; a multiple of 8 so that each XCD gets the same number
    uint64_t wg_per_xcd = ((uint64_t)n_cu * kWgPerCu + 7) / 8;
    if (wg_per_xcd > units_per_xcd / 4) wg_per_xcd = units_per_xcd / 4;
    uint32_t* claim = reinterpret_cast<uint32_t*>(const_cast<float*>(d_bin_const)) + kClaimOffset;
    if (lanes)
        hipLaunchKernelGGL(frame_rows_lanes_kernel<FMT>, dim3((uint32_t)(wg_per_xcd * 8)), dim3(kThreads), kLdsBytes,
                           stream, d_pcm, samples_per_clip, frames_per_clip, n_units, units_per_xcd, d_bin_const,
                           plan.d_bands, claim, d_frames, compact ? plan.sparse.frame_dw() : 128u * kBands,
                           compact ? plan.sparse.n_stored : (uint32_t)kBands, compact ? 4u : 3u);
    else
        hipLaunchKernelGGL(frame_rows_pruned_kernel<FMT>, dim3((uint32_t)(wg_per_xcd * 8)), dim3(kThreads), kLdsBytes,
                           stream, d_pcm, samples_per_clip, frames_per_clip, n_units, units_per_xcd, d_bin_const,
                           plan.d_bands, claim, d_frames, compact ? plan.sparse.frame_dw() : 128u * kBands, compact ? 5u : 3u);
    return hipGetLastError();
}

// band_form: 0 the band sums in lanes where the plan allows (rows_lanes_supported), 1 through LDS, 2 in lanes or an error
hipError_t launch_rows_pruned(const Plan& plan, const float* d_bin_const, const void* d_pcm, uint32_t fmt,
                              uint64_t n_clips, uint64_t samples_per_clip, uint32_t frames_per_clip, float* d_frames,
                              hipStream_t stream, bool compact, uint32_t band_form) {
    if (compact && !plan.sparse.ok) return hipErrorInvalidValue;
    if (band_form > 2 || (band_form == 2 && !plan.lanes_ok)) return hipErrorInvalidValue;
    const bool lanes = band_form != 1 && plan.lanes_ok;
    const uint64_t n_frames = n_clips * frames_per_clip;
    if (n_frames == 0) return hipSuccess;
    if (n_frames > 0x7fffffffull) return hipErrorInvalidValue;
    if (n_frames * 4 + 8 > 0x7fffffffull) return hipErrorInvalidValue;
    switch (fmt) {
        case 0: return launch_rows_fmt<0>(plan, d_bin_const, d_pcm, n_frames, samples_per_clip, frames_per_clip, d_frames, stream, compact, lanes);
        case 1: return launch_rows_fmt<1>(plan, d_bin_const, d_pcm, n_frames, samples_per_clip, frames_per_clip, d_frames, stream, compact, lanes);
        case 2: return launch_rows_fmt<2>(plan, d_bin_const, d_pcm, n_frames, samples_per_clip, frames_per_clip, d_frames, stream, compact, lanes);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace lbad
