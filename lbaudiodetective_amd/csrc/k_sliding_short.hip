// k_sliding_short.hip -- the two SYSTOLIC scans of a ragged corpus (the records rest in the lanes, the partial sums of a
// sliding offset travel): compare_short_kernel for short queries, corpora of short entries and the short entries of a split
// scan, compare_short_multi_kernel for batches of short queries.  When a launch takes which: sliding.cpp (sliding_choose); the
// task scan of everything else: k_sliding.hip.
#include "sliding_common.hpp"

#include <type_traits>

namespace lbad {
namespace {

#ifdef LBAD_SLIDE_STAMPS
// per wave of compare_short_multi_kernel: start, first chunk done, chunk 17, end (100 MHz stamps; tools/exp/short_multi_stamps.py)
__device__ unsigned long long g_short_times[1024 * 16 * 8];
#endif

// ---- short queries (up to 7 sub-fingerprints): the round-3 systolic scan --------------------------------------------
// A lane holds ONE record (two aligned, fully coalesced dwordx4 per lane: every record is read once, 16 cache lines per
// wave instruction -- the task kernel above reads a lane's four-record window from 64 different lines and is bound by
// the texture path when the steps are few), the query's sub-fingerprints a = 0, 1, ... are wave-uniform, and an
// accumulator per sliding offset travels one lane to the right per step (`v_add_f32 ... wave_shr:1`).  Every (query,
// record) pair is evaluated, also on the diagonals that leave their entry -- with a query of q against entries of n
// that is (q - 1) / n of the work, a tenth at q = 5 -- and the scan is HBM-bound.  Chunks of 64 records overlap by
// min(n_query, longest entry) - 1.  The place of a record inside its entry comes from the record (w3 / w7, see
// sliding_common.hpp): no side table, no search.
//   entry longer than the query ("A" lanes): a diagonal starts in step 0 in every lane and is complete after the last
//     step; it is an offset of the entry iff it stayed inside the entry (i >= n_query - 1).
//   entry not longer than the query ("B" lanes): a diagonal starts whenever it enters the entry's first lane (i == 0) and
//     is complete when it leaves the last one (r == 0); that lane keeps the maximum over the steps.
// Diagonals that did not start properly carry -inf.
struct Rec {
    uint32_t P[4], N[4];
    uint32_t isat, rem, idx;
};

__device__ __forceinline__ Rec unpack_rec(const uint4 a, const uint4 b) {
    Rec r;
    r.P[0] = a.x; r.P[1] = a.y; r.P[2] = a.z; r.P[3] = a.w & 0xFu;
    r.N[0] = b.x; r.N[1] = b.y; r.N[2] = b.z; r.N[3] = b.w & 0xFu;
    r.isat = (a.w >> 21) & 0xFu;
    r.rem = (a.w >> 25) & 0xFu;
    r.idx = (b.w >> 4) | ((a.w >> 17) & 0xFu) << 28;
    return r;
}

constexpr int kNegInf = (int)0xFF800000u;   // -inf; as a signed integer it sorts below the bits of every sum >= 0

// One chunk = 64 K consecutive records; lane l holds records K l .. K l + K - 1, so a diagonal moves from register
// set k - 1 to set k inside the lane and crosses to the next lane only from set K - 1 to set 0.
// MODE 0: every entry in the chunk is longer than the query; 1: none is; 2: mixed.
// QN queries of one length (round 5): step a of ALL queries before step a + 1 -- their sums travel side by side, a query's
// chain of dependent adds and look-ups is covered by the others' bit operations (query qi at q + qi q_stride).
template <int K, int MODE, int QN>
__device__ __forceinline__ void short_steps(const uint32_t (&P)[K][4], const uint32_t (&N)[K][4], const uint32_t (&nz)[K][4],
                                          const uint32_t (&tri)[K], const bool (&case_a)[K], const bool (&start_b)[K],
                                          const uint32_t* __restrict__ q, uint32_t q_stride, uint32_t nq, const float* s_tri,
                                          float (&acc)[QN][K], int (&smax)[QN][K]) {
    // MODE 2: the mask of a cell is the entry's NZ in A lanes and the query's in B lanes:
    //   m = sel_e & (nz_q | sel_a)   with sel_e = A ? nz_e : ~0,  sel_a = A ? ~0 : 0     (one v_bitop3)
    uint32_t sel_e[K][4], sel_a[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
#pragma unroll
        for (int qi = 0; qi < QN; ++qi) {
            acc[qi][k] = MODE == 0 ? 0.0f : __int_as_float(kNegInf);   // MODE 0: step 0 adds to the zeros, no reset needed
            smax[qi][k] = kNegInf;
        }
        sel_a[k] = case_a[k] ? 0xFFFFFFFFu : 0u;
#pragma unroll
        for (int w = 0; w < 4; ++w) sel_e[k][w] = case_a[k] ? nz[k][w] : 0xFFFFFFFFu;
    }
    for (uint32_t a = 0; a < nq; ++a) {
#pragma unroll
        for (int qi = 0; qi < QN; ++qi) {
            const uint32_t* __restrict__ qa = q + (size_t)qi * q_stride + (size_t)a * kQWords;
            uint32_t nzq[4] = {0, 0, 0, 0}, triq = 0;
            if (MODE != 0) {
                // the query's mask and table row in vector registers, once per step for the K cells (a VALU
                // instruction reads one scalar operand only)
#pragma unroll
                for (int w = 0; w < 4; ++w) asm("v_mov_b32 %0, %1" : "=v"(nzq[w]) : "s"(qa[8 + w]));
                asm("v_mov_b32 %0, %1" : "=v"(triq) : "s"(qa[12]));
            }
            float ratio[K];
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const uint32_t h0 = MODE == 0 ? tri[k] : MODE == 1 ? triq : (case_a[k] ? tri[k] : triq);
                uint32_t h = 0;
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    // a & ~(b ^ c), twice: two v_bitop3_b32 per word (left to itself the compiler builds xor, xor, bitop3)
                    uint32_t m = MODE == 0 ? nz[k][w] : nzq[w];
                    if (MODE == 2) m = __builtin_amdgcn_bitop3_b32(sel_e[k][w], nzq[w], sel_a[k], 0xE0);   // a & (b | c)
                    const uint32_t u = __builtin_amdgcn_bitop3_b32(m, P[k][w], qa[w], 0x90);
                    const uint32_t v = __builtin_amdgcn_bitop3_b32(u, N[k][w], qa[4 + w], 0x90);
                    // h += popc(v) as ONE accumulating v_bcnt (the compiler distributes the table's * 4 over the sum)
                    if (w == 0) asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(h) : "v"(v), "v"(h0));   // starts at the table row
                    else asm("v_bcnt_u32_b32 %0, %1, %0" : "+v"(h) : "v"(v));
                }
                ratio[k] = s_tri[h];
            }
            const float in0 = __uint_as_float(from_left_lane(__float_as_uint(acc[qi][K - 1])));
#pragma unroll
            for (int k = K - 1; k >= 0; --k) {
                float sh = k ? acc[qi][k - 1] : in0;
                if (MODE == 1) sh = start_b[k] ? 0.0f : sh;
                if (MODE == 2) sh = (start_b[k] || (a == 0 && case_a[k])) ? 0.0f : sh;
                acc[qi][k] = __fadd_rn(sh, ratio[k]);
                if (MODE != 0) smax[qi][k] = max(smax[qi][k], __float_as_int(acc[qi][k]));
            }
        }
    }
}

// QN queries of one length per launch (round 5): a chunk's records are fetched and unpacked once, the steps run per query
// (q: QN blocks of (nq + 1) kQWords words).
template <int K, int QN>
__global__ __launch_bounds__(kSlThreads, (K == 4 && QN == 1) ? 4 : 1) void compare_short_kernel(     // (four waves per SIMD: 128 registers, as round 4's)
    const uint4* __restrict__ recs, uint64_t n_pos, const uint32_t* __restrict__ q, uint32_t nq, uint32_t chunk_step,
    uint64_t n_chunks, uint4 range_mask, const float* __restrict__ tri_tbl, uint64_t index_base,
    unsigned int* __restrict__ score_bits, const ScanOut out, uint32_t only_upto) {
    // only_upto (0: every entry): the scan of a corpus that is split between the two kernels -- only entries of at most
    // this many sub-fingerprints are scored here (the task kernel has the others), chunks without one are passed over
    __shared__ float s_tri[kTriSize];
    __shared__ unsigned long long s_k[kSlThreads / 64][QN];
    for (uint32_t i = threadIdx.x; i < kTriSize; i += kSlThreads) s_tri[i] = tri_tbl[i];
    __syncthreads();

    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = (uint64_t)blockIdx.x * (kSlThreads / 64) + (threadIdx.x >> 6);
    const uint64_t n_waves = (uint64_t)gridDim.x * (kSlThreads / 64);
    const uint32_t rm[4] = {range_mask.x, range_mask.y, range_mask.z, range_mask.w};
    unsigned long long best[QN];
#pragma unroll
    for (int qi = 0; qi < QN; ++qi) best[qi] = 0ull;
    const uint32_t q_stride = (nq + 1u) * kQWords;

    for (uint64_t c = wave; c < n_chunks; c += n_waves) {
        const uint64_t p0 = c * chunk_step + (uint64_t)lane * K;
        uint32_t P[K][4], N[K][4], nz[K][4], tri[K], isat[K], rem[K], idx[K], n2[K];
        bool case_a[K], start_b[K], inb[K];
        bool some_a = false, some_b = false;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            inb[k] = p0 + k < n_pos;
            uint4 ra = make_uint4(0, 0, 0, 0), rb = make_uint4(0, 0, 0, 0);
            if (inb[k]) {
                ra = recs[2 * (p0 + k)];
                rb = recs[2 * (p0 + k) + 1];
            }
            const Rec r = unpack_rec(ra, rb);
            uint32_t possible = 0;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                P[k][w] = r.P[w];
                N[k][w] = r.N[w];
                nz[k][w] = (r.P[w] | r.N[w]) & rm[w];
                possible += __popc(nz[k][w]);
            }
            tri[k] = possible * (possible + 1u) / 2u;
            isat[k] = r.isat; rem[k] = r.rem; idx[k] = r.idx;
            const uint32_t ne = r.isat + r.rem + 1u;       // saturated (both fields at 15); exact whenever it is <= 16
            case_a[k] = ne > nq;                           // the entry is the longer side (Fp.m:123-131)
            n2[k] = case_a[k] ? nq : ne;
            start_b[k] = !case_a[k] && r.isat == 0u;
            if (only_upto && ne > only_upto) inb[k] = false;   // (not this scan's entry: its lanes never score)
            some_a |= case_a[k] && inb[k];
            some_b |= !case_a[k] && inb[k];
        }
        const bool any_a = __ballot(some_a) != 0ull, any_b = __ballot(some_b) != 0ull;
        if (only_upto && !any_a && !any_b) continue;       // (uniform)

        float acc[QN][K];
        int smax[QN][K];
        if (!any_b) short_steps<K, 0, QN>(P, N, nz, tri, case_a, start_b, q, q_stride, nq, s_tri, acc, smax);
        else if (!any_a) short_steps<K, 1, QN>(P, N, nz, tri, case_a, start_b, q, q_stride, nq, s_tri, acc, smax);
        else short_steps<K, 2, QN>(P, N, nz, tri, case_a, start_b, q, q_stride, nq, s_tri, acc, smax);
#pragma unroll
        for (int qi = 0; qi < QN; ++qi) {

            // a record closes a window iff the window lies inside its entry AND inside this chunk.  The exact
            // division (Fp.m:144) runs only where the sum can reach the lane's best so far.
            const float thr = __uint_as_float((uint32_t)(best[qi] >> 32)) * 0.99999f;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const bool closes = case_a[k] ? (isat[k] >= nq - 1u) : (rem[k] == 0u);
                const bool valid = inb[k] && closes && lane * K + k >= n2[k] - 1u;
                const float s = case_a[k] ? acc[qi][k] : __int_as_float(smax[qi][k]);
                const float n2f = (float)n2[k];
                const bool need = valid && ((QN == 1 && score_bits != nullptr) || s >= thr * n2f);
                if (__ballot(need) != 0ull) {
                    if (need) {
                        const float cand = __fdiv_rn(s, n2f);
                        const float match = (0.0f < cand) ? cand : 0.0f;     // MAX(match, cand) from match = 0
                        if (QN == 1 && score_bits) atomicMax(&score_bits[idx[k]], __float_as_uint(match));
                        const unsigned long long key = sl_key(match, index_base + idx[k]);
                        best[qi] = key > best[qi] ? key : best[qi];
                    }
                }
            }
        }
    }
#pragma unroll
    for (int qi = 0; qi < QN; ++qi) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned long long o = __shfl_xor(best[qi], off, 64);
            best[qi] = o > best[qi] ? o : best[qi];
        }
        if (lane == 0) s_k[threadIdx.x >> 6][qi] = best[qi];
    }
    __syncthreads();
    // The keys are max-ed in place (the host clears them in front of the launch): this scan runs six workgroups per CU,
    // and a ticket on top of the maximum -- two contended atomics and two fences for each of 1536 workgroups -- cost a
    // fifth of the HBM-bound scan's time (0.261 -> 0.309 ms at a query of 5) where the memset node costs 5 us.
    if (threadIdx.x == 0) {
        for (int qi = 0; qi < QN; ++qi) {
            unsigned long long m = s_k[0][qi];
            for (int i = 1; i < kSlThreads / 64; ++i) m = s_k[i][qi] > m ? s_k[i][qi] : m;
            if (m) atomicMax(&out.keys[out.pos[qi]], m);
        }
    }
}

// ---- round 6: SEVERAL short queries per launch ----------------------------------------------------------------------------
// compare_short_kernel<1, 8> above spent 22 vector instructions per (record, query sub-fingerprint) pair at 4 cycles each:
// every v_bitop3 took a query word as its SCALAR operand, one v_mov_dpp per pair moved the partial sum to the next lane, the
// division branch of the epilogue was taken by every chunk (a lane's own best is beaten by one of its next four windows
// with probability 1 / chunks seen, and one lane of 64 is enough), and the 40 table look-ups per record met on the LDS
// banks (63 % of the LDS cycles).  This kernel keeps the systolic idea (the records rest, the partial sums of a diagonal
// travel) and changes what surrounds it:
//   * FOUR records per lane (a chunk = 256 records per wave): a diagonal crosses a lane boundary once per four pairs;
//   * the query words of step a come from LDS as two broadcast ds_read_b128 per (query, step) into VECTOR registers and
//     serve the lane's four records;
//   * NO v_bitop3 READS THREE REGISTERS OF ONE BANK.  tools/ubench/operand_rates.hip (profiles/r06_operand_rates.txt): a
//     wave64 v_bitop3 / v_fma_f32 issues in 2 cycles unless all three sources lie on one of the four register banks
//     (register number mod 4), then in 4 -- and a compiler that puts every 16-byte load into a 4-aligned quad makes
//     (P[w], N[w], qP[w]) exactly such a triple (25 of the 32 bit operations of a step in the first build).  The record
//     words are used where the loads put them (register base even + w: the tuples of gfx950 are even-aligned) and the
//     query quads are stored ROTATED by one word (word w in register base + (w + 1 & 3)): a query word's bank differs in
//     parity from the bank of the record words it meets, whatever the allocator does;
//   * the records are not unpacked: the query words are cut to the RANGE instead (a pair outside it -- and every field
//     bit of w3 / w7 -- meets query Booleans 0 0 and can only "match" where the record's pair is 0 0 as well, which is no
//     hit); the mask of a pair is folded into the first bit operation (0xA4: (P | N) & ~(P ^ qP));
//   * one query after the other (their sums are independent): four running sums per lane, whatever the number of queries;
//   * only entries LONGER than the query are scored here ("A" lanes: a diagonal starts in step 0 in every lane and is an
//     offset of its entry iff it stayed inside it); the host sends the entries of at most n_query sub-fingerprints, where the
//     corpus has any, through compare_short_kernel in its only_upto mode (same keys, atomic maxima);
//   * RATIO = hits / possible without the table: with pf = (float)possible, rh = RN(1 / pf) and
//     rl = RN(fma(-pf, rh, 1) * rh), fma(hf, rh, RN(hf * rl)) IS the correctly rounded quotient for every
//     0 <= hits <= possible <= 100 (tools/verify_ratio_fma.c checks all 5151 pairs against the IEEE division with the very
//     operations used here); possible == 0 gives rh = rl = 0 -> +0.0 like the table's row 0.  (rh, rl) of the 101 values
//     of `possible` sit in LDS; hits are counted on top of the bits of 2^23, so hf is one subtraction;
//   * the exact division of the epilogue runs where a sum can reach the WAVE's best so far (a wave-uniform threshold,
//     refreshed where the branch is taken: about ln(chunks) times per wave and query instead of every time).
//   * the LAST FOUR PAIRS (96..99: a word of their own in either plane, two bit operations and a count for 4 % of the pairs)
//     come from LDS instead: per (query, step) a table of the 256 tails a record can have (its four P and four N Booleans)
//     holds 2^23's bits + the tail's hits -- the value the three remaining counts start from; the query length is a
//     template argument, so table and query words are read at immediate offsets (14.5 instead of 16.5 vector
//     instructions per pair; the look-ups meet on the banks, but nothing else uses the LDS here);
//   * ONE workgroup of sixteen waves per CU owns a contiguous run of chunks and its waves CLAIM them from a cursor in LDS.
//     With equal static shares the waves did not finish together: the SIMD serves its oldest wave first, the workgroups
//     placed first ended at 0.51 ms, the last at 1.09 (tools/exp/short_multi_stamps.py), and a SIMD's last wave, alone,
//     issues at a fraction of the rate four waves reach together -- the vector ALU idled 60 % of the scan.
#ifndef LBAD_SHORT_MULTI_MAX
#define LBAD_SHORT_MULTI_MAX 12
#endif
// longest query of a BATCH this kernel takes (instantiated for 1..12; the records' place fields reach 15).  Crossover re-measured in round 6,
// eight queries against 1 M entries of 20..70: 1.00 / 1.05 / 1.14 / 1.36 ms at 8 / 9 / 10 / 12 here, 1.24 / 1.25 / 1.34 / 1.45 through the task kernel.
static_assert(LBAD_SHORT_MULTI_MAX >= 7 && LBAD_SHORT_MULTI_MAX <= 12, "compare_short_multi_kernel is instantiated for query lengths 1..12");
constexpr int kShortMultiK = 4;
constexpr int kSmThreads = 1024;

template <int QN, int NQ>
__global__ __launch_bounds__(kSmThreads, 1) void compare_short_multi_kernel(
    const uint4* __restrict__ recs, uint64_t n_pos, const uint32_t* __restrict__ q, uint32_t chunk_step,
    uint64_t n_chunks, uint64_t chunks_per_group, uint4 range_mask, uint64_t index_base, const ScanOut out) {
    constexpr int K = kShortMultiK;
    constexpr uint32_t nq = NQ;
    __shared__ uint4 s_q[QN * NQ * 2];                           // per (query, step): P words, N words, each rotated by one
    __shared__ uint32_t s_tail[QN * NQ][256];                    // per (query, step) and record tail: bits of 2^23 + hits in pairs 96..99
    __shared__ float2 s_rr[kTriPairs + 1];                       // (rh, rl) of possible = 0 .. 100
    __shared__ unsigned long long s_k[kSmThreads / 64][QN];
    __shared__ unsigned int s_cursor;                            // chunks of this workgroup's run handed out so far
    const uint32_t q_stride = (nq + 1u) * kQWords;
    const uint32_t rm[4] = {range_mask.x, range_mask.y, range_mask.z, range_mask.w};
    for (uint32_t i = threadIdx.x; i < QN * nq * 2u; i += kSmThreads) {
        const uint32_t qi = i / (2u * nq), rest = i - qi * 2u * nq;              // rest = 2 a + (0: P, 1: N)
        const uint32_t* src = q + (size_t)qi * q_stride + (size_t)(rest >> 1) * kQWords + (rest & 1u) * 4u;
        s_q[i] = make_uint4(src[3] & rm[3], src[0] & rm[0], src[1] & rm[1], src[2] & rm[2]);
    }
    for (uint32_t i = threadIdx.x; i < QN * nq * 256u; i += kSmThreads) {
        const uint32_t qa = i >> 8, t = i & 255u, qi = qa / nq, a = qa - qi * nq;
        const uint32_t* src = q + (size_t)qi * q_stride + (size_t)a * kQWords;
        const uint32_t qp = src[3] & rm[3], qn = src[7] & rm[3], p = t & 15u, n = t >> 4;
        s_tail[qa][t] = 0x4B000000u + (uint32_t)__popc((p | n) & ~(p ^ qp) & ~(n ^ qn) & 15u);
    }
    if (threadIdx.x == 0) s_cursor = 0u;
    if (threadIdx.x <= kTriPairs) {
        const float pf = (float)threadIdx.x;
        const float r1 = threadIdx.x ? __fdiv_rn(1.0f, pf) : 0.0f;
        s_rr[threadIdx.x] = make_float2(r1, __fmul_rn(__fmaf_rn(-pf, r1, threadIdx.x ? 1.0f : 0.0f), r1));
    }
    __syncthreads();

    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t run_first = (uint64_t)blockIdx.x * chunks_per_group;
    const uint64_t run_left = run_first < n_chunks ? n_chunks - run_first : 0ull;
    const uint32_t run_chunks = (uint32_t)(run_left < chunks_per_group ? run_left : chunks_per_group);
    // the next chunk of the run (>= run_chunks: none left); one LDS atomic per wave and chunk
    auto claim = [&]() -> uint32_t {
        uint32_t got = 0;
        if (lane == 0) got = atomicAdd(&s_cursor, 1u);
        return __builtin_amdgcn_readfirstlane(got);
    };
    const float nqf = (float)nq;
    // wave-uniform: the wave's best key so far and what a sum must reach to matter (scalar registers: they change only in
    // the rare division branch, where the lanes' candidates are reduced over the wave at once)
    unsigned long long best[QN];
    float wthr[QN];
#pragma unroll
    for (int qi = 0; qi < QN; ++qi) { best[qi] = 0ull; wthr[qi] = 0.0f; }

    // The records of the NEXT chunk are requested before this chunk's steps run (a second set of 32 registers): waves that
    // run equal phases fall into step -- all of a CU's waves waited for their records at the same time, 0.36 of 0.88 ms with
    // nothing issued (knock-out LBAD_EXP_SM_NOLOAD).
    uint4 na[K], nb[K];
    auto request = [&](uint64_t c) {
        const uint64_t p0 = c * chunk_step + (uint64_t)lane * K;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            na[k] = make_uint4(0, 0, 0, 0);
            nb[k] = make_uint4(0, 0, 0, 0);
#ifdef LBAD_EXP_SM_NOLOAD
            na[k] = make_uint4(lane, k, c, 7);
            nb[k] = make_uint4(k, lane, 5, 0x50 + (lane << 8));
#else
            if (p0 + k < n_pos) {
                na[k] = recs[2 * (p0 + k)];
                nb[k] = recs[2 * (p0 + k) + 1];
            }
#endif
        }
    };
#ifdef LBAD_SLIDE_STAMPS
#define LBAD_SM_STAMP(slot) do { if (lane == 0) g_short_times[(blockIdx.x * (kSmThreads / 64) + (threadIdx.x >> 6)) * 8 + (slot)] = __builtin_amdgcn_s_memrealtime(); } while (0)
    uint32_t chunks_done = 0;
#else
#define LBAD_SM_STAMP(slot)
#endif
    LBAD_SM_STAMP(0);
    uint32_t cur = claim(), next = run_chunks;
    if (cur < run_chunks) request(run_first + cur);
    for (; cur < run_chunks; cur = next) {
        const uint64_t c = run_first + cur;
#ifdef LBAD_SLIDE_STAMPS
        if (chunks_done == 1) LBAD_SM_STAMP(1);
        if (chunks_done == 17) LBAD_SM_STAMP(2);
        ++chunks_done;
#endif
        const uint64_t p0 = c * chunk_step + (uint64_t)lane * K;
        uint4 ra[K], rb[K];
        float rh[K], rl[K];
        const uint32_t* tail[K];                           // the record's row of s_tail[0]
        bool valid[K];
#pragma unroll
        for (int k = 0; k < K; ++k) { ra[k] = na[k]; rb[k] = nb[k]; }
        next = claim();
        if (next < run_chunks) request(run_first + next);
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const Rec r = unpack_rec(ra[k], rb[k]);
            uint32_t possible = 0;
#pragma unroll
            for (int w = 0; w < 4; ++w) possible += __popc((r.P[w] | r.N[w]) & rm[w]);
            const float2 rr = s_rr[possible];
            rh[k] = rr.x;
            rl[k] = rr.y;
            tail[k] = &s_tail[0][r.P[3] | r.N[3] << 4];
            const uint32_t ne = r.isat + r.rem + 1u;       // saturated (both fields at 15); exact whenever it is <= 16
            // a record closes a window of an "A" entry iff the window lies inside its entry AND inside this chunk
            valid[k] = p0 + k < n_pos && ne > nq && r.isat >= nq - 1u && lane * K + k >= nq - 1u;
        }

#pragma unroll
        for (int qi = 0; qi < QN; ++qi) {
            float acc[K];
#pragma unroll
            for (int k = 0; k < K; ++k) acc[k] = 0.0f;
#ifdef LBAD_EXP_SM_STEPS
#pragma unroll
            for (int a = 0; a < LBAD_EXP_SM_STEPS; ++a) {
#else
#pragma unroll
            for (int a = 0; a < NQ; ++a) {
#endif
                const u32x4 qp4 = reinterpret_cast<const u32x4*>(s_q)[(qi * NQ + a) * 2];
                const u32x4 qn4 = reinterpret_cast<const u32x4*>(s_q)[(qi * NQ + a) * 2 + 1];
                // (both stay whole 16-byte reads into register quads: as three single words the rotation's parity argument
                // would no longer hold -- the compiler narrows a read whose .x nobody uses)
                asm volatile("" :: "v"(qp4), "v"(qn4));
                const uint32_t qP[3] = {qp4.y, qp4.z, qp4.w}, qN[3] = {qn4.y, qn4.z, qn4.w};    // (rotated by one; .x = pairs 96..99: in the table)
                float ratio[K];
                uint32_t h[K];
#pragma unroll
                for (int k = 0; k < K; ++k) h[k] = tail[k][(qi * NQ + a) * 256];
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const uint32_t P[3] = {ra[k].x, ra[k].y, ra[k].z}, N[3] = {rb[k].x, rb[k].y, rb[k].z};
#pragma unroll
                    for (int w = 0; w < 3; ++w) {
                        const uint32_t u = __builtin_amdgcn_bitop3_b32(P[w], N[w], qP[w], 0xA4);   // (P | N) & ~(P ^ qP)
                        const uint32_t v = __builtin_amdgcn_bitop3_b32(u, N[w], qN[w], 0x90);      // u & ~(N ^ qN)
                        asm("v_bcnt_u32_b32 %0, %1, %0" : "+v"(h[k]) : "v"(v));
                    }
                    const float hf = __fsub_rn(__uint_as_float(h[k]), 8388608.0f);
                    const float t = __fmul_rn(hf, rl[k]);
                    asm("v_fma_f32 %0, %1, %2, %3" : "=v"(ratio[k]) : "v"(hf), "v"(rh[k]), "v"(t));
                }
                const float in0 = __uint_as_float(from_left_lane(__float_as_uint(acc[K - 1])));
#pragma unroll
                for (int k = K - 1; k >= 0; --k) {
                    // (as single adds in place: packed, the compiler renames the sums with three moves per step)
                    const float from = k ? acc[k - 1] : in0;
                    asm("v_add_f32 %0, %1, %2" : "=v"(acc[k]) : "v"(from), "v"(ratio[k]));
                }
                // (a step at a time: left alone, the scheduler pulls the LDS reads of every unrolled step to the front and
                // spills 240 registers)
                __builtin_amdgcn_sched_barrier(0);
            }
            // The exact division (Fp.m:144) runs only where the sum can reach the wave's best so far.
            float m = __int_as_float(kNegInf);
#pragma unroll
            for (int k = 0; k < K; ++k) m = fmaxf(m, valid[k] ? acc[k] : __int_as_float(kNegInf));
#ifdef LBAD_EXP_SM_NOEPI
            if (__ballot(m >= 1e30f) != 0ull) {
#else
            if (__ballot(m >= wthr[qi]) != 0ull) {
#endif
                unsigned long long mine = 0ull;
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    if (valid[k] && acc[k] >= wthr[qi]) {
                        const float cand = __fdiv_rn(acc[k], nqf);
                        const float match = (0.0f < cand) ? cand : 0.0f;     // MAX(match, cand) from match = 0
                        const uint32_t idx = (rb[k].w >> 4) | ((ra[k].w >> 17) & 0xFu) << 28;       // (unpack_rec's idx)
                        const unsigned long long key = sl_key(match, index_base + idx);
                        mine = key > mine ? key : mine;
                    }
                }
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) {
                    const unsigned long long o = __shfl_xor(mine, off, 64);
                    mine = o > mine ? o : mine;
                }
                const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(mine >> 32));
                const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)mine);
                const unsigned long long wave_key = ((unsigned long long)hi << 32) | lo;
                if (wave_key > best[qi]) best[qi] = wave_key;
                // (scores are >= +0: their bits order like the values)
                wthr[qi] = __uint_as_float((uint32_t)(best[qi] >> 32)) * 0.99999f * nqf;
            }
        }
    }
    LBAD_SM_STAMP(3);
    if (lane == 0) {
#pragma unroll
        for (int qi = 0; qi < QN; ++qi) s_k[threadIdx.x >> 6][qi] = best[qi];
    }
    __syncthreads();
    if (threadIdx.x == 0) {                       // the keys are max-ed in place (the host clears them in front of the launch)
        for (int qi = 0; qi < QN; ++qi) {
            unsigned long long m = s_k[0][qi];
            for (int i = 1; i < kSmThreads / 64; ++i) m = s_k[i][qi] > m ? s_k[i][qi] : m;
            if (m) atomicMax(&out.keys[out.pos[qi]], m);
        }
    }
}

}  // namespace

uint32_t sliding_short_multi_max() { return LBAD_SHORT_MULTI_MAX; }

// 64 K records per wave and chunk (K = 4 records per lane once a window reaches back more than six records: the overlap of
// consecutive chunks stays a small part of a chunk)
hipError_t launch_sliding_short(const SlideCorpus& src, const SlideChoice& ch, const SlideScan& scan, const SlideCall& call,
                                const float* tri, uint32_t look, uint32_t only_upto) {
    if (!scan.d_queries) return hipErrorInvalidValue;
    const uint32_t K = look <= 6u ? 1u : 4u;
    const uint32_t step = 64u * K - look;
    const uint64_t span = 64ull * K;
    const uint64_t n_chunks = src.n_pos <= span ? 1u : (src.n_pos - span + step - 1u) / step + 1u;
    const uint64_t want = (n_chunks + (kSlThreads / 64) - 1) / (kSlThreads / 64);
    const uint64_t cap = (uint64_t)ch.cus * 6u;                   // 21 KB of LDS per workgroup
    const uint32_t grid = (uint32_t)(want < cap ? want : cap);
    const uint4 rm4 = sliding_range_mask(src.subfp_len, call.range);
    const ScanOut out = scan_out(scan);
    auto launch = [&](auto k, auto qn) {
        hipLaunchKernelGGL((compare_short_kernel<decltype(k)::value, decltype(qn)::value>), dim3(grid), dim3(kSlThreads), 0, call.stream,
                           src.recs, src.n_pos, scan.d_queries, call.n_query, step, n_chunks, rm4, tri, call.index_base,
                           call.d_score_bits, out, only_upto);
    };
    auto launch_k = [&](auto k) -> bool {
        switch (ch.n_take) {
            case 1: launch(k, std::integral_constant<int, 1>{}); return true;
            case 2: launch(k, std::integral_constant<int, 2>{}); return true;
            case 4: launch(k, std::integral_constant<int, 4>{}); return true;
            case 8: launch(k, std::integral_constant<int, 8>{}); return true;
            default: return false;
        }
    };
    if (!(K == 1 ? launch_k(std::integral_constant<int, 1>{}) : launch_k(std::integral_constant<int, 4>{}))) return hipErrorInvalidValue;
    return hipGetLastError();
}

// one workgroup of sixteen waves per CU, each with a contiguous run of chunks its waves claim from an LDS cursor
hipError_t launch_sliding_short_multi(const SlideCorpus& src, const SlideChoice& ch, const SlideScan& scan, const SlideCall& call) {
    if (!scan.d_queries) return hipErrorInvalidValue;
    const uint32_t look = call.n_query - 1u;
    const uint32_t step = 64u * kShortMultiK - look;
    const uint64_t span = 64ull * kShortMultiK;
    const uint64_t n_chunks = src.n_pos <= span ? 1u : (src.n_pos - span + step - 1u) / step + 1u;
    const uint64_t waves = kSmThreads / 64;
    const uint64_t want = (n_chunks + waves - 1) / waves;
    const uint64_t cap = ch.cus;
    const uint32_t grid = (uint32_t)(want < cap ? want : cap);
    const uint64_t per_group = (n_chunks + grid - 1) / grid;
    if (per_group >= 0xFFFFFFFFull) return hipErrorInvalidValue;
    const uint4 rm4 = sliding_range_mask(src.subfp_len, call.range);
    const ScanOut out = scan_out(scan);
    auto launch = [&](auto qn, auto nq) {
        hipLaunchKernelGGL((compare_short_multi_kernel<decltype(qn)::value, decltype(nq)::value>), dim3(grid), dim3(kSmThreads), 0,
                           call.stream, src.recs, src.n_pos, scan.d_queries, step, n_chunks, per_group, rm4, call.index_base, out);
    };
    // the instances: 2, 4, 8 queries of 1 .. LBAD_SHORT_MULTI_MAX sub-fingerprints
    auto launch_n = [&](auto qn) -> bool {
        switch (call.n_query) {
            case 1: launch(qn, std::integral_constant<int, 1>{}); return true;
            case 2: launch(qn, std::integral_constant<int, 2>{}); return true;
            case 3: launch(qn, std::integral_constant<int, 3>{}); return true;
            case 4: launch(qn, std::integral_constant<int, 4>{}); return true;
            case 5: launch(qn, std::integral_constant<int, 5>{}); return true;
            case 6: launch(qn, std::integral_constant<int, 6>{}); return true;
            case 7: launch(qn, std::integral_constant<int, 7>{}); return true;
#if LBAD_SHORT_MULTI_MAX > 7
            case 8: launch(qn, std::integral_constant<int, 8>{}); return true;
            case 9: launch(qn, std::integral_constant<int, 9>{}); return true;
            case 10: launch(qn, std::integral_constant<int, 10>{}); return true;
            case 11: launch(qn, std::integral_constant<int, 11>{}); return true;
            case 12: launch(qn, std::integral_constant<int, 12>{}); return true;
#endif
            default: return false;
        }
    };
    bool known = false;
    if (ch.n_take == 2) known = launch_n(std::integral_constant<int, 2>{});
    else if (ch.n_take == 4) known = launch_n(std::integral_constant<int, 4>{});
    else if (ch.n_take == 8) known = launch_n(std::integral_constant<int, 8>{});
    return known ? hipGetLastError() : hipErrorInvalidValue;
}

#ifdef LBAD_SLIDE_STAMPS
extern "C" int LBAudioDetectiveDebugShortTimes(unsigned long long* out, int n_words) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_short_times), sizeof(unsigned long long) * (size_t)n_words) == hipSuccess ? 0 : 1;
}
extern "C" int LBAudioDetectiveDebugShortTimesReset() {
    void* p = nullptr;
    if (hipGetSymbolAddress(&p, HIP_SYMBOL(g_short_times)) != hipSuccess) return 1;
    return hipMemset(p, 0, sizeof(unsigned long long) * 1024 * 16 * 8) == hipSuccess ? 0 : 1;
}
#endif

}  // namespace lbad
