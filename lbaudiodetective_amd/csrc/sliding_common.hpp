// sliding_common.hpp -- what the files of the ragged-corpus scan share: k_sliding.hip (the task scan and its plan),
// k_sliding_short.hip (the two systolic scans), k_records.hip (the records themselves) and sliding.cpp (the host side: query
// blocks, the choice of kernel, the launcher).  internal.hpp has what the api_*.cpp files see of them.
//
// A record (round 4 layout, 32 bytes, eight words):
//   w0..w2  P   first Boolean of pairs 0..95  (pairs = ceil(length / 2) <= 100), pair p at bit p & 31 of word p >> 5
//   w3      bits 0..3: P of pairs 96..99;  bits 4..16: the row of the quotient table for this record's `possible`
//           over the FULL range, possible (possible + 1) / 2;  bits 17..20: entry index, bits 28..31;
//           bits 21..24: index of the sub-fingerprint inside its entry, saturated at 15;  bits 25..28: sub-fingerprints
//           that follow it inside its entry, saturated at 15
//   w4..w6  N   second Boolean of pairs 0..95
//   w7      bits 0..3: N of pairs 96..99;  bits 4..31: entry index, bits 0..27
// 25 of the 32 bytes are the reference's information (25 B per sub-fingerprint).  Everything else is
// DERIVED (the table row from the Booleans, the place fields from the entries' counts) and is written by this
// library only: the loader recomputes it from the counts it has validated (restamp_records_kernel), so a corpus file
// cannot plant it.  The bits above the pairs never score: a hit needs both Booleans of a pair equal on both sides,
// and the query's words are zero there.  The place fields serve the scan of SHORT queries only (compare_short_kernel).
#pragma once

#include "internal.hpp"

namespace lbad {
// (an unnamed namespace per file, as before the scan was split by kernel: the kernels' argument types -- and with them the
// kernels' symbols -- stay what they were)
namespace {

constexpr int kSlThreads = 256;       // pack / plan kernels, the systolic scan of single queries
constexpr uint32_t kTriPairs = 100;
constexpr uint32_t kTriSize = (kTriPairs + 1) * (kTriPairs + 2) / 2;   // 5151 quotients
constexpr uint32_t kQWords = 16;      // per query sub-fingerprint: P[4] N[4] NZ[4] tri-base possible - -
constexpr uint32_t kSlideMaxGrid = 1024;      // most workgroups of a task scan (the plan holds a start per workgroup)
constexpr uint32_t kSlideQueryArgSubs = 47;   // longest query that travels as a kernel argument (4 KB)

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));    // four words as one register quad

__device__ __forceinline__ unsigned long long sl_key(float score, uint64_t global_index) {
    return ((unsigned long long)__float_as_uint(score) << 32) |
           (unsigned long long)(0xFFFFFFFFu - (uint32_t)global_index);
}

// value of lane l + 1 / lane l - 1 (the wave's last / first lane keeps `old`); full EXEC wherever these are used:
// a DPP read of a lane that is switched off does not deliver its register
__device__ __forceinline__ uint32_t from_right_lane(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x130 /* wave_shl:1 */, 0xF, 0xF, true);
}
__device__ __forceinline__ uint32_t from_left_lane(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x138 /* wave_shr:1 */, 0xF, 0xF, true);
}

// Where a scan leaves its result.  acc: n_keys words that are ZERO between scans (the scan's running maxima, also what a
// strong match is published through while the scan runs); ticket: workgroups that have finished; the last one moves acc to
// keys and clears both -- no memset in front of the scan.
struct ScanOut {
    unsigned long long* acc;
    unsigned int* ticket;
    unsigned long long* keys;
    uint32_t pos[8];              // query i's key goes to keys[pos[i]]
};

inline ScanOut scan_out(const SlideScan& scan) {
    ScanOut out;
    out.acc = scan.d_acc; out.ticket = scan.d_ticket; out.keys = scan.d_keys;
    for (int i = 0; i < 8; ++i) out.pos[i] = scan.key_pos[i];
    return out;
}

}  // namespace

// sliding.cpp
uint4 pair_mask(uint32_t limit);            // pair bits 0 .. ceil(limit / 2) - 1
const float* sliding_tri_table();           // the table of correctly rounded quotients on the current device (null: no memory)

// What the kernel files tell the choice (sliding.cpp: sliding_choose) about their builds -- a tuning macro is read in one file.
// k_sliding.hip: threads of the task kernel's instance for n_q queries, workgroups per CU, most queries an instance takes
uint32_t sliding_task_threads(uint32_t n_q);
uint32_t sliding_task_groups_per_cu();
uint32_t sliding_task_max_queries();
// k_sliding_short.hip: longest query of a batch compare_short_multi_kernel takes
uint32_t sliding_short_multi_max();

// The launches themselves, each in the file of its kernel; the SlideChoice names the instance, nothing is derived again.
// k_sliding.hip: compare_sliding_kernel (reads src.plan)
hipError_t launch_sliding_task(const SlideCorpus& src, const SlideChoice& ch, const SlideScan& scan, const SlideCall& call,
                               const float* tri);
// k_sliding_short.hip: compare_short_kernel<K, QN> with K from `look` (how far back a window reaches); only_upto: see the
// kernel.  compare_short_multi_kernel<QN, n_query>.  Both max their keys in place.
hipError_t launch_sliding_short(const SlideCorpus& src, const SlideChoice& ch, const SlideScan& scan, const SlideCall& call,
                                const float* tri, uint32_t look, uint32_t only_upto);
hipError_t launch_sliding_short_multi(const SlideCorpus& src, const SlideChoice& ch, const SlideScan& scan, const SlideCall& call);

}  // namespace lbad
