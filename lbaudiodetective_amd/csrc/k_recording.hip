// k_recording.hip -- scores and lags of a RAGGED corpus for ONE query of any length, a long recording above all: for every
// entry j the largest cell q_o of the pair's profile (what LBAudioDetectiveCorpusMatchProfile returns, what oc_cells computes)
// and the LOWEST offset that reaches it -- the ragged scan's score and the alignment's lag, bit for bit, with the occurrences
// pass' pair loop: n_e steps per pass of a pair whose entry is the shorter side, not n_query.
//
// The pair loop is the occurrences pass' as it is (occurrences_common.hpp): work items (entry, tile of kOcTile = 126 offsets),
// cases A and B, two neighbouring offsets per lane, the window once per block of kOcEntries entries in LDS, fingerprint2 through
// the scalar unit, FULL and masked instances.  The two edge cells a wave computes for the occurrences' peak test are not folded.
//   maxima  a kept cell with o < n_off is the 64-bit value  q_o bits << 32 | 0xFFFFFFFF - o.  Cells are finite and >= +0, so
//           their bit patterns order like the values, and the largest value is the largest cell at its lowest offset.  The
//           wave's maximum (DPP inside a row of 16 lanes, four rows through the scalar unit; the whole wave is there) goes to
//           partials[entry][tile], one writer per word; a tile without an offset of the pair gets 0.
//   fold    a second launch: an entry's partials -> its score (the maximum is >= +0 already) and, where asked for, its lag, +o
//           when the entry is longer than the query and -o otherwise.
// PARTIALS, not atomics: no word of memory has two writers, no workgroup waits for another, and nothing depends on launch
// order, grid or chunking -- a maximum does not depend on the order of its operands.
// Nothing is read beyond an entry's records plus one (inside kRecordSlack), or beyond the query's words.
#include "occurrences_common.hpp"

namespace lbad {
namespace {

constexpr uint32_t kFoldThreads = 256;

// the larger of v and the same value of the lane `ror` places to the right inside its row of 16 (full EXEC)
template <int ROR>
__device__ __forceinline__ unsigned long long rec_row_max(unsigned long long v) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, 0x120 + ROR /* row_ror:ROR */, 0xF, 0xF, true);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v >> 32), 0x120 + ROR, 0xF, 0xF, true);
    const unsigned long long o = ((unsigned long long)hi << 32) | lo;
    return o > v ? o : v;
}

// the wave's maximum, wave-uniform.  Called by whole waves.
__device__ __forceinline__ unsigned long long rec_wave_max(unsigned long long v) {
    v = rec_row_max<1>(v);
    v = rec_row_max<2>(v);
    v = rec_row_max<4>(v);
    v = rec_row_max<8>(v);                                     // every lane: its row's maximum
    unsigned long long best = 0ull;
#pragma unroll
    for (int row = 0; row < 4; ++row) {
        const unsigned long long r = ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), row * 16) << 32) |
                                     (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, row * 16);
        best = r > best ? r : best;
    }
    return best;
}

// Units of kOcEntries entries (oc_unit), as in occurrences_count_kernel.  partials[entry][tile] for every
// tile below a.tiles.
template <bool FULL>
__global__ __launch_bounds__(kOcThreads) void recording_maxima_kernel(const OcArgs a, unsigned long long* __restrict__ partials) {
    extern __shared__ uint4 s_dyn[];
    const OcLds s = oc_lds(s_dyn, a.win);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    oc_load_tri(a, s);
    const uint32_t units = oc_units(a, kOcEntries);
    for (uint32_t u = blockIdx.x; u < units; u += gridDim.x) {
        const OcUnit n = oc_unit(a, u, kOcEntries, wave);
        oc_stage_unit(a, s, n.wb);
        if (n.tile >= a.tiles) continue;                       // (this wave meets no barrier of the unit any more)
        const uint32_t first = n.tile * kOcTile;
        const uint32_t o = first - 1u + 2u * lane;
        for (uint32_t e = n.e0; e < n.e1; ++e) {
            uint32_t rec0, ne;
            oc_entry(a, e, &rec0, &ne);
            const uint32_t n_off = oc_offsets(a, ne);
            unsigned long long best = 0ull;
            if (first < n_off) {
                float q0, q1;
                (void)oc_cells<FULL>(a, s, n.wb, rec0, ne, o, &q0, &q1);
                // (lane 0's first and lane 63's second cell are the neighbouring tiles')
                const unsigned long long v0 = lane != 0u && o < n_off ? ((unsigned long long)__float_as_uint(q0) << 32) | (0xFFFFFFFFu - o) : 0ull;
                const unsigned long long v1 =
                    lane != 63u && o + 1u < n_off ? ((unsigned long long)__float_as_uint(q1) << 32) | (0xFFFFFFFFu - (o + 1u)) : 0ull;
                best = rec_wave_max(v0 > v1 ? v0 : v1);
            }
            if (lane == 0u) partials[(size_t)e * a.tiles + n.tile] = best;
        }
    }
}

// An entry's partials -> its score and lag.  `lanes` (a power of two, 1 .. 64) neighbouring lanes share an entry and read its
// partials side by side; whole waves, the lanes of entries beyond the chunk hold 0.
__global__ __launch_bounds__(kFoldThreads) void recording_fold_kernel(const unsigned long long* __restrict__ partials,
                                                                      const uint32_t* __restrict__ off, uint32_t first,
                                                                      uint32_t entries, uint32_t tiles, uint32_t lanes, uint32_t nq,
                                                                      float* __restrict__ scores, int32_t* __restrict__ lags) {
    const uint64_t t = (uint64_t)blockIdx.x * kFoldThreads + threadIdx.x;
    const uint64_t e = t / lanes;
    const uint32_t sub = (uint32_t)(t - e * lanes);
    unsigned long long best = 0ull;
    if (e < entries)
        for (uint32_t tile = sub; tile < tiles; tile += lanes) {
            const unsigned long long v = partials[(size_t)e * tiles + tile];
            best = v > best ? v : best;
        }
    for (uint32_t d = lanes >> 1; d != 0u; d >>= 1) {
        const unsigned long long o = __shfl_xor(best, (int)d, 64);
        best = o > best ? o : best;
    }
    if (e >= entries || sub != 0u) return;
    // (tile 0 holds offset 0 of every pair: best's low word is 0xFFFFFFFF - o of a cell that exists)
    scores[first + e] = __uint_as_float((uint32_t)(best >> 32));
    if (lags) {
        const uint32_t o = 0xFFFFFFFFu - (uint32_t)best;
        const uint32_t ne = off[first + e + 1u] - off[first + e];
        lags[first + e] = nq < ne ? (int32_t)o : -(int32_t)o;
    }
}

// lags[slot] = the lag of the entry key[slot] names; a zero key, or an index outside the corpus, gives 0
__global__ __launch_bounds__(kFoldThreads) void recording_lag_gather_kernel(const unsigned long long* __restrict__ keys, uint64_t n,
                                                                            uint32_t base, uint64_t count,
                                                                            const int32_t* __restrict__ entry_lags,
                                                                            int32_t* __restrict__ lags) {
    const uint64_t slot = (uint64_t)blockIdx.x * kFoldThreads + threadIdx.x;
    if (slot >= n) return;
    const unsigned long long key = keys[slot];
    const uint32_t j = 0xFFFFFFFFu - (uint32_t)key - base;     // (the low word is 0xFFFFFFFF - (index base + j))
    lags[slot] = key != 0ull && j < count ? entry_lags[j] : 0;
}

template <bool FULL>
hipError_t launch_maxima(const OcArgs& a, size_t lds, unsigned long long* partials, hipStream_t stream) {
    static size_t ready[kMaxDevices] = {};                     // (this instance)
    const hipError_t e = oc_allow_lds(ready, lds, recording_maxima_kernel<FULL>);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(recording_maxima_kernel<FULL>, oc_grid(oc_blocks(a.entries) * a.groups), dim3(kOcThreads), lds, stream, a, partials);
    return hipGetLastError();
}

}  // namespace

size_t recording_scratch_bytes(uint64_t entries, uint64_t tiles) { return (size_t)(entries * tiles * 8u); }

// entries of a chunk under a scratch limit: the largest whole number of entry blocks that fits (0: not even one), with
// entries x tiles within kOcMaxItems
uint64_t recording_chunk_entries(uint64_t tiles, uint64_t limit_bytes) {
    const uint64_t per_block = kOcEntries * 8u * tiles;
    const uint64_t blocks = limit_bytes / per_block;
    const uint64_t most = (kOcMaxItems / tiles) / kOcEntries;
    return (blocks < most ? blocks : most) * kOcEntries;
}

hipError_t launch_recording_chunk(const RecordingCall& c, void* d_scratch, uint64_t first_entry, uint64_t entries) {
    if (entries == 0) return hipSuccess;
    if (!oc_call_ok(c, occurrences_tiles(c.n_query, c.ne_min, c.ne_max), first_entry, entries) || !c.d_scores) return hipErrorInvalidValue;
    size_t lds = 0;
    const OcArgs a = oc_args(c, first_entry, entries, 0.0f, false, &lds);          // (no cell is tested here)
    if (!a.tri) return hipErrorOutOfMemory;
    unsigned long long* partials = static_cast<unsigned long long*>(d_scratch);
    const hipError_t e =
        c.range >= c.subfp_len ? launch_maxima<true>(a, lds, partials, c.stream) : launch_maxima<false>(a, lds, partials, c.stream);
    if (e != hipSuccess) return e;
    uint32_t lanes = 1;
    while (lanes < 64u && lanes < c.tiles) lanes <<= 1;
    const uint64_t threads = entries * lanes;
    hipLaunchKernelGGL(recording_fold_kernel, dim3((uint32_t)((threads + kFoldThreads - 1) / kFoldThreads)), dim3(kFoldThreads), 0, c.stream,
                       partials, c.d_off, a.first, a.entries, a.tiles, lanes, c.n_query, c.d_scores, c.d_lags);
    return hipGetLastError();
}

hipError_t launch_recording_lag_gather(const unsigned long long* d_keys, uint64_t n, uint64_t index_base, uint64_t count,
                                       const int32_t* d_entry_lags, int32_t* d_lags, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (n > 0x80000000ull || index_base + count > 0x100000000ull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(recording_lag_gather_kernel, dim3((uint32_t)((n + kFoldThreads - 1) / kFoldThreads)), dim3(kFoldThreads), 0, stream,
                       d_keys, n, (uint32_t)index_base, count, d_entry_lags, d_lags);
    return hipGetLastError();
}

}  // namespace lbad
