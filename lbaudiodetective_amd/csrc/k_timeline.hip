// k_timeline.hip -- the recording timeline: for ONE query of any length, a long recording above all, against a RAGGED corpus,
// the best entry at every offset of the query.  The cells are the occurrences pass' (what LBAudioDetectiveCorpusMatchProfile
// returns, what oc_cells computes); k_occurrences.hip lists them, k_recording.hip folds them per entry over the offsets, this
// file folds them per OFFSET over the entries that fit inside the query (n_entry <= n_query, case B: the query is fingerprint1).
//
// The pair loop is the occurrences pass' as it is (occurrences_common.hpp): a wave keeps one tile of kOcTile = 126 offsets and
// walks the entries of its unit with it, two neighbouring offsets per lane, the window once per unit in LDS, the entry's
// record of a step through the scalar unit, FULL and masked instances.  A lane's two offsets do not change over the walk:
//   maxima   a cell that counts (entry not longer than the query, o < n_off, not one of the wave's two edge cells, q_o >= t) is
//            the key  q_o bits << 32 | 0xFFFFFFFF - (index base + entry) ; cells are finite and > 0, so keys order like (score,
//            lower index first).  A lane keeps the running maximum of each of its two offsets in registers -- no cross-lane step
//            -- and stores both behind the walk to partials[entry block][tile x 126 + cell], every word of a tile below the
//            call's tiles written by exactly one lane (0 where nothing counted).  A unit walks kTlEntries entries.
//   fold     out[o] = max(out[o], max over the entry blocks of partials[block][o]): a workgroup takes 64 neighbouring offsets
//            (a wave reads a row's 512 bytes side by side), its waves share the rows and meet in LDS.  More than kTlFoldRows
//            blocks take two launches: slices of rows first, each into its own first row (read before by the lane that writes
//            it), then the slices' first rows into out.
//   lengths  after the last chunk: outLengths[o] = the length of the entry out[o] names, 0 for a zero key.
// PARTIALS, not atomics: no word of memory has two writers in a launch, no workgroup waits for another, and nothing depends on
// launch order, grid or chunking -- a maximum does not depend on the order of its operands.
// Nothing is read beyond an entry's records plus one (inside kRecordSlack), or beyond the query's words.
#include "occurrences_common.hpp"

namespace lbad {
namespace {

// entries a unit walks with one staged window (a multiple of kOcEntries; a chunk is a whole number of these).  The window
// depends on the tile group alone, so a longer walk stages it less often and shrinks the partials in proportion; 128 keeps
// the 1 M x 2 400 shape's partials (150 MB) inside the default scratch in ONE chunk and still leaves 100 k entries about
// 3 900 units, several per workgroup slot of the device.
constexpr uint32_t kTlEntries = 128;
constexpr uint32_t kTlFoldThreads = 256;
constexpr uint32_t kTlFoldWaves = kTlFoldThreads / 64;
constexpr uint32_t kTlFoldRows = 32;                   // rows a workgroup of the fold's first level takes; at most this many: one level
constexpr uint32_t kTlFoldSlices = 1024;               // slices of the first level at most (the second level's rows)
static_assert(kTlEntries % kOcEntries == 0 && kTlEntries != 0, "a unit is whole entry blocks of the occurrences pass");

// Units of kTlEntries entries (oc_unit).  key_low - e is the low word of chunk
// entry e's key.  partials[entry block][a.tiles x kOcTile].
template <bool FULL>
__global__ __launch_bounds__(kOcThreads) void timeline_maxima_kernel(const OcArgs a, uint32_t key_low,
                                                                    unsigned long long* __restrict__ partials) {
    extern __shared__ uint4 s_dyn[];
    const OcLds s = oc_lds(s_dyn, a.win);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    oc_load_tri(a, s);
    const uint32_t units = oc_units(a, kTlEntries);
    for (uint32_t u = blockIdx.x; u < units; u += gridDim.x) {
        const OcUnit n = oc_unit(a, u, kTlEntries, wave);
        oc_stage_unit(a, s, n.wb);
        if (n.tile >= a.tiles) continue;                       // (this wave meets no barrier of the unit any more)
        const uint32_t first = n.tile * kOcTile;
        const uint32_t o = first - 1u + 2u * lane;
        unsigned long long best0 = 0ull, best1 = 0ull;
        for (uint32_t e = n.e0; e < n.e1; ++e) {
            uint32_t rec0, ne;
            oc_entry(a, e, &rec0, &ne);
            if (ne > a.nq || first >= a.nq - ne + 1u) continue;            // (wave-uniform: no place inside the query, or none in this tile)
            float q0, q1;
            // (bit 0 / 1: the cell is the wave's own, o < n_off and q >= t)
            const uint32_t bits = oc_cells<FULL>(a, s, n.wb, rec0, ne, o, &q0, &q1);
            const uint32_t low = key_low - e;
            const unsigned long long v0 = bits & 1u ? ((unsigned long long)__float_as_uint(q0) << 32) | low : 0ull;
            const unsigned long long v1 = bits & 2u ? ((unsigned long long)__float_as_uint(q1) << 32) | low : 0ull;
            best0 = v0 > best0 ? v0 : best0;
            best1 = v1 > best1 ? v1 : best1;
        }
        // (cell o is the tile's 2 x lane - 1, cell o + 1 its 2 x lane; lane 0's first and lane 63's second are the neighbours')
        unsigned long long* __restrict__ row = partials + ((size_t)n.eb * a.tiles + n.tile) * kOcTile;
        if (lane != 0u) row[2u * lane - 1u] = best0;
        if (lane != 63u) row[2u * lane] = best1;
    }
}

// Word o < n of the rows [y x rows_per, (y + 1) x rows_per) below `rows` of src (`stride` words apart) folded to their maximum,
// y = blockIdx.y.  dst given: dst[o] = max(dst[o], that); dst == nullptr: into the slice's own first row.
__global__ __launch_bounds__(kTlFoldThreads) void timeline_fold_kernel(unsigned long long* src, uint32_t rows, uint32_t rows_per,
                                                                       uint64_t stride, uint32_t n, unsigned long long* dst) {
    __shared__ unsigned long long s_best[kTlFoldWaves][64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t o = blockIdx.x * 64u + lane;
    const uint32_t r0 = blockIdx.y * rows_per, r1 = rows - r0 < rows_per ? rows : r0 + rows_per;
    unsigned long long best = 0ull;
    if (o < n)
        for (uint32_t r = r0 + wave; r < r1; r += kTlFoldWaves) {
            const unsigned long long v = src[(size_t)r * stride + o];
            best = v > best ? v : best;
        }
    s_best[wave][lane] = best;
    __syncthreads();                                           // (every thread of the workgroup is here)
    if (wave != 0u || o >= n) return;
#pragma unroll
    for (uint32_t w = 1; w < kTlFoldWaves; ++w) best = s_best[w][lane] > best ? s_best[w][lane] : best;
    if (dst) {
        const unsigned long long old = dst[o];
        dst[o] = old > best ? old : best;
    } else {
        src[(size_t)r0 * stride + o] = best;                   // (row r0's word o: read above by this very lane, by nobody else)
    }
}

// lengths[o] = sub-fingerprints of the entry keys[o] names; a zero key, or an index outside the corpus, gives 0
__global__ __launch_bounds__(kTlFoldThreads) void timeline_lengths_kernel(const unsigned long long* __restrict__ keys, uint32_t n,
                                                                          uint32_t base, uint64_t count,
                                                                          const uint32_t* __restrict__ off,
                                                                          uint32_t* __restrict__ lengths) {
    const uint32_t o = blockIdx.x * kTlFoldThreads + threadIdx.x;
    if (o >= n) return;
    const unsigned long long key = keys[o];
    const uint32_t j = 0xFFFFFFFFu - (uint32_t)key - base;     // (the low word is 0xFFFFFFFF - (index base + j))
    lengths[o] = key != 0ull && j < count ? off[j + 1u] - off[j] : 0u;
}

inline uint64_t tl_blocks(uint64_t entries) { return (entries + kTlEntries - 1) / kTlEntries; }

template <bool FULL>
hipError_t launch_tl_maxima(const OcArgs& a, size_t lds, uint32_t key_low, unsigned long long* partials, hipStream_t stream) {
    static size_t ready[kMaxDevices] = {};                     // (this instance)
    const hipError_t e = oc_allow_lds(ready, lds, timeline_maxima_kernel<FULL>);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(timeline_maxima_kernel<FULL>, oc_grid(tl_blocks(a.entries) * a.groups), dim3(kOcThreads), lds, stream, a, key_low,
                       partials);
    return hipGetLastError();
}

}  // namespace

uint32_t timeline_block_entries() { return kTlEntries; }

uint64_t timeline_tiles(uint32_t n_query, uint32_t ne_min) {
    const uint64_t offsets = (uint64_t)n_query - (ne_min < n_query ? ne_min : n_query) + 1;
    return (offsets + kOcTile - 1) / kOcTile;
}

size_t timeline_scratch_bytes(uint64_t entries, uint64_t tiles) { return (size_t)(tl_blocks(entries) * tiles * kOcTile * 8u); }

// entries of a chunk under a scratch limit: the largest whole number of entry blocks that fits (0: not even one), with
// entries x tiles within kOcMaxItems
uint64_t timeline_chunk_entries(uint64_t tiles, uint64_t limit_bytes) {
    const uint64_t per_block = tiles * kOcTile * 8u;
    const uint64_t blocks = limit_bytes / per_block;
    const uint64_t most = (kOcMaxItems / tiles) / kTlEntries;
    return (blocks < most ? blocks : most) * kTlEntries;
}

hipError_t launch_timeline_chunk(const TimelineCall& c, void* d_scratch, uint64_t first_entry, uint64_t entries) {
    if (entries == 0) return hipSuccess;
    // (oc_call_ok's, and what ties the launch to the entries that take part and to the keys)
    if (!oc_call_ok(c, timeline_tiles(c.n_query, c.ne_min), first_entry, entries) || c.ne_min > c.n_query ||
        c.index_base + first_entry + entries > 0x100000000ull || !c.d_keys)
        return hipErrorInvalidValue;
    size_t lds = 0;
    const OcArgs a = oc_args(c, first_entry, entries, c.threshold, false, &lds);
    if (!a.tri) return hipErrorOutOfMemory;
    unsigned long long* partials = static_cast<unsigned long long*>(d_scratch);
    const uint32_t key_low = 0xFFFFFFFFu - (uint32_t)c.index_base - a.first;
    const hipError_t e = c.range >= c.subfp_len ? launch_tl_maxima<true>(a, lds, key_low, partials, c.stream)
                                                : launch_tl_maxima<false>(a, lds, key_low, partials, c.stream);
    if (e != hipSuccess) return e;
    // the offsets a pair reaches lie below tiles x 126; the words of out beyond them stay the caller's zeros
    const uint64_t stride = c.tiles * kOcTile;
    const uint32_t n = (uint32_t)(stride < c.n_query ? stride : c.n_query);
    const uint32_t blocks = (uint32_t)tl_blocks(entries);
    const uint32_t gx = (n + 63u) / 64u;
    if (blocks <= kTlFoldRows) {
        hipLaunchKernelGGL(timeline_fold_kernel, dim3(gx, 1), dim3(kTlFoldThreads), 0, c.stream, partials, blocks, blocks, stride, n, c.d_keys);
    } else {
        const uint32_t fit = (blocks + kTlFoldSlices - 1u) / kTlFoldSlices;
        const uint32_t rows_per = fit > kTlFoldRows ? fit : kTlFoldRows;
        const uint32_t slices = (blocks + rows_per - 1u) / rows_per;
        hipLaunchKernelGGL(timeline_fold_kernel, dim3(gx, slices), dim3(kTlFoldThreads), 0, c.stream, partials, blocks, rows_per, stride, n,
                           static_cast<unsigned long long*>(nullptr));
        hipLaunchKernelGGL(timeline_fold_kernel, dim3(gx, 1), dim3(kTlFoldThreads), 0, c.stream, partials, slices, slices,
                           stride * rows_per, n, c.d_keys);
    }
    return hipGetLastError();
}

hipError_t launch_timeline_lengths(const unsigned long long* d_keys, uint32_t n, uint64_t index_base, uint64_t count,
                                   const uint32_t* d_off, uint32_t* d_lengths, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (n > 0x7FFFFFFFu || index_base + count > 0x100000000ull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(timeline_lengths_kernel, dim3((n + kTlFoldThreads - 1u) / kTlFoldThreads), dim3(kTlFoldThreads), 0, stream, d_keys,
                       n, (uint32_t)index_base, count, d_off, d_lengths);
    return hipGetLastError();
}

}  // namespace lbad
