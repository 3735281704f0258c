// k_remove.hip -- entries taken out of a corpus on the device: a stable compaction of the planes (uniform corpus) or of the
// records (ragged corpus) in place, DESIGN.md 4.4g.
//
// The entries a call names are marked, the others keep their order and close up: old index i becomes i - (removed below i).
// Three rules hold for every launch here: no workgroup ever waits for another, nothing depends on which workgroup finishes
// first, and no launch reads a location that another workgroup of the same launch may write.  The last one rules out moving
// in place in one launch (the destination of a kept entry lies at or below its source, so inside the source of a lower tile
// that may not have been read yet): the data goes through a bounce buffer in ascending chunks -- gather a chunk's kept items
// into the buffer at their compacted positions, then put the buffer at its destination -- and stream order between the two
// launches is the only synchronisation.  A chunk's destination overlaps only sources that were read before.
//
//   mark      one lane per list element (a 64-bit key of the query calls, or a 64-bit index): a plain store of 1 into the
//             entry's flag word.  Idempotent, so duplicates need no atomic.  The flags were cleared by a memset in front.
//   count     one workgroup per tile of kRemoveTileEntries entries: kept entries of the tile (ballots per wave, the waves' sums
//             through LDS) and the tile's first removed index; one word each per tile, no atomics
//   offsets   ONE workgroup: exclusive scan of the tile counts (tiles + 1 words, the last one the total kept) and the minimum
//             of the tiles' first removed indices, to the head words the host reads
//   map       the count kernel's grid: every entry's new index (tile offset + rank inside the tile), 0xFFFFFFFF for a removed one
//   gather    one lane per entry (every plane, one uint4 each) or per record (two uint4, the entry-index field rewritten for
//             the new index: the place fields stay, the record moves with its entry) of a chunk: kept items to the bounce buffer
//   scatter   one lane per item of the bounce buffer: back to the corpus at the chunk's destination
#include "internal.hpp"

namespace lbad {
namespace {

constexpr uint32_t kRemoveTileEntries = 1024;    // entries per tile = per workgroup of the count and map launches
constexpr uint32_t kRmThreads = 256;
constexpr uint32_t kRmWaves = kRmThreads / 64;
constexpr uint32_t kRmGone = 0xFFFFFFFFu;        // the map's word of a removed entry; "no removed entry" among the first-removed words
static_assert(kRmThreads * 4 == kRemoveTileEntries, "a tile is one 16-byte load of flags per lane");

// kKeys: the list holds keys as the top-K, threshold and join calls write them (index = 0xFFFFFFFF - low word - index_base;
// zero keys and keys outside the corpus are skipped); otherwise indices (outside the corpus: skipped, the host refused them)
template <bool kKeys>
__global__ __launch_bounds__(kRmThreads) void remove_mark_kernel(const unsigned long long* __restrict__ list, uint64_t n_list,
                                                                 uint64_t index_base, uint64_t count, uint32_t* __restrict__ flags) {
    const uint64_t t = (uint64_t)blockIdx.x * kRmThreads + threadIdx.x;
    if (t >= n_list) return;
    const unsigned long long v = list[t];
    uint64_t j = v;
    if (kKeys) {
        if (v == 0ull) return;
        const uint64_t index = 0xFFFFFFFFu - (uint32_t)v;
        if (index < index_base) return;
        j = index - index_base;
    }
    if (j >= count) return;
    flags[j] = 1u;
}

// the four flags of a lane (entries e .. e + 3 of the tile, 16-byte aligned: the flag words are padded to whole tiles) as a
// mask of KEPT entries: bit c = entry e + c exists and is not marked
__device__ __forceinline__ uint32_t rm_kept(const uint32_t* __restrict__ flags, uint64_t e, uint64_t count) {
    const uint4 f = *reinterpret_cast<const uint4*>(flags + e);
    const uint32_t x[4] = {f.x, f.y, f.z, f.w};
    uint32_t m = 0;
#pragma unroll
    for (uint32_t c = 0; c < 4; ++c) m |= (e + c < count && x[c] == 0u ? 1u : 0u) << c;
    return m;
}

__global__ __launch_bounds__(kRmThreads) void remove_count_kernel(const uint32_t* __restrict__ flags, uint64_t count,
                                                                  uint32_t* __restrict__ tile_counts, uint32_t* __restrict__ tile_first) {
    __shared__ uint32_t wsum[kRmWaves], wfirst[kRmWaves];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t e = (uint64_t)blockIdx.x * kRemoveTileEntries + threadIdx.x * 4u;
    const uint32_t kept = rm_kept(flags, e, count);
    uint32_t gone = 0;                           // entries that exist and are marked
#pragma unroll
    for (uint32_t c = 0; c < 4; ++c) gone |= (e + c < count && !((kept >> c) & 1u) ? 1u : 0u) << c;
    uint32_t in_wave = 0;
#pragma unroll
    for (uint32_t c = 0; c < 4; ++c) in_wave += (uint32_t)__popcll(__ballot((kept >> c) & 1u));
    // the wave's first removed entry: the lowest lane with one (a lane's entries lie behind those of the lanes below it)
    const unsigned long long any = __ballot(gone != 0u);
    uint32_t first = kRmGone;
    if (any != 0ull) {
        const uint32_t src = (uint32_t)__ffsll((long long)any) - 1u;
        const uint32_t g = (uint32_t)__shfl((int)gone, (int)src, 64);
        first = (uint32_t)((uint64_t)blockIdx.x * kRemoveTileEntries + (wave * 64u + src) * 4u) + ((uint32_t)__ffs((int)g) - 1u);
    }
    if (lane == 0) { wsum[wave] = in_wave; wfirst[wave] = first; }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t total = 0, f = kRmGone;
#pragma unroll
        for (uint32_t i = 0; i < kRmWaves; ++i) {
            total += wsum[i];
            f = wfirst[i] < f ? wfirst[i] : f;
        }
        tile_counts[blockIdx.x] = total;
        tile_first[blockIdx.x] = f;
    }
}

// head[0]: entries kept, head[1]: the lowest removed index (kRmGone: none); tile_offsets: tiles + 1 words
__global__ __launch_bounds__(kRmThreads) void remove_offsets_kernel(const uint32_t* __restrict__ tile_counts,
                                                                    const uint32_t* __restrict__ tile_first, uint64_t tiles,
                                                                    uint32_t* __restrict__ tile_offsets, uint32_t* __restrict__ head) {
    __shared__ uint32_t wsum[kRmWaves], wfirst[kRmWaves];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t carry = 0, first = kRmGone;
    for (uint64_t c0 = 0; c0 < tiles; c0 += kRmThreads) {
        const uint64_t t = c0 + threadIdx.x;
        const uint32_t cnt = t < tiles ? tile_counts[t] : 0u;
        const uint32_t f = t < tiles ? tile_first[t] : kRmGone;
        first = f < first ? f : first;
        uint32_t incl = cnt;                     // inclusive scan over the wave (all entries of a corpus fit 32 bits)
#pragma unroll
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d, 64);
            if (lane >= d) incl += up;
        }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        uint32_t before = 0, chunk = 0;
#pragma unroll
        for (uint32_t i = 0; i < kRmWaves; ++i) {
            before += i < wave ? wsum[i] : 0u;
            chunk += wsum[i];
        }
        if (t < tiles) tile_offsets[t] = carry + before + (incl - cnt);
        carry += chunk;
        __syncthreads();                         // (wsum is the next chunk's)
    }
#pragma unroll
    for (uint32_t d = 32; d >= 1; d >>= 1) {
        const uint32_t other = (uint32_t)__shfl_xor((int)first, (int)d, 64);
        first = other < first ? other : first;
    }
    if (lane == 0) wfirst[wave] = first;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t f = kRmGone;
#pragma unroll
        for (uint32_t i = 0; i < kRmWaves; ++i) f = wfirst[i] < f ? wfirst[i] : f;
        tile_offsets[tiles] = carry;
        head[0] = carry;
        head[1] = f;
        head[2] = 0u;
        head[3] = 0u;
    }
}

// map: padded to whole tiles like the flags (the words behind the last entry become kRmGone)
__global__ __launch_bounds__(kRmThreads) void remove_map_kernel(const uint32_t* __restrict__ flags, uint64_t count,
                                                                const uint32_t* __restrict__ tile_offsets, uint32_t* __restrict__ map) {
    __shared__ uint32_t wsum[kRmWaves];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t e = (uint64_t)blockIdx.x * kRemoveTileEntries + threadIdx.x * 4u;
    const uint32_t kept = rm_kept(flags, e, count);
    uint32_t below = 0, all = 0;                 // kept entries in the wave's lower lanes / in the whole wave
#pragma unroll
    for (uint32_t c = 0; c < 4; ++c) {
        const unsigned long long b = __ballot((kept >> c) & 1u);
        below = __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, below));
        all += (uint32_t)__popcll(b);
    }
    if (lane == 0) wsum[wave] = all;
    __syncthreads();
    uint32_t at = tile_offsets[blockIdx.x] + below;
#pragma unroll
    for (uint32_t i = 0; i < kRmWaves; ++i) at += i < wave ? wsum[i] : 0u;
    uint32_t out[4];
#pragma unroll
    for (uint32_t c = 0; c < 4; ++c) {
        out[c] = (kept >> c) & 1u ? at : kRmGone;
        at += (kept >> c) & 1u;
    }
    *reinterpret_cast<uint4*>(map + e) = make_uint4(out[0], out[1], out[2], out[3]);
}

// uniform corpus: the kept entries of [e0, e1) to the bounce buffer (plane p at bounce + p * bstride), entry with new index m at
// slot m - base.  Reads the planes and the map, writes only the bounce buffer.
__global__ __launch_bounds__(kRmThreads) void remove_gather_planes_kernel(const uint4* __restrict__ planes, uint64_t stride,
                                                                          uint32_t n_planes, const uint32_t* __restrict__ map,
                                                                          uint64_t e0, uint64_t e1, uint32_t base,
                                                                          uint4* __restrict__ bounce, uint64_t bstride) {
    const uint64_t e = e0 + (uint64_t)blockIdx.x * kRmThreads + threadIdx.x;
    if (e >= e1) return;
    const uint32_t m = map[e];
    if (m == kRmGone) return;
    const uint64_t d = (uint64_t)(m - base);
    if (m < base || d >= bstride) return;        // (cannot happen: a chunk keeps at most its own entries)
    for (uint32_t p = 0; p < n_planes; ++p) bounce[(uint64_t)p * bstride + d] = planes[(uint64_t)p * stride + e];
}

// the first k slots of every plane of the bounce buffer to dst + p * stride + base (a ragged corpus: one "plane" of 2 x records
// uint4).  Reads only the bounce buffer.
__global__ __launch_bounds__(kRmThreads) void remove_scatter_kernel(const uint4* __restrict__ bounce, uint64_t bstride, uint32_t n_planes,
                                                                    uint4* __restrict__ dst, uint64_t stride, uint64_t base, uint64_t k) {
    const uint64_t i = (uint64_t)blockIdx.x * kRmThreads + threadIdx.x;
    if (i >= k) return;
    for (uint32_t p = 0; p < n_planes; ++p) dst[(uint64_t)p * stride + base + i] = bounce[(uint64_t)p * bstride + i];
}

// ragged corpus: the records [r0, r1) of kept entries to the bounce buffer, the record at new position q in slot q - base.  A
// record names its entry (sliding_common.hpp: 28 bits in word 7, 4 in word 3); its new position follows from the entry's old and
// new first record, and the field is rewritten for the new index -- what a fresh build stamps there.
__global__ __launch_bounds__(kRmThreads) void remove_gather_records_kernel(const uint4* __restrict__ recs, const uint32_t* __restrict__ old_off,
                                                                           const uint32_t* __restrict__ new_off,
                                                                           const uint32_t* __restrict__ map, uint64_t n_entries,
                                                                           uint64_t r0, uint64_t r1, uint64_t base,
                                                                           uint4* __restrict__ bounce, uint64_t slots) {
    const uint64_t r = r0 + (uint64_t)blockIdx.x * kRmThreads + threadIdx.x;
    if (r >= r1) return;
    uint4 a = recs[2 * r], b = recs[2 * r + 1];
    const uint32_t ent = (b.w >> 4) | (((a.w >> 17) & 0xFu) << 28);
    if (ent >= n_entries) return;                // (cannot happen: the library stamps every record it stores)
    const uint32_t m = map[ent];
    if (m == kRmGone) return;
    const uint64_t q = (uint64_t)new_off[m] + (r - old_off[ent]);
    if (q < base || q - base >= slots) return;   // (cannot happen: a chunk keeps at most its own records)
    a.w = (a.w & ~(0xFu << 17)) | ((m >> 28) << 17);
    b.w = (b.w & 0xFu) | (m << 4);
    bounce[2 * (q - base)] = a;
    bounce[2 * (q - base) + 1] = b;
}

uint32_t rm_blocks(uint64_t items) { return (uint32_t)((items + kRmThreads - 1) / kRmThreads); }

}  // namespace

uint32_t remove_tile_entries() { return kRemoveTileEntries; }

RemoveIndex remove_index_layout(void* d_block, uint64_t count) {
    const uint64_t tiles = (count + kRemoveTileEntries - 1) / kRemoveTileEntries;
    RemoveIndex ix;
    ix.tiles = tiles;
    const uint64_t map_at = (4 + tiles + 1 + 3) & ~3ull;              // (16-byte aligned: the map and the flags go as uint4)
    if (d_block) {                                                    // (null: only the sizes are wanted)
        ix.head = static_cast<uint32_t*>(d_block);
        ix.tile_offsets = ix.head + 4;
        ix.map = ix.head + map_at;
        ix.flags = ix.map + tiles * kRemoveTileEntries;
        ix.tile_counts = ix.flags + tiles * kRemoveTileEntries;
        ix.tile_first = ix.tile_counts + tiles;
    }
    ix.map_at = map_at;
    ix.words = map_at + 2 * tiles * kRemoveTileEntries + 2 * tiles;
    ix.head_words = 4 + tiles + 1;
    ix.map_words = map_at + count;
    return ix;
}

hipError_t launch_remove_index(const unsigned long long* d_list, uint64_t n_list, bool keys, uint64_t index_base, uint64_t count,
                               const RemoveIndex& ix, hipStream_t stream) {
    if (count == 0 || count > 0xFFFFFFFFull || (n_list + kRmThreads - 1) / kRmThreads > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(ix.flags, 0, (size_t)ix.tiles * kRemoveTileEntries * sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    if (n_list) {
        if (keys)
            hipLaunchKernelGGL(remove_mark_kernel<true>, dim3(rm_blocks(n_list)), dim3(kRmThreads), 0, stream, d_list, n_list, index_base,
                               count, ix.flags);
        else
            hipLaunchKernelGGL(remove_mark_kernel<false>, dim3(rm_blocks(n_list)), dim3(kRmThreads), 0, stream, d_list, n_list, index_base,
                               count, ix.flags);
    }
    const dim3 grid((uint32_t)ix.tiles);
    hipLaunchKernelGGL(remove_count_kernel, grid, dim3(kRmThreads), 0, stream, ix.flags, count, ix.tile_counts, ix.tile_first);
    hipLaunchKernelGGL(remove_offsets_kernel, dim3(1), dim3(kRmThreads), 0, stream, ix.tile_counts, ix.tile_first, ix.tiles,
                       ix.tile_offsets, ix.head);
    hipLaunchKernelGGL(remove_map_kernel, grid, dim3(kRmThreads), 0, stream, ix.flags, count, ix.tile_offsets, ix.map);
    return hipGetLastError();
}

hipError_t launch_remove_gather_planes(const uint4* d_planes, uint64_t stride, uint32_t n_planes, const uint32_t* d_map, uint64_t e0,
                                       uint64_t e1, uint32_t base, uint4* d_bounce, uint64_t bstride, hipStream_t stream) {
    if (e1 <= e0) return hipSuccess;
    hipLaunchKernelGGL(remove_gather_planes_kernel, dim3(rm_blocks(e1 - e0)), dim3(kRmThreads), 0, stream, d_planes, stride, n_planes,
                       d_map, e0, e1, base, d_bounce, bstride);
    return hipGetLastError();
}

hipError_t launch_remove_scatter(const uint4* d_bounce, uint64_t bstride, uint32_t n_planes, uint4* d_dst, uint64_t stride, uint64_t base,
                                 uint64_t k, hipStream_t stream) {
    if (k == 0) return hipSuccess;
    hipLaunchKernelGGL(remove_scatter_kernel, dim3(rm_blocks(k)), dim3(kRmThreads), 0, stream, d_bounce, bstride, n_planes, d_dst, stride,
                       base, k);
    return hipGetLastError();
}

hipError_t launch_remove_gather_records(const uint4* d_recs, const uint32_t* d_old_off, const uint32_t* d_new_off, const uint32_t* d_map,
                                        uint64_t n_entries, uint64_t r0, uint64_t r1, uint64_t base, uint4* d_bounce, uint64_t slots,
                                        hipStream_t stream) {
    if (r1 <= r0) return hipSuccess;
    hipLaunchKernelGGL(remove_gather_records_kernel, dim3(rm_blocks(r1 - r0)), dim3(kRmThreads), 0, stream, d_recs, d_old_off, d_new_off,
                       d_map, n_entries, r0, r1, base, d_bounce, slots);
    return hipGetLastError();
}

}  // namespace lbad
