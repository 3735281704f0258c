// k_gather.hip -- entries handed back out of a corpus on the device: the inverse of pack_planes_kernel (k_compare.hip, uniform
// corpus) and of pack_records_kernel (k_records.hip, ragged corpus), DESIGN.md 4.4h.
//
// A call names entries by the 64-bit keys of the top-K, threshold and join calls (index = 0xFFFFFFFF - low word - index_base; a
// zero key or a key of another entry is an empty row) and receives them in list order in the packed layout (Boolean b at bit
// b & 31 of word b >> 5, eight words per sub-fingerprint), with the rows' offsets beside them.  Count, scan, copy; as in
// k_remove.hip no workgroup ever waits for another and nothing depends on which workgroup finishes first, and here no atomic is
// needed either: every output location has exactly one writer.
//
//   lengths   one lane per key: the row's length in sub-fingerprints (n_sub or the ragged entry's count, 0 for an empty row) as
//             64 bits INTO the caller's offsets array, and one 64-bit sum per tile of kGatherTileKeys keys into the scratch
//   tiles     ONE workgroup: exclusive scan of the tile sums in place; the total to offsets[n_keys]
//   offsets   one workgroup per tile: the tile's lengths -> exclusive prefix sums, in place (a lane reads its own four words and
//             then writes them: no location has a reader in another lane)
//   copy      one lane per output sub-fingerprint, written only where its position is below the capacity.  Uniform: lane t is
//             sub-fingerprint t % n_sub of key t / n_sub, its field of lp bits read out of at most three 16-byte planes.
//             Ragged: lane p finds its row by binary search in the offsets and re-interleaves the record's P and N words.
//             Stores are the coalesced side: consecutive lanes write consecutive 32-byte slots.
#include "internal.hpp"

namespace lbad {
namespace {

constexpr uint32_t kGatherTileKeys = 1024;       // keys per tile = per workgroup of the lengths and offsets launches
constexpr uint32_t kGaThreads = 256;
constexpr uint32_t kGaWaves = kGaThreads / 64;
constexpr uint32_t kGaPerLane = kGatherTileKeys / kGaThreads;      // key c of lane l of tile t: t * tile + c * threads + l
constexpr uint32_t kGaCopyGridMax = 1u << 20;    // most workgroups of a copy launch (its lanes stride over the rest)
constexpr uint64_t kGaNone = ~0ull;
static_assert(kGaThreads * kGaPerLane == kGatherTileKeys, "a tile is a whole number of keys per lane");

// the entry a key names as remove_mark_kernel (k_remove.hip) reads it, kGaNone for an empty row
__device__ __forceinline__ uint64_t ga_entry(unsigned long long key, uint64_t index_base, uint64_t count) {
    if (key == 0ull) return kGaNone;
    const uint64_t index = 0xFFFFFFFFu - (uint32_t)key;
    if (index < index_base) return kGaNone;
    const uint64_t j = index - index_base;
    return j < count ? j : kGaNone;
}

// exclusive prefix sum of v over the workgroup (lane order) and the workgroup's total; wsum: kGaWaves words of LDS, free again
// when the call returns
__device__ __forceinline__ uint64_t ga_block_scan(uint64_t v, unsigned long long* wsum, uint64_t& total) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    unsigned long long incl = v;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const unsigned long long up = __shfl_up(incl, d, 64);
        if (lane >= d) incl += up;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    uint64_t before = 0, all = 0;
#pragma unroll
    for (uint32_t i = 0; i < kGaWaves; ++i) {
        before += i < wave ? wsum[i] : 0ull;
        all += wsum[i];
    }
    __syncthreads();                             // (wsum is the next call's)
    total = all;
    return before + (incl - v);
}

// off: the ragged corpus' record positions (null: uniform, every entry has n_sub sub-fingerprints)
__global__ __launch_bounds__(kGaThreads) void gather_lengths_kernel(const unsigned long long* __restrict__ keys, uint64_t n_keys,
                                                                    uint64_t index_base, uint64_t count,
                                                                    const uint32_t* __restrict__ off, uint32_t n_sub,
                                                                    unsigned long long* __restrict__ lengths,
                                                                    unsigned long long* __restrict__ tile_sums) {
    __shared__ unsigned long long wsum[kGaWaves];
    const uint64_t k0 = (uint64_t)blockIdx.x * kGatherTileKeys + threadIdx.x;
    uint64_t sum = 0;
#pragma unroll
    for (uint32_t c = 0; c < kGaPerLane; ++c) {
        const uint64_t k = k0 + (uint64_t)c * kGaThreads;
        if (k >= n_keys) continue;
        const uint64_t e = ga_entry(keys[k], index_base, count);
        uint64_t len = 0;
        if (e != kGaNone) len = off ? (uint64_t)(off[e + 1] - off[e]) : (uint64_t)n_sub;
        lengths[k] = len;
        sum += len;
    }
#pragma unroll
    for (uint32_t d = 32; d >= 1; d >>= 1) sum += __shfl_xor((unsigned long long)sum, d, 64);
    if ((threadIdx.x & 63u) == 0) wsum[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t total = 0;
#pragma unroll
        for (uint32_t i = 0; i < kGaWaves; ++i) total += wsum[i];
        tile_sums[blockIdx.x] = total;
    }
}

// tile_sums (tiles words): sums -> the sums of the tiles before, in place; *out_total: the sum of all
__global__ __launch_bounds__(kGaThreads) void gather_tiles_kernel(unsigned long long* __restrict__ tile_sums, uint64_t tiles,
                                                                  unsigned long long* __restrict__ out_total) {
    __shared__ unsigned long long wsum[kGaWaves];
    uint64_t carry = 0;
    for (uint64_t c0 = 0; c0 < tiles; c0 += kGaThreads) {
        const uint64_t t = c0 + threadIdx.x;
        const uint64_t v = t < tiles ? tile_sums[t] : 0ull;
        uint64_t chunk;
        const uint64_t before = ga_block_scan(v, wsum, chunk);
        if (t < tiles) tile_sums[t] = carry + before;
        carry += chunk;
    }
    if (threadIdx.x == 0) *out_total = carry;
}

// offsets (n_keys words): lengths -> exclusive prefix sums, in place, tile by tile
__global__ __launch_bounds__(kGaThreads) void gather_offsets_kernel(unsigned long long* __restrict__ offsets, uint64_t n_keys,
                                                                    const unsigned long long* __restrict__ tile_offsets) {
    __shared__ unsigned long long wsum[kGaWaves];
    const uint64_t k0 = (uint64_t)blockIdx.x * kGatherTileKeys + threadIdx.x;
    uint64_t carry = tile_offsets[blockIdx.x];
#pragma unroll
    for (uint32_t c = 0; c < kGaPerLane; ++c) {
        const uint64_t k = k0 + (uint64_t)c * kGaThreads;
        const uint64_t v = k < n_keys ? offsets[k] : 0ull;
        uint64_t chunk;
        const uint64_t before = ga_block_scan(v, wsum, chunk);
        if (k < n_keys) offsets[k] = carry + before;
        carry += chunk;
    }
}

// Uniform corpus.  The stream of entry e is n_sub fields of lp bits (lp = the length rounded up to even), word w of it at
// word w & 3 of planes[(w >> 2) * stride + e].  A field of at most 256 bits at any bit offset touches at most nine words, so
// at most three planes.  items = n_keys * n_sub.
__global__ __launch_bounds__(kGaThreads) void gather_copy_planes_kernel(const uint4* __restrict__ planes, uint64_t stride,
                                                                        uint64_t count, uint32_t n_planes, uint32_t n_sub, uint32_t lp,
                                                                        const unsigned long long* __restrict__ keys, uint64_t items,
                                                                        uint64_t index_base,
                                                                        const unsigned long long* __restrict__ offsets,
                                                                        uint64_t capacity, uint4* __restrict__ out) {
    for (uint64_t t = (uint64_t)blockIdx.x * kGaThreads + threadIdx.x; t < items; t += (uint64_t)gridDim.x * kGaThreads) {
        uint64_t i;
        uint32_t s;
        if (items <= 0xFFFFFFFFull) {            // (the same for every lane: a 32-bit division where it is enough)
            i = (uint32_t)t / n_sub;
            s = (uint32_t)t - (uint32_t)i * n_sub;
        } else {
            i = t / n_sub;
            s = (uint32_t)(t - i * n_sub);
        }
        const uint64_t e = ga_entry(keys[i], index_base, count);
        if (e == kGaNone) continue;
        const uint64_t p = offsets[i] + s;
        if (p >= capacity) continue;
        const uint32_t bit = s * lp;
        const uint32_t w0 = bit >> 5, sh = bit & 31u;
        const uint32_t pl0 = w0 >> 2, pl_last = ((bit + lp - 1u) >> 5) >> 2;
        uint32_t w[12];
#pragma unroll
        for (uint32_t j = 0; j < 3; ++j) {
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (pl0 + j <= pl_last && pl0 + j < n_planes) v = planes[(uint64_t)(pl0 + j) * stride + e];
            w[4 * j] = v.x; w[4 * j + 1] = v.y; w[4 * j + 2] = v.z; w[4 * j + 3] = v.w;
        }
        // the field's first word to place 0: whole words by two masked merges (no register is indexed by a variable), bits by a funnel
        const uint32_t by1 = 0u - (w0 & 1u), by2 = 0u - ((w0 >> 1) & 1u);       // all ones: move by one word / by two words
        uint32_t a[11], b[9], r[8];
#pragma unroll
        for (uint32_t j = 0; j < 11; ++j) a[j] = (w[j + 1] & by1) | (w[j] & ~by1);
#pragma unroll
        for (uint32_t j = 0; j < 9; ++j) b[j] = (a[j + 2] & by2) | (a[j] & ~by2);
#pragma unroll
        for (uint32_t j = 0; j < 8; ++j) {
            uint32_t v = __funnelshift_r(b[j], b[j + 1], sh);
            if (lp <= 32u * j) v = 0u;
            else if (lp - 32u * j < 32u) v &= (1u << (lp - 32u * j)) - 1u;
            r[j] = v;
        }
        out[2 * p] = make_uint4(r[0], r[1], r[2], r[3]);
        out[2 * p + 1] = make_uint4(r[4], r[5], r[6], r[7]);
    }
}

// 16 bits to the even positions of a word: the inverse of even_bits (k_records.hip)
__device__ __forceinline__ uint32_t ga_spread(uint32_t x) {
    x &= 0x0000FFFFu;
    x = (x | (x << 8)) & 0x00FF00FFu;
    x = (x | (x << 4)) & 0x0F0F0F0Fu;
    x = (x | (x << 2)) & 0x33333333u;
    x = (x | (x << 1)) & 0x55555555u;
    return x;
}

// Ragged corpus (the record: sliding_common.hpp).  Output position p belongs to the LAST row r with offsets[r] <= p (empty rows
// make runs of equal offsets); its record is off[entry of key r] + (p - offsets[r]).  pair_mask: the pairs the length has --
// the derived fields above the four pair bits of words 3 and 7 go with it.
__global__ __launch_bounds__(kGaThreads) void gather_copy_records_kernel(const uint4* __restrict__ recs, const uint32_t* __restrict__ off,
                                                                         uint64_t count, const unsigned long long* __restrict__ keys,
                                                                         uint64_t n_keys, uint64_t index_base,
                                                                         const unsigned long long* __restrict__ offsets,
                                                                         uint64_t capacity, uint4 pair_mask, uint4* __restrict__ out) {
    const uint64_t total = offsets[n_keys];
    const uint64_t end = total < capacity ? total : capacity;
    for (uint64_t p = (uint64_t)blockIdx.x * kGaThreads + threadIdx.x; p < end; p += (uint64_t)gridDim.x * kGaThreads) {
        uint64_t lo = 0, hi = n_keys;            // offsets[lo] <= p < offsets[hi] (offsets[0] = 0, offsets[n_keys] = total > p)
        while (hi - lo > 1) {
            const uint64_t mid = (lo + hi) >> 1;
            if (offsets[mid] <= p) lo = mid; else hi = mid;
        }
        const uint64_t e = ga_entry(keys[lo], index_base, count);
        if (e == kGaNone) continue;              // (cannot happen: an empty row holds no position)
        const uint64_t s = p - offsets[lo];
        const uint64_t first = off[e], next = off[e + 1];
        if (s >= next - first) continue;         // (cannot happen: the row is as long as its entry)
        const uint4 a = recs[2 * (first + s)], b = recs[2 * (first + s) + 1];
        const uint32_t P[4] = {a.x & pair_mask.x, a.y & pair_mask.y, a.z & pair_mask.z, a.w & pair_mask.w & 0xFu};
        const uint32_t N[4] = {b.x & pair_mask.x, b.y & pair_mask.y, b.z & pair_mask.z, b.w & pair_mask.w & 0xFu};
        uint32_t r[8];
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            r[2 * k] = ga_spread(P[k]) | (ga_spread(N[k]) << 1);
            r[2 * k + 1] = ga_spread(P[k] >> 16) | (ga_spread(N[k] >> 16) << 1);
        }
        out[2 * p] = make_uint4(r[0], r[1], r[2], r[3]);
        out[2 * p + 1] = make_uint4(r[4], r[5], r[6], r[7]);
    }
}

uint32_t ga_copy_grid(uint64_t items) { return strided_grid((items + kGaThreads - 1) / kGaThreads, kGaCopyGridMax); }

}  // namespace

uint32_t gather_tile_keys() { return kGatherTileKeys; }

size_t gather_scratch_bytes(uint64_t n_keys) { return (size_t)((n_keys + kGatherTileKeys - 1) / kGatherTileKeys) * sizeof(unsigned long long); }

hipError_t launch_gather(const GatherSource& src, const unsigned long long* d_keys, uint64_t n_keys, uint64_t index_base, void* d_scratch,
                         void* d_packed, uint64_t capacity, unsigned long long* d_offsets, hipStream_t stream) {
    if (n_keys == 0 || n_keys > 0x80000000ull || src.count > 0xFFFFFFFFull) return hipErrorInvalidValue;
    const uint64_t tiles = (n_keys + kGatherTileKeys - 1) / kGatherTileKeys;
    unsigned long long* tile_sums = static_cast<unsigned long long*>(d_scratch);
    hipLaunchKernelGGL(gather_lengths_kernel, dim3((uint32_t)tiles), dim3(kGaThreads), 0, stream, d_keys, n_keys, index_base, src.count,
                       src.ragged ? src.off : nullptr, src.n_sub, d_offsets, tile_sums);
    hipLaunchKernelGGL(gather_tiles_kernel, dim3(1), dim3(kGaThreads), 0, stream, tile_sums, tiles, d_offsets + n_keys);
    hipLaunchKernelGGL(gather_offsets_kernel, dim3((uint32_t)tiles), dim3(kGaThreads), 0, stream, d_offsets, n_keys, tile_sums);
    if (capacity != 0 && src.count != 0) {
        uint4* out = static_cast<uint4*>(d_packed);
        if (src.ragged) {
            // positions that can exist: below the capacity and below n_keys rows of the longest entry
            const uint64_t most = n_keys * (uint64_t)src.ne_max;
            const uint32_t pairs = (src.subfp_len + 1u) / 2u;
            uint32_t m[4];
            for (uint32_t k = 0; k < 4; ++k) m[k] = pairs >= 32u * (k + 1u) ? 0xFFFFFFFFu : (pairs > 32u * k ? (1u << (pairs - 32u * k)) - 1u : 0u);
            if (most != 0)
                hipLaunchKernelGGL(gather_copy_records_kernel, dim3(ga_copy_grid(most < capacity ? most : capacity)), dim3(kGaThreads), 0,
                                   stream, src.recs, src.off, src.count, d_keys, n_keys, index_base, d_offsets, capacity,
                                   make_uint4(m[0], m[1], m[2], m[3]), out);
        } else {
            const uint64_t items = n_keys * (uint64_t)src.n_sub;
            hipLaunchKernelGGL(gather_copy_planes_kernel, dim3(ga_copy_grid(items)), dim3(kGaThreads), 0, stream, src.planes, src.stride,
                               src.count, src.n_planes, src.n_sub, src.subfp_len + (src.subfp_len & 1u), d_keys, items, index_base,
                               d_offsets, capacity, out);
        }
    }
    return hipGetLastError();
}

}  // namespace lbad
