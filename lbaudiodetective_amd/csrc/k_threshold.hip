// k_threshold.hip -- every score of a row that reaches a threshold, compacted on the device (corpus threshold queries).
//
// Top-K ranks; a detection service asks which entries match at all.  Per row of n float32 scores and a threshold t > 0 the
// entries e with score >= t (a float compare: NaN never matches) become the 64-bit keys of the other queries,
//   key = (float bits of score << 32) | (0xFFFFFFFF - (index_base + e)),
// in ASCENDING entry index (a stable compaction), the first min(count, capacity) of them at keys + row * capacity, zero keys
// behind them, and the true count -- also when the list was cut -- in counts[row].  Three launches per group of rows, and no
// workgroup ever waits for another one:
//
//   count     grid = tiles x rows (grid-stride above kThMaxGrid workgroups): a workgroup counts the matches of one tile of
//             kThTile consecutive scores -- 16-byte loads, ballots per wave, the waves' sums through LDS -- and writes one
//             word per (row, tile).  No atomics.
//   offsets   one workgroup per row: exclusive scan of the row's tile counts in chunks of kThChunk with a 64-bit carry;
//             the tile offsets as 64 bits, the row total to counts[row]
//   scatter   the count kernel's grid: a tile without a match returns after reading its one word; otherwise the tile is read
//             again, every match's rank inside the tile follows from the ballots of its wave (matches in lower lanes, the
//             lane's own earlier components) and the waves' sums, and its key goes to slot offset + rank where that is below
//             the capacity.  Plain vector stores.
//
// The slots behind the matches are zeroed by a hipMemsetAsync of the key rows in front of the three launches.
//
// A row starts at scores + row * n, which is 16-byte aligned only by luck.  The tiles are therefore laid over the row from the
// 16-byte boundary at or below its first score: "virtual" position v = e + a with a = floats between that boundary and the
// row (0 .. 3).  A lane's four floats are one aligned 16-byte load where all four lie inside the row, 4-byte loads of the ones
// inside otherwise (the first and the last vector of a row); nothing outside the row is read.
#include "internal.hpp"

namespace lbad {
namespace {

constexpr uint32_t kThTile = 4096;           // scores per tile = per workgroup and step
constexpr uint32_t kThThreads = 256;
constexpr uint32_t kThWaves = kThThreads / 64;
constexpr uint32_t kThVecs = kThTile / (kThThreads * 4);     // 16-byte loads per lane and tile
constexpr uint32_t kThMaxGrid = 2048;        // workgroups of the count / scatter launches: 256 CUs x 8 resident ones
constexpr uint32_t kThPer = 4;               // tile counts per thread and chunk of the offsets scan
constexpr uint32_t kThChunk = kThThreads * kThPer;
static_assert(kThVecs * kThThreads * 4 == kThTile, "a tile is a whole number of 16-byte loads per lane");

// one row as the count and scatter kernels walk it
struct ThRow {
    const float* base;       // the 16-byte boundary at or below the row's first score
    uint32_t a;              // floats between base and the row
    uint64_t end;            // a + n: first virtual position behind the row
};

__device__ __forceinline__ ThRow th_row(const float* scores, uint64_t n, uint32_t row) {
    const float* r = scores + (size_t)row * n;
    ThRow o;
    o.a = (uint32_t)((reinterpret_cast<uintptr_t>(r) >> 2) & 3u);
    o.base = r - o.a;
    o.end = n + o.a;
    return o;
}

// the four floats at virtual position v (a multiple of 4) and which of them match: bit c = component c is inside the row
// and >= t.  A component outside the row reads nothing.
__device__ __forceinline__ uint32_t th_load(const ThRow& r, uint64_t v, float t, float (&x)[4]) {
    if (v >= r.a && v + 4 <= r.end) {
        const float4 f = *reinterpret_cast<const float4*>(r.base + v);
        x[0] = f.x; x[1] = f.y; x[2] = f.z; x[3] = f.w;
    } else {
#pragma unroll
        for (uint32_t c = 0; c < 4; ++c) x[c] = (v + c >= r.a && v + c < r.end) ? r.base[v + c] : -1.0f;     // (t > 0: -1 never matches)
    }
    uint32_t m = 0;
#pragma unroll
    for (uint32_t c = 0; c < 4; ++c) m |= (x[c] >= t ? 1u : 0u) << c;
    return m;
}

// wave `wave` of a workgroup owns kThVecs x 256 consecutive positions of the tile; vector j of lane l starts at
__device__ __forceinline__ uint64_t th_pos(uint64_t tile, uint32_t wave, uint32_t j, uint32_t lane) {
    return tile * kThTile + (uint64_t)((wave * kThVecs + j) * 256u + lane * 4u);
}

__global__ __launch_bounds__(kThThreads) void threshold_count_kernel(const float* __restrict__ scores, uint64_t n, uint32_t rows,
                                                                     uint64_t tiles, float t, uint32_t* __restrict__ tile_counts) {
    __shared__ uint32_t wsum[kThWaves];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t items = tiles * rows;
    for (uint64_t w = blockIdx.x; w < items; w += gridDim.x) {
        const uint32_t row = (uint32_t)(w / tiles);
        const uint64_t tile = w - (uint64_t)row * tiles;
        const ThRow r = th_row(scores, n, row);
        uint32_t in_wave = 0;                  // the wave's matches: one ballot per component of every vector (scalar adds)
#pragma unroll
        for (uint32_t j = 0; j < kThVecs; ++j) {
            float x[4];
            const uint32_t m = th_load(r, th_pos(tile, wave, j, lane), t, x);
#pragma unroll
            for (uint32_t c = 0; c < 4; ++c) in_wave += (uint32_t)__popcll(__ballot((m >> c) & 1u));
        }
        if (lane == 0) wsum[wave] = in_wave;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t total = 0;
#pragma unroll
            for (uint32_t i = 0; i < kThWaves; ++i) total += wsum[i];
            tile_counts[w] = total;
        }
        __syncthreads();                       // (wsum is the next item's)
    }
}

__global__ __launch_bounds__(kThThreads) void threshold_offsets_kernel(const uint32_t* __restrict__ tile_counts, uint64_t tiles,
                                                                       unsigned long long* __restrict__ tile_offsets,
                                                                       unsigned long long* __restrict__ row_counts) {
    __shared__ uint32_t wsum[kThWaves];
    const uint32_t row = blockIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t* cnt = tile_counts + (size_t)row * tiles;
    unsigned long long* off = tile_offsets + (size_t)row * tiles;
    unsigned long long carry = 0ull;
    for (uint64_t c0 = 0; c0 < tiles; c0 += kThChunk) {
        const uint64_t first = c0 + (uint64_t)threadIdx.x * kThPer;
        uint32_t c[kThPer], sum = 0;
#pragma unroll
        for (uint32_t j = 0; j < kThPer; ++j) {
            c[j] = first + j < tiles ? cnt[first + j] : 0u;
            sum += c[j];
        }
        uint32_t incl = sum;                   // inclusive scan over the wave (a chunk holds at most 2^22 matches)
#pragma unroll
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d, 64);
            if (lane >= d) incl += up;
        }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        uint32_t before = 0, chunk = 0;
#pragma unroll
        for (uint32_t i = 0; i < kThWaves; ++i) {
            before += i < wave ? wsum[i] : 0u;
            chunk += wsum[i];
        }
        unsigned long long at = carry + before + (incl - sum);
#pragma unroll
        for (uint32_t j = 0; j < kThPer; ++j) {
            if (first + j < tiles) off[first + j] = at;
            at += c[j];
        }
        carry += chunk;
        __syncthreads();                       // (wsum is the next chunk's)
    }
    if (threadIdx.x == 0) row_counts[row] = carry;
}

__global__ __launch_bounds__(kThThreads) void threshold_scatter_kernel(const float* __restrict__ scores, uint64_t n, uint32_t rows,
                                                                       uint64_t tiles, float t, uint64_t capacity, uint64_t index_base,
                                                                       const uint32_t* __restrict__ tile_counts,
                                                                       const unsigned long long* __restrict__ tile_offsets,
                                                                       unsigned long long* __restrict__ keys) {
    __shared__ uint32_t wsum[kThWaves];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t items = tiles * rows;
    for (uint64_t w = blockIdx.x; w < items; w += gridDim.x) {
        if (tile_counts[w] == 0u) continue;                     // (the same word for the whole workgroup)
        const unsigned long long tile_at = tile_offsets[w];
        if (tile_at >= capacity) continue;                      // the list is full in front of this tile
        const uint32_t row = (uint32_t)(w / tiles);
        const uint64_t tile = w - (uint64_t)row * tiles;
        const ThRow r = th_row(scores, n, row);
        float x[kThVecs][4];
        uint32_t m[kThVecs], rank[kThVecs], in_wave = 0;
#pragma unroll
        for (uint32_t j = 0; j < kThVecs; ++j) {
            m[j] = th_load(r, th_pos(tile, wave, j, lane), t, x[j]);
            // matches of this vector in lower lanes (the four component ballots under the mask of lower lanes) ...
            uint32_t below = 0, all = 0;
#pragma unroll
            for (uint32_t c = 0; c < 4; ++c) {
                const unsigned long long b = __ballot((m[j] >> c) & 1u);
                below = __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, below));
                all += (uint32_t)__popcll(b);
            }
            rank[j] = in_wave + below;                          // ... behind the wave's earlier vectors
            in_wave += all;
        }
        if (lane == 0) wsum[wave] = in_wave;
        __syncthreads();
        uint32_t before = 0;
#pragma unroll
        for (uint32_t i = 0; i < kThWaves; ++i) before += i < wave ? wsum[i] : 0u;
        unsigned long long* out = keys + (size_t)row * capacity;
#pragma unroll
        for (uint32_t j = 0; j < kThVecs; ++j) {
            const uint64_t e = th_pos(tile, wave, j, lane) - r.a;      // (only read where a component matched: inside the row)
            unsigned long long slot = tile_at + before + rank[j];
#pragma unroll
            for (uint32_t c = 0; c < 4; ++c) {
                if ((m[j] >> c) & 1u) {
                    if (slot < capacity)
                        out[slot] = ((unsigned long long)__float_as_uint(x[j][c]) << 32) |
                                    (unsigned long long)(0xFFFFFFFFu - (uint32_t)(index_base + e + c));
                    ++slot;
                }
            }
        }
        __syncthreads();                       // (wsum is the next item's)
    }
}

// tiles that cover a row of n scores wherever it starts (up to three floats in front of it, see above)
uint64_t th_tiles(uint64_t n) { return (n + 3 + kThTile - 1) / kThTile; }

}  // namespace

size_t threshold_scratch_bytes(uint64_t n, uint32_t rows) {
    return (size_t)rows * th_tiles(n) * (sizeof(unsigned long long) + sizeof(uint32_t));
}

hipError_t launch_threshold_keys(const float* d_scores, uint64_t n, uint32_t rows, float threshold, uint64_t capacity,
                                 uint64_t index_base, void* d_scratch, unsigned long long* d_keys, unsigned long long* d_counts,
                                 hipStream_t stream) {
    if (rows == 0) return hipSuccess;
    if (!(threshold > 0.0f) || capacity == 0 || rows > kThresholdRowsMax || n > 0x100000000ull || index_base + n > 0x100000000ull ||
        (reinterpret_cast<uintptr_t>(d_scores) & 3u))
        return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(d_keys, 0, (size_t)rows * capacity * sizeof(unsigned long long), stream);
    if (e != hipSuccess) return e;
    if (n == 0) return hipMemsetAsync(d_counts, 0, (size_t)rows * sizeof(unsigned long long), stream);
    const uint64_t tiles = th_tiles(n), items = tiles * rows;
    unsigned long long* offsets = static_cast<unsigned long long*>(d_scratch);
    uint32_t* counts = reinterpret_cast<uint32_t*>(offsets + items);
    const dim3 grid(strided_grid(items, kThMaxGrid));
    hipLaunchKernelGGL(threshold_count_kernel, grid, dim3(kThThreads), 0, stream, d_scores, n, rows, tiles, threshold, counts);
    hipLaunchKernelGGL(threshold_offsets_kernel, dim3(rows), dim3(kThThreads), 0, stream, counts, tiles, offsets, d_counts);
    hipLaunchKernelGGL(threshold_scatter_kernel, grid, dim3(kThThreads), 0, stream, d_scores, n, rows, tiles, threshold, capacity,
                       index_base, counts, offsets, d_keys);
    return hipGetLastError();
}

}  // namespace lbad
