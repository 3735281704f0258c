// k_groups.hip -- duplicate groups out of match keys on the device: the connected components of the graph whose edges are the
// keys of a join (CSR rows) or of a threshold batch (pitched rows), and the key list "every entry that is not its group's
// first", DESIGN.md 4.4i.
//
// The labels buffer is a forest: word x is the parent of vertex x, and a parent is BELOW its vertex.  A word that is not below
// its own index makes x a root, whatever it holds.  Every store of the hook pass puts a value below the index it is stored at,
// so (1) a chase  while ((p = parent[x]) < x) x = p;  is a strictly decreasing sequence of indices: it ends within x steps
// under any scheduling and while other workgroups hook; (2) every index read is one that was reached from a vertex below the
// entry count by going down, so every read is in range for ANY content of the buffer; (3) a root only ever becomes a
// non-root, never the reverse, and the root of a tree is the lowest index in it.  As in k_remove.hip and k_gather.hip no
// workgroup ever waits for another, nothing depends on which workgroup finishes first (the components of a graph are a
// function of its edge set), and every loop ends by its own arithmetic.
//
//   init      one lane per vertex: parent[x] = x                                              (only with a reset)
//   hook      one lane per key slot: its row by binary search in the offsets (CSR) or a division (pitched rows), the row's
//             entry and the key's entry, then a lock-free union: find both roots, hang the higher root under the lower one
//             with a compare-and-swap on the higher root's word, and after a lost race go on from the value the winner stored
//   flatten   one lane per vertex: chase to the root, store it as the label; roots counted by ballot, one 64-bit atomic add per
//             workgroup (a sum: its value does not depend on the order)
//
//   extra count / tiles / scatter: the stable compaction of the vertices whose label is not their own index into keys, on the
//             pattern of k_threshold.hip: count per tile, exclusive scan of the tile counts by one workgroup, scatter.
#include "internal.hpp"

namespace lbad {
namespace {

constexpr uint32_t kGrThreads = 256;
constexpr uint32_t kGrWaves = kGrThreads / 64;
constexpr uint32_t kGrGridMax = 1u << 16;        // most workgroups of a launch over slots or vertices (lanes stride over the rest)
constexpr uint32_t kGrTile = 1024;               // vertices per tile of the extra-key launches
constexpr uint32_t kGrPerLane = kGrTile / kGrThreads;
constexpr unsigned long long kGrScoreOne = 0x3F800000ull << 32;    // the bits of 1.0f in the score word
static_assert(kGrThreads * kGrPerLane == kGrTile, "a tile is a whole number of vertices per lane");

__device__ __forceinline__ uint32_t gr_load(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the entry a key names, read as ga_entry (k_gather.hip) reads it; false for a zero key and for a key of another index range.
// count <= 2^32: every entry fits 32 bits, and no value of them is left over to mean "none"
__device__ __forceinline__ bool gr_entry(unsigned long long key, uint64_t index_base, uint64_t count, uint32_t& entry) {
    if (key == 0ull) return false;
    const uint64_t index = 0xFFFFFFFFu - (uint32_t)key;
    if (index < index_base) return false;
    const uint64_t j = index - index_base;
    if (j >= count) return false;
    entry = (uint32_t)j;
    return true;
}

// the root above x: a strictly decreasing chase, at most x steps
__device__ __forceinline__ uint32_t gr_find(const uint32_t* parent, uint32_t x) {
    uint32_t p;
    while ((p = gr_load(parent + x)) < x) x = p;
    return x;
}

// a and b into one tree.  Every pass of the loop either ends it or lowers hi: the loop makes at most max(a, b) + 1 passes.
__device__ __forceinline__ void gr_union(uint32_t* parent, uint32_t a, uint32_t b) {
    uint32_t u = gr_find(parent, a), v = gr_find(parent, b);
    while (u != v) {
        const uint32_t hi = u > v ? u : v, lo = u > v ? v : u;
        const uint32_t seen = gr_load(parent + hi);
        uint32_t now = seen;
        if (seen >= hi) {                        // still a root: hang it under lo (lo < hi: the store keeps the forest's rule)
            now = atomicCAS(parent + hi, seen, lo);
            if (now == seen) return;
            if (now >= hi) return;               // (no store of this file does that: the buffer is written from elsewhere)
        }
        // hi has a parent below it now: somebody else's hook.  Go on from there; lo's side may have been hooked as well
        u = gr_find(parent, now);
        v = gr_find(parent, lo);
    }
}

__global__ __launch_bounds__(kGrThreads) void groups_init_kernel(uint32_t* __restrict__ parent, uint64_t n) {
    for (uint64_t x = (uint64_t)blockIdx.x * kGrThreads + threadIdx.x; x < n; x += (uint64_t)gridDim.x * kGrThreads) parent[x] = (uint32_t)x;
}

// offsets: n_rows + 1 words (CSR) or null (rows of `pitch` slots).  row_keys: the rows' entries as keys, or null (row r is
// entry first_row + r, and first_row + n_rows <= n: the host has checked it).  n_slots <= 2^31, pitch <= 2^31.
__global__ __launch_bounds__(kGrThreads) void groups_hook_kernel(const unsigned long long* __restrict__ keys, uint64_t n_slots,
                                                                 const unsigned long long* __restrict__ offsets, uint32_t pitch,
                                                                 uint64_t n_rows, uint64_t first_row,
                                                                 const unsigned long long* __restrict__ row_keys, uint64_t index_base,
                                                                 uint64_t n, uint32_t* parent) {
    uint64_t end = n_slots;
    if (offsets) {
        const uint64_t total = offsets[n_rows];
        end = total < end ? total : end;
    }
    for (uint64_t p = (uint64_t)blockIdx.x * kGrThreads + threadIdx.x; p < end; p += (uint64_t)gridDim.x * kGrThreads) {
        uint32_t b;
        if (!gr_entry(keys[p], index_base, n, b)) continue;
        uint64_t r;
        if (offsets) {
            if (offsets[0] > p) continue;        // (in front of the first row)
            uint64_t lo = 0, hi = n_rows;        // offsets[lo] <= p < offsets[hi]; mid stays inside [0, n_rows] whatever they hold
            while (hi - lo > 1) {
                const uint64_t mid = (lo + hi) >> 1;
                if (offsets[mid] <= p) lo = mid; else hi = mid;
            }
            r = lo;
        } else {
            r = (uint32_t)p / pitch;
        }
        if (r >= n_rows) continue;
        uint32_t a;
        if (row_keys) {
            if (!gr_entry(row_keys[r], index_base, n, a)) continue;
        } else {
            a = (uint32_t)(first_row + r);
        }
        if (a != b) gr_union(parent, a, b);
    }
}

// parent -> labels in place.  A store puts the root of x at x: below x and in x's tree, so a chase that runs beside it still
// goes down and still ends at the same root; a root's word becomes its own index.
__global__ __launch_bounds__(kGrThreads) void groups_flatten_kernel(uint32_t* parent, uint64_t n, unsigned long long* __restrict__ group_count) {
    __shared__ unsigned long long wtot[kGrWaves];
    const uint64_t step = (uint64_t)gridDim.x * kGrThreads;
    const uint64_t x0 = (uint64_t)blockIdx.x * kGrThreads + threadIdx.x;
    const uint64_t passes = (n + step - 1) / step;       // the same for every lane: the ballot below has all lanes of a wave
    unsigned long long mine = 0;                         // the roots this wave has seen (in every lane of it)
    for (uint64_t i = 0; i < passes; ++i) {
        const uint64_t x = x0 + i * step;
        bool root = false;
        if (x < n) {
            const uint32_t r = gr_find(parent, (uint32_t)x);
            root = r == (uint32_t)x;
            parent[x] = r;
        }
        mine += (unsigned long long)__popcll(__ballot(root));
    }
    if ((threadIdx.x & 63u) == 0) wtot[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0 && group_count) {
        unsigned long long total = 0;
#pragma unroll
        for (uint32_t w = 0; w < kGrWaves; ++w) total += wtot[w];
        if (total) atomicAdd(group_count, total);
    }
}

// ---- the extra keys ----

__device__ __forceinline__ bool gr_extra(const uint32_t* __restrict__ labels, uint64_t x, uint64_t n) { return x < n && labels[x] != (uint32_t)x; }

__global__ __launch_bounds__(kGrThreads) void groups_extra_count_kernel(const uint32_t* __restrict__ labels, uint64_t n,
                                                                        unsigned long long* __restrict__ tile_counts) {
    __shared__ uint32_t wsum[kGrWaves];
    const uint64_t x0 = (uint64_t)blockIdx.x * kGrTile + threadIdx.x;
    uint32_t c = 0;
#pragma unroll
    for (uint32_t k = 0; k < kGrPerLane; ++k) c += gr_extra(labels, x0 + (uint64_t)k * kGrThreads, n) ? 1u : 0u;
#pragma unroll
    for (uint32_t d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d, 64);
    if ((threadIdx.x & 63u) == 0) wsum[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t total = 0;
#pragma unroll
        for (uint32_t w = 0; w < kGrWaves; ++w) total += wsum[w];
        tile_counts[blockIdx.x] = total;
    }
}

// exclusive prefix sum of v over the workgroup (lane order) and the workgroup's total; wsum: kGrWaves words of LDS, free again
// when the call returns
__device__ __forceinline__ uint64_t gr_block_scan(uint64_t v, unsigned long long* wsum, uint64_t& total) {
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
    for (uint32_t i = 0; i < kGrWaves; ++i) {
        before += i < wave ? wsum[i] : 0ull;
        all += wsum[i];
    }
    __syncthreads();                             // (wsum is the next call's)
    total = all;
    return before + (incl - v);
}

// tile_counts (tiles words): counts -> the counts of the tiles before, in place; tile_counts[tiles]: the sum of all
__global__ __launch_bounds__(kGrThreads) void groups_extra_tiles_kernel(unsigned long long* __restrict__ tile_counts, uint64_t tiles) {
    __shared__ unsigned long long wsum[kGrWaves];
    uint64_t carry = 0;
    for (uint64_t c0 = 0; c0 < tiles; c0 += kGrThreads) {
        const uint64_t t = c0 + threadIdx.x;
        const uint64_t v = t < tiles ? tile_counts[t] : 0ull;
        uint64_t chunk;
        const uint64_t before = gr_block_scan(v, wsum, chunk);
        if (t < tiles) tile_counts[t] = carry + before;
        carry += chunk;
    }
    if (threadIdx.x == 0) tile_counts[tiles] = carry;
}

// one workgroup per tile: vertex k * threads + lane of the tile, k ascending, so positions ascend with the index.  Only
// positions below the capacity are written (the slots behind the keys are zero already)
__global__ __launch_bounds__(kGrThreads) void groups_extra_scatter_kernel(const uint32_t* __restrict__ labels, uint64_t n,
                                                                          uint64_t index_base,
                                                                          const unsigned long long* __restrict__ tile_offsets,
                                                                          uint64_t capacity, unsigned long long* __restrict__ out) {
    __shared__ unsigned long long wsum[kGrWaves];
    const uint64_t x0 = (uint64_t)blockIdx.x * kGrTile + threadIdx.x;
    uint64_t carry = tile_offsets[blockIdx.x];
#pragma unroll
    for (uint32_t k = 0; k < kGrPerLane; ++k) {
        const uint64_t x = x0 + (uint64_t)k * kGrThreads;
        const bool extra = gr_extra(labels, x, n);
        uint64_t chunk;
        const uint64_t pos = carry + gr_block_scan(extra ? 1ull : 0ull, wsum, chunk);
        if (extra && pos < capacity) out[pos] = kGrScoreOne | (unsigned long long)(0xFFFFFFFFu - (uint32_t)(index_base + x));
        carry += chunk;
    }
}

uint32_t gr_grid(uint64_t items) { return strided_grid((items + kGrThreads - 1) / kGrThreads, kGrGridMax); }

}  // namespace

hipError_t launch_group_labels(const unsigned long long* d_keys, uint64_t n_slots, const unsigned long long* d_offsets, uint64_t pitch,
                               uint64_t n_rows, uint64_t first_row, const unsigned long long* d_row_keys, uint64_t index_base, uint64_t n,
                               bool reset, uint32_t* d_labels, unsigned long long* d_group_count, hipStream_t stream) {
    if (n == 0 || n > 0x100000000ull || n_slots > 0x80000000ull || index_base + n > 0x100000000ull) return hipErrorInvalidValue;
    if (!d_offsets && n_slots != 0 && (pitch == 0 || pitch > 0x80000000ull)) return hipErrorInvalidValue;
    if (!d_row_keys && first_row + n_rows > n) return hipErrorInvalidValue;
    if (reset) hipLaunchKernelGGL(groups_init_kernel, dim3(gr_grid(n)), dim3(kGrThreads), 0, stream, d_labels, n);
    if (n_slots != 0 && n_rows != 0)
        hipLaunchKernelGGL(groups_hook_kernel, dim3(gr_grid(n_slots)), dim3(kGrThreads), 0, stream, d_keys, n_slots, d_offsets, (uint32_t)pitch,
                           n_rows, first_row, d_row_keys, index_base, n, d_labels);
    hipLaunchKernelGGL(groups_flatten_kernel, dim3(gr_grid(n)), dim3(kGrThreads), 0, stream, d_labels, n, d_group_count);
    return hipGetLastError();
}

size_t group_extra_scratch_bytes(uint64_t n) { return (size_t)((n + kGrTile - 1) / kGrTile + 1) * sizeof(unsigned long long); }

hipError_t launch_group_extra_keys(const uint32_t* d_labels, uint64_t n, uint64_t index_base, uint64_t capacity, void* d_scratch,
                                   unsigned long long* d_keys, hipStream_t stream) {
    if (n == 0 || n > 0x100000000ull || index_base + n > 0x100000000ull || capacity == 0) return hipErrorInvalidValue;
    const uint64_t tiles = (n + kGrTile - 1) / kGrTile;
    unsigned long long* tile_counts = static_cast<unsigned long long*>(d_scratch);
    hipLaunchKernelGGL(groups_extra_count_kernel, dim3((uint32_t)tiles), dim3(kGrThreads), 0, stream, d_labels, n, tile_counts);
    hipLaunchKernelGGL(groups_extra_tiles_kernel, dim3(1), dim3(kGrThreads), 0, stream, tile_counts, tiles);
    hipLaunchKernelGGL(groups_extra_scatter_kernel, dim3((uint32_t)tiles), dim3(kGrThreads), 0, stream, d_labels, n, index_base, tile_counts,
                       capacity, d_keys);
    return hipGetLastError();
}

}  // namespace lbad
