// k_ids.hip -- the caller's 64-bit ids of corpus entries on the device, DESIGN.md 4.4q.
//
// A corpus with ids holds one UInt64 per entry of its capacity (0: no id; the words at and above the count are zero).  Keys name
// entries by position (index = 0xFFFFFFFF - low word - index_base, as remove_mark_kernel and ga_entry read them); the kernels
// here go from keys to ids, from ids back to keys, and move the ids with their entries when a removal closes the corpus up.
// Every launch is a plain grid-stride loop over its items (grids from strided_grid); as in k_remove.hip no workgroup ever waits
// for another, and no launch but the insert reads what another workgroup of the same launch may write -- the insert meets the
// other workgroups only through atomics whose outcome does not depend on their order.
//
//   ids_from_keys   one lane per key: the id of the entry the key names, 0 for a zero key or a key of another entry
//   index init      one lane per slot of the id index: id word 0 (empty), index word 0xFFFFFFFF
//   index insert    one lane per entry with a non-zero id: linear probe from mix(id) & (slots - 1); an empty id word is claimed
//                   with a 64-bit atomicCAS, and on its own or an equal id the entry's index goes into the index word with
//                   atomicMin.  An id owns exactly ONE slot (a slot once taken stays taken, so every lane with that id walks the
//                   same taken slots up to it) and its index word ends as the LOWEST index with that id: the table as a lookup
//                   function is a function of the set of (id, index) pairs alone, whatever the grid or the order of the lanes.
//   keys_from_ids   one lane per id: the same probe, read only, until an equal id (its key) or an empty slot (a zero key)
//   compact gather  one lane per old entry from the lowest removed index on: a kept entry's id to the scratch at its new index
//   compact scatter one lane per word from the lowest removed index to the OLD count: the scratch's word, 0 from the new count on
//
// Every probe loop counts its steps and ends after `slots` of them by its own arithmetic, whatever the table holds; with
// slots >= 2 x entries a probe of a table the insert built ends at an empty slot long before.
#include "internal.hpp"

namespace lbad {
namespace {

constexpr uint32_t kIdThreads = 256;
constexpr uint32_t kIdGridMax = 1u << 16;        // most workgroups of a launch (its lanes stride over the rest)
constexpr uint64_t kIdMinSlots = 1024;
constexpr uint32_t kIdNone = 0xFFFFFFFFu;        // the index word of an empty slot; the removal's map word of a removed entry
constexpr unsigned long long kIdScoreOne = 0x3F800000ull << 32;      // the bits of 1.0f: a key is never zero by accident

// splitmix64's finaliser: every input bit reaches every output bit, so sequential ids and multiples of a power of two -- a
// catalogue's normal ids -- spread over the low bits the table uses
__device__ __forceinline__ uint64_t id_mix(uint64_t x) {
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}

// ids: null for a corpus without ids (every word of out is 0)
__global__ __launch_bounds__(kIdThreads) void ids_from_keys_kernel(const unsigned long long* __restrict__ keys, uint64_t n,
                                                                   uint64_t index_base, uint64_t count,
                                                                   const unsigned long long* __restrict__ ids,
                                                                   unsigned long long* __restrict__ out) {
    for (uint64_t i = (uint64_t)blockIdx.x * kIdThreads + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kIdThreads) {
        const unsigned long long key = keys[i];
        unsigned long long id = 0ull;
        if (key != 0ull && ids != nullptr) {
            const uint64_t index = 0xFFFFFFFFu - (uint32_t)key;
            if (index >= index_base && index - index_base < count) id = ids[index - index_base];
        }
        out[i] = id;
    }
}

__global__ __launch_bounds__(kIdThreads) void ids_index_init_kernel(unsigned long long* __restrict__ slot_ids,
                                                                    uint32_t* __restrict__ slot_index, uint64_t slots) {
    for (uint64_t s = (uint64_t)blockIdx.x * kIdThreads + threadIdx.x; s < slots; s += (uint64_t)gridDim.x * kIdThreads) {
        slot_ids[s] = 0ull;
        slot_index[s] = kIdNone;
    }
}

__global__ __launch_bounds__(kIdThreads) void ids_index_insert_kernel(const unsigned long long* __restrict__ ids, uint64_t count,
                                                                      unsigned long long* __restrict__ slot_ids,
                                                                      uint32_t* __restrict__ slot_index, uint64_t slots) {
    const uint64_t mask = slots - 1;
    for (uint64_t e = (uint64_t)blockIdx.x * kIdThreads + threadIdx.x; e < count; e += (uint64_t)gridDim.x * kIdThreads) {
        const unsigned long long id = ids[e];
        if (id == 0ull) continue;
        uint64_t s = id_mix(id) & mask;
        for (uint64_t step = 0; step < slots; ++step) {
            const unsigned long long seen = atomicCAS(&slot_ids[s], 0ull, id);
            if (seen == 0ull || seen == id) {
                atomicMin(&slot_index[s], (uint32_t)e);
                break;
            }
            s = (s + 1) & mask;
        }
    }
}

__global__ __launch_bounds__(kIdThreads) void keys_from_ids_kernel(const unsigned long long* __restrict__ list, uint64_t n,
                                                                   uint64_t index_base, uint64_t count,
                                                                   const unsigned long long* __restrict__ slot_ids,
                                                                   const uint32_t* __restrict__ slot_index, uint64_t slots,
                                                                   unsigned long long* __restrict__ out) {
    const uint64_t mask = slots - 1;
    for (uint64_t i = (uint64_t)blockIdx.x * kIdThreads + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kIdThreads) {
        const unsigned long long id = list[i];
        unsigned long long key = 0ull;
        if (id != 0ull && slot_ids != nullptr) {
            uint64_t s = id_mix(id) & mask;
            for (uint64_t step = 0; step < slots; ++step) {
                const unsigned long long seen = slot_ids[s];
                if (seen == id) {
                    const uint32_t index = slot_index[s];
                    if (index < count) key = kIdScoreOne | (unsigned long long)(0xFFFFFFFFu - (uint32_t)(index_base + index));
                    break;
                }
                if (seen == 0ull) break;
                s = (s + 1) & mask;
            }
        }
        out[i] = key;
    }
}

// old entries [first, count): a kept entry's id to scratch[new index - first] (a kept entry at or above the lowest removed
// index lands at or above it).  Reads the ids and the map, writes only the scratch.
__global__ __launch_bounds__(kIdThreads) void ids_compact_gather_kernel(const unsigned long long* __restrict__ ids,
                                                                        const uint32_t* __restrict__ map, uint64_t first, uint64_t count,
                                                                        unsigned long long* __restrict__ scratch, uint64_t n_scratch) {
    const uint64_t n = count - first;
    for (uint64_t i = (uint64_t)blockIdx.x * kIdThreads + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kIdThreads) {
        const uint32_t m = map[first + i];
        if (m == kIdNone || m < first) continue;     // (m < first cannot happen)
        const uint64_t d = (uint64_t)m - first;
        if (d >= n_scratch) continue;                // (cannot happen: at most count - first entries are kept)
        scratch[d] = ids[first + i];
    }
}

// ids[first + i] for i < count - first: the scratch's word below kept - first, 0 behind it.  Reads only the scratch.
__global__ __launch_bounds__(kIdThreads) void ids_compact_scatter_kernel(const unsigned long long* __restrict__ scratch, uint64_t first,
                                                                         uint64_t kept, uint64_t count,
                                                                         unsigned long long* __restrict__ ids) {
    const uint64_t n = count - first, live = kept - first;
    for (uint64_t i = (uint64_t)blockIdx.x * kIdThreads + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kIdThreads)
        ids[first + i] = i < live ? scratch[i] : 0ull;
}

uint32_t id_grid(uint64_t items) { return strided_grid((items + kIdThreads - 1) / kIdThreads, kIdGridMax); }

}  // namespace

uint64_t ids_index_slots(uint64_t count) {
    uint64_t slots = kIdMinSlots;
    while (slots < 2 * count) slots <<= 1;
    return slots;
}

hipError_t launch_ids_from_keys(const unsigned long long* d_keys, uint64_t n, uint64_t index_base, uint64_t count,
                                const unsigned long long* d_ids, unsigned long long* d_out, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (n > 0x80000000ull || index_base + count > 0x100000000ull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ids_from_keys_kernel, dim3(id_grid(n)), dim3(kIdThreads), 0, stream, d_keys, n, index_base, count, d_ids, d_out);
    return hipGetLastError();
}

hipError_t launch_ids_index_build(const unsigned long long* d_ids, uint64_t count, unsigned long long* d_slot_ids,
                                  uint32_t* d_slot_index, uint64_t slots, hipStream_t stream) {
    if (slots < kIdMinSlots || (slots & (slots - 1)) != 0 || slots < 2 * count || count > 0xFFFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ids_index_init_kernel, dim3(id_grid(slots)), dim3(kIdThreads), 0, stream, d_slot_ids, d_slot_index, slots);
    if (count)
        hipLaunchKernelGGL(ids_index_insert_kernel, dim3(id_grid(count)), dim3(kIdThreads), 0, stream, d_ids, count, d_slot_ids,
                           d_slot_index, slots);
    return hipGetLastError();
}

hipError_t launch_keys_from_ids(const unsigned long long* d_list, uint64_t n, uint64_t index_base, uint64_t count,
                                const unsigned long long* d_slot_ids, const uint32_t* d_slot_index, uint64_t slots,
                                unsigned long long* d_out, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (n > 0x80000000ull || index_base + count > 0x100000000ull) return hipErrorInvalidValue;
    if (d_slot_ids != nullptr && (slots < kIdMinSlots || (slots & (slots - 1)) != 0)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(keys_from_ids_kernel, dim3(id_grid(n)), dim3(kIdThreads), 0, stream, d_list, n, index_base, count, d_slot_ids,
                       d_slot_index, slots, d_out);
    return hipGetLastError();
}

hipError_t launch_ids_compact(unsigned long long* d_ids, const uint32_t* d_map, uint64_t first, uint64_t kept, uint64_t count,
                              unsigned long long* d_scratch, hipStream_t stream) {
    if (first >= count || kept < first || kept >= count) return hipErrorInvalidValue;
    const uint64_t n = count - first;
    if (kept > first)
        hipLaunchKernelGGL(ids_compact_gather_kernel, dim3(id_grid(n)), dim3(kIdThreads), 0, stream, d_ids, d_map, first, count, d_scratch,
                           n);
    hipLaunchKernelGGL(ids_compact_scatter_kernel, dim3(id_grid(n)), dim3(kIdThreads), 0, stream, d_scratch, first, kept, count, d_ids);
    return hipGetLastError();
}

}  // namespace lbad
