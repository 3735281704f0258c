// k_segments.hip -- recording segments on the device, DESIGN.md 4.4s: from a timeline's per-offset winners (keys and lengths,
// [recordings][per]) the non-overlapping spans per recording, greedy in descending key order (ties to the lower offset), compacted
// in start order into rows of `capacity` slots with the true count beside them.
//
// ONE launch; a workgroup owns a recording from start to end and takes the next one gridDim.x further on (grid from strided_grid).
// No workgroup reads what another writes, nothing waits for another workgroup, and there is no atomic on global memory.  The
// recording's state lives in dynamic LDS sized by `per` (sg_layout): the keys by offset (a winner with length 0 stored as 0: it
// is no candidate), the lengths clipped to the recording's end (16 bits: per <= 8192), the order (16-bit offsets), and two
// bitmasks of 64-bit words by offset: `taken` (offsets inside an accepted span) and `acc` (starts of accepted spans).
//
//   1. load     keys, clipped lengths, order[i] = i for i < n2 = the power of two >= max(per, 64); the pads hold key 0
//   2. sort     bitonic over `order`, comparing (keys[order] descending, order ascending): a strict total order, so the result is
//               THE priority order, candidates first.  log2(n2) (log2(n2) + 1) / 2 steps of n2 / 2 exchanges.
//   3. walk     wave 0 alone, 64 candidates of the order at a time.  Every lane tests its span against `taken` as the batch finds
//               it; a lane that overlaps is rejected for good (the mask only grows).  Then, while a lane is left: the LOWEST
//               surviving lane -- no candidate of higher priority that overlaps it was accepted -- is accepted, its span goes into
//               `taken` (all lanes, a word each) and its start into `acc`, and it and every survivor whose span meets the new one
//               leave.  Inside a batch the survivors need no second look at the mask: what was added since their test is exactly
//               the spans they were compared with.
//               Bounds: at most n2 / 64 batches (the loop's own count; it ends early at the first batch without a candidate,
//               the candidates being a prefix of the order); per batch at most 64 acceptances, since each trip removes at
//               least the accepted lane; a lane's test reads at most per / 64 + 1 words.
//   4. scatter  all waves: the number of accepted starts below each mask word (a prefix over <= 128 popcounts), then offset o
//               with its bit set goes to slot prefix + popcount(bits below o) of the row when that is below the capacity -- start
//               order -- with the key as it came and the length as it came (re-read: the LDS copy is clipped); zeros from
//               min(count, capacity) to the capacity; the true count.  Every word of the row is written exactly once.
#include "segments_common.hpp"

namespace lbad {
namespace {

constexpr uint32_t kSgMaxThreads = 1024;
constexpr uint32_t kSgMaxGrid = 1u << 16;        // most workgroups of a launch (they stride over the other recordings)
constexpr uint32_t kSgCap = LBAD_SEGMENTS_MAX_SUBFINGERPRINTS;

// where a recording's state lies in the dynamic LDS, every block 8-byte aligned
struct SgLayout {
    uint32_t n2, words;                                // sorted slots; 64-bit words of a mask
    uint32_t taken_at, acc_at, prefix_at, order_at, len_at, bytes;     // (the keys lie at 0)
};
__host__ __device__ constexpr SgLayout sg_layout(uint32_t per) {
    SgLayout l{};
    l.n2 = 64;
    while (l.n2 < per) l.n2 <<= 1;
    l.words = (per + 63) / 64;
    l.taken_at = l.n2 * 8;
    l.acc_at = l.taken_at + l.words * 8;
    l.prefix_at = l.acc_at + l.words * 8;
    l.order_at = l.prefix_at + ((l.words + 1 + 1) / 2) * 8;           // words + 1 counts of 32 bits
    l.len_at = l.order_at + l.n2 * 2;
    l.bytes = l.len_at + ((per + 3) / 4) * 8;
    return l;
}
static_assert(kSgCap <= 65535, "the order and the clipped lengths are 16 bits wide");
static_assert(sg_layout(kSgCap).bytes <= kSgLdsBudget, "the state of the longest recording fits a workgroup's LDS");

__global__ __launch_bounds__(kSgMaxThreads) void timeline_segments_kernel(const unsigned long long* __restrict__ in_keys,
                                                                          const uint32_t* __restrict__ in_lengths, uint32_t recordings,
                                                                          uint32_t per, uint32_t capacity, uint32_t* __restrict__ out_starts,
                                                                          unsigned long long* __restrict__ out_keys,
                                                                          uint32_t* __restrict__ out_lengths, uint32_t* __restrict__ out_counts) {
    extern __shared__ __align__(16) unsigned char sg_lds[];
    const SgLayout l = sg_layout(per);
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(sg_lds);
    unsigned long long* taken = reinterpret_cast<unsigned long long*>(sg_lds + l.taken_at);
    unsigned long long* acc = reinterpret_cast<unsigned long long*>(sg_lds + l.acc_at);
    uint32_t* prefix = reinterpret_cast<uint32_t*>(sg_lds + l.prefix_at);
    uint16_t* order = reinterpret_cast<uint16_t*>(sg_lds + l.order_at);
    uint16_t* len = reinterpret_cast<uint16_t*>(sg_lds + l.len_at);
    const uint32_t tid = threadIdx.x, nt = blockDim.x, n2 = l.n2, words = l.words;

    for (uint32_t r = blockIdx.x; r < recordings; r += gridDim.x) {
        const unsigned long long* rk = in_keys + (size_t)r * per;
        const uint32_t* rl = in_lengths + (size_t)r * per;
        // 1. load
        for (uint32_t i = tid; i < n2; i += nt) {
            unsigned long long k = 0ull;
            if (i < per) {
                const uint32_t n = rl[i];
                k = n != 0u ? rk[i] : 0ull;
                len[i] = (uint16_t)(n < per - i ? n : per - i);
            }
            keys[i] = k;
            order[i] = (uint16_t)i;
        }
        for (uint32_t w = tid; w < words; w += nt) {
            taken[w] = 0ull;
            acc[w] = 0ull;
        }
        __syncthreads();
        // 2. sort
        for (uint32_t k = 2; k <= n2; k <<= 1) {
            for (uint32_t j = k >> 1; j > 0; j >>= 1) {
                for (uint32_t i = tid; i < n2 / 2; i += nt) {
                    const uint32_t lo = ((i & ~(j - 1u)) << 1) | (i & (j - 1u)), hi = lo | j;
                    const uint32_t a = order[lo], b = order[hi];
                    const unsigned long long ka = keys[a], kb = keys[b];
                    const bool a_first = ka > kb || (ka == kb && a < b);
                    if (a_first != ((lo & k) == 0u)) {             // (a run with bit k clear ends best first, the others worst first)
                        order[lo] = (uint16_t)b;
                        order[hi] = (uint16_t)a;
                    }
                }
                __syncthreads();
            }
        }
        // 3. walk
        if (tid < 64u) {
            for (uint32_t base = 0; base < n2; base += 64u) {
                const uint32_t o = order[base + tid];
                bool alive = o < per && keys[o] != 0ull;
                if (__ballot(alive) == 0ull) break;
                const uint32_t e = alive ? o + len[o] : o;         // (a candidate's clipped length is >= 1: o < e <= per)
                if (alive) {
                    unsigned long long hit = 0ull;
                    for (uint32_t w = o >> 6; w <= ((e - 1u) >> 6); ++w) hit |= taken[w] & sg_span_bits(w, o, e);
                    alive = hit == 0ull;
                }
                unsigned long long live = __ballot(alive);
                while (live != 0ull) {                             // each trip clears at least the accepted lane's bit
                    const int src = __ffsll(live) - 1;
                    const uint32_t ao = __shfl(o, src), ae = __shfl(e, src);
                    for (uint32_t w = (ao >> 6) + tid; w <= ((ae - 1u) >> 6); w += 64u) taken[w] |= sg_span_bits(w, ao, ae);
                    if (tid == 0u) acc[ao >> 6] |= 1ull << (ao & 63u);
                    alive = alive && !(o < ae && ao < e);
                    live = __ballot(alive);
                }
                sg_wave_sync();
            }
        }
        __syncthreads();
        // 4. scatter
        for (uint32_t t = tid; t <= words; t += nt) {
            uint32_t s = 0;
            for (uint32_t w = 0; w < t; ++w) s += (uint32_t)__popcll(acc[w]);
            prefix[t] = s;
        }
        __syncthreads();
        const uint32_t count = prefix[words];
        uint32_t* os = out_starts + (size_t)r * capacity;
        unsigned long long* ok = out_keys + (size_t)r * capacity;
        uint32_t* ol = out_lengths ? out_lengths + (size_t)r * capacity : nullptr;
        for (uint32_t o = tid; o < per; o += nt) {
            const unsigned long long m = acc[o >> 6];
            if (((m >> (o & 63u)) & 1ull) == 0ull) continue;
            const uint32_t slot = prefix[o >> 6] + (uint32_t)__popcll(m & ((1ull << (o & 63u)) - 1ull));
            if (slot >= capacity) continue;
            os[slot] = o;
            ok[slot] = keys[o];
            if (ol) ol[slot] = rl[o];
        }
        for (uint32_t s = (count < capacity ? count : capacity) + tid; s < capacity; s += nt) {
            os[s] = 0u;
            ok[s] = 0ull;
            if (ol) ol[s] = 0u;
        }
        if (tid == 0u) out_counts[r] = count;
        __syncthreads();                                           // (the next recording's load overwrites the state)
    }
}

}  // namespace

size_t segments_lds_bytes(uint32_t per) { return per == 0 || per > kSgCap ? 0 : sg_layout(per).bytes; }

hipError_t launch_timeline_segments(const unsigned long long* d_keys, const uint32_t* d_lengths, uint32_t recordings, uint32_t per,
                                    uint32_t capacity, uint32_t* d_starts, unsigned long long* d_out_keys, uint32_t* d_out_lengths,
                                    uint32_t* d_counts, hipStream_t stream) {
    if (recordings == 0 || per == 0 || per > kSgCap || capacity == 0 || (uint64_t)recordings * per > 0x7FFFFFFFull ||
        (uint64_t)recordings * capacity > 0x7FFFFFFFull)
        return hipErrorInvalidValue;
    const SgLayout l = sg_layout(per);
    if (l.bytes > kSgLdsBudget) return hipErrorInvalidValue;
    // dynamic LDS above 48 KiB has to be allowed per device: the size set up on each, recorded once that has succeeded.  The
    // call takes no handle and may come from any thread: the words are atomics, and two threads that race here set the same
    // attribute to the same value twice at worst.
    static std::atomic<size_t> ready[kMaxDevices] = {};
    if (l.bytes > 48 * 1024) {
        const int dev = current_device();
        if (dev < 0 || dev >= kMaxDevices) return hipErrorInvalidDevice;
        if (l.bytes > ready[dev].load(std::memory_order_acquire)) {
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(timeline_segments_kernel),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)kSgLdsBudget);
            if (e != hipSuccess) return e;
            ready[dev].store(kSgLdsBudget, std::memory_order_release);
        }
    }
    const uint32_t threads = l.n2 / 2 < 64u ? 64u : l.n2 / 2 > kSgMaxThreads ? kSgMaxThreads : l.n2 / 2;
    hipLaunchKernelGGL(timeline_segments_kernel, dim3(strided_grid(recordings, kSgMaxGrid)), dim3(threads), l.bytes, stream, d_keys,
                       d_lengths, recordings, per, capacity, d_starts, d_out_keys, d_out_lengths, d_counts);
    return hipGetLastError();
}

}  // namespace lbad
