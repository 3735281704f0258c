// k_occurrence_segments.hip -- occurrence segments on the device, DESIGN.md 4.4z: from the rows of an occurrences call (keys, lags
// and the lengths of the entries the keys name, [recordings][cap_in], with the rows' counts) the non-overlapping spans per
// recording over ALL cells of the row, greedy in descending key order (ties to the lower start, then the lower slot), compacted in
// start order into rows of `cap_out` slots with the true count beside them.  The sibling of k_segments.hip, which sees one
// candidate per offset; here any number of candidates may start at one offset.
//
// ONE launch; a workgroup owns a recording from start to end and takes the next one gridDim.x further on (grid from strided_grid).
// No workgroup reads what another writes, nothing waits for another workgroup, and there is no atomic on global memory.  The
// recording's state lives in dynamic LDS sized by cap_in and per (os_layout): by SLOT the keys (a slot that is no candidate stored
// as 0), the span's start and end (16 bits: per <= 8192) and the order (16-bit slots); by OFFSET the slot accepted there (16 bits)
// and two bitmasks of 64-bit words: `taken` (offsets inside an accepted span) and `acc` (starts of accepted spans).
//
//   1. load     slot i < m = min(count, cap_in): the span [s, e) = [max(0, -lag), min(per, -lag + length)) in 64-bit signed
//               arithmetic; a candidate has a non-zero key, a non-zero length, s < per and s < e.  order[i] = i for i < n2 = the
//               power of two >= max(cap_in, 64); the slots from m on and the pads hold key 0 and the span [0, 0).
//   2. sort     bitonic over `order`, comparing (key descending, start ascending, slot ascending): a strict total order, so the
//               result is THE priority order, candidates first.  log2(n2) (log2(n2) + 1) / 2 steps of n2 / 2 exchanges.
//   3. walk     wave 0 alone, 64 candidates of the order at a time, as k_segments.hip walks: every lane tests its span against
//               `taken` as the batch finds it; then, while a lane is left, the LOWEST surviving lane is accepted -- its span goes
//               into `taken`, its start into `acc`, its slot into winner[start] -- and it and every survivor whose span meets
//               the new one leave.  Bounds: at most n2 / 64 batches (the loop's own count; it ends early at the first batch
//               without a candidate, the candidates being a prefix of the order); per batch at most 64 acceptances, since each
//               trip removes at least the accepted lane; a lane's test reads at most per / 64 + 1 words.
//   4. scatter  all waves: the number of accepted starts below each mask word, then offset o with its bit set goes to slot
//               prefix + popcount(bits below o) of the row when that is below cap_out -- start order; accepted spans do not
//               overlap, so a start is accepted once -- with key, lag and length read through winner[o] as they came; zeros from
//               min(count, cap_out) to cap_out; the true count.  Every word of the row is written exactly once.
//
// The second kernel is the uniform-corpus half of LBAudioDetectiveCorpusEntryLengthsFromKeysDevice (a ragged corpus goes through
// launch_timeline_lengths of k_timeline.hip): every key that names an entry of the corpus gets the corpus' one length.
#include "segments_common.hpp"

namespace lbad {
namespace {

constexpr uint32_t kOsMaxThreads = 1024;
constexpr uint32_t kOsMaxGrid = 1u << 16;        // most workgroups of a launch (they stride over the other recordings)
constexpr uint32_t kOsPerCap = LBAD_SEGMENTS_MAX_SUBFINGERPRINTS;
constexpr uint32_t kOsSlotCap = LBAD_OCCURRENCE_SEGMENTS_MAX_CANDIDATES;
constexpr uint32_t kOsLengthThreads = 256;

// where a recording's state lies in the dynamic LDS, every block 8-byte aligned
struct OsLayout {
    uint32_t n2, words;                                // sorted slots; 64-bit words of a mask
    uint32_t taken_at, acc_at, prefix_at, order_at, start_at, end_at, winner_at, bytes;     // (the keys lie at 0)
};
__host__ __device__ constexpr OsLayout os_layout(uint32_t cap_in, uint32_t per) {
    OsLayout l{};
    l.n2 = 64;
    while (l.n2 < cap_in) l.n2 <<= 1;
    l.words = (per + 63) / 64;
    l.taken_at = l.n2 * 8;
    l.acc_at = l.taken_at + l.words * 8;
    l.prefix_at = l.acc_at + l.words * 8;
    l.order_at = l.prefix_at + ((l.words + 1 + 1) / 2) * 8;           // words + 1 counts of 32 bits
    l.start_at = l.order_at + l.n2 * 2;
    l.end_at = l.start_at + l.n2 * 2;
    l.winner_at = l.end_at + l.n2 * 2;
    l.bytes = l.winner_at + ((per + 3) / 4) * 8;
    return l;
}
static_assert(kOsSlotCap <= 65536 && kOsPerCap <= 65535, "slots, starts and ends are 16 bits wide (an end may be `per` itself)");
static_assert(os_layout(kOsSlotCap, kOsPerCap).bytes <= kSgLdsBudget, "the state of the longest row and recording fits a workgroup's LDS");

__global__ __launch_bounds__(kOsMaxThreads) void occurrence_segments_kernel(
    const unsigned long long* __restrict__ in_keys, const int32_t* __restrict__ in_lags, const uint32_t* __restrict__ in_lengths,
    const unsigned long long* __restrict__ in_counts, uint32_t recordings, uint32_t cap_in, uint32_t per, uint32_t cap_out,
    uint32_t* __restrict__ out_starts, unsigned long long* __restrict__ out_keys, int32_t* __restrict__ out_lags,
    uint32_t* __restrict__ out_lengths, uint32_t* __restrict__ out_counts) {
    extern __shared__ __align__(16) unsigned char os_lds[];
    const OsLayout l = os_layout(cap_in, per);
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(os_lds);
    unsigned long long* taken = reinterpret_cast<unsigned long long*>(os_lds + l.taken_at);
    unsigned long long* acc = reinterpret_cast<unsigned long long*>(os_lds + l.acc_at);
    uint32_t* prefix = reinterpret_cast<uint32_t*>(os_lds + l.prefix_at);
    uint16_t* order = reinterpret_cast<uint16_t*>(os_lds + l.order_at);
    uint16_t* start = reinterpret_cast<uint16_t*>(os_lds + l.start_at);
    uint16_t* end = reinterpret_cast<uint16_t*>(os_lds + l.end_at);
    uint16_t* winner = reinterpret_cast<uint16_t*>(os_lds + l.winner_at);
    const uint32_t tid = threadIdx.x, nt = blockDim.x, n2 = l.n2, words = l.words;

    for (uint32_t r = blockIdx.x; r < recordings; r += gridDim.x) {
        const unsigned long long* rk = in_keys + (size_t)r * cap_in;
        const int32_t* rg = in_lags + (size_t)r * cap_in;
        const uint32_t* rl = in_lengths + (size_t)r * cap_in;
        uint32_t m = cap_in;
        if (in_counts) {
            const unsigned long long c = in_counts[r];
            m = c < cap_in ? (uint32_t)c : cap_in;
        }
        // 1. load
        for (uint32_t i = tid; i < n2; i += nt) {
            unsigned long long k = 0ull;
            uint32_t s = 0u, e = 0u;
            if (i < m) {
                const long long at = -(long long)rg[i];                // (the entry's first sub-fingerprint, in the recording's offsets)
                const uint32_t n = rl[i];
                const long long s64 = at > 0 ? at : 0, e64 = at + (long long)n < (long long)per ? at + (long long)n : (long long)per;
                if (n != 0u && s64 < (long long)per && s64 < e64) {
                    k = rk[i];
                    if (k != 0ull) {
                        s = (uint32_t)s64;
                        e = (uint32_t)e64;
                    }
                }
            }
            keys[i] = k;
            start[i] = (uint16_t)s;
            end[i] = (uint16_t)e;
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
                    bool a_first = ka > kb;
                    if (ka == kb) {
                        const uint32_t sa = start[a], sb = start[b];
                        a_first = sa < sb || (sa == sb && a < b);
                    }
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
                const uint32_t slot = order[base + tid];
                bool alive = keys[slot] != 0ull;
                if (__ballot(alive) == 0ull) break;
                const uint32_t o = start[slot], e = end[slot];     // (a candidate's span is not empty: o < e <= per)
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
                    if (tid == (uint32_t)src) {
                        acc[o >> 6] |= 1ull << (o & 63u);
                        winner[o] = (uint16_t)slot;
                    }
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
        uint32_t* os = out_starts + (size_t)r * cap_out;
        unsigned long long* ok = out_keys + (size_t)r * cap_out;
        int32_t* og = out_lags ? out_lags + (size_t)r * cap_out : nullptr;
        uint32_t* ol = out_lengths ? out_lengths + (size_t)r * cap_out : nullptr;
        for (uint32_t o = tid; o < per; o += nt) {
            const unsigned long long bits = acc[o >> 6];
            if (((bits >> (o & 63u)) & 1ull) == 0ull) continue;
            const uint32_t to = prefix[o >> 6] + (uint32_t)__popcll(bits & ((1ull << (o & 63u)) - 1ull));
            if (to >= cap_out) continue;
            const uint32_t slot = winner[o];
            os[to] = o;
            ok[to] = keys[slot];
            if (og) og[to] = rg[slot];
            if (ol) ol[to] = rl[slot];
        }
        for (uint32_t s = (count < cap_out ? count : cap_out) + tid; s < cap_out; s += nt) {
            os[s] = 0u;
            ok[s] = 0ull;
            if (og) og[s] = 0;
            if (ol) ol[s] = 0u;
        }
        if (tid == 0u) out_counts[r] = count;
        __syncthreads();                                           // (the next recording's load overwrites the state)
    }
}

// lengths[i] = n_sub where keys[i] names an entry of a uniform corpus of `count` entries behind `base`, 0 for a zero key or an
// index outside it (timeline_lengths_kernel's rule, without the offsets a uniform corpus does not keep)
__global__ __launch_bounds__(kOsLengthThreads) void entry_lengths_uniform_kernel(const unsigned long long* __restrict__ keys, uint32_t n,
                                                                                 uint32_t base, uint64_t count, uint32_t n_sub,
                                                                                 uint32_t* __restrict__ lengths) {
    const uint32_t i = blockIdx.x * kOsLengthThreads + threadIdx.x;
    if (i >= n) return;
    const unsigned long long key = keys[i];
    const uint32_t j = 0xFFFFFFFFu - (uint32_t)key - base;     // (the low word is 0xFFFFFFFF - (index base + j))
    lengths[i] = key != 0ull && j < count ? n_sub : 0u;
}

}  // namespace

size_t occurrence_segments_lds_bytes(uint32_t cap_in, uint32_t per) {
    return cap_in == 0 || cap_in > kOsSlotCap || per == 0 || per > kOsPerCap ? 0 : os_layout(cap_in, per).bytes;
}

hipError_t launch_occurrence_segments(const unsigned long long* d_keys, const int32_t* d_lags, const uint32_t* d_lengths,
                                      const unsigned long long* d_counts, uint32_t recordings, uint32_t cap_in, uint32_t per,
                                      uint32_t cap_out, uint32_t* d_starts, unsigned long long* d_out_keys, int32_t* d_out_lags,
                                      uint32_t* d_out_lengths, uint32_t* d_out_counts, hipStream_t stream) {
    if (recordings == 0 || cap_in == 0 || cap_in > kOsSlotCap || per == 0 || per > kOsPerCap || cap_out == 0 ||
        (uint64_t)recordings * cap_in > 0x7FFFFFFFull || (uint64_t)recordings * per > 0x7FFFFFFFull ||
        (uint64_t)recordings * cap_out > 0x7FFFFFFFull)
        return hipErrorInvalidValue;
    const OsLayout l = os_layout(cap_in, per);
    if (l.bytes > kSgLdsBudget) return hipErrorInvalidValue;
    // dynamic LDS above 48 KiB has to be allowed per device (k_segments.hip: the same words, the same race at worst)
    static std::atomic<size_t> ready[kMaxDevices] = {};
    if (l.bytes > 48 * 1024) {
        const int dev = current_device();
        if (dev < 0 || dev >= kMaxDevices) return hipErrorInvalidDevice;
        if (l.bytes > ready[dev].load(std::memory_order_acquire)) {
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(occurrence_segments_kernel),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)kSgLdsBudget);
            if (e != hipSuccess) return e;
            ready[dev].store(kSgLdsBudget, std::memory_order_release);
        }
    }
    const uint32_t threads = l.n2 / 2 < 64u ? 64u : l.n2 / 2 > kOsMaxThreads ? kOsMaxThreads : l.n2 / 2;
    hipLaunchKernelGGL(occurrence_segments_kernel, dim3(strided_grid(recordings, kOsMaxGrid)), dim3(threads), l.bytes, stream, d_keys,
                       d_lags, d_lengths, d_counts, recordings, cap_in, per, cap_out, d_starts, d_out_keys, d_out_lags, d_out_lengths,
                       d_out_counts);
    return hipGetLastError();
}

hipError_t launch_entry_lengths_uniform(const unsigned long long* d_keys, uint32_t n, uint64_t index_base, uint64_t count, uint32_t n_sub,
                                        uint32_t* d_lengths, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (n > 0x7FFFFFFFu || index_base + count > 0x100000000ull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(entry_lengths_uniform_kernel, dim3((n + kOsLengthThreads - 1u) / kOsLengthThreads), dim3(kOsLengthThreads), 0,
                       stream, d_keys, n, (uint32_t)index_base, count, n_sub, d_lengths);
    return hipGetLastError();
}

}  // namespace lbad
