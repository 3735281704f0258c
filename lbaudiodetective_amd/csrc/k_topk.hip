// k_topk.hip -- exact top-K of rows of float scores, selected on the device (corpus top-K queries).
//
// The best-match loop of LBAudioDetectiveTests.m:57-91 keeps one answer; a shortlist keeps the K best.  Every entry e of a row
// becomes the 64-bit key of the top-1 scans,
//   key = (float bits of score << 32) | (0xFFFFFFFF - (index_base + e)),
// a strict total order (score descending, then index ascending); a score that is not > 0 (+0, negative, NaN) gives no key.
// Positive floats order like their bits, so the K-th largest key is found by a radix select on the key itself:
//
//   init      per row: state {prefix 0, need K}, six zeroed 2048-bin histograms
//   hist<d>   digit d of every key whose higher digits equal the prefix, counted in LDS (integer atomics), one global add
//             per non-zero bin per workgroup
//   scan<d>   one workgroup per row: the bin that holds the need-th key from the top; the prefix takes it, need drops by
//             the keys above it.  Done as soon as every key >= prefix fits the candidate buffer (kCand keys; a further
//             histogram pass costs ~4 us, sorting and gathering thousands of candidates more)
//   gather    every key >= prefix to the row's candidate buffer (atomic cursors: order of arrival does not matter,
//             the keys are distinct and sorted next)
//   sort      one workgroup per row: bitonic sort of the candidates in LDS, the first K written out, 0-padded
//
// Digits, from the top: score bits 30..20, 19..9, 8..0, then the index half 31..21, 20..10, 9..0 (bit 63, the sign, is never
// set).  Scores of unrelated entries sit at 0.5 +- 0.03: the first digit splits them into a handful of bins, the second one
// to 2^-14 of the value, after which the candidates fit unless thousands of entries tie on all 32 score bits -- the index
// digits then cut the tie, and after the last digit exactly K keys are >= the prefix.  The sequence of launches is fixed
// (no host round trip); a pass whose row is done returns at once.
#include "internal.hpp"

namespace lbad {
namespace {

constexpr int kPasses = 6;
constexpr uint32_t kBins = 2048;
constexpr uint32_t kCand = 2048;         // candidate buffer per row (> kTopKMax): 16 KiB of keys, sorted in LDS by one workgroup
constexpr int kHistThreads = 1024;
constexpr int kScanThreads = 256;
constexpr int kSortThreads = 1024;

__host__ __device__ constexpr uint32_t digit_lo(int d) { return d == 0 ? 52 : d == 1 ? 41 : d == 2 ? 32 : d == 3 ? 21 : d == 4 ? 10 : 0; }
__host__ __device__ constexpr uint32_t digit_bits(int d) { return d == 2 ? 9 : d == 5 ? 10 : 11; }

struct RowState {
    unsigned long long prefix;   // the digits decided so far of the K-th key, lower bits 0
    uint32_t need;               // keys still to select among those that match the prefix
    uint32_t above;              // keys already known to be above the prefix's bin (all selected)
    uint32_t done;               // the candidates are every key >= prefix
    uint32_t n_cand;             // gather cursor
    uint32_t pad[2];
};
static_assert(sizeof(RowState) == 32, "RowState layout");

__device__ __forceinline__ unsigned long long score_key(float s, uint64_t global_index) {
    const uint32_t b = __float_as_uint(s);
    if (b - 1u >= 0x7F800000u) return 0ull;          // +0, negative, NaN: never selected (valid: 1 .. 0x7F800000)
    return ((unsigned long long)b << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)global_index);
}

__global__ __launch_bounds__(kScanThreads) void topk_init_kernel(uint32_t* __restrict__ hist, RowState* __restrict__ st, uint32_t k) {
    const uint32_t row = blockIdx.x;
    uint32_t* h = hist + (size_t)row * kPasses * kBins;
    for (uint32_t i = threadIdx.x; i < kPasses * kBins; i += kScanThreads) h[i] = 0u;
    if (threadIdx.x == 0) {
        RowState s = {};
        s.need = k;
        st[row] = s;
    }
}

template <int D>
__global__ __launch_bounds__(kHistThreads) void topk_hist_kernel(const float* __restrict__ scores, uint64_t n, uint64_t index_base,
                                                                 uint32_t* __restrict__ hist, const RowState* __restrict__ st) {
    constexpr uint32_t lo = digit_lo(D), hi = lo + digit_bits(D), mask = (1u << digit_bits(D)) - 1u;
    const uint32_t row = blockIdx.y;
    const unsigned long long prefix = st[row].prefix;
    if (st[row].done) return;
    __shared__ uint32_t h[kBins];
    for (uint32_t i = threadIdx.x; i <= mask; i += kHistThreads) h[i] = 0u;
    __syncthreads();
    const float* r = scores + (size_t)row * n;
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t e = (uint64_t)blockIdx.x * kHistThreads + threadIdx.x; e < n; e += (uint64_t)gridDim.x * kHistThreads) {
        const unsigned long long key = score_key(r[e], index_base + e);
        bool pending = key != 0ull && (key >> hi) == (prefix >> hi);
        const uint32_t bin = (uint32_t)(key >> lo) & mask;
        // most keys of a wave share a few bins (scores at 0.5 +- 0.03): the lanes of the first pending lane's bin add their
        // count in one atomic, for a few rounds; what is left adds one by one (same-address LDS atomics serialise)
#pragma unroll
        for (int round = 0; round < 4; ++round) {
            const unsigned long long waiting = __ballot(pending);
            if (waiting == 0ull) break;
            const uint32_t leader = (uint32_t)__ffsll((long long)waiting) - 1u;
            const uint32_t lead_bin = __shfl(bin, (int)leader);
            const bool same = pending && bin == lead_bin;
            const unsigned long long group = __ballot(same);
            if (lane == leader) atomicAdd(&h[lead_bin], (uint32_t)__popcll(group));
            pending = pending && !same;
        }
        if (pending) atomicAdd(&h[bin], 1u);
    }
    __syncthreads();
    uint32_t* g = hist + ((size_t)row * kPasses + D) * kBins;
    for (uint32_t i = threadIdx.x; i <= mask; i += kHistThreads)
        if (h[i]) atomicAdd(&g[i], h[i]);
}

// one workgroup per row: thread t owns PER bins counted from the top, a scan over the threads finds the need-th key's bin
template <int D>
__global__ __launch_bounds__(kScanThreads) void topk_scan_kernel(const uint32_t* __restrict__ hist, RowState* __restrict__ st) {
    constexpr uint32_t lo = digit_lo(D), nb = 1u << digit_bits(D), per = nb / kScanThreads;
    const uint32_t row = blockIdx.x;
    const RowState s = st[row];
    if (s.done) return;
    __shared__ uint32_t part[kScanThreads];
    const uint32_t* h = hist + ((size_t)row * kPasses + D) * kBins;
    const uint32_t t = threadIdx.x;
    uint32_t c[per], sum = 0;
#pragma unroll
    for (uint32_t j = 0; j < per; ++j) {
        c[j] = h[nb - 1 - (t * per + j)];
        sum += c[j];
    }
    part[t] = sum;
    __syncthreads();
    for (uint32_t off = 1; off < kScanThreads; off <<= 1) {         // inclusive scan (Hillis-Steele)
        const uint32_t add = t >= off ? part[t - off] : 0u;
        __syncthreads();
        part[t] += add;
        __syncthreads();
    }
    const uint32_t incl = part[t], excl = incl - sum, total = part[kScanThreads - 1];
    if (total < s.need) {                                            // fewer keys than wanted: every key matching the prefix
        if (t == 0) st[row].done = 1u;
        return;
    }
    if (excl < s.need && s.need <= incl) {
        uint32_t acc = excl;
#pragma unroll
        for (uint32_t j = 0; j < per; ++j) {
            if (acc + c[j] >= s.need) {
                const uint32_t bin = nb - 1 - (t * per + j);
                RowState w = s;
                w.prefix = s.prefix | ((unsigned long long)bin << lo);
                w.need = s.need - acc;
                w.above = s.above + acc;
                w.done = (w.above + c[j] <= kCand || D == kPasses - 1) ? 1u : 0u;
                st[row] = w;
                break;
            }
            acc += c[j];
        }
    }
}

// the workgroup collects its candidates in LDS first: one global atomic per workgroup, not one per candidate (thousands
// of candidates on one cursor serialise: 147 us at 10 M entries when every candidate took its own)
__global__ __launch_bounds__(kHistThreads) void topk_gather_kernel(const float* __restrict__ scores, uint64_t n, uint64_t index_base,
                                                                   RowState* __restrict__ st, unsigned long long* __restrict__ cand) {
    __shared__ unsigned long long local[kCand];
    __shared__ uint32_t n_local, base;
    const uint32_t row = blockIdx.y;
    const unsigned long long prefix = st[row].prefix;
    const float* r = scores + (size_t)row * n;
    if (threadIdx.x == 0) n_local = 0u;
    __syncthreads();
    for (uint64_t e = (uint64_t)blockIdx.x * kHistThreads + threadIdx.x; e < n; e += (uint64_t)gridDim.x * kHistThreads) {
        const unsigned long long key = score_key(r[e], index_base + e);
        if (key != 0ull && key >= prefix) {
            const uint32_t at = atomicAdd(&n_local, 1u);
            if (at < kCand) local[at] = key;                          // (the row's count is exact and <= kCand)
        }
    }
    __syncthreads();
    const uint32_t mine = n_local < kCand ? n_local : kCand;
    if (mine == 0u) return;
    if (threadIdx.x == 0) base = atomicAdd(&st[row].n_cand, mine);
    __syncthreads();
    unsigned long long* out = cand + (size_t)row * kCand;
    for (uint32_t i = threadIdx.x; i < mine; i += kHistThreads)
        if (base + i < kCand) out[base + i] = local[i];
}

__global__ __launch_bounds__(kSortThreads) void topk_sort_kernel(const RowState* __restrict__ st, const unsigned long long* __restrict__ cand,
                                                                 uint32_t k, unsigned long long* __restrict__ keys_out) {
    __shared__ unsigned long long v[kCand];
    const uint32_t row = blockIdx.x;
    const uint32_t n = st[row].n_cand < kCand ? st[row].n_cand : kCand;
    uint32_t p = 2;
    while (p < n) p <<= 1;
    const unsigned long long* in = cand + (size_t)row * kCand;
    for (uint32_t i = threadIdx.x; i < p; i += kSortThreads) v[i] = i < n ? in[i] : 0ull;
    __syncthreads();
    for (uint32_t len = 2; len <= p; len <<= 1) {                   // bitonic, descending
        for (uint32_t j = len >> 1; j > 0; j >>= 1) {
            for (uint32_t i = threadIdx.x; i < p; i += kSortThreads) {
                const uint32_t l = i ^ j;
                if (l > i) {
                    const unsigned long long a = v[i], b = v[l];
                    if (((i & len) == 0) ? (a < b) : (a > b)) { v[i] = b; v[l] = a; }
                }
            }
            __syncthreads();
        }
    }
    unsigned long long* out = keys_out + (size_t)row * k;
    for (uint32_t i = threadIdx.x; i < k; i += kSortThreads) out[i] = i < n ? v[i] : 0ull;
}

}  // namespace

size_t topk_scratch_bytes(uint32_t rows) {
    return (size_t)rows * (kPasses * kBins * sizeof(uint32_t) + sizeof(RowState) + kCand * sizeof(unsigned long long));
}

hipError_t launch_topk_keys(const float* d_scores, uint64_t n, uint32_t rows, uint32_t k, uint64_t index_base, void* d_scratch,
                            unsigned long long* d_keys, hipStream_t stream) {
    if (rows == 0) return hipSuccess;
    if (k == 0 || k > kTopKMax || rows > 65535u) return hipErrorInvalidValue;
    if (n == 0) return hipMemsetAsync(d_keys, 0, (size_t)rows * k * sizeof(unsigned long long), stream);
    uint32_t* hist = static_cast<uint32_t*>(d_scratch);
    RowState* st = reinterpret_cast<RowState*>(hist + (size_t)rows * kPasses * kBins);
    unsigned long long* cand = reinterpret_cast<unsigned long long*>(st + rows);
    const dim3 grid(strided_grid((n + kHistThreads - 1) / kHistThreads, 256), rows);   // (one count of a strided launch per call)
    hipLaunchKernelGGL(topk_init_kernel, dim3(rows), dim3(kScanThreads), 0, stream, hist, st, k);
#define LBAD_TOPK_PASS(D)                                                                                                    \
    hipLaunchKernelGGL(topk_hist_kernel<D>, grid, dim3(kHistThreads), 0, stream, d_scores, n, index_base, hist, st);        \
    hipLaunchKernelGGL(topk_scan_kernel<D>, dim3(rows), dim3(kScanThreads), 0, stream, hist, st);
    LBAD_TOPK_PASS(0)
    LBAD_TOPK_PASS(1)
    LBAD_TOPK_PASS(2)
    LBAD_TOPK_PASS(3)
    LBAD_TOPK_PASS(4)
    LBAD_TOPK_PASS(5)
#undef LBAD_TOPK_PASS
    hipLaunchKernelGGL(topk_gather_kernel, grid, dim3(kHistThreads), 0, stream, d_scores, n, index_base, st, cand);
    hipLaunchKernelGGL(topk_sort_kernel, dim3(rows), dim3(kSortThreads), 0, stream, st, cand, k, d_keys);
    return hipGetLastError();
}

}  // namespace lbad
