// k_align.hip -- where a corpus match lies: the sliding offset at which LBAudioDetectiveFingerprintCompareToFingerprint
// (LBAudioDetectiveFingerprint.m:119-149) reaches the score a corpus query returns.
//
// The reference slides the shorter fingerprint along the longer one (Fp.m:123-146) and keeps the best score; the loop
// variable `offset` that picked it is dropped.  For a (query, entry) pair the corpus passes the query as the first argument,
// so fingerprint1 is the entry when n_q < n_e ("A", Fp.m:123-131 swaps) and the query otherwise ("B", equal lengths included).
// With n1 >= n2 their counts:
//   q_o    = fl(fl(sum over i = 0 .. n2 - 1, in that order, of ratio(fp1[i + o], fp2[i])) / n2),   o = 0 .. n1 - n2
//   score  = max_o q_o (never below 0: the reference's MAX starts from 0),  offset = the lowest o with q_o == score
//   lag    = +offset in A (the query's sub-fingerprint 0 lies on the entry's sub-fingerprint lag),
//            -offset in B (the entry's sub-fingerprint 0 lies on the query's sub-fingerprint -lag)
// ratio is the compare of the scans (k_compare.hip, k_sliding.hip, k_sliding_short.hip): `possible` counts fingerprint1's non-zero pairs inside the
// range, hits the pairs where both Booleans agree, and the quotient is correctly rounded -- an IEEE division here, the same
// values the ragged scans read from their table (sliding.cpp: sliding_tri_table).  score is therefore, bit for bit, what LBAudioDetectiveCorpusScoresDevice returns.
//
// Alignment runs AFTER selection, on the pairs the top-1 / top-K paths hand over as 64-bit keys on the device
// (score bits << 32 | 0xFFFFFFFF - global index), so the tuned scans stay as they are.  Lanes own offsets: a workgroup is one
// wave and takes a tile of 64 consecutive offsets of one pair, every lane walking the i loop in the reference's order.  A pair
// with more tiles than that is spread over `parts` workgroups (tiles part, part + parts, ...); their maxima of the key
// (q_o bits << 32 | 0xFFFFFFFF - o: the lowest offset wins a tie) meet in one atomicMax per workgroup, and a second launch
// turns them into lags.  With one part per pair the workgroup writes its result itself.  A key that is zero or whose index
// lies outside [index_base, index_base + count) gives lag 0 and score 0; nothing outside the corpus or the queries is read.
//
// Both corpus layouts: the ragged records of sliding_common.hpp (32 bytes, pairs de-interleaved: P in w0..w2 + w3 bits 0..3, N in
// w4..w6 + w7 bits 0..3; the derived bits above them never meet the range mask) and the uniform planes of k_compare.hip (a
// tight bitstream of n_sub * Lp bits per entry, word w of entry e in plane w >> 2 at planes[(w >> 2) * stride + e]).  A query
// sub-fingerprint is eight words in the layout of its corpus: P[4] N[4] (ragged) or the packed slot words (uniform).
#include "internal.hpp"

namespace lbad {
namespace {

constexpr int kAlThreads = 64;                // one wave per workgroup
constexpr uint32_t kAlTile = kAlThreads;      // offsets per tile: one per lane
constexpr uint64_t kAlMaxGrid = 65536;        // workgroups of a launch (they stride over any work beyond)
constexpr uint64_t kAlSplitBudget = 16384;    // pairs x parts of a keys launch: how widely a long pair is spread
constexpr int kFinishThreads = 256;

struct Sub {
    uint32_t w[8];
};

struct AlignArgs {
    const uint4* recs;          // ragged: 2 x uint4 per record
    const uint32_t* off;        // ragged: count + 1 record positions
    const uint32_t* planes;     // uniform: the planes as words
    uint64_t stride;            // uniform: plane stride (the corpus' capacity)
    uint64_t count;             // entries
    uint64_t index_base;
    uint32_t n_sub;             // uniform: sub-fingerprints per entry
    uint32_t lp;                // uniform: bits per sub-fingerprint in the stream (the length rounded up to even)
    uint32_t mask[8];           // the range: pair bits of P / N (ragged, 4 words) or even bit positions (uniform, 8 words)
};

struct Pair {
    uint64_t e = 0, rec0 = 0;   // the entry and (ragged) its first record
    const uint32_t* q = nullptr;
    uint32_t n1 = 0, n2 = 0, n_off = 0;
    bool entry_long = false;    // "A": the entry is fingerprint1
};

// sub-fingerprint s of the pair's entry (k_compare.hip: load_sub for the planes)
template <bool RAGGED>
__device__ __forceinline__ Sub entry_sub(const AlignArgs& a, const Pair& p, uint32_t s) {
    Sub r;
    if (RAGGED) {
        const uint4* rec = a.recs + 2 * (p.rec0 + s);
        const uint4 x = rec[0], y = rec[1];
        r.w[0] = x.x; r.w[1] = x.y; r.w[2] = x.z; r.w[3] = x.w;
        r.w[4] = y.x; r.w[5] = y.y; r.w[6] = y.z; r.w[7] = y.w;
    } else {
        const uint32_t total = (a.n_sub * a.lp + 31u) >> 5;    // words in the entry's stream
        const uint32_t off = s * a.lp, w0 = off >> 5, sh = off & 31u;
        auto word = [&](uint32_t w) -> uint32_t {
            return w < total ? a.planes[((uint64_t)(w >> 2) * a.stride + p.e) * 4u + (w & 3u)] : 0u;
        };
        const uint32_t nwords = (a.lp + 31u) >> 5;
        uint32_t prev = word(w0);
#pragma unroll
        for (uint32_t j = 0; j < 8; ++j) {
            uint32_t v = 0u;
            if (j < nwords) {
                const uint32_t next = word(w0 + j + 1);
                v = sh ? ((prev >> sh) | (next << (32u - sh))) : prev;
                prev = next;
                const uint32_t remaining = a.lp - 32u * j;
                if (remaining < 32u) v &= (1u << remaining) - 1u;
            }
            r.w[j] = v;
        }
    }
    return r;
}

__device__ __forceinline__ Sub query_sub(const uint32_t* q, uint32_t s) {
    const uint4* p = reinterpret_cast<const uint4*>(q + 8 * (size_t)s);
    const uint4 x = p[0], y = p[1];
    Sub r;
    r.w[0] = x.x; r.w[1] = x.y; r.w[2] = x.z; r.w[3] = x.w;
    r.w[4] = y.x; r.w[5] = y.y; r.w[6] = y.z; r.w[7] = y.w;
    return r;
}

// Fp.m:151-176 with `a` the fingerprint1 side: possible from a's pairs inside the range, hits where both Booleans agree
template <bool RAGGED>
__device__ __forceinline__ float sub_ratio(const Sub& a, const Sub& b, const uint32_t (&m)[8]) {
    uint32_t possible = 0, hits = 0;
    if (RAGGED) {
#pragma unroll
        for (uint32_t w = 0; w < 4; ++w) {
            const uint32_t nz = (a.w[w] | a.w[4 + w]) & m[w];
            const uint32_t d = (a.w[w] ^ b.w[w]) | (a.w[4 + w] ^ b.w[4 + w]);
            possible += __popc(nz);
            hits += __popc(nz & ~d);
        }
    } else {
#pragma unroll
        for (uint32_t w = 0; w < 8; ++w) {
            const uint32_t nz = (a.w[w] | (a.w[w] >> 1)) & m[w];
            const uint32_t x = a.w[w] ^ b.w[w];
            possible += __popc(nz);
            hits += __popc(nz & ~(x | (x >> 1)));
        }
    }
    return possible ? __fdiv_rn((float)hits, (float)possible) : 0.0f;
}

// the pair of entry e and the query (first sub-fingerprint, count) = qd of the query words qw
template <bool RAGGED>
__device__ __forceinline__ Pair entry_pair(const AlignArgs& a, uint64_t e, const uint32_t* qw, uint2 qd) {
    Pair p;
    uint32_t ne;
    if (RAGGED) {
        const uint32_t r0 = a.off[e];
        p.rec0 = r0;
        ne = a.off[e + 1] - r0;
    } else {
        ne = a.n_sub;
    }
    p.e = e;
    p.q = qw + 8 * (size_t)qd.x;
    p.entry_long = qd.y < ne;                          // Fp.m:123-131
    p.n1 = p.entry_long ? ne : qd.y;
    p.n2 = p.entry_long ? qd.y : ne;
    p.n_off = p.n1 - p.n2 + 1;
    return p;
}

// the pair a key names; false (nothing to read) for a zero key or an index outside this corpus
template <bool RAGGED>
__device__ __forceinline__ bool key_pair(const AlignArgs& a, unsigned long long key, const uint32_t* qw, uint2 qd, Pair& p) {
    if (key == 0ull) return false;
    const uint64_t idx = 0xFFFFFFFFu - (uint32_t)key;
    if (idx < a.index_base || idx - a.index_base >= a.count) return false;
    p = entry_pair<RAGGED>(a, idx - a.index_base, qw, qd);
    return true;
}

// q_o of offset o < n_off: the float32 sum in sub-fingerprint order (Fp.m:139-142), one correctly rounded division
// (ragged: four steps unrolled, their loads in flight together; the planes' word-by-word extraction stays rolled, unrolled
// it runs out of scalar registers)
template <bool RAGGED>
__device__ __forceinline__ float offset_score(const AlignArgs& a, const Pair& p, uint32_t o) {
    constexpr int kUnroll = RAGGED ? 4 : 1;
    float sum = 0.0f;
    if (p.entry_long) {
#pragma unroll kUnroll
        for (uint32_t i = 0; i < p.n2; ++i)
            sum = __fadd_rn(sum, sub_ratio<RAGGED>(entry_sub<RAGGED>(a, p, o + i), query_sub(p.q, i), a.mask));
    } else {
#pragma unroll kUnroll
        for (uint32_t i = 0; i < p.n2; ++i)
            sum = __fadd_rn(sum, sub_ratio<RAGGED>(query_sub(p.q, o + i), entry_sub<RAGGED>(a, p, i), a.mask));
    }
    return __fdiv_rn(sum, (float)p.n2);
}

__device__ __forceinline__ unsigned long long wave_max(unsigned long long k) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(k, off, 64);
        k = o > k ? o : k;
    }
    return k;
}

__device__ __forceinline__ void put_result(bool ok, bool entry_long, unsigned long long best, int32_t* lag, float* score) {
    const uint32_t o = 0xFFFFFFFFu - (uint32_t)best;
    *lag = ok ? (entry_long ? (int32_t)o : -(int32_t)o) : 0;
    if (score) *score = ok ? __uint_as_float((uint32_t)(best >> 32)) : 0.0f;
}

// pairs = n_queries x k keys (pair / k is the query); work item w = (pair w / parts, part w % parts)
template <bool RAGGED>
__global__ __launch_bounds__(kAlThreads) void align_keys_kernel(AlignArgs a, const uint32_t* __restrict__ qw,
                                                                const uint2* __restrict__ qd,
                                                                const unsigned long long* __restrict__ keys, uint32_t k,
                                                                uint64_t pairs, uint32_t parts,
                                                                unsigned long long* __restrict__ best_out,
                                                                int32_t* __restrict__ lags, float* __restrict__ scores) {
    const uint32_t lane = threadIdx.x;
    for (uint64_t w = blockIdx.x; w < pairs * parts; w += gridDim.x) {
        const uint64_t pair = w / parts;
        const uint32_t part = (uint32_t)(w - pair * parts);
        Pair p;
        const bool ok = key_pair<RAGGED>(a, keys[pair], qw, qd[pair / k], p);
        unsigned long long best = 0ull;
        if (ok) {
            const uint32_t tiles = (uint32_t)(((uint64_t)p.n_off + kAlTile - 1) / kAlTile);
            for (uint32_t t = part; t < tiles; t += parts) {
                const uint32_t o = t * kAlTile + lane;
                if (o < p.n_off) {
                    const float q = offset_score<RAGGED>(a, p, o);
                    const unsigned long long key = ((unsigned long long)__float_as_uint(q) << 32) | (0xFFFFFFFFu - o);
                    best = key > best ? key : best;
                }
            }
        }
        best = wave_max(best);
        if (lane == 0) {
            if (parts == 1) put_result(ok, p.entry_long, best, lags + pair, scores ? scores + pair : nullptr);
            else if (best) atomicMax(best_out + pair, best);
        }
    }
}

// the parts' merged maxima -> lags (and scores)
template <bool RAGGED>
__global__ __launch_bounds__(kFinishThreads) void align_finish_kernel(AlignArgs a, const uint32_t* __restrict__ qw,
                                                                      const uint2* __restrict__ qd,
                                                                      const unsigned long long* __restrict__ keys, uint32_t k,
                                                                      uint64_t pairs, const unsigned long long* __restrict__ best_in,
                                                                      int32_t* __restrict__ lags, float* __restrict__ scores) {
    for (uint64_t pair = (uint64_t)blockIdx.x * kFinishThreads + threadIdx.x; pair < pairs;
         pair += (uint64_t)gridDim.x * kFinishThreads) {
        Pair p;
        const bool ok = key_pair<RAGGED>(a, keys[pair], qw, qd[pair / k], p);
        put_result(ok, p.entry_long, best_in[pair], lags + pair, scores ? scores + pair : nullptr);
    }
}

// every q_o of one pair, in offset order
template <bool RAGGED>
__global__ __launch_bounds__(kAlThreads) void align_profile_kernel(AlignArgs a, const uint32_t* __restrict__ qw, uint32_t n_query,
                                                                   uint64_t entry, float* __restrict__ out) {
    const Pair p = entry_pair<RAGGED>(a, entry, qw, make_uint2(0u, n_query));
    const uint32_t tiles = (uint32_t)(((uint64_t)p.n_off + kAlTile - 1) / kAlTile);
    for (uint32_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint32_t o = t * kAlTile + threadIdx.x;
        if (o < p.n_off) out[o] = offset_score<RAGGED>(a, p, o);
    }
}

// the range as the scans apply it (Fp.m:155: min(range, length) Booleans, an odd limit takes its whole last pair)
AlignArgs make_args(const AlignSource& s, uint64_t index_base) {
    AlignArgs a = {};
    a.recs = s.recs;
    a.off = s.off;
    a.planes = reinterpret_cast<const uint32_t*>(s.planes);
    a.stride = s.stride;
    a.count = s.count;
    a.index_base = index_base;
    a.n_sub = s.n_sub;
    a.lp = s.subfp_len + (s.subfp_len & 1u);
    const uint32_t lim = s.range < s.subfp_len ? s.range : s.subfp_len;
    const uint32_t pairs = (lim + 1u) / 2u;
    const uint32_t per_word = s.ragged ? 32u : 16u;        // pairs per mask word
    for (uint32_t w = 0; w < (s.ragged ? 4u : 8u); ++w) {
        const uint32_t first = per_word * w;
        const uint32_t n = pairs <= first ? 0u : (pairs - first >= per_word ? per_word : pairs - first);
        uint32_t m = 0u;
        for (uint32_t j = 0; j < n; ++j) m |= 1u << (s.ragged ? j : 2u * j);
        a.mask[w] = m;
    }
    return a;
}

uint32_t tiles_of(uint64_t n_off) { return (uint32_t)((n_off + kAlTile - 1) / kAlTile); }

}  // namespace

// Host: a query's sub-fingerprints as the kernels read them, appended to out (8 words each).  Ragged: the P / N pair words of
// build_sliding_query; uniform: pack_fingerprint's slot words.  Neither is range-masked: the range applies to fingerprint1's
// side, which is the entry or the query depending on the lengths, so the kernel masks.
void build_align_query(const LBAudioDetectiveFingerprint* q, bool ragged, std::vector<uint32_t>& out) {
    const size_t at = out.size();
    out.resize(at + 8 * (size_t)q->count, 0u);
    if (!ragged) {
        std::vector<uint32_t> slots;
        pack_fingerprint(q, slots);
        std::copy(slots.begin(), slots.begin() + 8 * (size_t)q->count, out.begin() + at);
        return;
    }
    const uint32_t L = q->length, pairs = (L + 1u) / 2u;
    for (uint32_t s = 0; s < q->count; ++s) {
        const Boolean* b = q->data.data() + (size_t)s * L;
        uint32_t* o = out.data() + at + 8 * (size_t)s;
        for (uint32_t p = 0; p < pairs; ++p) {
            if (b[2 * p]) o[p >> 5] |= 1u << (p & 31);
            if (2 * p + 1 < L && b[2 * p + 1]) o[4 + (p >> 5)] |= 1u << (p & 31);
        }
    }
}

uint32_t align_parts(uint64_t pairs, uint64_t max_offsets) {
    const uint64_t tiles = tiles_of(max_offsets);
    const uint64_t budget = pairs >= kAlSplitBudget ? 1 : kAlSplitBudget / pairs;
    const uint64_t parts = tiles < budget ? tiles : budget;
    return parts > 1 ? (uint32_t)parts : 1u;
}

hipError_t launch_align_keys(const AlignSource& src, const uint32_t* d_qwords, const uint2* d_qdesc, uint32_t n_queries, uint32_t k,
                             const unsigned long long* d_keys, uint64_t index_base, uint64_t max_offsets,
                             unsigned long long* d_best, int32_t* d_lags, float* d_scores, hipStream_t stream) {
    if (n_queries == 0 || k == 0) return hipSuccess;
    const uint64_t pairs = (uint64_t)n_queries * k;
    const uint32_t parts = align_parts(pairs, max_offsets);
    if (parts > 1 && !d_best) return hipErrorInvalidValue;
    const AlignArgs a = make_args(src, index_base);
    const uint64_t work = pairs * parts;
    const dim3 grid(strided_grid(work, kAlMaxGrid));
    if (parts > 1) {
        const hipError_t e = hipMemsetAsync(d_best, 0, pairs * sizeof(unsigned long long), stream);
        if (e != hipSuccess) return e;
    }
    if (src.ragged)
        hipLaunchKernelGGL(align_keys_kernel<true>, grid, dim3(kAlThreads), 0, stream, a, d_qwords, d_qdesc, d_keys, k, pairs, parts,
                           d_best, d_lags, d_scores);
    else
        hipLaunchKernelGGL(align_keys_kernel<false>, grid, dim3(kAlThreads), 0, stream, a, d_qwords, d_qdesc, d_keys, k, pairs, parts,
                           d_best, d_lags, d_scores);
    if (parts > 1) {
        const uint64_t blocks = (pairs + kFinishThreads - 1) / kFinishThreads;
        const dim3 fgrid(strided_grid(blocks, kAlMaxGrid));
        if (src.ragged)
            hipLaunchKernelGGL(align_finish_kernel<true>, fgrid, dim3(kFinishThreads), 0, stream, a, d_qwords, d_qdesc, d_keys, k, pairs,
                               d_best, d_lags, d_scores);
        else
            hipLaunchKernelGGL(align_finish_kernel<false>, fgrid, dim3(kFinishThreads), 0, stream, a, d_qwords, d_qdesc, d_keys, k, pairs,
                               d_best, d_lags, d_scores);
    }
    return hipGetLastError();
}

hipError_t launch_align_profile(const AlignSource& src, const uint32_t* d_qwords, uint32_t n_query, uint64_t entry, uint64_t n_offsets,
                                float* d_out, hipStream_t stream) {
    if (n_offsets == 0) return hipSuccess;
    const AlignArgs a = make_args(src, 0);
    const uint64_t tiles = tiles_of(n_offsets);
    const dim3 grid(strided_grid(tiles, kAlMaxGrid));
    if (src.ragged)
        hipLaunchKernelGGL(align_profile_kernel<true>, grid, dim3(kAlThreads), 0, stream, a, d_qwords, n_query, entry, d_out);
    else
        hipLaunchKernelGGL(align_profile_kernel<false>, grid, dim3(kAlThreads), 0, stream, a, d_qwords, n_query, entry, d_out);
    return hipGetLastError();
}

}  // namespace lbad
