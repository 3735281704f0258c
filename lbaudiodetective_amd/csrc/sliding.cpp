// sliding.cpp -- the host side of the ragged-corpus scan: the masks and the quotient table, the block of a query, the ONE
// place where a launch's kernel is decided (sliding_choose), and the launcher that performs what was decided.  No kernel lives
// here: k_sliding.hip has the task scan and its plan, k_sliding_short.hip the two systolic scans, k_records.hip the records.
#include "sliding_common.hpp"

#include <mutex>

namespace lbad {
namespace {

struct TriTable {
    std::mutex lock;
    float* d[kMaxDevices] = {};
};
TriTable g_tri;

}  // namespace

uint4 pair_mask(uint32_t limit) {
    const uint32_t pairs = (limit + 1u) / 2u;
    uint32_t m[4];
    for (uint32_t w = 0; w < 4; ++w) {
        const uint32_t base = 32u * w;
        m[w] = pairs <= base ? 0u : (pairs - base >= 32u ? 0xFFFFFFFFu : ((1u << (pairs - base)) - 1u));
    }
    return make_uint4(m[0], m[1], m[2], m[3]);
}

uint4 sliding_range_mask(uint32_t subfp_len, uint32_t range) {
    return pair_mask(range < subfp_len ? range : subfp_len);      // Fp.m:155
}

bool sliding_supported(uint32_t subfp_len) { return subfp_len >= 1 && subfp_len <= 2 * kTriPairs; }

// the table of correctly rounded quotients hits / possible, row `possible` at possible (possible + 1) / 2
const float* sliding_tri_table() {
    const int dev = current_device();
    if (dev < 0 || dev >= kMaxDevices) return nullptr;
    std::lock_guard<std::mutex> g(g_tri.lock);
    if (g_tri.d[dev]) return g_tri.d[dev];
    std::vector<float> t(kTriSize, 0.0f);
    for (uint32_t p = 1; p <= kTriPairs; ++p)
        for (uint32_t h = 0; h <= p; ++h) t[p * (p + 1) / 2 + h] = (float)h / (float)p;   // Fp.m:175
    float* d = nullptr;
    if (hipMalloc(reinterpret_cast<void**>(&d), kTriSize * sizeof(float)) != hipSuccess) return nullptr;
    if (hipMemcpy(d, t.data(), kTriSize * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(d);
        return nullptr;
    }
    g_tri.d[dev] = d;
    return d;
}

// Host: the query block of the scan from unpacked Booleans (n_query x subfp_len): 16 words per sub-fingerprint
void build_sliding_query(const Boolean* bools, uint32_t n_query, uint32_t subfp_len, uint32_t range,
                         std::vector<uint32_t>& out) {
    static_assert(sliding_block_words(1) == 2 * kQWords, "a block is kQWords per sub-fingerprint");
    out.assign(sliding_block_words(n_query), 0u);      // one zero sub-fingerprint of slack (fetch-ahead)
    const uint4 rm4 = sliding_range_mask(subfp_len, range);
    const uint32_t rm[4] = {rm4.x, rm4.y, rm4.z, rm4.w};
    const uint32_t pairs = (subfp_len + 1u) / 2u;
    for (uint32_t s = 0; s < n_query; ++s) {
        const Boolean* b = bools + (size_t)s * subfp_len;
        uint32_t* o = out.data() + (size_t)s * kQWords;
        for (uint32_t p = 0; p < pairs; ++p) {
            if (b[2 * p]) o[p >> 5] |= 1u << (p & 31);
            if (2 * p + 1 < subfp_len && b[2 * p + 1]) o[4 + (p >> 5)] |= 1u << (p & 31);
        }
        uint32_t possible = 0;
        for (uint32_t w = 0; w < 4; ++w) {
            o[8 + w] = (o[w] | o[4 + w]) & rm[w];
            possible += (uint32_t)__builtin_popcount(o[8 + w]);
        }
        o[12] = possible * (possible + 1u) / 2u;
        o[13] = possible;
    }
}

// ---- which kernel a launch takes ---------------------------------------------------------------------------------------------------
// The systolic scan (compare_short_kernel) takes
//   * queries of up to LBAD_SHORT_QUERY = 7 sub-fingerprints: one record per lane, HBM-bound (0.26 ms at 5 against 0.31 of the
//     task kernel), and
//   * corpora whose LONGEST entry has at most 15 records (the records' place fields saturate at 15, which bounds the reach
//     of a window at 14), whatever the query: "B" work on short entries costs the task kernel a window fill per n steps
//     (4 M entries of 8..15 against a query of 100: 2.1 ms systolic, 15.5 ms task kernel).
// Queries of 8..15 against longer entries went to the systolic scan's four-records-per-lane form until round 5; with the
// whole-line window fill the task kernel is 12-15 % faster there (1 M entries of 20..70: 0.315 / 0.336 / 0.352 ms at
// 8 / 12 / 15 against 0.370 / 0.382 / 0.404) and its batches of eight 13-30 %.
#ifndef LBAD_SHORT_QUERY
#define LBAD_SHORT_QUERY 7
#endif
namespace {

constexpr uint32_t kShortEntries = 15;
// the query in LDS (dynamic, 64 bytes per sub-fingerprint): up to kQueryLds sub-fingerprints; longer queries are read
// through the scalar cache
constexpr uint32_t kQueryLds = 480;
constexpr uint32_t kMultiLdsWords = 7000;     // dynamic LDS a launch of several queries may ask for (28 KB next to 131 KB of tables and queues)
// the scan may be SPLIT for queries of at least this many sub-fingerprints; the entries shorter than this then go through
// the systolic scan (a second launch over the records)
constexpr uint32_t kSlideSplitBelow = 16;

bool takes_short(uint32_t n_query, uint32_t ne_max) { return n_query <= LBAD_SHORT_QUERY || ne_max <= kShortEntries; }
// a BATCH of such queries goes through compare_short_multi_kernel (needs an entry longer than the query)
bool takes_multi(uint32_t n_query, uint32_t ne_max) { return n_query <= sliding_short_multi_max() && ne_max > n_query; }

// How many of `n_left` queries of n_query sub-fingerprints ONE launch takes: the systolic scan of short queries up to
// eight, the task scan four or two while their blocks fit the LDS next to the tables.
uint32_t queries_per_launch(uint32_t n_query, uint32_t ne_max, uint32_t n_left) {
    if (n_left <= 1) return n_left;
    if (takes_multi(n_query, ne_max)) return n_left >= 8 ? 8u : (n_left >= 4 ? 4u : 2u);    // compare_short_multi_kernel
    if (takes_short(n_query, ne_max)) {
        // one record per lane (windows of up to seven records): eight queries side by side; four records per lane: four (eight
        // would need 213 registers -- two waves per SIMD -- and gain nothing over two launches of four)
        const uint32_t look = (n_query < ne_max ? n_query : ne_max) - 1u;
        const uint32_t most = look <= 6u ? 8u : 4u;
        return n_left >= most ? most : (n_left >= 4 ? 4u : 2u);
    }
    const uint32_t most = sliding_task_max_queries();
    uint32_t g = n_left >= most ? most : (n_left >= 4 ? 4u : 2u);
    while (g > 1 && (uint64_t)g * (n_query + 1u) * kQWords > kMultiLdsWords) g >>= 1;
    return g;
}

// Split the scan?  An entry of n <= 15 sub-fingerprints against a longer query of nq costs the task kernel a pass of nq steps
// per four of its nq - n + 1 offsets, n of which meet the entry: measured 2 300 G (step, offset) slots per second whatever
// n is.  The systolic scan spends nq steps on EVERY record of a chunk that holds such an entry (2 200 G record-steps per
// second, and not less than reading the records once).  Worth a second launch when the short entries' slots are well above
// the whole corpus' record-steps.  Kernel variant 3 forces the split (where one exists), 4 forbids it.
uint32_t split_below(const SlideCorpusStats& c, uint64_t nq) {
    if (takes_short((uint32_t)nq, c.ne_max) || nq < kSlideSplitBelow || c.variant == 4) return 0;
    uint64_t slots = 0, entries = 0;
    for (const auto& kv : *c.len_hist) {
        const uint64_t ne = kv.first;
        if (ne >= kSlideSplitBelow || ne > nq) continue;
        slots += kv.second * ((nq - ne + 4) / 4) * 4 * nq;
        entries += kv.second;
    }
    if (entries == 0) return 0;
    if (c.variant == 3) return kSlideSplitBelow;
    return slots > 2 * c.n_pos * nq + 20000000ull ? kSlideSplitBelow : 0;     // (+ 10 us of slots: a second launch is not free)
}

// tasks of either kind for queries of nq sub-fingerprints, from the histogram of entry lengths (Fp.m:123-136: an entry
// longer than the query slides the query along itself, any other entry slides along the query; "B" entries shorter than
// b_min are left out -- the split's systolic launch has them)
void count_tasks(const SlideCorpusStats& c, uint64_t nq, uint64_t b_min, uint64_t& tasks_a, uint64_t& tasks_b) {
    tasks_a = tasks_b = 0;
    for (const auto& kv : *c.len_hist) {
        const uint64_t ne = kv.first;
        if (ne > nq) tasks_a += kv.second * ((ne - nq + 4) / 4);
        else if (ne >= b_min) tasks_b += kv.second * ((nq - ne + 4) / 4);
    }
}

// Shape of a task scan: one workgroup per CU, each with 1 / grid of the tasks of either kind (whole entries).
SlideShape task_shape(uint64_t tasks_a, uint64_t tasks_b, uint32_t n_q, uint32_t cus) {
    SlideShape sh;
    const uint64_t waves = sliding_task_threads(n_q) / 64;
    const uint64_t passes = (tasks_a + 63) / 64 + (tasks_b + 63) / 64;
    const uint64_t want = (passes + waves - 1) / waves;
    uint64_t cap = (uint64_t)cus * sliding_task_groups_per_cu();
    if (cap > kSlideMaxGrid) cap = kSlideMaxGrid;
    sh.grid = (uint32_t)(want < cap ? (want ? want : 1) : cap);
    auto chunk = [&](uint64_t tasks) -> uint32_t {
        if (tasks == 0) return 0u;
        const uint64_t per = (tasks + sh.grid - 1) / sh.grid;
        return (uint32_t)(per ? per : 1);
    };
    sh.chunk_a = chunk(tasks_a);
    sh.chunk_b = chunk(tasks_b);
    return sh;
}

}  // namespace

SlideChoice sliding_choose(const SlideCorpusStats& c, const SlideGroup& g, uint32_t cus) {
    SlideChoice ch;
    const uint32_t nq = g.n_query;
    if (nq == 0 || g.n_left == 0 || !c.len_hist) return ch;
    const uint32_t n_take = g.scores ? 1u : queries_per_launch(nq, c.ne_max, g.n_left);
    ch.cus = cus;
    ch.b_min = split_below(c, nq);
    count_tasks(c, nq, ch.b_min, ch.tasks_a, ch.tasks_b);
    if (ch.tasks_a > 0xFFFFFFFFull || ch.tasks_b > 0xFFFFFFFFull || ch.tasks_a + ch.tasks_b == 0) return ch;   // the plan counts in 32 bits
    ch.shape = task_shape(ch.tasks_a, ch.tasks_b, n_take, cus);
    ch.n_take = n_take;
    if (n_take > 1 && takes_multi(nq, c.ne_max) && ch.tasks_a != 0) {
        // several queries of up to LBAD_SHORT_MULTI_MAX (12) sub-fingerprints, keys only: the entries longer than the query
        // through compare_short_multi_kernel, the others -- where the corpus has any -- through the systolic scan in its
        // only_upto mode, which maxes into the same keys
        ch.kernel = SlideKernel::ShortMulti;
        ch.look = nq - 1u;
        ch.maxes_keys = true;
        ch.second = ch.tasks_b != 0;
        if (ch.second) { ch.second_look = nq - 1u; ch.second_only_upto = nq; }
        return ch;
    }
    if (takes_short(nq, c.ne_max)) {
        ch.kernel = SlideKernel::Short;
        ch.look = (nq < c.ne_max ? nq : c.ne_max) - 1u;
        ch.maxes_keys = true;
        return ch;
    }
    ch.kernel = SlideKernel::Task;
    const uint4 rm = sliding_range_mask(c.subfp_len, g.range), all = pair_mask(c.subfp_len);
    ch.full = rm.x == all.x && rm.y == all.y && rm.z == all.z && rm.w == all.w;
    ch.qlds = n_take > 1 || nq <= kQueryLds;
    ch.threads = sliding_task_threads(n_take);
    ch.reads_plan = true;
    // The corpus is split: "B" entries of fewer than b_min sub-fingerprints are no tasks (an entry of n records costs the
    // task kernel a pass of n_query steps per four offsets whatever n is: 15.5 ms against 2.1 for 4 M entries of 8..15 and a
    // query of 100).  The systolic scan takes them -- every record once, n_query steps per record, nothing for chunks
    // without such an entry -- and maxes into the keys the task kernel has just written (same stream).
    ch.second = ch.b_min != 0;
    if (ch.second) { ch.second_look = ch.b_min - 2u; ch.second_only_upto = ch.b_min - 1u; }
    // a query of up to kSlideQueryArgSubs sub-fingerprints fits the kernel's argument segment -- unless a systolic launch
    // follows, which reads the block from the device
    ch.q_in_args = g.host_blocks && n_take == 1 && nq <= kSlideQueryArgSubs && !ch.second;
    return ch;
}

void sliding_choice_words(const SlideChoice& ch, uint32_t n_query, uint32_t* w) {
    for (int i = 0; i < 21; ++i) w[i] = 0;
    if (ch.n_take == 0) return;
    w[0] = ch.n_take; w[1] = (uint32_t)ch.kernel;
    if (ch.kernel == SlideKernel::Task) { w[2] = ch.full; w[3] = ch.qlds; w[4] = ch.n_take; w[5] = ch.threads; }
    else if (ch.kernel == SlideKernel::Short) { w[2] = ch.look <= 6u ? 1u : 4u; w[3] = ch.n_take; }
    else { w[2] = ch.n_take; w[3] = n_query; }
    w[6] = ch.b_min;
    w[7] = (uint32_t)ch.tasks_a; w[8] = (uint32_t)(ch.tasks_a >> 32); w[9] = (uint32_t)ch.tasks_b; w[10] = (uint32_t)(ch.tasks_b >> 32);
    w[11] = ch.shape.grid; w[12] = ch.shape.chunk_a; w[13] = ch.shape.chunk_b;
    w[14] = ch.reads_plan; w[15] = ch.q_in_args; w[16] = ch.maxes_keys;
    w[17] = ch.second; w[18] = ch.second_look; w[19] = ch.second_only_upto; w[20] = ch.kernel == SlideKernel::Task ? 0u : ch.look;
}

// The launches the choice names, on call.stream.  (The caller has zeroed the keys where choice.maxes_keys.)
hipError_t launch_compare_sliding(const SlideCorpus& src, const SlideChoice& ch, const SlideScan& scan, const SlideCall& call) {
    if (src.n_entries == 0 || call.n_query == 0 || ch.n_take == 0) return hipErrorInvalidValue;
    if (call.n_query >= (1u << 20)) return hipErrorInvalidValue;                             // (run_pass: 32-bit lane offsets)
    if (ch.n_take > 1 && call.d_score_bits) return hipErrorInvalidValue;
    const float* tri = sliding_tri_table();
    if (!tri) return hipErrorOutOfMemory;
    hipError_t launched = hipErrorInvalidValue;
    switch (ch.kernel) {
        case SlideKernel::Task: launched = launch_sliding_task(src, ch, scan, call, tri); break;
        case SlideKernel::Short: launched = launch_sliding_short(src, ch, scan, call, tri, ch.look, 0u); break;
        case SlideKernel::ShortMulti: launched = launch_sliding_short_multi(src, ch, scan, call); break;
    }
    if (launched != hipSuccess || !ch.second) return launched;
    return launch_sliding_short(src, ch, scan, call, tri, ch.second_look, ch.second_only_upto);
}

}  // namespace lbad
