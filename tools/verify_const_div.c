/* Exhaustive check of the constant-division shortcut used by k_haar_select32.hip and k_rows_pruned.hip:
 *     q0 = x * r;  e = fma(-d, q0, x);  q = fma(e, r, q0)        with r = RN(1 / d)
 * against the correctly rounded x / d.
 *
 * Without arguments: EVERY float32 bit pattern x, for the three divisors the Haar uses (sqrtf(2), sqrtf(32),
 * sqrtf(128)).  Prints, per divisor, how many inputs disagree and the magnitude range that contains every disagreement.
 *
 * With a list of divisors (the band means of stage 1, whose dividends are sums of squares: +0, positive finite or
 * +inf, never NaN and never negative):
 *     verify_const_div [--lo BITS] [--hi BITS] D [D ...]
 * checks every NON-NEGATIVE bit pattern in [lo, hi] (default 0 .. 0x7f800000: +0, the denormals, every finite value
 * and +inf) and prints, per divisor, one line
 *     d = 3 (bits 40400000), r bits 3eaaaaab: exact on [00000000, 00000000] and [LLLLLLLL, HHHHHHHH], N mismatches ...
 * where [L, H] is the largest run of bit patterns around 1.0f without a mismatch inside the checked range, followed
 * by the runs of mismatches below and above it.  +0 is reported on its own: it sits below the denormals, which fail.
 * build: gcc -O2 -mfma -fopenmp -ffp-contract=off tools/verify_const_div.c -o /tmp/verify_const_div -lm */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static inline float from_bits(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static inline uint32_t to_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

static inline int same_quotient(float x, float d, float r) {
    const float want = x / d;
    const float q0 = x * r;
    const float e = fmaf(-d, q0, x);
    const float q = fmaf(e, r, q0);
    if (to_bits(q) == to_bits(want)) return 1;
    return want != want && q != q; /* both NaN */
}

static int haar_divisors(void) {
    const float ds[3] = {sqrtf(2.0f), sqrtf(32.0f), sqrtf(128.0f)};
    for (int t = 0; t < 3; ++t) {
        const float d = ds[t], r = 1.0f / d;
        unsigned long long bad = 0;
        uint32_t lo_bad = 0xFFFFFFFFu, hi_bad = 0;
#pragma omp parallel for reduction(+ : bad) reduction(min : lo_bad) reduction(max : hi_bad) schedule(static)
        for (long long i = 0; i < (1LL << 32); ++i) {
            const uint32_t u = (uint32_t)i;
            if (!same_quotient(from_bits(u), d, r)) {
                ++bad;
                const uint32_t mag = u & 0x7fffffffu;
                if (mag < lo_bad) lo_bad = mag;
                if (mag > hi_bad) hi_bad = mag;
            }
        }
        printf("d = %.9g (bits %08x), r = %.9g: %llu mismatches", d, to_bits(d), r, bad);
        if (bad) printf(", |x| bits in [%08x, %08x] = [%g, %g]", lo_bad, hi_bad, from_bits(lo_bad), from_bits(hi_bad));
        printf("\n");
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) return haar_divisors();
    const uint32_t one = 0x3F800000u;
    uint32_t lo = 0u, hi = 0x7F800000u;
    int a = 1;
    for (; a + 1 < argc; a += 2) {
        if (!strcmp(argv[a], "--lo")) lo = (uint32_t)strtoul(argv[a + 1], NULL, 16);
        else if (!strcmp(argv[a], "--hi")) hi = (uint32_t)strtoul(argv[a + 1], NULL, 16);
        else break;
    }
    if (a >= argc || lo > hi || hi > 0x7F800000u) {
        fprintf(stderr, "usage: %s [--lo HEXBITS] [--hi HEXBITS] divisor [divisor ...]\n", argv[0]);
        return 2;
    }
    printf("# dividend bit patterns checked: [%08x, %08x]\n", lo, hi);
    for (; a < argc; ++a) {
        const float d = strtof(argv[a], NULL), r = 1.0f / d;
        /* mismatches below 1.0f: count and [first, last]; the same above */
        unsigned long long n_below = 0, n_above = 0;
        uint32_t below_first = 0xFFFFFFFFu, below_last = 0, above_first = 0xFFFFFFFFu, above_last = 0;
#pragma omp parallel for reduction(+ : n_below, n_above) reduction(min : below_first, above_first) \
    reduction(max : below_last, above_last) schedule(static)
        for (long long i = (long long)lo; i <= (long long)hi; ++i) {
            const uint32_t u = (uint32_t)i;
            if (same_quotient(from_bits(u), d, r)) continue;
            if (u < one) {
                ++n_below;
                if (u < below_first) below_first = u;
                if (u > below_last) below_last = u;
            } else {
                ++n_above;
                if (u < above_first) above_first = u;
                if (u > above_last) above_last = u;
            }
        }
        const uint32_t run_lo = n_below ? below_last + 1 : lo, run_hi = n_above ? above_first - 1 : hi;
        printf("d = %.9g (bits %08x), r bits %08x: ", d, to_bits(d), to_bits(r));
        if (run_lo > run_hi) printf("exact nowhere around 1.0");
        else printf("exact on [%08x, %08x] = [%g, %g]", run_lo, run_hi, from_bits(run_lo), from_bits(run_hi));
        if (lo == 0u) printf(", +0 %s", below_first == 0u ? "FAILS" : "exact");
        printf(", %llu mismatches", n_below + n_above);
        if (n_below) printf(", below in [%08x, %08x]", below_first, below_last);
        if (n_above) printf(", above in [%08x, %08x]", above_first, above_last);
        printf("\n");
        fflush(stdout);
    }
    return 0;
}
