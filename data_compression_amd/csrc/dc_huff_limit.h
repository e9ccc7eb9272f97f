/* dc_huff_limit.h -- the arithmetic of a length-limited n-ary code (dc_gpu.h "Length-limited
 * tables"): given how many present symbols Huffman put at each length, with every
 * length past the cap D counted at D, repair the counts until they fit a D-digit code (Kraft)
 * and then spend the room that is left. No dependency but <stdint.h>, so the table kernel
 * (dc_core.hip), libdc_core's host export dc_huff_limit_classes and a stand-alone checker
 * (tests/c/huff_limit_check.c, built with the sanitizers) compile the same function. */
#ifndef DC_HUFF_LIMIT_H
#define DC_HUFF_LIMIT_H
#include <stdint.h>

#ifdef __HIPCC__
#define DC_HL_FN static __host__ __device__ __forceinline__
#else
#define DC_HL_FN static inline
#endif

/* A cap of D digits at arity n is one the packed code can hold: 1 <= D <= max_d (DC_MAX_DIGITS)
 * and D * w <= 32 with w = ceil(log2 n). Returns w, or 0 for an invalid pair. */
DC_HL_FN int dc_huff_limit_cap_ok(int n, int D, int max_d)
{
    if (n < 2 || n > 256 || D < 1 || D > max_d) return 0;
    int w = 0;
    while ((1 << w) < n) ++w;
    return D * w <= 32 ? w : 0;
}

/* n^D when it is <= cap, else cap + 1 (n >= 2, D >= 0, cap < 2^63: no product wraps). */
DC_HL_FN uint64_t dc_huff_limit_pow_sat(int n, int D, uint64_t cap)
{
    uint64_t p = 1;
    for (int i = 0; i < D; ++i) {
        if (p > cap / (uint64_t)n) return cap + 1;
        p *= (uint64_t)n;
    }
    return p <= cap ? p : cap + 1;
}

/* cnt[d], 1 <= d <= D: the present symbols of length min(l, D); cnt[0] is not read; k their
 * number. D * ceil(log2 n) <= 32 (dc_huff_limit_cap_ok), so n^D <= 2^32 and, with k < 2^31, the
 * Kraft sum K = sum cnt[d] n^(D-d) stays below 2^63.
 *   -1 (DC_E_ARG)  sum cnt != k, or n^D < k: no D-digit code holds k symbols (cnt unchanged)
 *    0             cnt repaired in place:
 *   demote   while K > n^D: one symbol of the longest length d < D in use moves to d + 1
 *            (K falls by (n-1) n^(D-d-1); with all k at D, K = k <= n^D, so this ends);
 *   promote  for d = D down to 2: while a symbol of length d can move to d - 1 with K still
 *            <= n^D, it does (K grows by (n-1) n^(D-d)).
 * Returns the number of moves made through *steps when steps is not NULL. */
DC_HL_FN int dc_huff_limit_repair(int n, int D, uint32_t *cnt, uint64_t k, uint32_t *steps)
{
    uint64_t sum = 0;
    for (int d = 1; d <= D; ++d) sum += cnt[d];
    if (sum != k || k >> 31) return -1;
    const uint64_t B = dc_huff_limit_pow_sat(n, D, (uint64_t)1 << 32);
    if (B < k) return -1;
    uint64_t K = 0, p = 1;   /* p = n^(D-d) */
    for (int d = D; d >= 1; --d) {
        K += (uint64_t)cnt[d] * p;
        if (d > 1) p *= (uint64_t)n;
    }
    uint32_t moves = 0;
    while (K > B) {
        int d = D - 1;
        uint64_t q = 1;      /* q = n^(D-d-1) */
        while (d >= 1 && cnt[d] == 0) { --d; q *= (uint64_t)n; }
        if (d < 1) return -1;   /* cannot happen: K > B >= k needs a symbol above D */
        --cnt[d];
        ++cnt[d + 1];
        K -= (uint64_t)(n - 1) * q;
        ++moves;
    }
    uint64_t c = (uint64_t)(n - 1);   /* (n-1) n^(D-d) */
    for (int d = D; d >= 2; --d) {
        while (cnt[d] > 0 && K + c <= B) {
            --cnt[d];
            ++cnt[d - 1];
            K += c;
            ++moves;
        }
        c *= (uint64_t)n;
    }
    if (steps) *steps = moves;
    return 0;
}
#endif
