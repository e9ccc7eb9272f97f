/* dc_range_span.h -- the arithmetic of dc_huff_range_span (dc_host.h): which groups and which
 * payload bits of a stream the symbols [first, first + count) need. Pure host code with no
 * dependency but <stdint.h>, so libdc_core.so (dc_host.hip) and a stand-alone checker
 * (tests/c/range_span_check.c, built with the sanitizers) compile the same function. */
#ifndef DC_RANGE_SPAN_H
#define DC_RANGE_SPAN_H
#include <stdint.h>

/* 0, or -1 (DC_E_ARG): a null pointer, a sync_syms that is no power of two in 16..1024,
 * first + count > n. count 0 (first <= n) gives the one group `first` lies in (the last group
 * for first == n); n == 0 gives all zeros. */
static inline int dc_range_span_calc(uint64_t n, uint32_t sync_syms, const uint64_t *h_sync_base, uint64_t end_bit,
                                     uint64_t first, uint64_t count, uint64_t out[4])
{
    if (!out || sync_syms < 16 || sync_syms > 1024 || (sync_syms & (sync_syms - 1))) return -1;
    if (first > n || count > n - first) return -1;
    out[0] = out[1] = out[2] = out[3] = 0;
    if (n == 0) return 0;
    if (!h_sync_base) return -1;
    const uint64_t gsyms = 64ull * sync_syms;   /* symbols per group of 64 chunks */
    const uint64_t groups = (n + gsyms - 1) / gsyms;
    uint64_t g0 = first / gsyms, g1;
    if (g0 >= groups) g0 = groups - 1;           /* first == n on a group boundary */
    g1 = count ? (first + count - 1) / gsyms : g0;
    out[0] = g0;
    out[1] = g1;
    out[2] = h_sync_base[g0];
    out[3] = g1 + 1 < groups ? h_sync_base[g1 + 1] : end_bit;
    return 0;
}
#endif
