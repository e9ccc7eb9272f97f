/* Stand-alone check of the batch codec's range arithmetic (csrc/dc_batch_range.h), meant to be
 * built with the host sanitizers; it needs no device and no library:
 *
 *   cc -std=c11 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
 *      -Idata_compression_amd/csrc tests/c/batch_range_check.c -o batch_range_check && ./batch_range_check
 *
 * Exhaustively over small S, len, first and count: the chunk interval is exactly the set of
 * chunks that hold a byte of the range (marked byte by byte in an array allocated to the exact
 * chunk count, so an interval past the segment's chunks is a caught write), and the argument
 * tests agree with the same tests done in 128-bit sums. Then the u64 edges, where a test written
 * as a sum would wrap. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "dc_batch_range.h"

static int fails;
#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

typedef unsigned __int128 u128;

static void chunks_small(uint32_t S, uint32_t len)
{
    const uint32_t nch = (len + S - 1) / S;
    unsigned char *hit = (unsigned char *)malloc(nch ? nch : 1);
    for (uint32_t first = 0; first <= len; ++first)
        for (uint32_t count = 0; count <= len - first; ++count) {
            uint64_t lo, hi;
            dc_batch_range_chunks(first, count, S, &lo, &hi);
            CHECK(lo <= hi);
            if (count == 0) {
                CHECK(lo == hi && lo == first / S);
                continue;
            }
            CHECK(hi <= nch);
            memset(hit, 0, nch);
            for (uint32_t k = first; k < first + count; ++k) hit[k / S] = 1;
            for (uint32_t c = 0; c < nch; ++c) CHECK(hit[c] == (c >= lo && c < hi));
        }
    free(hit);
}

static int args_wide(uint32_t len, uint64_t first, uint64_t count, uint64_t out_off, uint64_t out_cap)
{
    if ((u128)first + count > len) return -1;
    if ((u128)out_off + count > out_cap) return -6;
    return 0;
}

int main(void)
{
    const uint32_t syncs[4] = {1, 3, 4, 16};   /* (the kernels take powers of two from 16; the arithmetic takes any S > 0) */
    for (int s = 0; s < 4; ++s)
        for (uint32_t len = 0; len <= 70; ++len) chunks_small(syncs[s], len);
    chunks_small(64, 130);

    /* the argument tests against 128-bit sums: small values, then values at the u64 edges */
    const uint64_t edge[10] = {0, 1, 2, 7, 8, 9, ~0ull - 8, ~0ull - 1, ~0ull, 1ull << 63};
    for (uint32_t len = 0; len <= 9; ++len)
        for (int a = 0; a < 10; ++a)
            for (int b = 0; b < 10; ++b)
                for (int c = 0; c < 10; ++c)
                    for (int d = 0; d < 10; ++d)
                        CHECK(dc_batch_range_args(len, edge[a], edge[b], edge[c], edge[d]) ==
                              args_wide(len, edge[a], edge[b], edge[c], edge[d]));
    CHECK(dc_batch_range_args(65536, ~0ull, 2, 0, 100) == -1);        /* first + count wraps to 1 */
    CHECK(dc_batch_range_args(65536, 65535, 1, ~0ull, ~0ull) == -6);  /* out_off + count wraps to 0 */
    CHECK(dc_batch_range_args(65536, 65535, 1, ~0ull - 1, ~0ull) == 0);
    CHECK(dc_batch_range_args(65536, 0, 65536, 0, 65535) == -6);
    CHECK(dc_batch_range_args(65536, 0, 65537, 0, ~0ull) == -1);
    CHECK(dc_batch_range_args(0, 0, 0, 0, 0) == 0);

    /* segment lengths */
    uint32_t len = 77;
    CHECK(dc_batch_range_seg_len(5, 4, 65536, &len) == -1 && len == 77);
    CHECK(dc_batch_range_seg_len(0, 65537, 65536, &len) == -1 && len == 77);
    CHECK(dc_batch_range_seg_len(0, ~0ull, 65536, &len) == -1);
    CHECK(dc_batch_range_seg_len(~0ull, 0, 65536, &len) == -1);
    CHECK(dc_batch_range_seg_len(~0ull - 65536, ~0ull, 65536, &len) == 0 && len == 65536);
    CHECK(dc_batch_range_seg_len(9, 9, 65536, &len) == 0 && len == 0);

    /* the chunk interval at the u64 edges: against 128-bit arithmetic */
    const uint32_t big_s[3] = {16, 64, 1024};
    for (int s = 0; s < 3; ++s)
        for (int a = 0; a < 10; ++a)
            for (int b = 0; b < 10; ++b) {
                const uint64_t first = edge[a], count = edge[b];
                if ((u128)first + count > ((u128)1 << 64)) continue;   /* ranges whose end fits */
                uint64_t lo, hi;
                dc_batch_range_chunks(first, count, big_s[s], &lo, &hi);
                CHECK(lo == first / big_s[s]);
                CHECK((u128)hi == (count ? ((u128)first + count - 1) / big_s[s] + 1 : (u128)lo));
            }
    printf(fails ? "batch_range_check: %d failures\n" : "batch_range_check: ok\n", fails);
    return fails != 0;
}
