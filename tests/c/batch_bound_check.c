/* Stand-alone check of the batch codec's buffer bounds (csrc/dc_batch_bound.h), meant to be
 * built with the host sanitizers; it needs no device and no library:
 *
 *   cc -std=c11 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
 *      -Idata_compression_amd/csrc tests/c/batch_bound_check.c -o batch_bound_check && ./batch_bound_check
 *
 * The formulas at the values of tests/test_batch_cpu.py, and the claim behind them: a layout
 * computed segment by segment (payload rounded up to 16 bytes, ceil(len / S) sync entries, the
 * stored fallback as the worst case) never passes the bounds, whatever the segment lengths. The
 * offset arrays are allocated exactly, so a write past them is caught. */
#include <stdio.h>
#include <stdlib.h>

#include "dc_batch_bound.h"

static int fails;
#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

static void layout(uint64_t count, uint32_t S, uint32_t seed)
{
    uint64_t *pay_off = (uint64_t *)malloc((count + 1) * sizeof(uint64_t));
    uint64_t *sync_off = (uint64_t *)malloc((count + 1) * sizeof(uint64_t));
    uint64_t total = 0;
    pay_off[0] = sync_off[0] = 0;
    for (uint64_t i = 0; i < count; ++i) {
        seed = seed * 1664525u + 1013904223u;
        const uint64_t len = (seed >> 8) % 65537u;            /* 0 .. 65536 */
        const uint64_t bytes = len;                           /* stored: the worst case */
        pay_off[i + 1] = pay_off[i] + (bytes + 15) / 16 * 16;
        sync_off[i + 1] = sync_off[i] + (len + S - 1) / S;
        total += len;
    }
    CHECK(pay_off[count] <= dc_batch_payload_bound_calc(total, count));
    CHECK(sync_off[count] <= dc_batch_sync_bound_calc(total, count, S));
    free(pay_off);
    free(sync_off);
}

int main(void)
{
    const uint64_t totals[4] = {0, 1, 65536, (1ull << 33) + 5}, counts[3] = {0, 1, 300};
    const uint32_t syncs[3] = {16, 64, 1024};
    for (int a = 0; a < 4; ++a)
        for (int b = 0; b < 3; ++b) {
            CHECK(dc_batch_payload_bound_calc(totals[a], counts[b]) == totals[a] + 16 * counts[b]);
            for (int s = 0; s < 3; ++s)
                CHECK(dc_batch_sync_bound_calc(totals[a], counts[b], syncs[s]) ==
                      (totals[a] + syncs[s] - 1) / syncs[s] + counts[b]);
        }
    CHECK(dc_batch_sync_bound_calc(12345, 7, 0) == 0);
    CHECK(dc_batch_sync_bound_calc(~0ull, 0, 16) == (~0ull) / 16 + 1);   /* no overflow in the rounding */
    for (int s = 0; s < 3; ++s) {
        layout(0, syncs[s], 1);
        layout(1, syncs[s], 2);
        layout(300, syncs[s], 3);
        layout(4099, syncs[s], 4);
    }
    printf(fails ? "batch_bound_check: %d failures\n" : "batch_bound_check: ok\n", fails);
    return fails != 0;
}
