/* Stand-alone check of the nybble batch codec's output bound (csrc/dc_nyb_batch_bound.h), meant
 * to be built with the host sanitizers; it needs no device and no library:
 *
 *   cc -std=c11 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
 *      -Idata_compression_amd/csrc tests/c/nyb_batch_bound_check.c -o nyb_batch_bound_check && ./nyb_batch_bound_check
 *
 * The formula at the values of tests/test_nyb_batch_cpu.py, and the claim behind it: offsets
 * computed buffer by buffer (the LITERAL form as the worst case: len + 1 bytes, 1 byte for an
 * empty buffer) never pass the bound, and reach it when every buffer is LITERAL. The offset array
 * is allocated exactly, so a write past it is caught. */
#include <stdio.h>
#include <stdlib.h>

#include "dc_nyb_batch_bound.h"

static int fails;
#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

/* the longest stream of a buffer of len bytes: the nybble form is kept only below len bytes */
static uint64_t worst(uint64_t len) { return len + 1; }

static void layout(uint64_t count, uint32_t seed, int all_literal)
{
    uint64_t *off = (uint64_t *)malloc((count + 1) * sizeof(uint64_t));
    uint64_t total = 0;
    off[0] = 0;
    for (uint64_t i = 0; i < count; ++i) {
        seed = seed * 1664525u + 1013904223u;
        const uint64_t len = (seed >> 8) % 70001u;             /* 0 .. 70000 */
        uint64_t stream = worst(len);
        if (!all_literal && len >= 6 && (seed & 1u)) stream = len / 2 + 2 + (seed >> 4) % (len - len / 2 - 2);   /* a nybble form: < len */
        CHECK(stream <= worst(len));
        off[i + 1] = off[i] + stream;
        total += len;
    }
    CHECK(off[count] <= dc_nyb_batch_bound_calc(total, count));
    if (all_literal) CHECK(off[count] == dc_nyb_batch_bound_calc(total, count));
    free(off);
}

int main(void)
{
    const uint64_t totals[4] = {0, 1, 65536, (1ull << 33) + 5}, counts[3] = {0, 1, 300};
    for (int a = 0; a < 4; ++a)
        for (int b = 0; b < 3; ++b) CHECK(dc_nyb_batch_bound_calc(totals[a], counts[b]) == totals[a] + counts[b]);
    CHECK(dc_nyb_batch_bound_calc(0, 1) == 1);   /* one empty buffer: ' ' */
    for (int lit = 0; lit < 2; ++lit) {
        layout(0, 1, lit);
        layout(1, 2, lit);
        layout(300, 3, lit);
        layout(4099, 4, lit);
    }
    printf(fails ? "nyb_batch_bound_check: %d failures\n" : "nyb_batch_bound_check: ok\n", fails);
    return fails != 0;
}
