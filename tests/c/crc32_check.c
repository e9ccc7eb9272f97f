/* Stand-alone check of the CRC-32 arithmetic (csrc/dc_crc32.h), meant to be built with the host
 * sanitizers; it needs no device and no library:
 *
 *   cc -std=c11 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
 *      -Idata_compression_amd/csrc tests/c/crc32_check.c -o crc32_check && ./crc32_check
 *
 * The check value; the table-driven update against the bitwise one on every length 0..300 (each
 * buffer allocated to its exact length, so a read past it is caught), whole and in running form;
 * the combine against the direct CRC at every split of a 257-byte buffer, len_b 0 and 1 among
 * them; x^(8 n) at n = 2^32 + 5 and n = 2^40 against xpow(a + b) = xpow(a) xpow(b); the tables of
 * a constant product against the product; and the folding scheme of the kernels
 * (dc_crc_kernels.inc: 64 registers over tiles aligned to the buffer's end, the head masked, the
 * start value in the first four bytes, the last granule as a running tail) as a plain C model on
 * every length 0..2100 at every 16-B phase. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "dc_crc32.h"

static int fails;
#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

static uint32_t T[4][256], MK[4][256];
static uint32_t rnd_state = 12345u;
static uint8_t rnd(void)
{
    rnd_state = rnd_state * 1664525u + 1013904223u;
    return (uint8_t)(rnd_state >> 24);
}

/* the reference: the register a bit at a time, in zlib's running form */
static uint32_t dc_crc32_update_bitwise(uint32_t crc, const uint8_t *p, size_t n)
{
    crc = ~crc;
    for (size_t i = 0; i < n; ++i) {
        crc ^= p[i];
        for (int k = 0; k < 8; ++k) crc = (crc >> 1) ^ ((crc & 1u) ? DC_CRC_POLY : 0u);
    }
    return ~crc;
}

static uint32_t mulk(uint32_t s)
{
    return MK[0][s & 255u] ^ MK[1][(s >> 8) & 255u] ^ MK[2][(s >> 16) & 255u] ^ MK[3][s >> 24];
}

/* the kernels' scheme on region[0 .. 16 ng): the aligned granules that hold x[0 .. n) = region[sh .. sh + n) */
static uint32_t fold_model(const uint8_t *region, uint32_t sh, uint32_t n)
{
    if (n == 0) return 0;
    const uint32_t ng = (sh + n + 15) / 16, nga = ng - 1;
    const uint32_t nt = (nga + 63) / 64, pad = nt * 64 - nga;
    const int init = n >= 4;
    uint8_t *m = (uint8_t *)calloc(16u * ng, 1);   /* masked, with the start value in */
    for (uint32_t k = 0; k < n; ++k) m[sh + k] = region[sh + k] ^ (uint8_t)((init && k < 4) ? 0xFF : 0);
    uint32_t c = 0;
    if (nt) {
        uint32_t s[64] = {0};
        for (uint32_t t = 0; t < nt; ++t)
            for (uint32_t l = 0; l < 64; ++l) {
                const uint32_t gp = t * 64 + l;
                uint32_t r = 0;
                if (gp >= pad) {
                    const uint8_t *g = m + 16u * (gp - pad);
                    for (int j = 0; j < 4; ++j) {
                        const uint32_t d = (uint32_t)g[4 * j] | ((uint32_t)g[4 * j + 1] << 8) |
                                           ((uint32_t)g[4 * j + 2] << 16) | ((uint32_t)g[4 * j + 3] << 24);
                        r = dc_crc32_slice4((const uint32_t(*)[256])T, r ^ d);
                    }
                }
                s[l] = mulk(s[l]) ^ r;
            }
        for (uint32_t l = 0; l < 64; ++l) c ^= dc_crc32_mul(s[l], dc_crc32_xpow8(16u * (63u - l)));
    }
    const uint32_t e = ((sh + n - 1) & 15u) + 1u;
    for (uint32_t k = 0; k < e; ++k) c = T[0][(c ^ m[16u * nga + k]) & 255u] ^ (c >> 8);
    free(m);
    return c ^ (init ? 0u : dc_crc32_mul(0xFFFFFFFFu, dc_crc32_xpow8(n))) ^ 0xFFFFFFFFu;
}

int main(void)
{
    dc_crc32_slice_tables(T, 4);
    CHECK(dc_crc32_update_bitwise(0, (const uint8_t *)"123456789", 9) == 0xCBF43926u);
    CHECK(dc_crc32_update_tables((const uint32_t(*)[256])T, 0, (const uint8_t *)"123456789", 9) == 0xCBF43926u);
    CHECK(T[0][1] == 0x77073096u && T[0][255] == 0x2D02EF8Du);

    for (size_t n = 0; n <= 300; ++n) {
        uint8_t *b = (uint8_t *)malloc(n ? n : 1);
        for (size_t i = 0; i < n; ++i) b[i] = rnd();
        const uint32_t want = dc_crc32_update_bitwise(0, b, n);
        CHECK(dc_crc32_update_tables((const uint32_t(*)[256])T, 0, b, n) == want);
        const size_t a = n / 3, c = n - n / 4;   /* three pieces, running */
        uint32_t r = dc_crc32_update_tables((const uint32_t(*)[256])T, 0, b, a);
        r = dc_crc32_update_tables((const uint32_t(*)[256])T, r, b + a, c - a);
        r = dc_crc32_update_tables((const uint32_t(*)[256])T, r, b + c, n - c);
        CHECK(r == want);
        free(b);
    }

    {   /* combine at every split, len_b = 0 and 1 included */
        uint8_t b[257];
        for (int i = 0; i < 257; ++i) b[i] = rnd();
        const uint32_t whole = dc_crc32_update_bitwise(0, b, 257);
        for (size_t k = 0; k <= 257; ++k)
            CHECK(dc_crc32_combine_calc(dc_crc32_update_bitwise(0, b, k), dc_crc32_update_bitwise(0, b + k, 257 - k),
                                        257 - k) == whole);
        CHECK(dc_crc32_combine_calc(whole, 0, 0) == whole);
        CHECK(dc_crc32_combine_calc(0, whole, 257) == whole);   /* an empty A */
    }

    /* the product and the powers */
    CHECK(dc_crc32_mul(DC_CRC_X0, 0xDEADBEEFu) == 0xDEADBEEFu && dc_crc32_mul(0xDEADBEEFu, DC_CRC_X0) == 0xDEADBEEFu);
    CHECK(dc_crc32_mul(0x12345678u, 0x9ABCDEF0u) == dc_crc32_mul(0x9ABCDEF0u, 0x12345678u));
    CHECK(dc_crc32_xpow8(0) == DC_CRC_X0 && dc_crc32_xpow8(1) == DC_CRC_X8);
    {
        uint32_t p = DC_CRC_X0;
        for (uint64_t n = 0; n <= 70; ++n, p = dc_crc32_mul(p, DC_CRC_X8)) CHECK(dc_crc32_xpow8(n) == p);
    }
    const uint64_t big[2] = {(1ull << 32) + 5, 1ull << 40};
    for (int i = 0; i < 2; ++i) {
        const uint64_t n = big[i];
        const uint64_t cut[5] = {1, 5, 1ull << 31, n / 3, n - 1};
        for (int k = 0; k < 5; ++k)
            CHECK(dc_crc32_xpow8(n) == dc_crc32_mul(dc_crc32_xpow8(cut[k]), dc_crc32_xpow8(n - cut[k])));
        uint32_t sq = DC_CRC_X8;   /* n = 2^e: e squarings of x^8, then the low part */
        for (int e = 0; e < (i ? 40 : 32); ++e) sq = dc_crc32_mul(sq, sq);
        CHECK(dc_crc32_xpow8(n) == dc_crc32_mul(sq, dc_crc32_xpow8(i ? 0 : 5)));
    }
    CHECK(dc_crc32_xpow8(~0ull) == dc_crc32_mul(dc_crc32_xpow8(1ull << 63), dc_crc32_xpow8((1ull << 63) - 1)));

    /* the tables of a constant product */
    const uint32_t w = dc_crc32_xpow8(1024);
    dc_crc32_mul_tables(MK, w);
    for (int i = 0; i < 1000; ++i) {
        const uint32_t s = ((uint32_t)rnd() << 24) | ((uint32_t)rnd() << 16) | ((uint32_t)rnd() << 8) | rnd();
        CHECK(mulk(s) == dc_crc32_mul(s, w));
    }

    /* the kernels' folding scheme */
    for (uint32_t sh = 0; sh < 16; ++sh)
        for (uint32_t n = 0; n <= 2100; n += (sh == 0 || n < 40 || (n > 1000 && n < 1100) || n > 2030) ? 1 : 7) {
            const uint32_t bytes = 16u * ((sh + n + 15) / 16);
            uint8_t *region = (uint8_t *)malloc(bytes ? bytes : 1);
            for (uint32_t i = 0; i < bytes; ++i) region[i] = rnd();   /* the neighbours are not zeros */
            CHECK(fold_model(region, sh, n) == dc_crc32_update_bitwise(0, region + sh, n));
            free(region);
        }

    printf(fails ? "crc32_check: %d failures\n" : "crc32_check: ok\n", fails);
    return fails != 0;
}
