/* Stand-alone check of the rules a Huffman container read from a file is held to
 * (csrc/dc_container_check.h), meant to be built with the host sanitizers; it needs no device and
 * no library:
 *
 *   cc -std=c11 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
 *      -Idata_compression_amd/csrc tests/c/container_check.c -o container_check && ./container_check
 *
 * A synthetic DCH1 container (chunk c is 40 + c % 7 bits long) of n = 8192 symbols at S = 16, and
 * the malformed entries of tests/container_model.py built from it, the wild ones included (bits of
 * 2^64 - 1, bases of 2^63, lengths of 0xFFFF). Every container is allocated exactly and once more
 * at an odd address, so a read past it or an aligned load from it is caught. */
#include <stdio.h>
#include <stdlib.h>

#include "dc_container_check.h"

static int fails;
#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

typedef struct {
    uint8_t *p;
    uint64_t m, n, bits, ng, nc;
    uint32_t S;
} cont;

static void put64(uint8_t *p, uint64_t v) { memcpy(p, &v, 8); }
static void put32(uint8_t *p, uint32_t v) { memcpy(p, &v, 4); }
static void put16(uint8_t *p, uint16_t v) { memcpy(p, &v, 2); }
static uint8_t *base_at(const cont *c, uint64_t g) { return c->p + DCC_HEADER + 8 * g; }
static uint8_t *len_at(const cont *c, uint64_t k) { return c->p + DCC_HEADER + 8 * c->ng + 2 * k; }

static cont make(uint64_t n, uint32_t S)
{
    cont c;
    uint64_t bit = 0, k;
    c.n = n;
    c.S = S;
    c.nc = (n + S - 1) / S;
    c.ng = (c.nc + 63) / 64;
    c.bits = 0;
    for (k = 0; k < c.nc; ++k) c.bits += (k + 1 < c.nc ? 40 + k % 7 : 2 * (n - k * S));
    c.m = DCC_HEADER + 8 * c.ng + 2 * c.nc + (c.bits + 7) / 8;
    c.p = (uint8_t *)calloc(c.m ? c.m : 1, 1);
    put32(c.p, DCC_MAGIC);
    c.p[4] = 1; c.p[5] = 2; c.p[6] = 1; c.p[7] = 0;
    put64(c.p + 8, n);
    put64(c.p + 16, c.bits);
    put32(c.p + 24, S);
    for (k = 0; k < 256; ++k) c.p[32 + k] = (uint8_t)(k < 8 ? 3 : 0);
    for (k = 0; k < c.nc; ++k) {
        if (k % 64 == 0) put64(base_at(&c, k / 64), bit);
        put16(len_at(&c, k), (uint16_t)(k + 1 < c.nc ? 40 + k % 7 : 2 * (n - k * S)));
        bit += dcc_get16(len_at(&c, k));
    }
    return c;
}

/* the verdict on the first m bytes, from an exact allocation and from one at an odd address */
static int verdict(const cont *c, uint64_t m)
{
    dcc_dch1 h;
    uint8_t *a = (uint8_t *)malloc(m ? m : 1), *b = (uint8_t *)malloc(m + 1);
    int ra, rb;
    memcpy(a, c->p, m);
    memcpy(b + 1, c->p, m);
    ra = dcc_dch1_check(a, m, &h);
    rb = dcc_dch1_check(b + 1, m, &h);
    CHECK(ra == rb);
    free(a);
    free(b);
    return ra;
}

#define WITH(want, ...) do { cont c = make(8192, 16); __VA_ARGS__; CHECK(verdict(&c, c.m) == (want)); free(c.p); } while (0)

static void arithmetic(void)
{
    uint64_t r = 0;
    CHECK(dcc_add(UINT64_MAX, 1, &r) == -1 && dcc_add(UINT64_MAX - 1, 1, &r) == 0 && r == UINT64_MAX);
    CHECK(dcc_ceil_div(UINT64_MAX, 8) == (1ull << 61) && dcc_ceil_div(UINT64_MAX - 6, 8) == (1ull << 61));
    CHECK(dcc_ceil_div(0, 8) == 0 && dcc_ceil_div(1, 8) == 1 && dcc_ceil_div(8, 8) == 1 && dcc_ceil_div(9, 8) == 2);
    CHECK(dcc_chunks(UINT64_MAX, 16) == (1ull << 60) && dcc_groups(UINT64_MAX, 16) == (1ull << 54));
    CHECK(dcc_index_bytes(UINT64_MAX, 16) == (1ull << 57) + (1ull << 61));
    CHECK(dcc_bits_fit(32, 1) && !dcc_bits_fit(33, 1) && dcc_bits_fit(0, 0) && !dcc_bits_fit(1, 0));
    CHECK(dcc_bits_fit(UINT64_MAX, 1ull << 59) && !dcc_bits_fit(UINT64_MAX, (1ull << 59) - 1));
    CHECK(dcc_sync_ok(16) && dcc_sync_ok(1024) && !dcc_sync_ok(0) && !dcc_sync_ok(8) && !dcc_sync_ok(48) && !dcc_sync_ok(2048));
    CHECK(dcc_digit_bits(2) == 1 && dcc_digit_bits(3) == 2 && dcc_digit_bits(4) == 2 && dcc_digit_bits(5) == 3 &&
          dcc_digit_bits(9) == 4 && dcc_digit_bits(16) == 4);
}

static void sizes(void)
{
    const uint32_t syncs[3] = {16, 64, 1024};
    for (int i = 0; i < 3; ++i) {
        const uint64_t S = syncs[i], ns[] = {0, 1, S - 1, S, S + 1, 64 * S - 1, 64 * S, 64 * S + 1, 3 * 64 * S + 5};
        for (size_t j = 0; j < sizeof(ns) / sizeof(ns[0]); ++j) {
            cont c = make(ns[j], syncs[i]);
            CHECK(verdict(&c, c.m) == 0);
            if (c.m > DCC_HEADER) CHECK(verdict(&c, c.m - 1) == -1);
            CHECK(verdict(&c, DCC_HEADER - 1) == -1);
            /* the groups alone, as a range read checks them */
            for (uint64_t g0 = 0; g0 < c.ng; ++g0)
                for (uint64_t g1 = g0; g1 < c.ng; ++g1)
                    CHECK(dcc_index_groups(c.n, c.S, base_at(&c, 0), len_at(&c, 0), c.bits, 0, g0, g1) == 0);
            if (c.ng) CHECK(dcc_index_groups(c.n, c.S, base_at(&c, 0), len_at(&c, 0), c.bits, 0, 0, c.ng) == -1);
            free(c.p);
        }
    }
}

static void malformed(void)
{
    WITH(0, (void)0);
    WITH(-1, c.p[4] = 2);
    WITH(-1, c.p[5] = 0);
    WITH(-1, c.p[5] = 1);
    WITH(-1, c.p[5] = 17);
    WITH(0, (c.p[5] = 16, c.p[6] = 4));
    WITH(-1, c.p[6] = 2);
    WITH(-1, c.p[7] = 1);
    WITH(-1, put32(c.p + 24, 0));
    WITH(-1, put32(c.p + 24, 8));
    WITH(-1, put32(c.p + 24, 48));
    WITH(-1, put32(c.p + 24, 2048));
    WITH(0, c.p[32 + 255] = DCC_MAX_DIGITS);
    WITH(-1, c.p[32 + 255] = DCC_MAX_DIGITS + 1);
    WITH(-1, put64(c.p + 8, c.n + 1));
    WITH(0, put64(c.p + 8, c.n - 1));                    /* every count and sum as before: safe to decode */
    WITH(-1, put64(c.p + 8, UINT64_MAX));
    WITH(-1, put64(c.p + 8, 0));
    WITH(-1, put64(c.p + 16, UINT64_MAX));
    WITH(-1, put64(c.p + 16, UINT64_MAX - 6));
    WITH(-1, put64(c.p + 16, 1ull << 63));
    WITH(-1, put64(c.p + 16, c.bits + 1));
    WITH(-1, put64(c.p + 16, c.bits - 1));
    WITH(-1, put64(base_at(&c, 0), 1));
    WITH(-1, put64(base_at(&c, 1), dcc_get64(base_at(&c, 1)) + 1));
    WITH(-1, put64(base_at(&c, 1), dcc_get64(base_at(&c, 1)) - 1));
    WITH(-1, put64(base_at(&c, 1), 1ull << 63));
    WITH(-1, put64(base_at(&c, 1), UINT64_MAX));
    WITH(-1, put64(base_at(&c, 1), c.bits + 1));
    WITH(-1, put64(base_at(&c, c.ng - 1), UINT64_MAX - 5));   /* base + lengths wraps */
    WITH(-1, { for (uint64_t g = 0; g < c.ng / 2; ++g) { uint64_t a = dcc_get64(base_at(&c, g)), b = dcc_get64(base_at(&c, c.ng - 1 - g));
               put64(base_at(&c, g), b); put64(base_at(&c, c.ng - 1 - g), a); } });
    WITH(-1, put16(len_at(&c, 70), (uint16_t)(dcc_get16(len_at(&c, 70)) + 1)));
    WITH(-1, put16(len_at(&c, 70), (uint16_t)(dcc_get16(len_at(&c, 70)) - 1)));
    WITH(-1, put16(len_at(&c, 70), 0xFFFF));
    /* a chunk over 32 bits per symbol whose sums hold: 16 symbols, 513 bits */
    WITH(-1, { put16(len_at(&c, 70), 513); put64(c.p + 16, c.bits + 513 - 40); for (uint64_t g = 2; g < c.ng; ++g)
               put64(base_at(&c, g), dcc_get64(base_at(&c, g)) + 513 - 40); c.m += 64; c.p = (uint8_t *)realloc(c.p, c.m);
               memset(c.p + c.m - 64, 0, 64); });
    WITH(0, { const uint16_t a = (uint16_t)dcc_get16(len_at(&c, 70)), b = (uint16_t)dcc_get16(len_at(&c, 71));
           put16(len_at(&c, 70), b); put16(len_at(&c, 71), a); });   /* sums hold: the rule cannot see it */
    {   /* a range read checks the groups it uploads and no others */
        cont c = make(8192, 16);
        put16(len_at(&c, 70), 0xFFFF);   /* group 1 */
        CHECK(dcc_index_groups(c.n, c.S, base_at(&c, 0), len_at(&c, 0), c.bits, 0, 0, 0) == 0);
        CHECK(dcc_index_groups(c.n, c.S, base_at(&c, 0), len_at(&c, 0), c.bits, 0, 1, 1) == -1);
        CHECK(dcc_index_groups(c.n, c.S, base_at(&c, 0), len_at(&c, 0), c.bits, 0, 0, 7) == -1);
        CHECK(dcc_index_groups(c.n, c.S, base_at(&c, 0), len_at(&c, 0), c.bits, 0, 2, 7) == 0);
        free(c.p);
    }
    {   /* bit_base: a stream that starts at bit 77 */
        cont c = make(8192, 16);
        for (uint64_t g = 0; g < c.ng; ++g) put64(base_at(&c, g), dcc_get64(base_at(&c, g)) + 77);
        CHECK(dcc_index(c.n, c.S, base_at(&c, 0), len_at(&c, 0), c.bits, 77) == 0);
        CHECK(dcc_index(c.n, c.S, base_at(&c, 0), len_at(&c, 0), c.bits, 76) == -1);
        CHECK(dcc_index(c.n, c.S, base_at(&c, 0), len_at(&c, 0), c.bits, UINT64_MAX) == -1);
        free(c.p);
    }
}

int main(void)
{
    arithmetic();
    sizes();
    malformed();
    printf(fails ? "container_check: %d failures\n" : "container_check: ok\n", fails);
    return fails != 0;
}
