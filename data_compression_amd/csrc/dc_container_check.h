/* dc_container_check.h -- what a Huffman container read from a file must satisfy before any of
 * it reaches the device: overflow-safe size arithmetic, the header rule of the "DCH1" container
 * (include/dc_host.h) and the rule of the sync index (include/dc_gpu.h: u64 group bases, u16 chunk
 * bit lengths). Pure host code with no dependency but <stdint.h> and <string.h>, so libdc_core.so
 * (dc_host.hip) and a stand-alone checker (tests/c/container_check.c, built with the sanitizers)
 * compile the same functions. Every function returns 0, or -1 for a container that is not valid
 * (the callers' DC_E_STREAM). Fields are read with memcpy: a container may lie at any address.
 *
 * The index rule. An index (n, S, bases[ng], lens[nc], bits, bit_base) is valid when S is a power
 * of two in 16..1024, nc = ceil(n / S), ng = ceil(nc / 64), bases[0] == bit_base, bases[g + 1] ==
 * bases[g] + the sum of group g's lengths, the last group's base + its lengths == bit_base + bits,
 * and every chunk of k symbols has len <= 32 k (a code is at most 32 bits). Then every chunk
 * starts inside [bit_base, bit_base + bits], which is what the decoder's loads assume. */
#ifndef DC_CONTAINER_CHECK_H
#define DC_CONTAINER_CHECK_H
#include <stdint.h>
#include <string.h>

#define DCC_HEADER 288u          /* bytes before the index of a DCH1 container */
#define DCC_MAGIC 0x31484344u    /* "DCH1" little-endian */
#define DCC_SYNC_MAX 1024u       /* DC_SYNC_MAX */
#define DCC_MAX_DIGITS 128u      /* DC_MAX_DIGITS */
#define DCC_GROUP 64u            /* chunks per group */

static inline int dcc_add(uint64_t a, uint64_t b, uint64_t *r)
{
    if (a > UINT64_MAX - b) return -1;
    *r = a + b;
    return 0;
}
static inline uint64_t dcc_ceil_div(uint64_t a, uint64_t d) { return a / d + (a % d != 0); }   /* no a + d - 1 to wrap */
static inline int dcc_sync_ok(uint64_t S) { return S >= 16 && S <= DCC_SYNC_MAX && (S & (S - 1)) == 0; }
static inline uint64_t dcc_chunks(uint64_t n, uint32_t S) { return dcc_ceil_div(n, S); }
static inline uint64_t dcc_groups(uint64_t n, uint32_t S) { return dcc_ceil_div(dcc_chunks(n, S), DCC_GROUP); }
/* 8 ng + 2 nc: nc <= 2^60 for S >= 16, so the sum stays below 2^62 */
static inline uint64_t dcc_index_bytes(uint64_t n, uint32_t S) { return dcc_groups(n, S) * 8 + dcc_chunks(n, S) * 2; }
static inline uint64_t dcc_get64(const uint8_t *p) { uint64_t v; memcpy(&v, p, 8); return v; }
static inline uint32_t dcc_get32(const uint8_t *p) { uint32_t v; memcpy(&v, p, 4); return v; }
static inline uint32_t dcc_get16(const uint8_t *p) { uint16_t v; memcpy(&v, p, 2); return v; }
/* bits <= 32 n without forming 32 n */
static inline int dcc_bits_fit(uint64_t bits, uint64_t n) { return dcc_ceil_div(bits, 32) <= n; }

/* The index rule for groups g0..g1 (g1 < ng) of an index given as its little-endian bytes: bases
 * = the ng group bases, lens = the nc chunk lengths. Each group's base lies at or after bit_base,
 * its chunks obey len <= 32 k, base + lengths is the next group's base (the last group: bit_base +
 * bits), and never passes bit_base + bits. Group 0's base is bit_base. */
static inline int dcc_index_groups(uint64_t n, uint32_t S, const uint8_t *bases, const uint8_t *lens, uint64_t bits,
                                   uint64_t bit_base, uint64_t g0, uint64_t g1)
{
    uint64_t end, g;
    if (!dcc_sync_ok(S) || !bases || !lens || dcc_add(bit_base, bits, &end)) return -1;
    const uint64_t nc = dcc_chunks(n, S), ng = dcc_groups(n, S);
    if (g0 > g1 || g1 >= ng) return -1;
    for (g = g0; g <= g1; ++g) {
        const uint64_t base = dcc_get64(bases + 8 * g);
        const uint64_t c1 = (g + 1) * DCC_GROUP < nc ? (g + 1) * DCC_GROUP : nc;
        uint64_t sum = 0, next, c;
        if (base < bit_base || (g == 0 && base != bit_base)) return -1;
        for (c = g * DCC_GROUP; c < c1; ++c) {
            const uint64_t k = c + 1 < nc ? S : n - c * S;   /* symbols of chunk c */
            const uint64_t len = dcc_get16(lens + 2 * c);
            if (len > 32 * k) return -1;
            sum += len;
        }
        if (dcc_add(base, sum, &next) || next > end) return -1;
        if (g + 1 < ng ? dcc_get64(bases + 8 * (g + 1)) != next : next != end) return -1;
    }
    return 0;
}

/* the whole index; n == 0 has no group and no bits */
static inline int dcc_index(uint64_t n, uint32_t S, const uint8_t *bases, const uint8_t *lens, uint64_t bits,
                            uint64_t bit_base)
{
    if (!dcc_sync_ok(S) || !dcc_bits_fit(bits, n)) return -1;
    if (n == 0) return 0;
    return dcc_index_groups(n, S, bases, lens, bits, bit_base, 0, dcc_groups(n, S) - 1);
}

typedef struct dcc_dch1 {
    uint64_t n, bits;        /* symbols, payload bits */
    uint64_t ng, nc;         /* groups and chunks of the index */
    uint64_t ib, nbytes;     /* index bytes, payload bytes: the payload is at DCC_HEADER + ib */
    uint32_t S;
    int n_ary;
} dcc_dch1;

/* digit width of n_ary (2..16): 1, 2, 2, 3, .., 4 */
static inline int dcc_digit_bits(int n_ary)
{
    int w = 0;
    while ((1 << w) < n_ary) ++w;
    return w;
}

/* The header rule: magic, version 1, n_ary 2..16, w its digit width, flags 0, S valid, every length byte <= DCC_MAX_DIGITS, bits <= 32 n, and header + index +
 * payload inside the m bytes given. Fills *h. */
static inline int dcc_dch1_header(const uint8_t *in, uint64_t m, dcc_dch1 *h)
{
    uint64_t need;
    int i;
    if (!in || !h || m < DCC_HEADER || dcc_get32(in) != DCC_MAGIC || in[4] != 1) return -1;
    h->n_ary = in[5];
    if (h->n_ary < 2 || h->n_ary > 16 || in[6] != dcc_digit_bits(h->n_ary) || in[7] != 0) return -1;
    h->n = dcc_get64(in + 8);
    h->bits = dcc_get64(in + 16);
    h->S = dcc_get32(in + 24);
    if (!dcc_sync_ok(h->S) || !dcc_bits_fit(h->bits, h->n)) return -1;
    for (i = 0; i < 256; ++i)
        if (in[32 + i] > DCC_MAX_DIGITS) return -1;
    h->nc = dcc_chunks(h->n, h->S);
    h->ng = dcc_groups(h->n, h->S);
    h->ib = dcc_index_bytes(h->n, h->S);
    h->nbytes = dcc_ceil_div(h->bits, 8);
    if (dcc_add(DCC_HEADER, h->ib, &need) || dcc_add(need, h->nbytes, &need) || need > m) return -1;
    return 0;
}

/* header and whole index of a DCH1 container */
static inline int dcc_dch1_check(const uint8_t *in, uint64_t m, dcc_dch1 *h)
{
    if (dcc_dch1_header(in, m, h)) return -1;
    return dcc_index(h->n, h->S, in + DCC_HEADER, in + DCC_HEADER + 8 * h->ng, h->bits, 0);
}
#endif
