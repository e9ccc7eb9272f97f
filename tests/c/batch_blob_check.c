/* Stand-alone check of the "DCHB" container rule (csrc/dc_batch_blob.h), meant to be built with
 * the host sanitizers; it needs no device and no library:
 *
 *   cc -std=c11 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
 *      -Idata_compression_amd/csrc tests/c/batch_blob_check.c -o batch_blob_check && ./batch_blob_check
 *
 * The section arithmetic against 128-bit sums for counts whose section sizes straddle a multiple
 * of 16 and at the largest count; every header field at its edges; totals of 2^64 - 1, where a
 * sum written plainly would wrap; and the whole rule on containers allocated to their exact size
 * (a read past blob_bytes is a caught read), whole and with each directory field damaged. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "dc_batch_blob.h"

static int fails;
#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

typedef unsigned __int128 u128;
#define TABLE_BYTES 123457u   /* any size: the workspace takes it as it is */

static u128 up(u128 v, u128 a) { return (v + a - 1) / a * a; }

static void layout_case(uint64_t n, uint32_t kind, uint32_t flags, uint32_t K)
{
    dc_bb_info I;
    memset(&I, 0, sizeof(I));
    CHECK(dc_bb_layout(n, kind, flags, K, &I) == 0);
    u128 at = 64;
    CHECK(I.len_off == at); at += up(4 * (u128)n, 16);
    CHECK(I.bits_off == at); at += up(4 * (u128)n, 16);
    CHECK(I.mode_off == at); at += up(n, 16);
    if (kind == DC_BB_KIND_SET) { CHECK(I.tid_off == at); at += up(n, 16); } else CHECK(I.tid_off == 0);
    if (flags & 1) { CHECK(I.crc_off == at); at += up(4 * (u128)n, 16); } else CHECK(I.crc_off == 0);
    CHECK(I.rec_off == at);
    const u128 rec = kind == 0 ? 256 * (u128)n : kind == 1 ? 128 * (u128)n : 256 * (u128)K;
    CHECK(I.rec_bytes == rec);
    CHECK(I.payload_off == at + rec && I.payload_off % 16 == 0);
    /* the workspace: every array at a multiple of the alignment, none overlapping the next */
    dc_bb_work(&I, TABLE_BYTES);
    const uint64_t w[10] = {I.w_items, I.w_pay_off, I.w_sync_off, I.w_seg_off, I.w_status, I.w_cstatus, I.w_lens,
                            I.w_lengths, I.w_table, I.work_bytes};
    const u128 need[9] = {24 * (u128)n, 8 * ((u128)n + 1), 8 * ((u128)n + 1), 8 * ((u128)n + 1), 4 * (u128)n, 4,
                          kind == 1 ? 256 * (u128)n : 0, kind == 2 ? 4 * 259 : 0, kind == 2 ? TABLE_BYTES : 0};
    for (int k = 0; k < 9; ++k) CHECK(w[k] % DC_BB_WORK_ALIGN == 0 && (u128)w[k] + need[k] <= w[k + 1]);
}

/* a container of n stored segments of lengths len0, len0 + 1, ... (mod 40) at S = 16, kind 3 with
 * K = 2 and CRCs so that every section exists; allocated to its exact size */
static uint8_t *make(uint64_t n, uint32_t len0, uint64_t *m, dc_bb_info *I)
{
    memset(I, 0, sizeof(*I));
    CHECK(dc_bb_layout(n, DC_BB_KIND_SET, DC_BB_FLAG_CRC, 2, I) == 0);
    uint64_t total = 0, pay = 0, sync = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const uint32_t len = (len0 + (uint32_t)i) % 40;
        total += len;
        pay += dc_bb_pay_item(8 * len);
        sync += dc_bb_sync_item(len, 16);
    }
    uint64_t so, bb;
    CHECK(dc_bb_tail(I->payload_off, pay, sync, &so, &bb) == 0);
    uint8_t *b = (uint8_t *)calloc(bb, 1);
    for (uint64_t i = 0; i < n; ++i) {
        const uint32_t len = (len0 + (uint32_t)i) % 40;
        dc_bb_put32(b + I->len_off + 4 * i, len);
        dc_bb_put32(b + I->bits_off + 4 * i, 8 * len);
        b[I->tid_off + i] = 255;   /* a stored segment's tid is not read */
    }
    dc_bb_header_write(b, DC_BB_KIND_SET, DC_BB_FLAG_CRC, 2, 2, 16, n, total, sync, pay, bb);
    *m = bb;
    return b;
}

static int whole(const uint8_t *b, uint64_t m)
{
    dc_bb_info J;
    memset(&J, 0, sizeof(J));
    return dc_bb_check(b, m, TABLE_BYTES, &J);
}

static void reseal(uint8_t *b) { dc_bb_put32(b + 60, dc_bb_crc(b, 60)); }

/* the header with the bytes [at, at + size) set to v, its CRC made right: the rule's answer */
static int header_with(const uint8_t *b, uint64_t m, int at, int size, uint64_t v)
{
    uint8_t h[64];
    dc_bb_info J;
    memcpy(h, b, 64);
    for (int k = 0; k < size; ++k) h[at + k] = (uint8_t)(v >> (8 * k));
    reseal(h);
    memset(&J, 0, sizeof(J));
    return dc_bb_header(h, m, TABLE_BYTES, &J);
}

int main(void)
{
    /* section sizes either side of a multiple of 16: 4 n at n = 3, 4, 5; n at 15, 16, 17 */
    for (uint32_t kind = 0; kind < 4; ++kind)
        for (uint32_t flags = 0; flags < 2; ++flags) {
            const uint32_t K = kind < 2 ? 0 : kind == 2 ? 1 : 64;
            for (uint64_t n = 0; n <= 70; ++n) layout_case(n, kind, flags, K);
            layout_case(DC_BB_COUNT_MAX - 1, kind, flags, K);
            layout_case(DC_BB_COUNT_MAX, kind, flags, K);
            dc_bb_info I;
            CHECK(dc_bb_layout(DC_BB_COUNT_MAX + 1, kind, flags, K, &I) == -1);
            CHECK(dc_bb_layout(~0ull, kind, flags, K, &I) == -1);
            CHECK(dc_bb_layout(1, kind, flags | 2, K, &I) == -1);
            CHECK(dc_bb_layout(1, kind, flags | 128, K, &I) == -1);
        }
    {   /* kind and K */
        dc_bb_info I;
        CHECK(dc_bb_layout(1, 4, 0, 0, &I) == -1 && dc_bb_layout(1, 255, 0, 0, &I) == -1);
        CHECK(dc_bb_layout(1, 0, 0, 1, &I) == -1 && dc_bb_layout(1, 1, 0, 1, &I) == -1);
        CHECK(dc_bb_layout(1, 2, 0, 0, &I) == -1 && dc_bb_layout(1, 2, 0, 2, &I) == -1 && dc_bb_layout(1, 2, 0, 1, &I) == 0);
        CHECK(dc_bb_layout(1, 3, 0, 0, &I) == -1 && dc_bb_layout(1, 3, 0, 65, &I) == -1);
        CHECK(dc_bb_layout(1, 3, 0, 1, &I) == 0 && dc_bb_layout(1, 3, 0, 64, &I) == 0);
    }

    /* the tail and the bound at the u64 edges */
    {
        uint64_t so, bb;
        CHECK(dc_bb_tail(64, 0, 0, &so, &bb) == 0 && so == 64 && bb == 64);
        CHECK(dc_bb_tail(64, 16, 1, &so, &bb) == 0 && so == 80 && bb == 96);
        CHECK(dc_bb_tail(64, 8, 0, &so, &bb) == -1);                 /* pay_total is no multiple of 16 */
        CHECK(dc_bb_tail(64, ~0ull, 0, &so, &bb) == -1);
        CHECK(dc_bb_tail(64, ~0ull - 15, 0, &so, &bb) == -1);        /* 64 + (2^64 - 16) wraps */
        CHECK(dc_bb_tail(64, ~0ull - 15 - 64, 0, &so, &bb) == 0 && bb == ~0ull - 15);
        CHECK(dc_bb_tail(64, ~0ull - 15 - 64, 1, &so, &bb) == -1);   /* the sync section then wraps */
        CHECK(dc_bb_tail(64, 0, ~0ull, &so, &bb) == -1);             /* 2 sync_total wraps */
        CHECK(dc_bb_tail(64, 0, 1ull << 63, &so, &bb) == -1);
        CHECK(dc_bb_tail(64, 0, (1ull << 63) - 1, &so, &bb) == -1);  /* 2^64 - 2 pads past 2^64 */
        CHECK(dc_bb_tail(0, 0, (1ull << 63) - 8, &so, &bb) == 0 && bb == ~0ull - 15);
        CHECK(dc_bb_bound(~0ull, 1, 64, 0, 0, 0) == 0 && dc_bb_bound(~0ull - 100, 0, 16, 0, 0, 0) == 0);
        CHECK(dc_bb_bound(0, 0, 64, 0, 0, 0) == 64);
        CHECK(dc_bb_bound(0, 0, 48, 0, 0, 0) == 0 && dc_bb_bound(0, 0, 8, 0, 0, 0) == 0 && dc_bb_bound(0, 0, 2048, 0, 0, 0) == 0);
        CHECK(dc_bb_bound(1ull << 62, DC_BB_COUNT_MAX, 16, 0, 1, 0) ==
              (uint64_t)(64 + 3 * up(4 * (u128)DC_BB_COUNT_MAX, 16) + up(DC_BB_COUNT_MAX, 16) + 256 * (u128)DC_BB_COUNT_MAX +
                         up(((u128)1 << 62) + 16 * (u128)DC_BB_COUNT_MAX, 16) +
                         up(2 * ((((u128)1 << 62) / 16) + DC_BB_COUNT_MAX), 16)));
        CHECK(dc_bb_pay_item(0) == 0 && dc_bb_pay_item(1) == 16 && dc_bb_pay_item(128) == 16 && dc_bb_pay_item(129) == 32);
        CHECK(dc_bb_pay_item(~0u) == 0x20000000ull);                 /* (2^32 + 6) / 8 rounded up to 16: no u32 wrap */
        CHECK(dc_bb_sync_item(0, 16) == 0 && dc_bb_sync_item(16, 16) == 1 && dc_bb_sync_item(17, 16) == 2);
        CHECK(dc_bb_sync_item(~0u, 16) == 0x10000000ull);
    }

    /* whole containers, exact allocations; every header field at its edges */
    for (uint64_t n = 0; n <= 35; ++n) {
        uint64_t m;
        dc_bb_info I;
        uint8_t *b = make(n, 7, &m, &I);
        CHECK(whole(b, m) == 0);
        CHECK(whole(b, m - 1) == -1 && whole(b, 63) == -1 && whole(b, 0) == -1);   /* m one byte short */
        CHECK(whole(b, m + 1) == 0);                                               /* (only m bytes are read) */
        free(b);
    }
    {
        uint64_t m;
        dc_bb_info I;
        uint8_t *b = make(19, 7, &m, &I);
        const uint64_t pay = dc_bb_get64(b + 40), sync = dc_bb_get64(b + 32), total = dc_bb_get64(b + 24);
        CHECK(header_with(b, m, 0, 0, 0) == 0);
        CHECK(header_with(b, m, 0, 1, 'E') == -1 && header_with(b, m, 3, 1, 'b') == -1);          /* magic */
        CHECK(header_with(b, m, 4, 1, 0) == -1 && header_with(b, m, 4, 1, 2) == -1);              /* version */
        CHECK(header_with(b, m, 5, 1, 4) == -1 && header_with(b, m, 5, 1, 255) == -1);            /* kind */
        CHECK(header_with(b, m, 6, 1, 3) == -1 && header_with(b, m, 6, 1, 0x81) == -1);           /* reserved flag bits */
        CHECK(header_with(b, m, 7, 1, 0) == -1 && header_with(b, m, 7, 1, 65) == -1);             /* K of kind 3 */
        CHECK(header_with(b, m, 8, 2, 1) == -1 && header_with(b, m, 8, 2, 257) == -1 && header_with(b, m, 8, 2, 0) == -1);
        CHECK(header_with(b, m, 8, 2, 256) == 0 && header_with(b, m, 8, 2, 3) == 0);
        CHECK(header_with(b, m, 10, 2, 48) == -1 && header_with(b, m, 10, 2, 8) == -1 && header_with(b, m, 10, 2, 2048) == -1);
        CHECK(header_with(b, m, 10, 2, 1024) == 0);   /* (the header rule alone: the totals rule sees the sync count) */
        CHECK(header_with(b, m, 12, 4, 1) == -1 && header_with(b, m, 56, 4, 1u << 31) == -1);     /* reserved words */
        CHECK(header_with(b, m, 16, 8, DC_BB_COUNT_MAX + 1) == -1 && header_with(b, m, 16, 8, ~0ull) == -1);
        CHECK(header_with(b, m, 16, 8, 33) == -1);                                                /* the sections move */
        CHECK(header_with(b, m, 16, 8, 20) == 0);   /* (4 x 20 and 20 pad as 4 x 19 and 19 do: segment 19 is then the zero gap, empty and stored) */
        CHECK(header_with(b, m, 40, 8, pay + 8) == -1 && header_with(b, m, 40, 8, pay + 16) == -1);
        CHECK(header_with(b, m, 40, 8, ~0ull) == -1 && header_with(b, m, 40, 8, ~0ull - 15) == -1);
        CHECK(header_with(b, m, 32, 8, sync + 8) == -1 && header_with(b, m, 32, 8, ~0ull) == -1);
        CHECK(header_with(b, m, 48, 8, m + 1) == -1 && header_with(b, m, 48, 8, m - 1) == -1 && header_with(b, m, 48, 8, ~0ull) == -1);
        CHECK(header_with(b, m, 24, 8, total + 1) == 0 && header_with(b, m, 24, 8, ~0ull) == 0);  /* (the totals rule's) */
        for (int bit = 0; bit < 32; ++bit) {   /* a header CRC bit */
            uint8_t h[64];
            dc_bb_info J;
            memcpy(h, b, 64);
            h[60 + bit / 8] ^= (uint8_t)(1u << (bit % 8));
            CHECK(dc_bb_header(h, m, TABLE_BYTES, &J) == -1);
        }
        /* totals of 2^64 - 1 under a right CRC: the whole rule refuses, and reads nothing past m */
        const int at[4] = {24, 32, 40, 48};
        for (int k = 0; k < 4; ++k) {
            uint8_t *d = (uint8_t *)malloc(m);
            memcpy(d, b, m);
            dc_bb_put64(d + at[k], ~0ull);
            reseal(d);
            CHECK(whole(d, m) == -1);
            dc_bb_put64(d + at[k], dc_bb_get64(b + at[k]) + 1);
            reseal(d);
            CHECK(whole(d, m) == -1);
            free(d);
        }
        /* the directory */
        const uint64_t i = 9;   /* len 16, bits 128 */
        CHECK(dc_bb_get32(b + I.len_off + 4 * i) == 16);
#define DAMAGED(stmt, want) do { uint8_t *d = (uint8_t *)malloc(m); memcpy(d, b, m); stmt; CHECK(whole(d, m) == (want)); free(d); } while (0)
        DAMAGED(dc_bb_put32(d + I.len_off + 4 * i, 17), -1);
        DAMAGED(dc_bb_put32(d + I.len_off + 4 * i, 65537), -1);
        DAMAGED(dc_bb_put32(d + I.len_off + 4 * i, ~0u), -1);
        DAMAGED(dc_bb_put32(d + I.bits_off + 4 * i, 127), -1);
        DAMAGED(dc_bb_put32(d + I.bits_off + 4 * i, 129), -1);
        DAMAGED(dc_bb_put32(d + I.bits_off + 4 * i, ~0u), -1);
        DAMAGED(d[I.mode_off + i] = 2, -1);
        DAMAGED(d[I.mode_off + i] = 255, -1);
        DAMAGED(d[I.mode_off + i] = 1, -1);                                    /* tid 255 >= K */
        DAMAGED((d[I.mode_off + i] = 1, d[I.tid_off + i] = 2), -1);            /* tid = K */
        DAMAGED((d[I.mode_off + i] = 1, d[I.tid_off + i] = 1), 0);             /* mode 1 at bits = 8 len is legal */
        DAMAGED((d[I.mode_off + i] = 1, d[I.tid_off + i] = 1, dc_bb_put32(d + I.bits_off + 4 * i, 127)), 0);   /* the same 16 payload bytes */
        DAMAGED((d[I.mode_off + i] = 1, d[I.tid_off + i] = 1, dc_bb_put32(d + I.bits_off + 4 * i, 0)), -1);    /* the payload scan ends short */
        DAMAGED(d[m - 1] = 9, 0);                                              /* gap bytes are not inspected */
        free(b);
    }
    /* the per-segment rule at its edges */
    CHECK(dc_bb_seg(65536, 8 * 65536, 0, 0, 0, 0) == 0 && dc_bb_seg(65537, 8 * 65537, 0, 0, 0, 0) == -1);
    CHECK(dc_bb_seg(0, 0, 0, 0, 0, 0) == 0 && dc_bb_seg(0, 0, 1, 0, 0, 0) == 0 && dc_bb_seg(0, 1, 1, 0, 0, 0) == -1);
    CHECK(dc_bb_seg(5, 40, 1, 0, 0, 0) == 0 && dc_bb_seg(5, 41, 1, 0, 0, 0) == -1 && dc_bb_seg(5, 39, 0, 0, 0, 0) == -1);
    CHECK(dc_bb_seg(5, 39, 1, 63, 3, 64) == 0 && dc_bb_seg(5, 39, 1, 64, 3, 64) == -1 && dc_bb_seg(5, 40, 0, 64, 3, 64) == 0);
    CHECK(dc_bb_seg(5, 39, 1, 200, 2, 1) == 0);   /* tid belongs to kind 3 alone */
    printf(fails ? "batch_blob_check: %d failures\n" : "batch_blob_check: ok\n", fails);
    return fails != 0;
}
