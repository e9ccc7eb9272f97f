/* dc_batch_blob.h -- the rule of the "DCHB" container of a Huffman batch (dc_gpu.h "Huffman batch
 * v1: container DCHB"): the section arithmetic, the header rule, the per-segment rule and the
 * totals rule, none of which forms a sum that can wrap. No dependency but <stdint.h>, <string.h>
 * and dc_crc32.h, and no allocation, so the kernels (dc_batch_blob_kernels.inc), the host entry
 * points (dc_core.hip) and a stand-alone checker (tests/c/batch_blob_check.c, built with the
 * sanitizers) compile the same functions. Every rule returns 0, or -1 for what is not valid (the
 * callers' DC_E_STREAM or DC_E_ARG). Fields are read byte by byte: a container may lie at any
 * address of host memory. */
#ifndef DC_BATCH_BLOB_H
#define DC_BATCH_BLOB_H
#include <stdint.h>
#include <string.h>

#include "dc_crc32.h"

#ifdef __HIPCC__
#define DC_BB_FN static __host__ __device__ __forceinline__
#else
#define DC_BB_FN static inline
#endif

#define DC_BB_MAGIC 0x42484344u       /* "DCHB" little-endian */
#define DC_BB_VERSION 1u
#define DC_BB_HEADER 64u              /* header bytes */
#define DC_BB_KIND_OWN 0u             /* own tables, 256-byte records */
#define DC_BB_KIND_OWN4 1u            /* own tables, 128-byte nybble records */
#define DC_BB_KIND_SHARED 2u          /* one shared table */
#define DC_BB_KIND_SET 3u             /* a table set */
#define DC_BB_FLAG_CRC 1u             /* a CRC-32 per segment is stored */
#define DC_BB_COUNT_MAX (1ull << 28)  /* DC_RANGES_MAX */
#define DC_BB_SEG_MAX 65536u          /* DC_BATCH_SEG_MAX */
#define DC_BB_SET_MAX 64u             /* DC_BATCH_SET_MAX */
#define DC_BB_SYNC_MAX 1024u          /* DC_SYNC_MAX */
#define DC_BB_WORK_ALIGN 256u         /* every array of open's workspace starts at a multiple of this */

/* the header's fields, then where the sections lie (an absent section: offset 0), what open's
 * workspace takes, and the arrays in it */
typedef struct dc_bb_info {
    uint32_t version, kind, flags, K;
    int32_t n_ary;
    uint32_t sync_syms;
    uint64_t count, total_bytes, sync_total, pay_total, blob_bytes;
    uint64_t len_off, bits_off, mode_off, tid_off, crc_off, rec_off, rec_bytes, payload_off, sync_off;
    uint64_t work_bytes;
    uint64_t w_items, w_pay_off, w_sync_off, w_seg_off, w_status, w_cstatus, w_lens, w_lengths, w_table;
} dc_bb_info;

DC_BB_FN int dc_bb_add(uint64_t a, uint64_t b, uint64_t *r)
{
    if (a > UINT64_MAX - b) return -1;
    *r = a + b;
    return 0;
}
DC_BB_FN int dc_bb_pad16(uint64_t a, uint64_t *r)
{
    if (a > UINT64_MAX - 15u) return -1;
    *r = (a + 15u) & ~(uint64_t)15u;
    return 0;
}
DC_BB_FN int dc_bb_sync_ok(uint32_t S) { return S >= 16 && S <= DC_BB_SYNC_MAX && (S & (S - 1)) == 0; }
DC_BB_FN uint32_t dc_bb_get32(const uint8_t *p)
{
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
DC_BB_FN uint64_t dc_bb_get64(const uint8_t *p) { return (uint64_t)dc_bb_get32(p) | ((uint64_t)dc_bb_get32(p + 4) << 32); }
DC_BB_FN void dc_bb_put32(uint8_t *p, uint32_t v)
{
    for (int k = 0; k < 4; ++k) p[k] = (uint8_t)(v >> (8 * k));
}
DC_BB_FN void dc_bb_put64(uint8_t *p, uint64_t v)
{
    dc_bb_put32(p, (uint32_t)v);
    dc_bb_put32(p + 4, (uint32_t)(v >> 32));
}

/* CRC-32 (zlib's) of n bytes without a table: the header's 60 bytes, on either side */
DC_BB_FN uint32_t dc_bb_crc(const uint8_t *p, uint32_t n)
{
    uint32_t crc = 0xFFFFFFFFu;
    for (uint32_t i = 0; i < n; ++i) crc = dc_crc32_byte_entry((crc ^ p[i]) & 255u) ^ (crc >> 8);
    return ~crc;
}

/* what the host knows before anything has run: kind, flags and K are a legal triple */
DC_BB_FN int dc_bb_kind_ok(uint32_t kind, uint32_t flags, uint32_t K)
{
    if (kind > DC_BB_KIND_SET || (flags & ~DC_BB_FLAG_CRC)) return -1;
    if (kind <= DC_BB_KIND_OWN4) return K == 0 ? 0 : -1;
    if (kind == DC_BB_KIND_SHARED) return K == 1 ? 0 : -1;
    return K >= 1 && K <= DC_BB_SET_MAX ? 0 : -1;
}

/* The offsets of sections 1 to 7 (len, bits, mode, tid, crc, records, payload) into I, from
 * count, kind, flags and K alone. count <= 2^28, so the largest section (256 count) is 2^36 bytes
 * and no sum here comes near 2^64. -1: count, kind, flags or K is not legal. */
DC_BB_FN int dc_bb_layout(uint64_t count, uint32_t kind, uint32_t flags, uint32_t K, dc_bb_info *I)
{
    if (count > DC_BB_COUNT_MAX || dc_bb_kind_ok(kind, flags, K)) return -1;
    uint64_t at = DC_BB_HEADER;
    const uint64_t p4 = (4 * count + 15u) & ~(uint64_t)15u, p1 = (count + 15u) & ~(uint64_t)15u;
    I->count = count; I->kind = kind; I->flags = flags; I->K = K;
    I->len_off = at; at += p4;
    I->bits_off = at; at += p4;
    I->mode_off = at; at += p1;
    I->tid_off = 0;
    if (kind == DC_BB_KIND_SET) { I->tid_off = at; at += p1; }
    I->crc_off = 0;
    if (flags & DC_BB_FLAG_CRC) { I->crc_off = at; at += p4; }
    I->rec_off = at;
    I->rec_bytes = kind == DC_BB_KIND_OWN ? 256 * count : kind == DC_BB_KIND_OWN4 ? 128 * count : 256ull * K;
    at += I->rec_bytes;   /* (a multiple of 16) */
    I->payload_off = at;
    return 0;
}

/* sync_off and blob_bytes from the two device-known totals: -1 when pay_total is no multiple of
 * 16 or a sum would pass 2^64 */
DC_BB_FN int dc_bb_tail(uint64_t payload_off, uint64_t pay_total, uint64_t sync_total, uint64_t *sync_off,
                        uint64_t *blob_bytes)
{
    uint64_t sb;
    if ((pay_total & 15u) || sync_total > (UINT64_MAX - 15u) / 2) return -1;
    if (dc_bb_add(payload_off, pay_total, sync_off) || dc_bb_pad16(2 * sync_total, &sb)) return -1;
    return dc_bb_add(*sync_off, sb, blob_bytes);
}

/* Bytes that always hold a sealed batch of `count` segments of total_bytes bytes in all: the host
 * sections, the payload bound total_bytes + 16 count and the sync bound ceil(total_bytes / S) +
 * count entries. 0: an argument is not legal, or the bound does not fit 64 bits. */
DC_BB_FN uint64_t dc_bb_bound(uint64_t total_bytes, uint64_t count, uint32_t S, uint32_t kind, uint32_t flags, uint32_t K)
{
    dc_bb_info I;
    uint64_t pay, so, bb;
    if (!dc_bb_sync_ok(S) || dc_bb_layout(count, kind, flags, K, &I)) return 0;
    if (dc_bb_add(total_bytes, 16 * count, &pay) || dc_bb_pad16(pay, &pay)) return 0;
    const uint64_t sync = total_bytes / S + (total_bytes % S != 0) + count;   /* <= 2^60 + 2^28 */
    if (dc_bb_tail(I.payload_off, pay, sync, &so, &bb)) return 0;
    return bb;
}

/* where open's arrays lie in its workspace: three item arrays (count u64 each, scanned into the
 * three offset arrays of count + 1), the statuses, the container status word, kind 1's unpacked
 * records, kind 2's widened lengths (i32[259]) and its table of table_bytes bytes */
DC_BB_FN void dc_bb_work(dc_bb_info *I, uint64_t table_bytes)
{
    const uint64_t A = DC_BB_WORK_ALIGN, n = I->count;
    uint64_t at = 0;
#define DC_BB_TAKE(field, bytes) do { I->field = at; at += ((uint64_t)(bytes) + A - 1) / A * A; } while (0)
    DC_BB_TAKE(w_items, 24 * n);
    DC_BB_TAKE(w_pay_off, 8 * (n + 1));
    DC_BB_TAKE(w_sync_off, 8 * (n + 1));
    DC_BB_TAKE(w_seg_off, 8 * (n + 1));
    DC_BB_TAKE(w_status, 4 * n);
    DC_BB_TAKE(w_cstatus, 4);
    DC_BB_TAKE(w_lens, I->kind == DC_BB_KIND_OWN4 ? 256 * n : 0);
    DC_BB_TAKE(w_lengths, I->kind == DC_BB_KIND_SHARED ? 4 * 259 : 0);
    DC_BB_TAKE(w_table, I->kind == DC_BB_KIND_SHARED ? table_bytes : 0);
#undef DC_BB_TAKE
    I->work_bytes = at;
}

/* The header rule on the 64 header bytes of a container of which m bytes are at hand; fills I
 * (the workspace fields with dc_bb_work(I, table_bytes)). */
DC_BB_FN int dc_bb_header(const uint8_t *h, uint64_t m, uint64_t table_bytes, dc_bb_info *I)
{
    if (m < DC_BB_HEADER || dc_bb_get32(h) != DC_BB_MAGIC) return -1;
    if (dc_bb_get32(h + 60) != dc_bb_crc(h, 60)) return -1;
    if (h[4] != DC_BB_VERSION) return -1;
    const uint32_t n_ary = (uint32_t)h[8] | ((uint32_t)h[9] << 8), S = (uint32_t)h[10] | ((uint32_t)h[11] << 8);
    if (n_ary < 2 || n_ary > 256 || !dc_bb_sync_ok(S) || dc_bb_get32(h + 12) != 0 || dc_bb_get32(h + 56) != 0) return -1;
    if (dc_bb_layout(dc_bb_get64(h + 16), h[5], h[6], h[7], I)) return -1;
    I->version = h[4];
    I->n_ary = (int32_t)n_ary;
    I->sync_syms = S;
    I->total_bytes = dc_bb_get64(h + 24);
    I->sync_total = dc_bb_get64(h + 32);
    I->pay_total = dc_bb_get64(h + 40);
    I->blob_bytes = dc_bb_get64(h + 48);
    uint64_t bb;
    if (dc_bb_tail(I->payload_off, I->pay_total, I->sync_total, &I->sync_off, &bb)) return -1;
    if (bb != I->blob_bytes || bb > m) return -1;
    dc_bb_work(I, table_bytes);
    return 0;
}

/* the 64 header bytes of a container */
DC_BB_FN void dc_bb_header_write(uint8_t *h, uint32_t kind, uint32_t flags, uint32_t K, uint32_t n_ary, uint32_t S,
                                 uint64_t count, uint64_t total_bytes, uint64_t sync_total, uint64_t pay_total,
                                 uint64_t blob_bytes)
{
    dc_bb_put32(h, DC_BB_MAGIC);
    h[4] = (uint8_t)DC_BB_VERSION; h[5] = (uint8_t)kind; h[6] = (uint8_t)flags; h[7] = (uint8_t)K;
    h[8] = (uint8_t)n_ary; h[9] = (uint8_t)(n_ary >> 8); h[10] = (uint8_t)S; h[11] = (uint8_t)(S >> 8);
    dc_bb_put32(h + 12, 0);
    dc_bb_put64(h + 16, count);
    dc_bb_put64(h + 24, total_bytes);
    dc_bb_put64(h + 32, sync_total);
    dc_bb_put64(h + 40, pay_total);
    dc_bb_put64(h + 48, blob_bytes);
    dc_bb_put32(h + 56, 0);
    dc_bb_put32(h + 60, dc_bb_crc(h, 60));
}

/* The per-segment rule: len <= DC_BATCH_SEG_MAX, mode <= 1, bits <= 8 len with equality when mode
 * is 0, tid < K for a mode-1 segment of a table set. */
DC_BB_FN int dc_bb_seg(uint32_t len, uint32_t bits, uint32_t mode, uint32_t tid, uint32_t kind, uint32_t K)
{
    if (len > DC_BB_SEG_MAX || mode > 1u) return -1;
    if (bits > 8u * len || (mode == 0 && bits != 8u * len)) return -1;   /* (8 len <= 2^19) */
    if (kind == DC_BB_KIND_SET && mode == 1u && tid >= K) return -1;
    return 0;
}
/* what a segment adds to the three scans, for any field values (a u32 cannot wrap a u64 here) */
DC_BB_FN uint64_t dc_bb_pay_item(uint32_t bits) { return ((((uint64_t)bits + 7u) >> 3) + 15u) & ~(uint64_t)15u; }
DC_BB_FN uint64_t dc_bb_sync_item(uint32_t len, uint32_t S) { return (uint64_t)len / S + (len % S != 0); }

/* the totals rule: the three scans end at the header's totals */
DC_BB_FN int dc_bb_totals(uint64_t sum_len, uint64_t sum_pay, uint64_t sum_sync, const dc_bb_info *I)
{
    return sum_len == I->total_bytes && sum_pay == I->pay_total && sum_sync == I->sync_total ? 0 : -1;
}

/* The whole container rule on a blob of m bytes in host memory (gap bytes, payload pads, records,
 * payload, sync entries and CRCs are not inspected: the decoders hold those to their own rules). */
DC_BB_FN int dc_bb_check(const uint8_t *blob, uint64_t m, uint64_t table_bytes, dc_bb_info *I)
{
    if (!blob || dc_bb_header(blob, m, table_bytes, I)) return -1;
    uint64_t sl = 0, sp = 0, ss = 0;   /* <= 2^28 items of < 2^33 each */
    for (uint64_t i = 0; i < I->count; ++i) {
        const uint32_t len = dc_bb_get32(blob + I->len_off + 4 * i), bits = dc_bb_get32(blob + I->bits_off + 4 * i);
        const uint32_t tid = I->tid_off ? blob[I->tid_off + i] : 0u;
        if (dc_bb_seg(len, bits, blob[I->mode_off + i], tid, I->kind, I->K)) return -1;
        sl += len;
        sp += dc_bb_pay_item(bits);
        ss += dc_bb_sync_item(len, I->sync_syms);
    }
    return dc_bb_totals(sl, sp, ss, I);
}
#endif
