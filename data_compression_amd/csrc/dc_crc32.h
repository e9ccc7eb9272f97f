/* dc_crc32.h -- the arithmetic of CRC-32 as zlib, PNG and gzip compute it (dc_gpu.h "Checksums"):
 * the reflected polynomial 0xEDB88320, the register started at all ones and inverted at the end.
 * No dependency but <stdint.h> and <stddef.h> and no allocation, so the kernels
 * (dc_crc_kernels.inc), the host calls (dc_core.hip) and a stand-alone checker
 * (tests/c/crc32_check.c, built with the sanitizers) compile the same functions.
 *
 * A register value is a residue mod P in reflected form: bit 31 is x^0, bit 30 is x^1, ...,
 * bit 0 is x^31. The raw register after a message M from a zero start is M(x) x^32 mod P, which
 * leading zero bytes do not change; a start value I adds I x^(8 |M|), so
 *   crc(M)     = raw(M) ^ 0xFFFFFFFF x^(8 |M|) ^ 0xFFFFFFFF
 *   crc(A || B) = crc(A) x^(8 |B|) ^ crc(B)            (the start and end terms cancel)
 * and for |M| >= 4 the start value is nothing but 0xFF xored into M's first four bytes. */
#ifndef DC_CRC32_H
#define DC_CRC32_H
#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define DC_CRC_FN static __host__ __device__ __forceinline__
#else
#define DC_CRC_FN static inline
#endif

#define DC_CRC_POLY 0xEDB88320u
#define DC_CRC_X0 0x80000000u   /* x^0 */
#define DC_CRC_X8 0x00800000u   /* x^8: one byte */

/* a b mod P: 32 shift-and-xor steps at most */
DC_CRC_FN uint32_t dc_crc32_mul(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (uint32_t m = DC_CRC_X0; m; m >>= 1) {
        if (a & m) p ^= b;
        b = (b >> 1) ^ ((b & 1u) ? DC_CRC_POLY : 0u);   /* b x */
    }
    return p;
}

/* x^(8 n) mod P, the weight of n bytes, for any n: square and multiply over the bits of n (the
 * exponent 8 n itself is never formed, so n >= 2^61 does not wrap) */
DC_CRC_FN uint32_t dc_crc32_xpow8(uint64_t n)
{
    uint32_t p = DC_CRC_X0, sq = DC_CRC_X8;
    for (; n; n >>= 1) {
        if (n & 1u) p = dc_crc32_mul(p, sq);
        if (n > 1) sq = dc_crc32_mul(sq, sq);
    }
    return p;
}

/* crc(A || B) from crc(A), crc(B) and |B| */
DC_CRC_FN uint32_t dc_crc32_combine_calc(uint32_t crc_a, uint32_t crc_b, uint64_t len_b)
{
    return dc_crc32_mul(crc_a, dc_crc32_xpow8(len_b)) ^ crc_b;
}

/* ---- the slicing tables: T[0] is the byte table, T[k][i] = T[0][i] advanced by k zero bytes, so
 * one dword c (the register xor four message bytes) advances as
 * T[3][c & 255] ^ T[2][c >> 8 & 255] ^ T[1][c >> 16 & 255] ^ T[0][c >> 24]. */
DC_CRC_FN uint32_t dc_crc32_byte_entry(uint32_t i)
{
    for (int k = 0; k < 8; ++k) i = (i >> 1) ^ ((i & 1u) ? DC_CRC_POLY : 0u);
    return i;
}
DC_CRC_FN void dc_crc32_slice_tables(uint32_t (*T)[256], int nslices)
{
    for (uint32_t i = 0; i < 256; ++i) T[0][i] = dc_crc32_byte_entry(i);
    for (int k = 1; k < nslices; ++k)
        for (uint32_t i = 0; i < 256; ++i) T[k][i] = (T[k - 1][i] >> 8) ^ T[0][T[k - 1][i] & 255u];
}
/* the tables of the product by a constant w: s w = M[0][s & 255] ^ M[1][s >> 8 & 255] ^
 * M[2][s >> 16 & 255] ^ M[3][s >> 24] */
DC_CRC_FN void dc_crc32_mul_tables(uint32_t (*M)[256], uint32_t w)
{
    for (int j = 0; j < 4; ++j)
        for (uint32_t i = 0; i < 256; ++i) M[j][i] = dc_crc32_mul(i << (8 * j), w);
}

DC_CRC_FN uint32_t dc_crc32_slice4(const uint32_t (*T)[256], uint32_t c)
{
    return T[3][c & 255u] ^ T[2][(c >> 8) & 255u] ^ T[1][(c >> 16) & 255u] ^ T[0][c >> 24];
}

/* ---- the running form (zlib's: start from crc = 0, hand each result to the next piece), with
 * T = dc_crc32_slice_tables(T, 4): four bytes a step, the bytes read one by one (any alignment,
 * either byte order of the host) */
DC_CRC_FN uint32_t dc_crc32_update_tables(const uint32_t (*T)[256], uint32_t crc, const uint8_t *p, size_t n)
{
    size_t i = 0;
    crc = ~crc;
    for (; i + 4 <= n; i += 4) {
        const uint32_t d = (uint32_t)p[i] | ((uint32_t)p[i + 1] << 8) | ((uint32_t)p[i + 2] << 16) |
                           ((uint32_t)p[i + 3] << 24);
        crc = dc_crc32_slice4(T, crc ^ d);
    }
    for (; i < n; ++i) crc = T[0][(crc ^ p[i]) & 255u] ^ (crc >> 8);
    return ~crc;
}
#endif
