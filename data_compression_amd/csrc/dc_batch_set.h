/* dc_batch_set.h -- when a lens record of a table set may code a segment (dc_gpu.h "Huffman batch
 * v1, table set"): every length fits the packed code, and the lengths satisfy Kraft, so that the
 * canonical code of the record is prefix-free. No dependency but <stdint.h>, so the select kernel
 * (dc_batch_set_kernels.inc) and libdc_core's host export dc_huff_batch_set_table_ok compile the
 * same function. */
#ifndef DC_BATCH_SET_H
#define DC_BATCH_SET_H
#include <stdint.h>

#ifdef __HIPCC__
#define DC_BS_FN static __host__ __device__ __forceinline__
#else
#define DC_BS_FN static inline
#endif

/* w = ceil(log2 n), the bits of a digit (2 <= n <= 256) */
DC_BS_FN int dc_batch_set_w(int n)
{
    int w = 0;
    while ((1 << w) < n) ++w;
    return w;
}

/* n^d by d products (d <= 32 and n^d <= 2^32 where it is called: no table of powers, which on the
 * device would live in scratch memory) */
DC_BS_FN uint64_t dc_batch_set_pow(int n, uint32_t d)
{
    uint64_t p = 1;
    for (uint32_t i = 0; i < d; ++i) p *= (uint64_t)n;
    return p;
}

/* lens: 256 code lengths in digits. 1 when the record is valid at arity n (2..256), else 0:
 *   every length L has L * w <= 32;
 *   with Lmax the longest, the sum over L_s > 0 of n^(Lmax - L_s) is at most n^Lmax.
 * n^Lmax <= 2^(w Lmax) <= 2^32 and there are 256 terms, so u64 sums hold everything. A record of
 * zeros is valid. Entry s is read at index (s + rot) & 255: the sum does not depend on the order,
 * and callers that run side by side on neighbouring records (one lane a record) give each a
 * rotation of its own to keep their reads on different LDS banks. */
DC_BS_FN int dc_batch_set_table_ok(const uint8_t *lens, int n, uint32_t rot)
{
    if (n < 2 || n > 256) return 0;
    const uint32_t w = (uint32_t)dc_batch_set_w(n);
    uint32_t lmax = 0;
    for (uint32_t s = 0; s < 256; ++s) {
        const uint32_t L = lens[(s + rot) & 255u];
        if (L * w > 32u) return 0;
        lmax = L > lmax ? L : lmax;
    }
    uint64_t sum = 0;
    for (uint32_t s = 0; s < 256; ++s) {
        const uint32_t L = lens[(s + rot) & 255u];
        if (L) sum += dc_batch_set_pow(n, lmax - L);
    }
    return sum <= dc_batch_set_pow(n, lmax);
}
#endif
