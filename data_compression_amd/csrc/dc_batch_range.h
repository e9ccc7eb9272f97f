/* dc_batch_range.h -- the arithmetic of a byte range of a batch segment (dc_gpu.h "Huffman batch
 * v1: byte ranges"): which chunks of the segment the bytes [first, first + count) touch, and the
 * argument tests of a range, none of which forms a sum that can wrap. No dependency but
 * <stdint.h>, so the range kernels (dc_batch_range_kernels.inc) and a stand-alone checker
 * (tests/c/batch_range_check.c, built with the sanitizers) compile the same functions. */
#ifndef DC_BATCH_RANGE_H
#define DC_BATCH_RANGE_H
#include <stdint.h>

#ifdef __HIPCC__
#define DC_BR_FN static __host__ __device__ __forceinline__
#else
#define DC_BR_FN static inline
#endif

/* The chunks [*c_lo, *c_hi) of S symbols each (S > 0) that hold a byte of [first, first + count):
 * c_lo = floor(first / S), c_hi = floor((first + count - 1) / S) + 1, written so that no term
 * passes 2^64 for any first and count whose true end is below 2^64 + S. count 0 touches no
 * chunk: c_lo == c_hi == floor(first / S). */
DC_BR_FN void dc_batch_range_chunks(uint64_t first, uint64_t count, uint32_t S, uint64_t *c_lo, uint64_t *c_hi)
{
    const uint64_t lo = first / S;
    *c_lo = lo;
    if (count == 0) {
        *c_hi = lo;
        return;
    }
    /* first + count - 1 = S (lo + q) + (first % S + r), with count - 1 = S q + r */
    *c_hi = lo + (count - 1) / S + (first % S + (count - 1) % S) / S + 1;
}

/* A segment given by its offsets [beg, end): 0 and its length in *len, or -1 (DC_E_ARG) when the
 * offsets decrease or the length passes seg_max (DC_BATCH_SEG_MAX). */
DC_BR_FN int dc_batch_range_seg_len(uint64_t beg, uint64_t end, uint32_t seg_max, uint32_t *len)
{
    if (end < beg || end - beg > seg_max) return -1;
    *len = (uint32_t)(end - beg);
    return 0;
}

/* The range [first, first + count) of a segment of len bytes, to out[out_off .. out_off + count)
 * of out_cap bytes: -1 (DC_E_ARG) when it passes the segment, else -6 (DC_E_CAPACITY) when it
 * passes the output, else 0. Each test compares against a difference, never a sum. */
DC_BR_FN int dc_batch_range_args(uint32_t len, uint64_t first, uint64_t count, uint64_t out_off, uint64_t out_cap)
{
    if (first > len || count > len - first) return -1;
    if (out_off > out_cap || count > out_cap - out_off) return -6;
    return 0;
}
#endif
