/* dc_small_batch_bound.h -- output bound of the batched small front-end (dc_gpu.h "small batch v1").
 * Pure host arithmetic with no dependency but <stdint.h>, so libdc_core.so and a stand-alone
 * checker (tests/c/small_batch_bound_check.c, built with the sanitizers) compile the same function. */
#ifndef DC_SMALL_BATCH_BOUND_H
#define DC_SMALL_BATCH_BOUND_H
#include <stdint.h>

/* Bytes that always hold the streams of `count` buffers of `total_bytes` bytes in all, back to
 * back: a buffer of len >= 1 bytes codes to at most len + 1 bytes (the LITERAL form: ' ' and the
 * bytes; the pruned form is kept only when it is shorter than len), an empty one to the single
 * byte ' '. Exact: a batch of buffers with fewer than two pairs each takes all of it. */
static inline uint64_t dc_small_batch_bound_calc(uint64_t total_bytes, uint64_t count)
{
    return total_bytes + count;
}
#endif
