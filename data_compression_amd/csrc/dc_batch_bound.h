/* dc_batch_bound.h -- buffer bounds of the batched Huffman codec (dc_gpu.h "Huffman batch").
 * Pure host arithmetic with no dependency but <stdint.h>, so libdc_core.so and a stand-alone
 * checker (tests/c/batch_bound_check.c, built with the sanitizers) compile the same functions. */
#ifndef DC_BATCH_BOUND_H
#define DC_BATCH_BOUND_H
#include <stdint.h>

/* Payload bytes that always hold a batch of `count` segments of `total_bytes` bytes in all: a
 * segment never takes more than its own bytes (the stored fallback) rounded up to 16. */
static inline uint64_t dc_batch_payload_bound_calc(uint64_t total_bytes, uint64_t count)
{
    return total_bytes + 16ull * count;
}

/* u16 sync entries that always hold the batch's index: a segment of len bytes takes
 * ceil(len / S) <= len / S + 1 entries. The kernels store and load every entry as a u16 of its
 * own (no whole-dword access), so the bound carries no slack. 0 for S == 0. */
static inline uint64_t dc_batch_sync_bound_calc(uint64_t total_bytes, uint64_t count, uint32_t sync_syms)
{
    if (!sync_syms) return 0;
    return total_bytes / sync_syms + (total_bytes % sync_syms != 0) + count;
}
#endif
