/*
 * dc_gpu.h -- device-resident extended API of libdc_core.so (MI355X / gfx950).
 *
 * This is the API the drop-in shims (dc_huffman.h, dc_nybble.h), bench.py and the
 * multi-GPU driver are built on. All pointers named d_* are device pointers (HBM);
 * every call is asynchronous on the context's HIP stream unless it says otherwise.
 * Every function returns 0 (DC_OK) or a negative DC_E_* status; none of them prints.
 *
 * Reference interfaces these stages replace (file:line in carycode/data_compression):
 *   dc_huff_hist          histogram()                          n_ary_huffman.c:461-493
 *   dc_huff_table*        huffman() + convert_lengths_to_encode_table()
 *                                                              n_ary_huffman.c:1161-1208, :1382-1612
 *   dc_huff_plan/pack     represent_items_with_codes() (stub)  n_ary_huffman.c:1621-1678
 *   dc_huff_decode        decompress() data block (missing)     n_ary_huffman.c:2014-2094
 *   dc_nyb_*              compress_bytestring/decompress_bytestring
 *                                                              nybble_compression.c:734-1038
 * The Huffman bitstream layout is build-defined (DESIGN.md "Huffman bitstream v1").
 */
#ifndef DC_GPU_H
#define DC_GPU_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    DC_OK = 0,
    DC_E_ARG = -1,           /* bad argument */
    DC_E_HIP = -2,           /* a HIP runtime call failed (no device, launch failure, ...) */
    DC_E_CODE_TOO_LONG = -3, /* a byte's packed code exceeds 32 bits */
    DC_E_NOCODE = -4,        /* the input holds a byte that has no code */
    DC_E_STATE = -5,         /* stage called out of order (e.g. pack before hist of that input) */
    DC_E_CAPACITY = -6,      /* output buffer too small */
    DC_E_STREAM = -7,        /* corrupt compressed stream */
    DC_E_FALLBACK = -8,      /* the fused C5 path does not apply to this input: run the two stages */
    DC_E_CHECKSUM = -9       /* a decoded buffer's CRC-32 is not the one stored for it ("checksums") */
};

#define DC_BLOCK_BYTES 32768u   /* encoder block: one histogram + one bit offset each */
#define DC_LUT_BITS 12          /* decoder first-level lookup table: 2^12 entries */
#define DC_MAX_SYMS 1024        /* max_symbol_value + 1 supported by the table kernel */
#define DC_MAX_DIGITS 128       /* longest code length (in base-n digits) handled */
#define DC_LUT2_CAP 7168        /* second-level decode entries (escape prefixes x 2^k) */
#define DC_LUT14_BITS 14        /* the exact redo's first level: 2^14 entries */
#define DC_LUT15_BITS 15        /* the fast decoder's first level: 2^15 entries */
#define DC_SYNC_MAX 1024        /* largest sync granularity (u16 chunk bit lengths) */

typedef struct dc_ctx dc_ctx;

/* Device-resident code table, written by the table kernels (layout is ABI). */
typedef struct dc_dtable {
    uint32_t code[256];             /* packed MSB-first code bits of byte s           */
    uint32_t nbits[256];            /* its bit length (0: byte has no code)           */
    uint32_t lut[1 << DC_LUT_BITS]; /* next 12 bits -> sym0 | bits(all)<<8 | sym1<<16 |
                                       bits(sym0)<<24 | count(1|2)<<29; 0: code > 12 b */
    uint32_t first[DC_MAX_DIGITS + 1]; /* canonical first value per digit length      */
    uint32_t count[DC_MAX_DIGITS + 1];
    uint32_t start[DC_MAX_DIGITS + 1];
    uint64_t lim[33];               /* left-justified limit per bit length (n = 2^w)  */
    uint16_t syms[DC_MAX_SYMS];     /* symbols sorted by (length, value)               */
    int32_t lengths[DC_MAX_SYMS];   /* Huffman lengths in digits (huffman())          */
    int32_t enc_len[DC_MAX_SYMS];   /* convert_lengths_to_encode_table() outputs      */
    uint32_t enc_val[DC_MAX_SYMS];
    int32_t n_ary, w, max_symbol_value, max_bits;
    int32_t min_len, max_len, status, last_written; /* last_written: index M assigned */
    /* decoder tables indexed by the LSB-first window (the stream's bits in order):
     * dlut: next 12 bits -> bits | sym << 8; bits 0: a longer code (or no code), whose
     *       12-bit prefix has escape id sym; dlut2: [id << dlut2_k | next dlut2_k bits] ->
     *       bits | sym << 8, 0: longer than 12 + dlut2_k bits or invalid (dlut2_k 0: none).
     * The second level exists when, with E = the escape ids (12-bit windows of no code of <= 12
     * bits, an incomplete code's windows of no code at all among them) and K = max_bits - 12
     * clamped to 1..8: 1 <= E <= 256, E << K <= DC_LUT2_CAP and max_bits <= 32. Then dlut2_k = K;
     * otherwise dlut2_k = 0, dlut2 is all 0 and every code past 12 bits takes the canonical
     * search. Past 256 escapes the id in dlut is the id mod 256 (unused: there is no dlut2). */
    uint16_t dlut[1 << DC_LUT_BITS];
    uint16_t dlut2[DC_LUT2_CAP];
    int32_t dlut2_k, dec_ready;   /* dec_ready: lut/dlut/dlut2/dlut14/dlut15 are current */
    int32_t fixed8;               /* every byte's code is 8 bits (or absent): pack and decode are byte maps */
    /* fixed8 with the coded bytes one contiguous range: code = byte - fixed8_lo for the
     * fixed8_count bytes fixed8_lo.., so the maps are byte-wise subtractions (flat or random
     * bytes: n = 2 on all 256 values codes every byte as itself) */
    int32_t fixed8_affine, fixed8_lo, fixed8_count;
    /* dlut14: next 14 bits -> bits | sym << 8 for codes of <= 14 bits; bits 0: longer, sym =
     * the escape id of its 12-bit prefix (as dlut); 16-B aligned for vector copies. Codes of 13
     * and 14 bits come from the second level, so they are resolved only when it exists and
     * dlut2_k >= 2; otherwise their entries are escapes like those of longer codes */
    uint16_t dlut14[1 << DC_LUT14_BITS];
    /* dlut15: next 15 bits -> bits | sym << 8 for codes of <= 15 bits (the fast decoder's
     * table); codes of 13..15 bits only when the second level exists and dlut2_k >= 3. Unlike
     * dlut14, an entry of no resolved code is 0, not the escape id: the fast decoder tests the
     * minimum over a chunk's entries against 0. So under a table whose longest code is 13 or 14
     * bits (dlut2_k 1 or 2) every chunk that holds a code past 12 bits takes the exact redo */
    uint16_t dlut15[1 << DC_LUT15_BITS];
} dc_dtable;

/* Node list of the n-ary Huffman tree (generate_huffman_tree's in-out list[],
 * n_ary_huffman.c:868-1005): nodes 0..M leaves, M+1.. the dummy leaves, then the internal
 * nodes in creation order. parent 0 = none (the root, or a leaf of count 0); left/right =
 * an internal node's first two children in pick order (:978-979); count = leaf frequency,
 * 1 for a dummy, the children's sum for an internal node. */
#define DC_TREE_NODES 4096
typedef struct dc_tree {
    int32_t nodes, first_internal, dummies, status;
    int32_t parent[DC_TREE_NODES];
    int32_t left[DC_TREE_NODES];
    int32_t right[DC_TREE_NODES];
    uint64_t count[DC_TREE_NODES];
} dc_tree;

/* ---- context ------------------------------------------------------------------------ */
/* stream: the hipStream_t to launch on (e.g. torch's current stream); NULL is the
 * default (legacy) stream. dc_ctx_create_owned makes a private non-blocking stream.
 * Both fail with DC_E_HIP when no HIP device is usable. */
int dc_ctx_create(dc_ctx **out, int device, void *stream);
int dc_ctx_create_owned(dc_ctx **out, int device);
void dc_ctx_destroy(dc_ctx *ctx);
int dc_ctx_sync(dc_ctx *ctx);
void *dc_ctx_stream(dc_ctx *ctx);
/* Per-stage HIP-event timing (on the stream the kernels run on). enable=1 starts
 * recording; dc_ctx_timings() synchronises and returns up to max stages. */
int dc_ctx_set_timing(dc_ctx *ctx, int enable);
int dc_ctx_timings(dc_ctx *ctx, const char **names, float *ms, int max);
/* Tuning options of a context (defaults suit MI355X; each is also read once from the
 * environment at context creation, for A/B runs: DC_HIST_GRID, DC_PACK_GRID, DC_D8_STATIC,
 * DC_DECODE_V7). Out-of-range values return DC_E_ARG and leave the option unchanged. */
enum {
    DC_OPT_HIST_GRID = 1,         /* histogram workgroups, 0 = default (512)              */
    DC_OPT_PACK_GRID = 2,         /* pack: workgroups (k_huff_pack, k_fe_pack; 0 = a block pair each)
                                     or blocks per wave (k_huff_pack_w; 0 = ~4096 waves) */
    DC_OPT_DECODE_STATIC_PCT = 3, /* fast decoder: statically dealt share of work, 0..100  */
    DC_OPT_DECODE_GENERAL = 4,    /* 1: decode with the general (any-S) decoder            */
    DC_OPT_HIST_PREFETCH = 5,     /* histogram: 32 KiB blocks in flight ahead, 1..2, 0 = 2 */
    DC_OPT_DECODE_VARIANT = 6,    /* fast decoder: 0 one code per lookup (k_huff_decode8),
                                     1 up to 3 codes per lookup (k_huff_decode9) */
    DC_OPT_NYB_ADEC_V1 = 7,       /* adaptive nybble decode: 0 tokens + control words + the
                                     SGPR-list resolve (k_nyb_resolve_c); 1 the one-pass
                                     single-wave k_nyb_adec; 2 tokens + r2's VGPR-list resolve;
                                     3 tokens + the plain-code resolve (k_nyb_resolve_s) (A/B) */
    DC_OPT_PACK_BLOCK = 8,        /* A/B builds only (-DDC_AB_KERNELS): a product build accepts 0
                                     alone. 2: the wave-per-range pack (k_huff_pack_w) instead of
                                     the workgroup-per-block one (k_huff_pack); 3: the same at 4
                                     codes a lane (0.386 vs 0.380 ms on 1 GiB C2); r6 (all slower,
                                     DESIGN.md 'Round 6'): 4 the block by LDS-DMA, 5 half-block
                                     stages, 6 one table read per byte (fold), 7 the next block's
                                     loads issued as pass B frees each piece */
    DC_OPT_NYB_WTILE_OFF = 9,     /* 1: the static nybble encode and the nybble decode write each
                                     4096-element tile with a workgroup (k_fsm_write) instead of a
                                     wave (k_nyb_enc_wtile / k_nyb_dec_wtile) */
    DC_OPT_BATCH_GRID = 10,       /* batch codec: workgroups of its persistent kernels, 0 = what a
                                     256-CU device holds at once (768 plan, 512 pack / decode; the
                                     shared-table mode: 1024 plan, 512 pack / decode) */
    DC_OPT_NYB_ADEC_SEG = 11      /* adaptive nybble decode (dc_nyb_decompress, modify = 1): tokens
                                     per launch of the resolve (k_nyb_resolve_c), 0 = the default
                                     of 16 Mi, which is also the largest value; the lists and the
                                     previous byte pass from one launch to the next in device
                                     memory. The output does not depend on it. */
};
int dc_ctx_set_option(dc_ctx *ctx, int option, int64_t value);
const char *dc_version(void);
size_t dc_dtable_size(void);

/* ---- device memory helpers (plain hipMalloc/hipMemcpy wrappers for ctypes users) --- */
int dc_malloc(void **d_ptr, size_t bytes);
int dc_free(void *d_ptr);
int dc_memcpy_h2d(dc_ctx *ctx, void *d_dst, const void *h_src, size_t bytes);
int dc_memcpy_d2h(dc_ctx *ctx, void *h_dst, const void *d_src, size_t bytes);
int dc_memset(dc_ctx *ctx, void *d_dst, int value, size_t bytes);
/* HBM reference rate: a float4 (16-B) device-to-device copy of `bytes` (multiple of 16,
 * 16-B aligned), nt loads and stores, one uint4 per lane over the full grid (one 256-thread
 * workgroup per 4 KiB; bench.py's copy probe) */
int dc_copy_probe(dc_ctx *ctx, const void *d_src, void *d_dst, uint64_t bytes);

/* ---- Huffman, device-resident stages ------------------------------------------------- */
/* (1) byte histogram of d_in[0..n) -> d_hist[256] (u64). Keeps per-block histograms in
 *     the context for dc_huff_plan on the SAME (d_in, n). */
int dc_huff_hist(dc_ctx *ctx, const uint8_t *d_in, uint64_t n, uint64_t *d_hist);
/* (2a) table from byte histogram d_hist[256]; symbols 256..max_symbol_value count 0. */
int dc_huff_table(dc_ctx *ctx, const uint64_t *d_hist, int max_symbol_value, int n_ary,
                  dc_dtable *d_table);
/* (2b) table from an arbitrary frequency array d_freq[max_symbol_value+1] (u64). */
int dc_huff_table_freq(dc_ctx *ctx, const uint64_t *d_freq, int max_symbol_value, int n_ary,
                       dc_dtable *d_table);
/* (2c) table from given lengths d_lengths[max_symbol_value+1] (skips the merge). */
int dc_huff_table_lengths(dc_ctx *ctx, const int32_t *d_lengths, int max_symbol_value,
                          int n_ary, dc_dtable *d_table);
/* (2d) the table of (2b) plus its whole node list (generate_huffman_tree) into d_tree */
int dc_huff_tree(dc_ctx *ctx, const uint64_t *d_freq, int max_symbol_value, int n_ary, dc_dtable *d_table,
                 dc_tree *d_tree);
/* (2e) summarize_tree_with_lengths' walk for any node list: d_depth[i] (i < leaves) = parent
 *      hops from node i to the root (-1: the walk exceeds the list, a cycle) */
int dc_tree_depths(dc_ctx *ctx, const int32_t *d_parent, int list_length, int leaves, int32_t *d_depth);
/* (3) the encode plan of the input of the last dc_huff_hist under d_table: its payload bit
 *     count into *d_total_bits (device u64) and the missing-code flag (dc_huff_pack_status).
 *     The per-block bit offsets are computed at pack time by two plan kernels before the
 *     pack (k_block_local: bits per 32 KiB block and a scan per 64 blocks; k_block_final_wide:
 *     the absolute offsets, and the zeroing of the payload words two blocks share). */
int dc_huff_plan(dc_ctx *ctx, const dc_dtable *d_table, uint64_t *d_total_bits);
/* (2+3 fused) the table of d_hist (dc_huff_table) and the plan of this context's last
 *     dc_huff_hist under it (dc_huff_plan) in ONE launch: a sharded encode's step after the
 *     all-reduce of the histograms (the table of the global histogram, the bits of the shard). */
int dc_huff_table_plan(dc_ctx *ctx, const uint64_t *d_hist, int max_symbol_value, int n_ary, dc_dtable *d_table,
                       uint64_t *d_total_bits);
/* (1+2+3 fused) histogram, table and plan of d_in[0..n) in ONE launch: the histogram's last
 *     workgroup builds the table (as dc_huff_table) and the plan total (as dc_huff_plan) from
 *     the histogram it holds. The single-stream encoder's path (a sharded encode must reduce
 *     the histograms between the two, so it calls them separately). */
int dc_huff_encode_plan(dc_ctx *ctx, const uint8_t *d_in, uint64_t n, int max_symbol_value, int n_ary,
                        uint64_t *d_hist, dc_dtable *d_table, uint64_t *d_total_bits);
/* ---- Length-limited tables -------------------------------------------------------------
 * The twins of (2a), (2b), (2+3 fused) and (1+2+3 fused) with max_digits added: a table none of
 * whose codes is longer than max_digits base-n digits (max_digits * w bits, w = ceil(log2 n)).
 * Each is asynchronous and makes no host read.
 *   max_digits == 0   no cap: the call IS its twin, the same kernels and the same table.
 *   max_digits > DC_MAX_DIGITS, or max_digits * w > 32: DC_E_ARG from the host, nothing launched.
 *   fewer than k = #{count > 0} codes of max_digits digits exist (n^max_digits < k): the table's
 *   status is DC_E_ARG (dc_huff_table_status), and nothing else about that table is promised.
 * The rule, on the lengths l[] the uncapped call gives (DESIGN.md "Length-limited tables"): when
 * no l passes D = max_digits the table is the uncapped one, byte for byte. Otherwise the present
 * symbols are counted per length min(l, D), the counts are repaired (dc_huff_limit_classes below),
 * and the symbols in the order (count descending, higher symbol value first among equal counts)
 * take the lengths in ascending order: cnt[1] symbols length 1, the next cnt[2] length 2, ...
 * Symbols of count 0 keep length 0. The canonical stage then runs on these lengths exactly as
 * dc_huff_table_lengths would: lengths[] holds the capped lengths, and enc_*, code / nbits,
 * first / count / start / syms, lim, min_len / max_len / max_bits, fixed8* and last_written
 * follow from them; dec_ready is cleared; status is DC_OK. The plan of a capped table is the plan
 * under the capped nbits. Every consumer (pack, all decoders, the shared-table batch calls, DCH1)
 * takes such a table as it takes any other.
 * Useful caps at n = 2: 15 bits, every code resolves from dlut15 (the S = 64 fast decoder redoes
 * no chunk for its code lengths); 12 bits, every code resolves from the first-level dlut and no
 * dlut2 exists. Caps of 13 or 14 bits are worse than 15 for the fast decoder: dlut2_k is then 1
 * or 2, and every chunk with a code past 12 bits takes the exact redo (dlut15 above).
 * Launches: dc_huff_table_limit, dc_huff_table_freq_limit and dc_huff_table_plan_limit ONE
 * (k_huff_table_limit: one 256-thread workgroup, as their twins); dc_huff_encode_plan_limit TWO
 * (the histogram as dc_huff_hist launches it, then k_huff_table_limit on it with the plan): one
 * more than dc_huff_encode_plan, so that the histogram kernels are the uncapped ones. */
int dc_huff_table_limit(dc_ctx *ctx, const uint64_t *d_hist, int max_symbol_value, int n_ary, int max_digits,
                        dc_dtable *d_table);
/* any max_symbol_value up to DC_MAX_SYMS - 1 */
int dc_huff_table_freq_limit(dc_ctx *ctx, const uint64_t *d_freq, int max_symbol_value, int n_ary, int max_digits,
                             dc_dtable *d_table);
int dc_huff_table_plan_limit(dc_ctx *ctx, const uint64_t *d_hist, int max_symbol_value, int n_ary, int max_digits,
                             dc_dtable *d_table, uint64_t *d_total_bits);
int dc_huff_encode_plan_limit(dc_ctx *ctx, const uint8_t *d_in, uint64_t n, int max_symbol_value, int n_ary,
                              int max_digits, uint64_t *d_hist, dc_dtable *d_table, uint64_t *d_total_bits);
/* The repair of the length counts, pure host arithmetic (no device, no context; the table kernel
 * runs the same function, csrc/dc_huff_limit.h). cnt[d], 1 <= d <= max_digits, holds the number
 * of present symbols of length min(l, max_digits) and k their total (cnt[0] is not read), with
 * B = n^max_digits and K = sum cnt[d] n^(max_digits - d):
 *   demote   while K > B: one symbol of the largest d < max_digits with cnt[d] > 0 moves to d + 1;
 *   promote  for d = max_digits down to 2: while cnt[d] > 0 and K + (n-1) n^(max_digits-d) <= B,
 *            one symbol of length d moves to d - 1.
 * Returns DC_OK with cnt repaired in place, or DC_E_ARG (cnt unchanged) for a NULL cnt, an invalid
 * n_ary or max_digits (as the calls above; 0 is invalid here), sum cnt != k, or B < k. */
int dc_huff_limit_classes(int n_ary, int max_digits, uint32_t *cnt, uint64_t k);
/* (4) pack at global bit offset bit_base into d_words (word 0 = stream word bit_base/32,
 *     MSB-first bytes; 16-B aligned). Capacity: dc_huff_words_needed().
 *     Sync index (DESIGN.md "Sync index v1"), both arrays NULL for none: chunks of
 *     sync_syms symbols (power of two, 16..DC_SYNC_MAX): d_sync_len[c] = bit length of
 *     chunk c (u16, dc_huff_sync_chunks entries); d_sync_base[g] = absolute bit offset of
 *     chunk 64g (u64, dc_huff_sync_groups entries). */
int dc_huff_pack(dc_ctx *ctx, const uint8_t *d_in, uint64_t n, const dc_dtable *d_table,
                 uint64_t bit_base, uint32_t *d_words, uint64_t words_cap,
                 uint64_t *d_sync_base, uint16_t *d_sync_len, uint32_t sync_syms);
uint64_t dc_huff_sync_chunks(uint64_t n, uint32_t sync_syms);
uint64_t dc_huff_sync_groups(uint64_t n, uint32_t sync_syms);
uint64_t dc_huff_words_needed(uint64_t bit_base, uint64_t total_bits);
/* inspection (synchronising): the exclusive per-block bit offsets of the last plan (nblocks+1
 * entries, last = total; recomputed on demand) and the per-block u16 histograms of the last
 * dc_huff_hist */
int dc_huff_plan_offsets(dc_ctx *ctx, uint64_t *h_off, uint64_t max_entries, uint64_t *h_n);
int dc_huff_block_hist(dc_ctx *ctx, uint16_t *h_bh, uint64_t max_entries);
/* (4') the same without any host round trip (graph/timing friendly): with a byte without a
 *     code, or words_cap below the words the stream touches, the pack writes no code bit and no
 *     sync entry. The plan kernels run before it looks, so d_words is not left as it was: the
 *     words that hold a block's first bit, and the stream's partial last word, are zeroed where
 *     they lie below words_cap; nothing else is written. Here words_cap need only cover the
 *     stream's words (dc_huff_words_needed's slack is the decoder's; dc_huff_pack insists on it).
 *     Read the outcome with dc_huff_pack_status() (synchronising). The outcome is the plan's: after
 *     DC_E_CAPACITY every later pack of the same plan reads DC_E_CAPACITY too, so plan again before
 *     packing into a larger buffer. */
int dc_huff_pack_async(dc_ctx *ctx, const uint8_t *d_in, uint64_t n, const dc_dtable *d_table,
                       uint64_t bit_base, uint32_t *d_words, uint64_t words_cap,
                       uint64_t *d_sync_base, uint16_t *d_sync_len, uint32_t sync_syms);
/* ... with the stream's bit offset read by the kernels from device memory (*d_bit_base, a
 * u64 written earlier on the stream, e.g. a shard's exclusive prefix of the ranks' payload
 * bits): a sharded encode then needs no host read of the gathered bit counts. */
int dc_huff_pack_async_dev(dc_ctx *ctx, const uint8_t *d_in, uint64_t n, const dc_dtable *d_table,
                           const uint64_t *d_bit_base, uint32_t *d_words, uint64_t words_cap,
                           uint64_t *d_sync_base, uint16_t *d_sync_len, uint32_t sync_syms);
int dc_huff_pack_status(dc_ctx *ctx, const dc_dtable *d_table);
/* the outcome of one particular plan + pack: gen = dc_huff_plan_gen() read right after its
 * plan (dc_huff_plan / dc_huff_encode_plan), so later encodes on the context do not answer
 * for it. DC_E_STATE when more than 30 plans have run since (its flags are recycled). */
uint32_t dc_huff_plan_gen(dc_ctx *ctx);
int dc_huff_pack_status_gen(dc_ctx *ctx, const dc_dtable *d_table, uint32_t gen);
/* C5 fused front-end encode (small_compression.c:582-665 front-end, then n-ary Huffman of its
 * output M), without M ever written to memory: the stream and sync index are exactly those of
 * dc_small_compress followed by dc_huff_encode_plan + dc_huff_pack_async on M (the same payload
 * bits, the same sync chunks of S symbols of M), from the input bytes d_in (16-B aligned, n >= 2).
 * (1-3) the histogram of M per 32 KiB block of the input, the table and the plan total in one
 *     launch (as dc_huff_encode_plan);
 * (4) two plan launches (block bit offsets, each block's first symbol index, the sync-length
 *     words of chunks spanning block boundaries zeroed) and the pack. d_sync_len (4-B aligned)
 *     and d_sync_base are required, sized for dc_small_huff_symbols() symbols: at most n + 1.
 *     Sizing: the kernels clear and add d_sync_len as whole dwords (two u16 lengths at a time),
 *     so allocate ceil(chunks / 2) * 2 + 2 u16 entries, chunks = ceil((n + 1) / S): with an odd
 *     chunk count the last dword reaches one entry past the last chunk.
 * dc_huff_pack_status then returns DC_E_FALLBACK (nothing usable written) when the front-end
 * output falls back to LITERAL (small_compression.c:655-662), when every byte value occurs in
 * M (the pack marks a pair's start with a byte value that has no code), or when a 32 KiB block
 * codes to more bits than the pack's stage holds beside its sync list; the caller then runs
 * the two stages. dc_small_huff_symbols reads the symbol count of M (synchronising).
 * words_cap need only cover the words the stream has a bit in (as dc_huff_pack_async), and no
 * word from words_cap on is touched. After DC_E_FALLBACK the outputs are not as they were: the
 * plan kernels have zeroed the block-boundary words and length dwords, and for an over-long block
 * the other blocks have been packed; nothing outside the documented sizes is written. */
int dc_small_huff_plan(dc_ctx *ctx, const uint8_t *d_in, uint64_t n, int max_symbol_value, int n_ary,
                       uint64_t *d_hist, dc_dtable *d_table, uint64_t *d_total_bits);
int dc_small_huff_pack_async(dc_ctx *ctx, const uint8_t *d_in, uint64_t n, const dc_dtable *d_table,
                             uint64_t bit_base, uint32_t *d_words, uint64_t words_cap,
                             uint64_t *d_sync_base, uint16_t *d_sync_len, uint32_t sync_syms);
int dc_small_huff_symbols(dc_ctx *ctx, uint64_t *h_symbols);
/* The same fused encode for one contiguous shard of the input (dist.ShardedSmall at world > 1;
 * the front-end's only halo is one byte each side). d_shard: 4 x int64 on the
 * device, read by the kernels (no host synchronisation): {global bit of the shard's first code,
 * global index of its first symbol of M, the input byte before the shard (-1: the shard starts the
 * stream: type byte 8, raw first byte), the input byte after it (-1: none)}.
 * dc_small_huff_shard_hist: the shard's histogram of M (no table; the caller all-reduces the
 * shards' histograms and runs dc_huff_table_plan, which also plans this shard's bits).
 * dc_small_huff_shard_pack_async: the shard's codes at that global bit (d_words: word 0 = the
 * stream's word d_shard[0] / 32, the shared first and last words holding only this shard's bits,
 * OR-merged by the gather), its local sync index (chunks of S symbols from its own first symbol:
 * its own decode) and its part of the stream's sync index (d_gsync_len: u16 per global chunk c
 * at entry c - (c0 & ~1), c0 = its first chunk, the first and last entries partial: the gather adds
 * the neighbours' parts; d_gsync_base: the groups that start in the shard, from group
 * ceil(first symbol / 64 S)). Fallbacks as dc_small_huff_pack_async, except the LITERAL test,
 * which belongs to the whole stream (the caller's). Sizes: d_sync_len / d_sync_base as for
 * dc_small_huff_pack_async (n + 1 symbols, u16 lengths rounded up to whole dwords + 2 entries);
 * d_gsync_len / d_gsync_base for n + 1 + 2 S symbols (the shard's chunks counted from c0 & ~1,
 * plus the partial chunks it shares at either end), the lengths rounded the same way.
 * n >= 2; d_in 16-B aligned. words_cap: the words the shard has a bit in, counted from the word of
 * d_shard[0]; no word from words_cap on is touched. (A last 32 KiB block that is one byte, a space
 * before the letter after the shard, holds no symbol; when it starts on a word boundary it has no
 * word, and the pack leaves the word at index = the shard's words alone.) Entry 0 of d_gsync_len
 * is written as zero when c0 is odd, and so is the entry after the last chunk when that chunk is
 * even: the plan zeroes whole dwords. */
int dc_small_huff_shard_hist(dc_ctx *ctx, const uint8_t *d_in, uint64_t n, const int64_t *d_shard,
                             uint64_t *d_hist);
int dc_small_huff_shard_pack_async(dc_ctx *ctx, const uint8_t *d_in, uint64_t n, const dc_dtable *d_table,
                                   const int64_t *d_shard, uint32_t *d_words, uint64_t words_cap,
                                   uint64_t *d_sync_base, uint16_t *d_sync_len, uint64_t *d_gsync_base,
                                   uint16_t *d_gsync_len, uint32_t sync_syms);
/* C5 decode: the Huffman decode of the m-symbol front-end stream M into d_m (16-B aligned,
 * >= m bytes), counting the symbols >= 0x80 of every group of 64 chunks on the way (S = 64), then
 * the front-end inverse (small_compression.c's decompress_bytestring, dc_small_decompress) into
 * d_out (>= 2 m bytes) from those counts, without the inverse's own counting pass over M. *h_len =
 * the decoded length (synchronising). Other sync sizes, a LITERAL stream or an unaligned d_m
 * take the two stages unchanged. */
int dc_small_huff_decode(dc_ctx *ctx, const uint32_t *d_words, uint64_t bit_base, uint64_t words,
                         const uint64_t *d_sync_base, const uint16_t *d_sync_len, uint32_t sync_syms, uint64_t m,
                         const dc_dtable *d_table, uint8_t *d_m, uint8_t *d_out, uint64_t *h_len);
/* Status word written by the table / plan kernels (host-synchronising read). */
int dc_huff_table_status(dc_ctx *ctx, const dc_dtable *d_table, int32_t *max_bits);
/* (5) decode n symbols. d_words/bit_base and the sync index as written by pack. The
 * decoder tables (dc_dtable dlut*) are rebuilt first unless this context's last pack built
 * them for d_table; a table rewritten since by other means (another context, a copy) and
 * not packed or rebuilt through this context is reported by dc_huff_decode_status as
 * DC_E_STREAM (the decoder checks dec_ready), never decoded with stale tables. */
int dc_huff_decode(dc_ctx *ctx, const uint32_t *d_words, uint64_t bit_base, uint64_t words,
                   const uint64_t *d_sync_base, const uint16_t *d_sync_len, uint32_t sync_syms,
                   uint64_t n, const dc_dtable *d_table, uint8_t *d_out);
/* ... with the bit offset in device memory (as dc_huff_pack_async_dev) */
int dc_huff_decode_dev(dc_ctx *ctx, const uint32_t *d_words, const uint64_t *d_bit_base, uint64_t words,
                       const uint64_t *d_sync_base, const uint16_t *d_sync_len, uint32_t sync_syms,
                       uint64_t n, const dc_dtable *d_table, uint8_t *d_out);
/* (5r) random access: decode nranges symbol ranges of the stream: range r = symbols
 * [d_first[r], d_first[r] + d_count[r]) -> d_out[d_out_off[r] ..), any byte alignment.
 * d_first / d_count / d_out_off: device u64 arrays, read by the kernels (no host round trip),
 * so a gather list computed on the GPU can be used as it is. Asynchronous.
 * The stream arguments are those of dc_huff_decode (d_words 16-B aligned, the same payload slack,
 * any valid sync_syms, any table; stale decoder tables are rebuilt or reported the same way).
 * Only the chunks a range touches are read: the payload bits from its first chunk's start to its
 * last chunk's end, and the index entries of its groups. No byte of d_out outside the requested
 * ranges is written. Output ranges that overlap are the caller's business: which range's bytes
 * land there is unspecified. count 0 is legal (writes nothing); nranges 0 returns DC_OK
 * without a launch. A bad range (first + count > n, or out_off + count > out_cap) writes
 * nothing and is reported by dc_huff_decode_status as DC_E_ARG; every other range of the call is
 * still decoded. At most DC_RANGES_MAX ranges per call: the context keeps 16 B of scratch per
 * range, and one workgroup scans the per-range group counts (time linear in nranges). */
#define DC_RANGES_MAX (1ull << 28)
int dc_huff_decode_ranges(dc_ctx *ctx, const uint32_t *d_words, uint64_t bit_base, uint64_t words,
                          const uint64_t *d_sync_base, const uint16_t *d_sync_len, uint32_t sync_syms,
                          uint64_t n, const dc_dtable *d_table,
                          const uint64_t *d_first, const uint64_t *d_count, const uint64_t *d_out_off,
                          uint64_t nranges, uint8_t *d_out, uint64_t out_cap);
/* one range given by value (grid sized on the host, no device arrays, no scan launch) into
 * d_out[0 .. count), any alignment; first + count > n returns DC_E_ARG at once */
int dc_huff_decode_range(dc_ctx *ctx, const uint32_t *d_words, uint64_t bit_base, uint64_t words,
                         const uint64_t *d_sync_base, const uint16_t *d_sync_len, uint32_t sync_syms,
                         uint64_t n, const dc_dtable *d_table,
                         uint64_t first, uint64_t count, uint8_t *d_out);
/* status of the last dc_huff_decode / dc_huff_decode_range(s) on this context (synchronising):
 * DC_E_STREAM for a corrupt stream or stale tables; DC_E_ARG when only a bad range of
 * dc_huff_decode_ranges was flagged; 0 otherwise */
int dc_huff_decode_status(dc_ctx *ctx);
/* chunks of the last S = 64 dc_huff_decode on this context that took the exact redo (codes
 * longer than the 15-bit table, partial or over-long groups); synchronising, diagnostic */
int dc_huff_decode_redo_count(dc_ctx *ctx, uint64_t *count);
/* ---- Huffman batch v1: many small buffers, one table each, one call --------------
 * The reference's own design is blocks of <= 65000 bytes with a table each
 * (n_ary_huffman.c:1210-1255, :1866-1883); this is its device-resident form for thousands of
 * independent buffers. A batch is `count` segments d_in[d_in_off[i] .. d_in_off[i+1]) (d_in_off:
 * device u64, count + 1 entries; any byte alignment; length 0 legal; at most DC_BATCH_SEG_MAX
 * bytes each). One n_ary (2..256) and one sync size (a power of two, 16..DC_SYNC_MAX) hold for
 * the batch. For segment i of length len with byte histogram h:
 *   lens   d_lens[256 i + s], s < 256 (u8, in digits): the first 256 lengths dc_huff_table(h, 258,
 *          n_ary) gives; the codes are those of dc_huff_table_lengths on them (256..258 at 0).
 *   mode   d_mode[i] = 1 (Huffman) when every present byte's packed code is <= 32 bits and
 *          bits < 8 len; else 0 (stored: the payload is the segment's bytes). len 0 is stored.
 *   bits   d_bits[i] (u32): the payload bits (mode 1) or 8 len (mode 0).
 *   payload  ceil(bits / 8) bytes at d_payload + d_pay_off[i], MSB-first: exactly the stream
 *          dc_huff_pack writes for the segment alone at bit_base 0. d_pay_off (u64, count + 1
 *          entries): pay_off[0] = 0, pay_off[i + 1] = pay_off[i] + round_up_16(ceil(bits / 8));
 *          the pad bytes are zero, so d_payload[0 .. pay_off[count]) is deterministic, and
 *          every segment's payload is 16-B aligned (d_payload must be): with a table from
 *          dc_huff_table_lengths and group bases summed from its sync entries, a Huffman-mode
 *          segment also decodes with dc_huff_decode.
 *   sync   d_sync_len (u16) holds ceil(len / sync_syms) entries per segment from
 *          d_sync_off[i] (u64, count + 1 entries, the exclusive prefix of the entry counts):
 *          entry c = the bit length of symbols [c S, min((c + 1) S, len)); 8 bits a symbol in a
 *          stored segment. No group bases: a segment has at most 4096 chunks, scanned in LDS.
 * d_status[i] (i32) receives each segment's outcome; a bad segment never stops the others:
 *   DC_E_ARG       longer than DC_BATCH_SEG_MAX, or offsets that decrease: nothing is written
 *                  for it (not even lens / mode / bits), and it takes 0 payload bytes and 0 sync
 *                  entries
 *   DC_E_CAPACITY  its payload or sync entries would pass payload_cap / sync_cap (decode: its
 *                  output would pass out_cap): nothing of it is written; nothing is ever written
 *                  past a cap
 *   DC_E_STREAM    (decode) the mode byte is neither 0 nor 1, a length exceeds DC_MAX_DIGITS or
 *                  gives a code over 32 bits, the offsets do not fit bits / the asked length,
 *                  the chunk lengths do not sum to bits, or a chunk does not decode to exactly
 *                  its symbols in exactly its bits (an invalid or over-long code, a present
 *                  byte whose length was lost): nothing of the segment is written
 * Sizing: dc_huff_batch_payload_bound = total_bytes + 16 count (exact as an upper bound: the
 * stored fallback); dc_huff_batch_sync_bound = ceil(total_bytes / S) + count u16 entries, no
 * slack: the batch kernels access every entry as a u16 of its own. Both are pure host
 * arithmetic (csrc/dc_batch_bound.h). */
#define DC_BATCH_SEG_MAX 65536u
typedef struct dc_hbatch {
    uint64_t count;          /* segments                                                  */
    int32_t n_ary;
    uint32_t sync_syms;
    uint8_t *d_lens;         /* 256 x count                                               */
    uint8_t *d_mode;         /* count                                                     */
    uint32_t *d_bits;        /* count                                                     */
    uint64_t *d_pay_off;     /* count + 1                                                 */
    uint8_t *d_payload;      /* payload_cap bytes, 16-B aligned                           */
    uint64_t payload_cap;
    uint64_t *d_sync_off;    /* count + 1                                                 */
    uint16_t *d_sync_len;    /* sync_cap entries                                          */
    uint64_t sync_cap;
    int32_t *d_status;       /* count: written by the last encode / decode of the batch   */
} dc_hbatch;
uint64_t dc_huff_batch_payload_bound(uint64_t total_bytes, uint64_t count);
uint64_t dc_huff_batch_sync_bound(uint64_t total_bytes, uint64_t count, uint32_t sync_syms);
/* Encode: fills every array of *batch (batch->count must equal count). Asynchronous, no host
 * read anywhere, and the same launches for any count and any segment sizes: one plan kernel
 * (a workgroup per segment on a persistent grid: histogram, lengths, canonical codes, the
 * compact record), two scans (d_pay_off, d_sync_off) and one pack kernel. count 0 returns DC_OK
 * without a launch. At most DC_RANGES_MAX segments. */
int dc_huff_encode_batch(dc_ctx *ctx, const uint8_t *d_in, const uint64_t *d_in_off, uint64_t count,
                         const dc_hbatch *batch);
/* Encode with length-limited tables: dc_huff_encode_batch exactly (the same arrays, bounds,
 * statuses and launches, no host read), but segment i's table is the one dc_huff_table_limit(h, 258,
 * n_ary, max_digits) builds from its histogram ("Length-limited tables" above):
 *   lens   the first 256 lengths of that capped table; none passes max_digits.
 *   mode, bits  decided under the capped code: Huffman when sum h[s] * nbits[s] < 8 len, else
 *          stored. A segment the unlimited call codes may be stored here (4096 bytes holding all
 *          256 values at n = 2, max_digits = 8: every length is 8, the bits are 8 len).
 *   no code  fewer than k = #{h > 0} codes of max_digits digits exist (n^max_digits < k): the
 *          segment is stored, its status is DC_OK (a stored segment always decodes) and its lens
 *          record is 256 zeros; the decoders read lens for mode 1 alone.
 * Payload, offsets, sync entries, pads and caps mean what they mean above, and every decode call
 * takes such a batch as it takes any other: the code is rebuilt from lens.
 *   max_digits == 0   the call IS dc_huff_encode_batch: the same kernels, every array byte-identical.
 *   max_digits > DC_MAX_DIGITS, or max_digits * w > 32: DC_E_ARG from the host, nothing launched.
 * With max_digits <= 15 every record has a nybble form (below). The cap is repaired by one lane
 * per segment, a few dozen serial steps when it binds. */
int dc_huff_encode_batch_limit(dc_ctx *ctx, const uint8_t *d_in, const uint64_t *d_in_off, uint64_t count,
                               int max_digits, const dc_hbatch *batch);
/* ---- Huffman batch v1: nybble records ---------------------------------------------------------
 * The lens records in half the bytes, once no length passes 15 (the reference's "256 nybbles",
 * n_ary_huffman.c:2415-2420). A storage form only: the batch calls read 256-byte records, so a
 * caller packs after the encode and unpacks before the decode. Record i is 128 bytes at
 * d_lens4 + 128 i; byte j = lens[2j] << 4 | lens[2j + 1] (the high nybble first, as the bitstream
 * and the nybble codec put things).
 * Pack: d_status[i] (i32, count entries) = DC_OK, or DC_E_CODE_TOO_LONG for a record that holds a
 * length above 15: its 128 bytes are written as zeros, every other record is unaffected, and the
 * lowest failing index goes to the context's first-failure slot (dc_huff_batch_status). A zero
 * record unpacks to all-zero lengths, under which the decoders fail a mode-1 segment with
 * DC_E_STREAM: never a wrong byte. Every record of dc_huff_encode_batch_limit with max_digits <= 15
 * packs; an uncapped record packs when the segment's tree is at most 15 deep.
 * Unpack: always succeeds, writes all 256 bytes of every record, and leaves the first-failure slot
 * as it is.
 * Both: asynchronous, one launch for any count, no host read; count 0 returns DC_OK without a
 * launch; DC_E_ARG for more than DC_RANGES_MAX records, a NULL pointer with count > 0, d_lens not
 * 16-B or d_lens4 not 8-B aligned, or buffers that overlap. DC_OPT_BATCH_GRID sizes their grids. */
int dc_huff_batch_lens_pack(dc_ctx *ctx, const uint8_t *d_lens, uint64_t count, uint8_t *d_lens4, int32_t *d_status);
int dc_huff_batch_lens_unpack(dc_ctx *ctx, const uint8_t *d_lens4, uint64_t count, uint8_t *d_lens);
/* Decode: segment i -> d_out[d_out_off[i] .. d_out_off[i + 1]) (device u64, count + 1 entries,
 * any alignment). The length asked for must be the segment's (the format does not store it).
 * Asynchronous, one launch. No byte of d_out outside the requested ranges is written, and none
 * of a segment that fails. dc_huff_decode_batch_scatter: the same with each segment's range
 * given by its own start and end, d_out[d_out_beg[i] .. d_out_end[i]) (count entries each), so
 * the outputs may lie anywhere in d_out, with gaps and in any order. */
int dc_huff_decode_batch(dc_ctx *ctx, const dc_hbatch *batch, uint8_t *d_out, const uint64_t *d_out_off,
                         uint64_t out_cap);
int dc_huff_decode_batch_scatter(dc_ctx *ctx, const dc_hbatch *batch, uint8_t *d_out, const uint64_t *d_out_beg,
                                 const uint64_t *d_out_end, uint64_t out_cap);
/* 0, or the status of the lowest-numbered failing segment of the last batch call on this
 * context (synchronising) */
int dc_huff_batch_status(dc_ctx *ctx);
/* ---- Huffman batch v1, shared table: every segment under ONE dc_dtable ------------------------
 * A mode of the same dc_hbatch for thousands of small, similar buffers (pages, records, rows):
 * the table is built once (from the whole batch, or from a training sample), stored once, and
 * every segment still decodes alone. Everything is as in batch v1 except that there is no
 * per-segment lens record (batch->d_lens is neither read nor written and may be NULL) and
 * *d_table holds for the whole batch. With nb[s] = d_table->nbits[s], code[s] = d_table->code[s],
 * for segment i of length len:
 *   mode   1 when len > 0, every byte of the segment has nb != 0, and bits = sum nb[byte] < 8 len;
 *          else 0 (stored, bits = 8 len). A byte without a code under the table (also one whose
 *          code passes 32 bits: the table kernels leave its nbits 0) makes that segment stored; it
 *          is never an error, so a trained table is safe on any input.
 *   payload, pay_off, sync_len, sync_off, the zero pads, the 16-B alignment, both bound functions,
 *          the statuses and "nothing is written for a failed segment or past a cap": batch v1's.
 *          A mode-1 payload is bit for bit what dc_huff_pack writes for the segment alone at bit 0
 *          under d_table, so it also decodes with dc_huff_decode under that table.
 * batch->n_ary must equal the table's n_ary, and the table's status must be DC_OK or
 * DC_E_CODE_TOO_LONG (such a table is usable: its over-long codes are "no code"). The kernels read
 * both on the device (no host read); otherwise every segment gets DC_E_ARG and nothing is written.
 * The table is const: the kernels read code / nbits (decode also first / count / start / syms /
 * min_len / max_len), never dec_ready or dlut*, and write nothing into it, so one table serves
 * many contexts and streams at once, and a table rebuilt elsewhere by dc_huff_table_lengths from
 * the same lengths (dc_huff_table_get_lengths) decodes the batch. What to store: the lengths once,
 * then mode, bits, the payload and the u16 index per segment.
 * Decoding under a different table is reported as DC_E_STREAM whenever a chunk then fails to
 * decode to exactly its symbols in exactly its bits; as in batch v1 there is no checksum, so a
 * wrong table that happens to satisfy every chunk is not detected ("checksums" below: the CRC-32
 * per segment a caller can keep beside the batch and verify after the decode). A window that decodes to a
 * symbol >= 256 (the table's canonical arrays hold up to DC_MAX_SYMS symbols) is a corrupt stream,
 * never a byte written.
 * Host argument rules are batch v1's without the d_lens test, and d_table must not be NULL. All
 * three calls are asynchronous and make no host read; count 0 returns DC_OK without a launch;
 * dc_huff_batch_status answers for them; DC_OPT_BATCH_GRID sizes their grids. Encode: one plan
 * kernel (no histogram, no table work), the two scans, one pack kernel. Decode: one launch, the
 * first-level table and the long-code arrays built once per workgroup, not per segment. Once a
 * segment's table is in LDS, its pack and its decode (validation, chunk checks, commit, write) are
 * the same device code in both modes (csrc/dc_batch_kernels.inc). */
int dc_huff_encode_batch_shared(dc_ctx *ctx, const uint8_t *d_in, const uint64_t *d_in_off, uint64_t count,
                                const dc_dtable *d_table, const dc_hbatch *batch);
int dc_huff_decode_batch_shared(dc_ctx *ctx, const dc_hbatch *batch, const dc_dtable *d_table,
                                uint8_t *d_out, const uint64_t *d_out_off, uint64_t out_cap);
int dc_huff_decode_batch_shared_scatter(dc_ctx *ctx, const dc_hbatch *batch, const dc_dtable *d_table,
                                        uint8_t *d_out, const uint64_t *d_out_beg, const uint64_t *d_out_end,
                                        uint64_t out_cap);
/* the table's lengths in digits, entries 0 .. max_symbol_value (what dc_huff_table_lengths takes
 * back): all a shared batch needs stored beside its arrays. *h_count receives max_symbol_value + 1;
 * DC_E_CAPACITY (nothing copied) when max_entries is smaller. Synchronising. */
int dc_huff_table_get_lengths(dc_ctx *ctx, const dc_dtable *d_table, int32_t *h_lengths, int max_entries, int *h_count);
/* ---- Huffman batch v1: byte ranges of segments in one call ------------------------------------
 * Random access into a batch by its per-chunk u16 bit lengths, with no change to the format.
 * Range r is the bytes [d_first[r], d_first[r] + d_count[r]) of segment d_seg[r]; it goes to
 * d_out[d_out_off[r] .. d_out_off[r] + d_count[r]), at any byte alignment. d_seg_off (batch->count
 * + 1 entries) gives the segment lengths as d_in_off did at encode (the format does not store
 * them); only the differences d_seg_off[i + 1] - d_seg_off[i] are used. Every array is a device
 * u64 array that the kernels read, so a gather list computed on the GPU works as it is. None of
 * them may be written while the call runs.
 * dc_huff_decode_batch_ranges is for a batch of own tables (d_lens), dc_huff_decode_batch_shared_
 * ranges for one coded under *d_table (d_lens is not read).
 * Asynchronous, no host read, one launch whatever nranges is. nranges 0 returns DC_OK without a
 * launch; nranges > DC_RANGES_MAX returns DC_E_ARG. Host argument rules are the whole-segment
 * decoders'; in addition d_seg_off, the four range arrays and d_rstatus must not be NULL when
 * nranges > 0. batch->d_status is neither read nor written.
 * d_rstatus[r] (i32, nranges entries) receives the range's outcome; a bad range never stops the
 * others. The tests run in this order, and the first that fails decides:
 *   1  DC_E_ARG       d_seg[r] >= batch->count
 *   2  DC_E_ARG       the segment's offsets decrease, or its length len exceeds DC_BATCH_SEG_MAX
 *   3  DC_E_ARG       first > len or count > len - first (no sum is formed: first = 2^64 - 1 with
 *                     count = 2 is refused, not wrapped)
 *   4  DC_E_CAPACITY  out_off > out_cap or count > out_cap - out_off
 *   5  DC_OK          count == 0: nothing further is read
 *   6  DC_E_ARG       (shared) the table's arity is not the batch's, or its status is neither
 *                     DC_OK nor DC_E_CODE_TOO_LONG: every range that comes this far
 *      DC_E_STREAM    the segment's record fails the whole-segment decoder's tests against len
 *                     (mode, bits, pay_off, sync_off), or (own tables) its lens give no code
 *   7  DC_E_STREAM    a touched chunk does not decode to exactly its symbols in exactly its bits,
 *                     a stored segment's touched entry is not 8 x its symbols, or the last
 *                     touched chunk ends past bits
 * A range with any status but DC_OK writes no byte, and no byte of d_out outside the requested
 * ranges is ever written. Output ranges that overlap are the caller's business.
 * What is read and verified: only the chunks a range touches, plus the u16 entries of the
 * segment's chunks before them (at most 4096 entries, 8 KiB), summed for the first touched
 * chunk's bit position. Corruption elsewhere in the segment is NOT seen by a range read: only a
 * whole-segment decode checks that the chunk lengths sum to bits and that every chunk decodes.
 * The context's first-failure slot keeps the lowest failing range index: dc_huff_batch_status
 * answers for these calls as for the others. DC_OPT_BATCH_GRID sizes their grids.
 * Cost. Shared table: the tables are copied once per workgroup; ranges are dealt four consecutive
 * at a time, four of at most 8 KiB each one to a wave, a group with a longer range one after the
 * other to the workgroup. Own tables: each workgroup takes a contiguous run of range indices and
 * rebuilds the segment's code (from its 256 lens) only when d_seg[r] differs from the range
 * before, so a list sorted by segment pays one table build per segment (per workgroup that meets
 * it) and an unsorted list pays one per range. */
/* The range arithmetic as the kernels compile it (csrc/dc_batch_range.h), pure host code, for a
 * caller that plans or checks a gather list on the host. dc_huff_batch_range_chunks: the chunks
 * [*c_lo, *c_hi) of sync_syms symbols that hold a byte of [first, first + count) (count 0: none,
 * c_lo == c_hi); DC_E_ARG for a NULL pointer or an invalid sync_syms. dc_huff_batch_range_args:
 * tests 2 to 4 above for a segment of offsets [seg_beg, seg_end): DC_E_ARG, DC_E_CAPACITY or DC_OK. */
int dc_huff_batch_range_chunks(uint64_t first, uint64_t count, uint32_t sync_syms, uint64_t *c_lo, uint64_t *c_hi);
int dc_huff_batch_range_args(uint64_t seg_beg, uint64_t seg_end, uint64_t first, uint64_t count, uint64_t out_off,
                             uint64_t out_cap);
int dc_huff_decode_batch_ranges(dc_ctx *ctx, const dc_hbatch *batch, const uint64_t *d_seg_off,
                                const uint64_t *d_seg, const uint64_t *d_first, const uint64_t *d_count,
                                const uint64_t *d_out_off, uint64_t nranges, uint8_t *d_out, uint64_t out_cap,
                                int32_t *d_rstatus);
int dc_huff_decode_batch_shared_ranges(dc_ctx *ctx, const dc_hbatch *batch, const dc_dtable *d_table,
                                       const uint64_t *d_seg_off, const uint64_t *d_seg, const uint64_t *d_first,
                                       const uint64_t *d_count, const uint64_t *d_out_off, uint64_t nranges,
                                       uint8_t *d_out, uint64_t out_cap, int32_t *d_rstatus);
/* ---- Huffman batch v1, table set: K tables, each segment under its cheapest ---------------------
 * The middle ground between a table per segment and one table for all
 * (n_ary_huffman.c:1210-1255: "remembering the last 2 or so Huffman tables ... emit a reference
 * indicating 'same as #2 table'"; regions of text, upper-case text and base-64 each under a table
 * that fits): a mode of the same dc_hbatch for a batch of mixed content. No format changes.
 * The set: K lens records, 1 <= K <= DC_BATCH_SET_MAX, d_set (u8[256 K], 16-B aligned). Record k
 * is 256 code lengths in digits, exactly a lens record of the own-table batch; its code is that
 * of dc_huff_table_lengths on those lengths with symbols 256..258 at 0. Each segment carries one
 * more byte, d_tid[i] (u8[count]): the record it is coded under. dc_hbatch does not change:
 * d_set, K and d_tid are call arguments; batch->d_lens is neither read nor written, may be NULL.
 * With w = ceil(log2 n_ary):
 *   valid    record k is valid when every length L has L w <= 32 and the lengths satisfy Kraft:
 *            with Lmax the longest, the sum over L_s > 0 of n^(Lmax - L_s) is <= n^Lmax
 *            (dc_huff_batch_set_table_ok, csrc/dc_batch_set.h). 256 zeros are valid and code nothing.
 *   usable   record k is usable for segment i when it is valid and L_k[s] > 0 for every byte
 *            value s the segment holds.
 *   select   for a segment of len > 0 with histogram h, cost_k = sum h[s] L_k[s] w. The segment
 *            takes the usable k of least cost, the lowest k of equal costs: tid[i] = k, or 0
 *            when no record is usable. mode[i] = 1 when a record is usable and cost < 8 len;
 *            else 0 (stored, bits = 8 len). len 0: stored, 0 bits, tid 0. An invalid record is
 *            never chosen and never an error: a set of invalid records stores every segment.
 * Everything else is batch v1's: bits, the payload (a mode-1 payload is bit for bit what
 * dc_huff_encode_batch_shared writes for the segment under dc_huff_table_lengths(record tid[i])),
 * pay_off, sync_len, sync_off, the zero pads, both bound functions, the statuses and their order,
 * "nothing is written for a failed segment or past a cap" (a DC_E_ARG segment writes no tid
 * either), the first-failure slot, DC_OPT_BATCH_GRID, no host read, launches that do not depend
 * on count.
 * Decode: batch v1's tests in its order (output range, cap, the record); then for a mode-1
 * segment DC_E_STREAM when tid[i] >= K or record tid[i] gives no code (a length over
 * DC_MAX_DIGITS or a code over 32 bits: the own-table decoder's rule; Kraft is the encoder's
 * guard alone). A stored segment never reads tid or the set; a bad tid fails its own segment only.
 * As in every mode a chunk must decode to exactly its symbols in exactly its bits, which a wrong
 * but valid record can pass: keep a CRC-32 per segment (dc_crc32_batch) to see that.
 * Host argument rules are the shared mode's with the set in the table's place: DC_E_ARG, nothing
 * launched, for K == 0, K > DC_BATCH_SET_MAX, d_set not 16-B aligned, n_ary outside 2..256, or
 * d_set / d_tid NULL with work to do; count 0 (ranges: nranges 0) returns DC_OK without a launch.
 * dc_huff_batch_status answers for all of these calls.
 * What to store: the K records once (dc_huff_batch_lens_pack takes K records as it takes count),
 * then per segment mode, bits and tid, the payload and the u16 index.
 * Cost. The plan keeps the set (<= 16 KiB) in LDS; pack, decode and ranges give each workgroup a
 * contiguous run of segments or ranges and rebuild a table only when tid differs from the one
 * before, so data made of long regions pays a table build per region, not per segment. The
 * whole-segment decode deals segments four consecutive at a time as the shared mode does: four of
 * at most 8 KiB each whose coded ones name one record go one to a wave, any other group one
 * segment after the other to the workgroup. */
#define DC_BATCH_SET_MAX 64
/* pure host: 1 when the 256 lengths are a valid record at n_ary, else 0 (also for a NULL pointer
 * or n_ary outside 2..256) */
int dc_huff_batch_set_table_ok(const uint8_t *lens256, int n_ary);
/* the plan alone, one launch: d_tid, d_mode, d_bits, d_status exactly as the encode writes them,
 * and nothing else. For training a set, and for sizing a batch before committing to it. */
int dc_huff_batch_set_select(dc_ctx *ctx, const uint8_t *d_in, const uint64_t *d_in_off, uint64_t count, int n_ary,
                             const uint8_t *d_set, uint32_t K, uint8_t *d_tid, uint8_t *d_mode, uint32_t *d_bits,
                             int32_t *d_status);
int dc_huff_encode_batch_set(dc_ctx *ctx, const uint8_t *d_in, const uint64_t *d_in_off, uint64_t count,
                             const uint8_t *d_set, uint32_t K, uint8_t *d_tid, const dc_hbatch *batch);
int dc_huff_decode_batch_set(dc_ctx *ctx, const dc_hbatch *batch, const uint8_t *d_set, uint32_t K,
                             const uint8_t *d_tid, uint8_t *d_out, const uint64_t *d_out_off, uint64_t out_cap);
int dc_huff_decode_batch_set_scatter(dc_ctx *ctx, const dc_hbatch *batch, const uint8_t *d_set, uint32_t K,
                                     const uint8_t *d_tid, uint8_t *d_out, const uint64_t *d_out_beg,
                                     const uint64_t *d_out_end, uint64_t out_cap);
/* byte ranges ("byte ranges of segments" above) of a table-set batch: test 6 is DC_E_STREAM for a
 * mode-1 segment whose tid is >= K or whose record gives no code. A list sorted by tid pays one
 * table build per record and workgroup. */
int dc_huff_decode_batch_set_ranges(dc_ctx *ctx, const dc_hbatch *batch, const uint8_t *d_set, uint32_t K,
                                    const uint8_t *d_tid, const uint64_t *d_seg_off, const uint64_t *d_seg,
                                    const uint64_t *d_first, const uint64_t *d_count, const uint64_t *d_out_off,
                                    uint64_t nranges, uint8_t *d_out, uint64_t out_cap, int32_t *d_rstatus);
/* d_hist (u64[256 K]) is zeroed, then hist[k][s] = the number of bytes s in the segments with
 * valid offsets and d_tid[i] == k; segments with bad offsets or d_tid[i] >= K are skipped. One
 * launch, no host read. DC_E_ARG for K outside 1..DC_BATCH_SET_MAX or a NULL pointer. */
int dc_huff_batch_set_hist(dc_ctx *ctx, const uint8_t *d_in, const uint64_t *d_in_off, uint64_t count,
                           const uint8_t *d_tid, uint32_t K, uint64_t *d_hist);
/* ---- Huffman batch v1: container DCHB ---------------------------------------------------------
 * The form of a batch that can be written to a file and read back (the reference asks for a
 * version number "in the header of the output file / stream", n_ary_huffman.c:211-232, a reader
 * that fails politely on foreign or future files, :1944-1973, and blocks that carry their own
 * decompressed length "so a parallel processor can skip ahead", small_compression.c:924-926). One
 * blob holds everything a decode needs; pay_off, sync_off and the segment offsets are not stored:
 * they are the exclusive scans of round_up_16(ceil(bits / 8)), ceil(len / S) and len, which open
 * derives with the scan kernel the encoder uses. Per segment the blob stores len, bits and mode,
 * 9 bytes (10 with a tid, 13 or 14 with a CRC).
 * Format "DCHB" version 1. Little-endian. Every section starts at a multiple of 16 bytes from
 * the start of the blob; gap bytes are zero. The blob must be 16-B aligned on the device, which
 * gives the payload the alignment the decoders require.
 *   header, 64 bytes:
 *      0  u32 magic "DCHB"             4  u8 version = 1
 *      5  u8 kind: 0 own tables, 256-byte records; 1 own tables, 128-byte nybble records (the
 *         layout of dc_huff_batch_lens_pack); 2 one shared table; 3 table set
 *      6  u8 flags: bit 0 = a CRC-32 per segment is stored; every other bit 0
 *      7  u8 K, records in the record section: 0 for kinds 0 and 1, 1 for kind 2,
 *         1..DC_BATCH_SET_MAX for kind 3
 *      8  u16 n_ary (2..256)          10  u16 sync_syms (a power of two, 16..DC_SYNC_MAX)
 *     12  u32 0                       16  u64 count (at most DC_RANGES_MAX)
 *     24  u64 total_bytes = sum of len
 *     32  u64 sync_total (u16 entries) 40  u64 pay_total (bytes, a multiple of 16)
 *     48  u64 blob_bytes (the whole container)
 *     56  u32 0                       60  u32 CRC-32 (dc_crc32_host) of header bytes 0..59
 *   sections, in this order: len u32[count]; bits u32[count]; mode u8[count]; tid u8[count]
 *   (kind 3 only); crc u32[count] (flag bit 0 only); records: u8[256 count] for kind 0,
 *   u8[128 count] for kind 1, u8[256 K] for kinds 2 and 3; payload u8[pay_total], the batch's
 *   d_payload[0 .. pay_off[count]) verbatim, 16-B pads included; sync u16[sync_total], the batch's
 *   d_sync_len[0 .. sync_off[count]) verbatim.
 *   The offsets of every section up to the payload depend on count, kind, flags and K alone
 *   (dc_huff_batch_blob_layout), so a caller can have the encoder write the payload in place; only
 *   the sync section, at payload_off + pay_total, and blob_bytes depend on device values.
 *   The record of kind 2 holds the shared table's lengths in digits for bytes 0..255.
 * The container rule (csrc/dc_batch_blob.h; what dc_huff_batch_blob_check enforces on the host and
 * dc_huff_batch_blob_info plus dc_huff_batch_open on the device): the header as above, reserved
 * fields zero, the header CRC; len[i] <= DC_BATCH_SEG_MAX; mode[i] <= 1; bits[i] <= 8 len[i] with
 * equality when mode is 0; tid[i] < K for a mode-1 segment of kind 3; the three scans end at
 * total_bytes, pay_total and sync_total; blob_bytes is the sum of the padded sections and at most
 * the m bytes given, with no arithmetic that can wrap. Gap bytes, payload pads, records, payload
 * bytes, sync entries and CRCs are NOT inspected by the rule: the decoders hold records, payload
 * and sync entries to their own tests (DC_E_STREAM per segment), and decode with verify the CRCs.
 * dc_hblob_info: the header's fields, the section offsets (0: the section is absent), and the
 * bytes and offsets of open's workspace. */
typedef struct dc_hblob_info {
    uint32_t version, kind, flags, K;
    int32_t n_ary;
    uint32_t sync_syms;
    uint64_t count, total_bytes, sync_total, pay_total, blob_bytes;
    uint64_t len_off, bits_off, mode_off, tid_off, crc_off, rec_off, rec_bytes, payload_off, sync_off;
    uint64_t work_bytes;
    uint64_t w_items, w_pay_off, w_sync_off, w_seg_off, w_status, w_cstatus, w_lens, w_lengths, w_table;
} dc_hblob_info;
/* Pure host (csrc/dc_batch_blob.h). bound: bytes that always hold a seal, the host sections plus
 * round_up_16(dc_huff_batch_payload_bound) and the padded dc_huff_batch_sync_bound entries; 0 for
 * arguments that are not legal or a bound past 2^64. layout: the host-known fields of *info
 * (count, kind, flags, K, the offsets up to payload_off, the workspace) or DC_E_ARG. info: the
 * header rule on the 64 header bytes of a container of which m bytes exist, then every field of
 * *info; DC_E_STREAM for a header that breaks it. check: the whole container rule on a blob in
 * host memory, DC_OK or DC_E_STREAM. */
uint64_t dc_huff_batch_blob_bound(uint64_t total_bytes, uint64_t count, uint32_t sync_syms, int kind, int flags,
                                  uint32_t K);
int dc_huff_batch_blob_layout(uint64_t count, int kind, int flags, uint32_t K, dc_hblob_info *info);
int dc_huff_batch_blob_info(const uint8_t *header64, uint64_t m, dc_hblob_info *info);
int dc_huff_batch_blob_check(const uint8_t *blob, uint64_t m);
/* Seal an encoded batch into d_blob (blob_cap bytes, 16-B aligned). d_in_off: the encode's.
 * tables: NULL for kinds 0 and 1 (batch->d_lens is read), the dc_dtable for kind 2, the set (16-B
 * aligned) for kind 3; d_tid for kind 3, d_crc (u32[count], dc_crc32_batch) with flag bit 0.
 * Asynchronous, no host read, launches that do not depend on count; count 0 seals a valid
 * 64-byte container. d_info (device u64[2]) receives blob_bytes and the container status:
 *   DC_OK          the container is complete
 *   DC_E_CAPACITY  blob_bytes would pass blob_cap: no byte at or past the cap is written, and no
 *                  header (sections that end below the cap may have been written). When even
 *                  the host-known sections do not fit (payload_off > blob_cap) nothing at all
 *                  is written into the blob, and d_status and the first-failure slot are NOT
 *                  written either: d_info alone answers for such a call
 *   DC_E_ARG       kind 2: the table is of another arity, is no usable table, or has a code for a
 *                  symbol at or above 256; any kind: a segment the encode failed with payload
 *                  bytes or sync entries to its name (DC_E_CAPACITY at encode). No header.
 * d_status[i] (i32): DC_OK; or the encode's status for a segment with batch->d_status[i] != DC_OK,
 * which is sealed as an empty stored segment (len 0, bits 0, mode 0: what the encoder gave it, 0
 * payload bytes and 0 sync entries); or DC_E_CODE_TOO_LONG for a kind 1 record with a length
 * above 15, written as zeros (dc_huff_batch_lens_pack's rule: a mode-1 segment under it decodes
 * to DC_E_STREAM, never to a wrong byte). The lowest failing index goes to the first-failure slot.
 * Kind 0 records are copied as they are, except that the record of a segment the encode failed
 * (kinds 0 and 1) is written as zeros: the encode never wrote it, and a container is a function
 * of what was encoded, not of what the buffer held before. The payload is not copied when batch->d_payload ==
 * d_blob + payload_off (encoded in place); any other overlap of the blob with the batch's arrays,
 * d_in_off, tables, d_tid, d_crc, d_info or d_status is DC_E_ARG from the host. The header is written last, by the device. */
int dc_huff_batch_seal(dc_ctx *ctx, const dc_hbatch *batch, const uint64_t *d_in_off, int kind, int flags,
                       const void *tables, uint32_t K, const uint8_t *d_tid, const uint32_t *d_crc, uint8_t *d_blob,
                       uint64_t blob_cap, uint64_t *d_info, int32_t *d_status);
/* Open a container that lies in device memory (16-B aligned, m bytes). *info: dc_huff_batch_blob_
 * info of its 64 header bytes (the caller has them in host memory, or fetches them with one
 * 64-byte copy); its offsets are checked again here against count, kind, flags, K, the totals and
 * m (DC_E_ARG), so the caps below are section sizes whatever filled it. d_work: work_bytes >=
 * info->work_bytes, 256-B aligned, not overlapping the blob. Asynchronous, no host read,
 * launches that do not depend on count: one pass applies the per-segment rule and writes the
 * items of three scans, three scans, one kernel applies the totals rule; kind 1 unpacks its
 * records into d_work, kind 2 builds its table there (dc_huff_table_lengths).
 * The view: batch (d_mode, d_bits, d_payload, d_sync_len point into the blob, payload_cap =
 * pay_total, sync_cap = sync_total; d_pay_off, d_sync_off, d_status in d_work; d_lens in the blob
 * for kind 0, in d_work for kind 1, NULL otherwise), d_seg_off (count + 1 u64: what the decode
 * calls take as d_out_off and the range calls as d_seg_off), d_cstatus (one i32: DC_OK, or
 * DC_E_STREAM when a scan does not end at its total), and what the decode calls of the kind take:
 * d_tid, d_set and K (kind 3), d_table (kind 2), d_crc (flag bit 0). batch.d_status[i] is DC_OK
 * or DC_E_STREAM for a segment that breaks its rule (the first-failure slot has the lowest);
 * the next decode overwrites it.
 * Safety: a decode of an opened container neither reads nor writes out of bounds whatever open
 * reported, because every decode kernel holds each segment's offsets inside payload_cap and
 * sync_cap and to exact agreement with bits and the asked length before its first access
 * (hb_record_check), and those caps are the host-checked section sizes. The statuses only have
 * to tell the truth. */
typedef struct dc_hblob_view {
    dc_hbatch batch;
    uint64_t *d_seg_off;
    int32_t *d_cstatus;
    const uint8_t *d_tid;
    const uint32_t *d_crc;
    const uint8_t *d_set;
    uint32_t K;
    const dc_dtable *d_table;
    uint64_t total_bytes;
} dc_hblob_view;
int dc_huff_batch_open(dc_ctx *ctx, const uint8_t *d_blob, uint64_t m, const dc_hblob_info *info, void *d_work,
                       uint64_t work_bytes, dc_hblob_view *view);

/* base64url text (6 bits per char, MSB-first) of bits [bit_base, bit_base+bits) */
int dc_huff_base64url(dc_ctx *ctx, const uint32_t *d_words, uint64_t bit_base, uint64_t bits,
                      char *d_text);
/* Digit text of bits [bit_base, bit_base+bits) (n_ary_huffman.c:46-78,
 * :371-455, :745-748): one character per b-bit field, MSB-first, the last zero-padded.
 *   DC_TEXT_BASE64URL  b = 6, the int2digit alphabet (:371-378)
 *   DC_TEXT_BASE16     b = 4, "0123456789ABCDEF" (RFC 4648)
 *   DC_TEXT_DIGITS     b = w, one base-n digit per character, "0123456789abcdef" (n <= 16)
 *   DC_TEXT_Z85        b = 8, 4 trits (n = 3) or 2 base-9 digits (n = 9) -> the first 81
 *                      characters of Z85 (:379-407)
 *   DC_TEXT_TRITS5     b = 10, 5 trits (n = 3) -> one byte 1..243 (:745-748)
 * d_words[0] is the word holding bit bit_base (as dc_huff_pack writes a stream).
 * A field with a digit >= n (never produced by the encoder) renders as '~' (byte 0 in
 * TRITS5). dc_huff_text_bits returns b, 0 for an unsupported (format, n). *nchar (host,
 * may be NULL) receives ceil(bits / b). */
enum { DC_TEXT_BASE64URL = 0, DC_TEXT_BASE16 = 1, DC_TEXT_DIGITS = 2, DC_TEXT_Z85 = 3, DC_TEXT_TRITS5 = 4 };
int dc_huff_text_bits(int format, int n_ary);
int dc_huff_text(dc_ctx *ctx, const uint32_t *d_words, uint64_t bit_base, uint64_t bits, int format, int n_ary,
                 char *d_text, uint64_t *nchar);
/* inverse: nchar characters -> the first `bits` bits at bit 0 of d_words (ceil(bits/32)
 * words; bits past `bits` zeroed). base64url also takes '+' '/' (digit2int :443-446),
 * base16 lowercase. An invalid character: dc_huff_text_parse_status (synchronising)
 * returns DC_E_STREAM. */
int dc_huff_text_parse(dc_ctx *ctx, const char *d_text, uint64_t nchar, int format, int n_ary, uint64_t bits,
                       uint32_t *d_words);
int dc_huff_text_parse_status(dc_ctx *ctx);
/* sync granularity (symbols per chunk): a fixed default, and the choice from the
 * planned payload (keeps a 64-chunk group within the decoder's LDS stage) */
uint32_t dc_huff_default_sync(uint64_t n);
uint32_t dc_huff_choose_sync(uint64_t n, uint64_t total_bits);

/* ---- nybble codec (nybble_compression.c), device-resident ---------------------------- */
/* Full reference byte stream (header, packed nybbles, LITERAL fallback) of d_in[0..n).
 * d_out capacity >= n + 2. *h_out_len receives the length (host, synchronising). */
int dc_nyb_compress(dc_ctx *ctx, const uint8_t *d_in, uint64_t n, int modify, uint8_t *d_out,
                    uint64_t *h_out_len);
/* Decode m compressed bytes; d_out capacity >= 2*m. *h_out_len as above. */
int dc_nyb_decompress(dc_ctx *ctx, const uint8_t *d_in, uint64_t m, int modify, uint8_t *d_out,
                      uint64_t *h_out_len);
/* Chunked container "DCNK" (build-defined; SURVEY §8(e)/(f)4: adaptive streams decode in
 * parallel only with independent chunks). Chunk k = bytes [kK, kK+K) stored as the
 * reference's own stream of that chunk (compress_bytestring on it), so each chunk decodes
 * alone. Layout: u32 'DCNK', u32 version 1, u32 modify, u32 K, u64 n, u64 nchunks,
 * u64 off[nchunks+1] (relative to the payload), payload. K >= 16; d_out / d_in 8-B aligned.
 * Decode returns DC_E_STREAM when a chunk does not decode to exactly its length (a corrupt
 * container, or input bytes >= 0x80, which the reference codec does not round-trip). Input
 * byte 0 is outside the reference's domain (NUL-terminated strings) and not exact here: the
 * one-lane-per-chunk kernels pad their lists with zero bytes (see "nybble batch v1" below). */
uint64_t dc_nyb_chunked_bound(uint64_t n, uint32_t K);
int dc_nyb_compress_chunked(dc_ctx *ctx, const uint8_t *d_in, uint64_t n, int modify, uint32_t K, uint8_t *d_out,
                            uint64_t out_cap, uint64_t *h_out_len);
int dc_nyb_chunked_info(dc_ctx *ctx, const uint8_t *d_in, uint64_t m, uint64_t *h_n, int *h_modify, uint32_t *h_K);
int dc_nyb_decompress_chunked(dc_ctx *ctx, const uint8_t *d_in, uint64_t m, uint8_t *d_out, uint64_t out_cap,
                              uint64_t *h_out_len);
/* Batched decode of many independent reference streams (the throughput path for many
 * separate nybble_decompress / decompress_bytestring calls, beside the DCNK container): stream i
 * = d_in[d_in_off[i] .. d_in_off[i+1]) (device u64 offsets, count+1 entries), each a whole
 * stream as compress_bytestring writes it, decoded as decompress_bytestring(modify) does
 * (nybble_compression.c:734-817; any type byte but 0xAF / ' ' copies the stream). One lane per
 * stream (a single stream's adaptive decode is sequential). d_out_off (device, count+1) receives
 * the output offsets, *h_total the total; DC_E_CAPACITY when it exceeds out_cap (nothing
 * decoded), DC_E_STREAM when a 0xAF stream's walk leaves its bytes inconsistent, DC_E_ARG for an
 * offset range that ends before it starts. Synchronising. */
int dc_nyb_decompress_batch(dc_ctx *ctx, const uint8_t *d_in, const uint64_t *d_in_off, uint64_t count, int modify,
                            uint8_t *d_out, uint64_t out_cap, uint64_t *d_out_off, uint64_t *h_total);
/* ---- byte-stream batch v1: what the nybble and the small batch calls share ---------------------
 * Two codecs, one shape (dc_nyb_* / dc_small_*: "nybble batch v1" and "small batch v1" below say
 * what is their own: format, byte domain, cost, what a failed stream's range holds on decode). The
 * format is nothing but the codec's own streams back to back plus their offsets: no header, no
 * container. All four calls are asynchronous on the context's stream, make no host read, and
 * launch the same kernels for any count and any lengths, so a round trip can be enqueued or
 * captured (the first call at a larger count grows the context's 16 B of scratch per buffer).
 * count 0 returns DC_OK without a launch; count > DC_RANGES_MAX, a NULL context or (with
 * count > 0) any NULL pointer returns DC_E_ARG. A bad buffer never stops the others.
 * d_status[i] (i32, count entries) receives each buffer's outcome, and dc_huff_batch_status
 * (there is no nybble or small twin: the context keeps one first-failure slot for every batch
 * call) reports the lowest failing index of the last such call, synchronising.
 *
 * dc_*_batch_bound = total_bytes + count: a buffer of len >= 1 bytes codes to at most len + 1
 * bytes (the LITERAL form), an empty one to the single byte ' '. Exact, and pure host arithmetic
 * (csrc/dc_nyb_batch_bound.h, csrc/dc_small_batch_bound.h).
 *
 * dc_*_compress_batch: buffer i = d_in[d_in_off[i] .. d_in_off[i+1]) (device u64, count + 1
 * entries; any alignment, any length, 0 too). Stream i is exactly what the codec's single call
 * writes for that buffer alone. The streams lie back to back in d_out: the call writes
 * d_out_off[0] = 0 and d_out_off[i+1] = d_out_off[i] + (length of stream i), count + 1 entries,
 * always the true lengths, so d_out_off[count] is the capacity the batch needs even when out_cap
 * was too small.
 *   DC_E_ARG       the buffer's offsets decrease: it takes 0 output bytes, and nothing of it is
 *                  read or written
 *   DC_E_CAPACITY  d_out_off[i+1] > out_cap: nothing of it is written
 * Nothing is ever written at or past d_out + out_cap, and no byte of d_out that belongs to no
 * good stream is written.
 *
 * dc_nyb_decompress_batch_async / dc_small_decompress_batch: stream i = d_in[d_in_off[i] ..
 * d_in_off[i+1]) is decoded into d_out[d_out_off[i] .. d_out_off[i+1]), where the CALLER gives
 * d_out_off (count + 1 entries): the format stores no length, so the length asked for must be the
 * stream's. One launch.
 *   DC_E_ARG       either offset pair decreases: nothing is read or written
 *   DC_E_CAPACITY  d_out_off[i+1] > out_cap: nothing is written
 *   DC_E_STREAM    the stream does not decode to exactly the asked length
 * No byte outside a stream's own asked range is ever written.
 *
 * The status of entry i, in this order, from its two offset pairs alone (DC_E_STREAM is what the
 * codec finds in an entry that passed): DC_E_ARG when d_in_off[i+1] < d_in_off[i], or, on decode,
 * d_out_off[i+1] < d_out_off[i]; else DC_E_CAPACITY when d_out_off[i+1] > out_cap (on encode also
 * when d_out_off[i+1] < d_out_off[i]: the call's own sum of the lengths wrapped 2^64). So an entry
 * whose input pair decreases is DC_E_ARG even past the point where the capacity ran out. */

/* ---- nybble batch v1: many buffers of their own lengths, one call each way -------------------
 * The streams are the reference's own ("byte-stream batch v1" above has the calls' contract).
 *
 * dc_nyb_compress_batch: stream i is exactly what dc_nyb_compress writes for that buffer alone
 * (type byte 0xAF, the raw first byte, nybbles; ' ' and the raw bytes when the nybble form is not
 * shorter; ' ' alone for length 0), with the static or the adaptive (modify) lists.
 * Byte domain: for buffers of bytes 1..255 the streams are the reference's. Byte 0 is outside the
 * reference's domain (its API takes NUL-terminated strings), and the one-lane-per-stream kernels
 * keep their lists padded with zero bytes, which is not exact for a zero input byte: such input
 * stays inside every bound above and gives the same output on every run, but its streams need not
 * be the reference's nor decode to the input. The DCNK container has the same limit.
 * Cost: a length walk, a scan and an encode straight to the final place (the scratch-slot form of
 * DCNK would need the input total on the host, and slots that stay disjoint beside a decreasing
 * offset pair), so each buffer is walked twice. One lane codes one buffer, 64 buffers a wave, and a
 * wave runs for as long as its longest buffer: batches of very unequal lengths are best sorted by
 * length (tools/nyb_batch_bench.py records the difference). There is no maximum buffer length.
 *
 * dc_nyb_decompress_batch_async: the type dispatch is dc_nyb_decompress_batch's (0xAF nybbles, ' '
 * raw, any other type byte copies the whole stream). The contents of a FAILED stream's own range
 * are unspecified: there is no framing to verify before the walk, and a verify pass (a second walk
 * of every stream) is not worth its cost here. */
uint64_t dc_nyb_batch_bound(uint64_t total_bytes, uint64_t count);
int dc_nyb_compress_batch(dc_ctx *ctx, const uint8_t *d_in, const uint64_t *d_in_off, uint64_t count, int modify,
                          uint8_t *d_out, uint64_t out_cap, uint64_t *d_out_off, int32_t *d_status);
int dc_nyb_decompress_batch_async(dc_ctx *ctx, const uint8_t *d_in, const uint64_t *d_in_off, uint64_t count, int modify,
                                  uint8_t *d_out, const uint64_t *d_out_off, uint64_t out_cap, int32_t *d_status);
/* Shard bodies (data_compression_amd/dist.py ShardedNybble). A shard buffer is
 * d_in[0 .. len): d_in[0] is the context byte (the stream's first byte on the first shard, the
 * previous shard's last byte after it) and the shard's elements are bytes 1 .. len-1, as in
 * compress_bytestring's loop (nybble_compression.c:908-996).
 * Adaptive (modify) move-to-front lists: 16 contexts x 8 bytes, most recent first.
 *   dc_nyb_mtf_summary: the lists after the shard's elements, started empty (h_cnt[c] valid
 *     entries of list c); summaries compose: lists after A then B = first 8 distinct of
 *     (B's list, A's list) per context.
 *   dc_nyb_body_plan: with the shard's entry lists h_lists (adaptive; ignored when static),
 *     h_plan[0..3] = the shard's transducer (bytes out from state 0, from state 1, exit state
 *     from 0, from 1; state 1 = the previous element's hit nybble is pending) and h_plan[4] =
 *     the rank of the shard's last element (0xFF = miss).
 *   dc_nyb_body_write: the shard's body from the entry state (pend_rank = the pending byte's
 *     rank, or -1), the odd-tail byte when is_last; no header and no LITERAL fallback (decided
 *     over the whole stream). The adaptive ranks come from the preceding dc_nyb_body_plan on
 *     the same d_in/len. d_out capacity >= 2*len. *h_state_out = exit state.
 *     A shard of no elements (len = 1) leaves the state as it entered: it writes nothing, but
 *     for the one byte d_in[0] (the byte whose nybble is pending) when is_last and
 *     pend_rank >= 0, the stream's odd tail.
 * Static decode of a shard of the compressed stream after its 2-byte header: m bytes, plus
 * one byte of right halo (the next shard's first byte) when len = m + 1:
 *   dc_nyb_dbody_plan: h_plan[0..3] as above (state 1 = start at the low nybble);
 *   dc_nyb_dbody_write: decoded bytes from entry state s_in; d_out capacity >= 2*m. */
int dc_nyb_mtf_summary(dc_ctx *ctx, const uint8_t *d_in, uint64_t len, uint8_t *h_lists, uint8_t *h_cnt);
int dc_nyb_body_plan(dc_ctx *ctx, const uint8_t *d_in, uint64_t len, int modify, const uint8_t *h_lists,
                     uint64_t *h_plan);
int dc_nyb_body_write(dc_ctx *ctx, const uint8_t *d_in, uint64_t len, int modify, int pend_rank, int is_last,
                      uint8_t *d_out, uint64_t *h_out_len, int *h_state_out);
int dc_nyb_dbody_plan(dc_ctx *ctx, const uint8_t *d_in, uint64_t len, uint64_t m, uint64_t *h_plan);
int dc_nyb_dbody_write(dc_ctx *ctx, const uint8_t *d_in, uint64_t len, uint64_t m, int s_in, uint8_t *d_out,
                       uint64_t *h_out_len, int *h_state_out);

/* ---- small front-end (small_compression.c:507-665), device-resident ----------------- */
int dc_small_compress(dc_ctx *ctx, const uint8_t *d_in, uint64_t n, uint8_t *d_out,
                      uint64_t *h_out_len);
int dc_small_decompress(dc_ctx *ctx, const uint8_t *d_in, uint64_t m, uint8_t *d_out,
                        uint64_t *h_out_len);
/* ---- small batch v1: many buffers of their own lengths, one call each way ---------------------
 * The streams are the front-end's own ("byte-stream batch v1" above has the calls' contract).
 * DC_OPT_BATCH_GRID sizes the grids.
 *
 * dc_small_compress_batch: stream i is exactly what dc_small_compress writes for that buffer
 * alone. With P = the positions i >= 1, i + 1 < len, that hold ' ' before a..z: for P >= 2 the
 * pruned form (the type byte 8, the raw first byte, then every byte as itself but a pair as the
 * one byte 0x80 + letter: len + 1 - P bytes), else the LITERAL form (' ' and the bytes), ' ' alone
 * for length 0. All 256 byte values are in the domain, 0 included.
 * Cost: three launches, a count pass (P -> the stream's length), a scan and a write pass straight
 * to the final place (it knows the form from the length: len + 1 is LITERAL). One WAVE codes one
 * buffer, in tiles of 1 KiB, and takes buffers in a fixed stride: 64 unequal buffers do not wait
 * for the longest one, but a batch of very unequal lengths runs faster sorted by length, which
 * shares the long buffers evenly among the waves (tools/small_batch_bench.py records the
 * difference). A buffer is never split between waves: buffers of many MiB belong in
 * dc_small_compress, which spreads one stream over the device. There is no maximum buffer length.
 *
 * dc_small_decompress_batch: the type dispatch is dc_small_decompress's: type 8 with m >= 2 bytes
 * gives byte 1 raw, then ' ', b - 0x80 for every later byte b >= 0x80 and b itself otherwise; ' '
 * gives the m - 1 bytes after it; an empty stream, a lone type 8 and any other type byte give
 * nothing (length 0).
 * A stream with any status but DC_OK writes NO byte (the decoded length is a count over the
 * stream: the kernel counts first and writes only when it matches), and no byte outside a good
 * stream's own range is ever written. A pruned stream that holds a raw input byte >= 0x80 after
 * position 0 decodes to more bytes than went in (the reference's own limit): asked at its input
 * length it is DC_E_STREAM, never wrong bytes. */
uint64_t dc_small_batch_bound(uint64_t total_bytes, uint64_t count);
int dc_small_compress_batch(dc_ctx *ctx, const uint8_t *d_in, const uint64_t *d_in_off, uint64_t count,
                            uint8_t *d_out, uint64_t out_cap, uint64_t *d_out_off, int32_t *d_status);
int dc_small_decompress_batch(dc_ctx *ctx, const uint8_t *d_in, const uint64_t *d_in_off, uint64_t count,
                              uint8_t *d_out, const uint64_t *d_out_off, uint64_t out_cap, int32_t *d_status);
/* Shard bodies (data_compression_amd/dist.py ShardedSmall): the front-end
 * output of stream bytes d_in[1 .. nelem] (no header, no LITERAL fallback), reading d_in[0]
 * as left context when left_halo (a shard after the first: d_in[0] = the previous shard's
 * last byte; else d_in[0] is the stream's raw first byte) and d_in[nelem + 1] (when
 * nelem + 1 < len) as the right halo. Pairs never overlap, so the bodies of consecutive
 * shards concatenate to the whole stream's body. d_out capacity >= nelem. */
int dc_small_compress_body(dc_ctx *ctx, const uint8_t *d_in, uint64_t len, int left_halo, uint64_t nelem,
                           uint8_t *d_out, uint64_t *h_out_len);
/* The same in two calls, so the caller can place the output once its size is known (a
 * sharded encoder aligns its re-cut segment, dist.ShardedSmall): _plan returns the body
 * length; _write, on the same input and arguments (DC_E_STATE otherwise), writes it. */
int dc_small_compress_body_plan(dc_ctx *ctx, const uint8_t *d_in, uint64_t len, int left_halo, uint64_t nelem,
                                uint64_t *h_len);
int dc_small_compress_body_write(dc_ctx *ctx, const uint8_t *d_in, uint64_t len, int left_halo, uint64_t nelem,
                                 uint8_t *d_out, uint64_t *h_len);
/* decode of a body (every byte: >= 0x80 -> ' ' + byte - 0x80); d_out capacity >= 2*m */
int dc_small_decompress_body(dc_ctx *ctx, const uint8_t *d_in, uint64_t m, uint8_t *d_out, uint64_t *h_out_len);

/* ---- checksums: CRC-32 per buffer on the device, verified after decode ------------------------
 * No batch format here carries a checksum, and no decoder can tell a damaged stored segment, a
 * code swapped for another of its length, a damaged literal byte or a wrong shared table from the
 * real thing. These calls give the caller one more per-buffer array to keep beside mode / bits /
 * the offsets: the CRC-32 of every buffer before it is encoded, checked against the decoded
 * bytes. They change no format and no other call.
 *
 * The algorithm is CRC-32 as zlib, PNG and gzip compute it (reflected polynomial 0xEDB88320, the
 * register started at all ones and inverted at the end), so any host tool can check a stored
 * value. The arithmetic is csrc/dc_crc32.h.
 *
 * dc_crc32_host: the host's running form, as zlib's crc32(): start from crc = 0 and hand each
 * result to the next piece. dc_crc32_combine: crc(A || B) from crc(A), crc(B) and |B|, any |B|.
 * Both are pure host arithmetic.
 *
 * dc_crc32_batch: buffer i = d_in[d_beg[i] .. d_end[i]), two device u64 arrays of count entries
 * that the kernel reads; for the usual offsets array of count + 1 entries pass off and off + 1
 * (the two may alias this way). Buffers may have any byte alignment, any length (0 included: its
 * CRC is 0; there is no maximum), any order, overlaps and gaps (the scatter layouts of
 * dc_huff_decode_batch_scatter). d_crc[i] receives the buffer's CRC-32, d_status[i]
 *   DC_E_ARG       d_end[i] < d_beg[i]
 *   DC_E_CAPACITY  d_end[i] > in_cap
 *   DC_OK          otherwise;
 * in the two failing cases nothing of the buffer is read and d_crc[i] is 0. A bad buffer never
 * stops the others, and nothing past entry count - 1 of either output is written. (Loads are whole
 * aligned 16-B granules: up to 15 bytes beside a buffer, inside d_in's allocation, are read and
 * masked.)
 *
 * dc_crc32_verify_batch: d_status is in-out, so the status array a decode call just wrote can be
 * handed straight on. An entry that is nonzero on entry is skipped: its buffer is not read (a
 * failed nybble stream's range is unspecified) and its status stays. An entry that is DC_OK on
 * entry gets the two tests above and then becomes DC_E_CHECKSUM when the buffer's CRC is not
 * d_expect[i].
 *
 * Both batch calls: asynchronous on the context's stream, no host read, ONE launch whatever the
 * count (a wave per buffer in tiles of DC_CRC_TILE bytes, on a persistent grid that
 * DC_OPT_BATCH_GRID sizes); count 0 returns DC_OK without a launch; DC_E_ARG for a NULL context,
 * a NULL pointer with count > 0, or count > DC_RANGES_MAX. The context's first-failure slot
 * (dc_huff_batch_status) gets the lowest index whose status is nonzero after the call, for verify
 * the carried-over entries included: one dc_huff_batch_status after decode plus verify answers
 * for both. A buffer is never split between waves: long buffers in a batch are correct, and
 * dc_crc32 is the call for one huge buffer.
 *
 * dc_crc32: one buffer of any size and alignment spread over the whole device, e.g. a 1 GiB
 * stream, a DCH1 blob or a whole payload array: a wave per piece of DC_CRC_PIECE bytes writes the
 * piece's CRC times x^(8 * the bytes after the piece) into context scratch (4 B per piece), and a
 * one-workgroup launch xors them into *d_crc (device). Two launches, asynchronous, no host read;
 * n = 0 writes 0 without a launch. */
#define DC_CRC_TILE 1024u        /* bytes a wave takes at a time: 64 lanes x 16 B */
#define DC_CRC_PIECE 131072u     /* dc_crc32: bytes per wave */
uint32_t dc_crc32_host(uint32_t crc, const void *data, size_t n);
uint32_t dc_crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b);
int dc_crc32(dc_ctx *ctx, const uint8_t *d_in, uint64_t n, uint32_t *d_crc);
int dc_crc32_batch(dc_ctx *ctx, const uint8_t *d_in, uint64_t in_cap, const uint64_t *d_beg, const uint64_t *d_end,
                   uint64_t count, uint32_t *d_crc, int32_t *d_status);
int dc_crc32_verify_batch(dc_ctx *ctx, const uint8_t *d_in, uint64_t in_cap, const uint64_t *d_beg,
                          const uint64_t *d_end, uint64_t count, const uint32_t *d_expect, int32_t *d_status);

#ifdef __cplusplus
}
#endif
#endif
