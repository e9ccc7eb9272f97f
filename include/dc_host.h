/*
 * dc_host.h -- host-buffer convenience layer of libdc_core.so.
 *
 * Each call uploads its input to HBM, runs the device-resident stages of dc_gpu.h on a
 * per-thread context (device: $DC_DEVICE, default 0) and copies the result back. Used by
 * the drop-in shims (dc_huffman.h, dc_nybble.h, dc_small.h) and by the parity tests.
 * Host code only moves bytes and assembles headers; no compute falls back to the CPU:
 * without a usable HIP device every call returns DC_E_HIP.
 */
#ifndef DC_HOST_H
#define DC_HOST_H
#include <stdint.h>
#include "dc_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

dc_ctx *dc_host_ctx(void);
/* copy n host bytes into the per-thread 16-B aligned input buffer (device) */
int dc_host_upload(const void *h, uint64_t n, const uint8_t **d_out);
/* per-thread device scratch buffers: which = 0 out, 1 sync, 2 table, 3 hist, 4 lengths, 5 aux */
int dc_host_scratch(int which, uint64_t bytes, void **d_out);

/* ---- "DCH1" Huffman container (DESIGN.md "Container v1") -------------------------------
 * [0]  "DCH1"  [4] u8 version=1, u8 n_ary, u8 w (bits per digit), u8 flags=0
 * [8]  u64 n symbols   [16] u64 payload bits   [24] u32 sync_syms, u32 0
 * [32] u8 code length (digits) of byte 0..255
 * [288] sync index (dc_gpu.h): u64 group bases (dc_huff_sync_groups entries), then
 *       u16 chunk bit lengths (dc_huff_sync_chunks entries)
 * then the MSB-first payload, ceil(bits/8) bytes, zero-padded.
 * lengths == NULL: lengths from the input's own histogram (n_ary_huffman.c:2509-2530 flow),
 * else from lengths[0..max_symbol_value] (the caller's huffman() output).
 * sync_syms == 0: dc_huff_default_sync(n). */
uint64_t dc_huff_compress_bound(uint64_t n, uint32_t sync_syms);
int dc_huff_compress_host(const uint8_t *in, uint64_t n, int n_ary, const int32_t *lengths,
                          int max_symbol_value, uint32_t sync_syms, uint8_t *out, uint64_t cap,
                          uint64_t *out_len);
/* reads either container: "DCH1" by its magic, anything else as netstrings */
int dc_huff_decompress_host(const uint8_t *in, uint64_t m, uint8_t *out, uint64_t cap,
                            uint64_t *out_len);
int dc_huff_container_info(const uint8_t *in, uint64_t m, uint64_t *n, int *n_ary, uint64_t *bits);
/* Is a container that was read from a file safe to decode? Host arithmetic only: no device, no
 * context. DC_OK or DC_E_STREAM. "DCH1": the header rule (version 1, n_ary 2..16, w its digit
 * width, flags 0, a valid sync_syms, every length <= DC_MAX_DIGITS, bits <= 32 n, header + index +
 * payload <= m without wrap) and the index rule (bases[0] == 0, each base + its group's lengths ==
 * the next base, the last == bits, a chunk of k symbols <= 32 k bits), so that every chunk starts
 * inside the payload. Anything else is read as netstrings: block syntax and types, each segment's
 * metadata against its text, the output size without wrap (its index is text that only the device
 * parses: dc_huff_decompress_netstring applies the index rule itself). Both decompress calls and
 * the range read run these checks before their first device call (the range read on the groups it
 * uploads). */
int dc_huff_container_check(const uint8_t *in, uint64_t m);
/* Range reads by the sync index.
 * dc_huff_range_span: pure host arithmetic (no device): the part of a stream that symbols
 * [first, first+count) need. out[0] = first group g0, out[1] = last group g1, out[2] = first
 * payload bit (h_sync_base[g0]), out[3] = end payload bit (h_sync_base[g1+1], or end_bit, the
 * stream's bit_base + payload bits, for the last group). h_sync_base: the stream's group bases
 * in host memory. first + count > n or an invalid sync_syms: DC_E_ARG. The stream from group g0
 * on is itself a stream of dc_gpu.h: bit_base = out[2], the index pointers advanced to group g0
 * and chunk 64 g0, n - g0 * 64 * sync_syms symbols.
 * dc_huff_decompress_range_host: symbols [first, first+count) of a DCH1 container in host
 * memory. Uploads only the code lengths, the index entries of groups g0..g1 and their payload
 * bytes, and decodes with dc_huff_decode_range. first + count past the container's n: DC_E_ARG;
 * count > cap: DC_E_CAPACITY. A netstring container returns DC_E_ARG: its index is base64url
 * text spread over blocks, so it has no random access (decompress it whole). */
int dc_huff_range_span(uint64_t n, uint32_t sync_syms, const uint64_t *h_sync_base, uint64_t end_bit,
                       uint64_t first, uint64_t count, uint64_t out[4]);
int dc_huff_decompress_range_host(const uint8_t *in, uint64_t m, uint64_t first, uint64_t count,
                                  uint8_t *out, uint64_t cap, uint64_t *out_len);

/* ---- netstring container: the reference's block format (n_ary_huffman.c:1866-1943) -----
 * A sequence of netstrings "<len>:<payload>," (payload <= 32768 bytes, :1826-1827) whose
 * payload starts with a 2-byte type (:1915-1920). Written:
 *   raw    "<k+2>:\n\n<k bytes>,"   the reference compress()'s pass-through block
 *                                   (:1806-1814), byte-identical for inputs < 32767 B;
 *                                   longer inputs: consecutive blocks of <= 32766 bytes
 *   #dc1   "\n#dc1 n=<n_ary> syms=<N> bits=<payload bits> S=<sync_syms> M=<max symbol>"
 *   X      "\nX<M>:" + one character per symbol 0..M, its code length in digits
 *          ("0".."9" as the reference's "%d" (:1736-1741), then "A".."Z" for 10..35)
 *   #dcidx "\n#dcidx:" + base64url (int2digit alphabet) of the sync index bytes (dc_gpu.h:
 *          u64 group bases then u16 chunk bit lengths, little-endian), split over blocks
 *   Z      "\nZ" + base64url of the bitstream v1 (6 bits per character, MSB-first, the
 *          last character zero-padded), split over consecutive Z blocks
 * The Huffman form is written only when it is smaller than the raw form (which bounds the
 * output: dc_huff_netstring_bound). A reader skips unknown "#" blocks (:2077-2080), so the
 * reference's decompress() sees the index blocks as metadata. Decompression accepts any
 * sequence of raw blocks and Huffman segments (#dc1, X, #dcidx..., Z...), whitespace between
 * blocks, and "%i" lengths (:1825); the output is the concatenation of the segments. */
uint64_t dc_huff_netstring_bound(uint64_t n);
int dc_huff_compress_netstring(const uint8_t *in, uint64_t n, int n_ary, const int32_t *lengths,
                               int max_symbol_value, uint32_t sync_syms, uint8_t *out, uint64_t cap,
                               uint64_t *out_len);
int dc_huff_decompress_netstring(const uint8_t *in, uint64_t m, uint8_t *out, uint64_t cap,
                                 uint64_t *out_len);
/* decompressed size of a netstring container (walks the block headers on the host) */
int dc_huff_netstring_info(const uint8_t *in, uint64_t m, uint64_t *out_n);

/* ---- nybble / small byte codecs on explicit-length host buffers -------------------------- */
int dc_nyb_compress_host(const uint8_t *in, uint64_t n, int modify, uint8_t *out, uint64_t cap,
                         uint64_t *len);
int dc_nyb_decompress_host(const uint8_t *in, uint64_t m, int modify, uint8_t *out,
                           uint64_t cap, uint64_t *len);
int dc_small_compress_host(const uint8_t *in, uint64_t n, uint8_t *out, uint64_t cap,
                           uint64_t *len);
int dc_small_decompress_host(const uint8_t *in, uint64_t m, uint8_t *out, uint64_t cap,
                             uint64_t *len);

/* ---- many small host buffers <-> one "DCHB" container (dc_gpu.h "container DCHB") ----------
 * compress: buffer i is in[h_off[i] .. h_off[i + 1]) (count + 1 offsets that do not decrease,
 * each buffer at most DC_BATCH_SEG_MAX bytes). The input is uploaded, encoded with the payload
 * in place, sealed, and blob_bytes are copied back to out (cap bytes; dc_huff_batch_blob_bound
 * always holds them); *out_len = blob_bytes. kind and flags are the header's (flag bit 0: a
 * CRC-32 per buffer is computed and stored). max_digits: kinds 0 and 1 cap every buffer's own
 * table (0: no cap; kind 1 stores nybble records, so give at most 15); with lengths_or_set ==
 * NULL it also caps the table built here. lengths_or_set: kind 2, the 256 code lengths in digits
 * of the shared table; kind 3, K records of 256 lengths; NULL for kinds 2 and 3 builds the shared
 * table from the whole input (kind 3: a set of that one record, K is ignored); ignored for kinds
 * 0 and 1. Returns DC_E_ARG for arguments the format does not take, DC_E_CAPACITY when cap is
 * too small, and otherwise the status of the first buffer that failed (DC_E_ARG for one that is
 * too long, DC_E_CODE_TOO_LONG for a kind 1 record deeper than 15): nothing is written then.
 * decompress: dc_huff_batch_blob_check runs before the first device call (DC_E_STREAM); then the
 * blob is uploaded, opened and decoded, stored CRCs are verified, and the first failing status
 * is returned (DC_E_STREAM, DC_E_CHECKSUM), nothing copied. out receives total_bytes bytes
 * (DC_E_CAPACITY when cap is smaller), h_off_out (may be NULL) the count + 1 offsets of the
 * buffers in out, *count their number: dc_huff_batch_blob_info sizes both beforehand. */
int dc_huff_batch_compress_host(const uint8_t *in, const uint64_t *h_off, uint64_t count, int n_ary,
                                uint32_t sync_syms, int kind, int flags, int max_digits,
                                const uint8_t *lengths_or_set, uint32_t K, uint8_t *out, uint64_t cap,
                                uint64_t *out_len);
int dc_huff_batch_decompress_host(const uint8_t *blob, uint64_t m, uint8_t *out, uint64_t cap,
                                  uint64_t *h_off_out, uint64_t *count);

#ifdef __cplusplus
}
#endif
#endif
