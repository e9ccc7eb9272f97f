// dc_batch_blob_kernels.inc -- the "DCHB" container of a Huffman batch (dc_huff_batch_seal /
// dc_huff_batch_open, dc_gpu.h "Huffman batch v1: container DCHB"); included by dc_core.hip after
// the batch and checksum kernels (hb_fail, HB_THREADS, hbl_pack4, ld_nt / st_nt). The rule of the
// format is dc_batch_blob.h; the kernels here move bytes and apply it. Every launch has a grid
// that does not depend on count, and nothing here is read by the host.
// Seal:
//   k_hbb_dir       a lane per segment: len (from in_off), bits, mode, tid, crc and the seal's
//                   status; a segment the encode failed is sealed empty (len 0, bits 0, mode 0) under
//                   the encode's status; the lens sum goes to *total (a wave reduce, one atomic a wave)
//   k_hbb_lens      the records of kinds 0 and 1 in k_hb_lens_pack's lane mapping: copied, or packed
//                   to nybbles (a record that does not pack is zeros with DC_E_CODE_TOO_LONG); zeros
//                   for a segment the encode failed, whose record it never wrote
//   k_hbb_table_rec kind 2's record: the table's lengths of bytes 0..255, read on the device
//   k_hbb_move      16 B a lane, grid-stride, the ragged tail byte by byte: a section whose length the
//                   host knows (kind 3's set), the payload (pay_off[count] bytes) or the sync
//                   index (sync_off[count] entries, to payload_off + pay_off[count]); the two whose
//                   length is the device's write nothing when the container would pass blob_cap
//   k_hbb_header    last, one wave: the gap bytes zeroed, then the header with its totals and CRC,
//                   and d_info
// Open:
//   k_hbb_open_seg  a lane per segment: the per-segment rule, and the three items of the scans
//   k_scan_u64      three times: seg_off, pay_off, sync_off
//   k_hbb_open_end  the totals rule into the container status word
//   k_hbb_widen     kind 2: the record as i32[259] for dc_huff_table_lengths

#define HBB_GAPS 6   /* sections that may end in a gap: len, bits, mode, tid, crc, sync */

struct HbbSeal {
    uint8_t *blob;
    uint64_t blob_cap;
    dc_bb_info I;            // the host-known part: count, kind, flags, K, the offsets of sections 1 to 7
    uint32_t n_ary, S;
    const uint64_t *pay_off, *sync_off;   // the batch's: [count] are the two totals
    uint64_t pay_cap, sync_cap;           // the batch's caps: a total past one was never written
    uint64_t *info;          // d_info: blob_bytes, the container status
    unsigned long long *total;   // the sum of the sealed lens
    int dir;                 // the directory fits under blob_cap and was written
};

// the container's end as the device knows it; false: the sums do not fit, or pass cap
static __device__ __forceinline__ bool hbb_fits(uint64_t payload_off, uint64_t pay_total, uint64_t sync_total, uint64_t cap,
                                                uint64_t *sync_at, uint64_t *blob_bytes)
{
    if (dc_bb_tail(payload_off, pay_total, sync_total, sync_at, blob_bytes)) {
        *blob_bytes = ~0ull;
        return false;
    }
    return *blob_bytes <= cap;
}

__global__ __launch_bounds__(HB_THREADS) void k_hbb_dir(HbbSeal Z, const uint64_t *__restrict__ in_off,
                                                        const uint8_t *__restrict__ mode, const uint32_t *__restrict__ bits,
                                                        const int32_t *__restrict__ enc_status, const uint8_t *__restrict__ tid,
                                                        const uint32_t *__restrict__ crc, int32_t *__restrict__ status,
                                                        unsigned long long *__restrict__ first)
{
    const uint64_t count = Z.I.count, stride = (uint64_t)gridDim.x * HB_THREADS;
    uint32_t *const o_len = reinterpret_cast<uint32_t *>(Z.blob + Z.I.len_off);
    uint32_t *const o_bits = reinterpret_cast<uint32_t *>(Z.blob + Z.I.bits_off);
    uint8_t *const o_mode = Z.blob + Z.I.mode_off, *const o_tid = Z.blob + Z.I.tid_off;
    uint32_t *const o_crc = reinterpret_cast<uint32_t *>(Z.blob + Z.I.crc_off);
    uint64_t sum = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * HB_THREADS + threadIdx.x; i < count; i += stride) {
        const int st = enc_status[i];
        uint32_t len = 0, sb = 0, md = 0, td = 0, cr = 0;
        if (st == DC_OK) {
            len = (uint32_t)(in_off[i + 1] - in_off[i]);   // (<= DC_BATCH_SEG_MAX by the encode's plan)
            sb = bits[i];
            md = mode[i];
            if (Z.I.tid_off) td = tid[i];
            if (Z.I.crc_off) cr = crc[i];
            status[i] = DC_OK;
        } else {
            // the encode gave it no payload byte and no sync entry (DC_E_ARG); one that has some
            // (DC_E_CAPACITY) cannot be sealed as empty: the scans would not end at the totals
            if (Z.pay_off[i + 1] != Z.pay_off[i] || Z.sync_off[i + 1] != Z.sync_off[i]) Z.info[1] = (uint64_t)(int64_t)DC_E_ARG;
            hb_fail(status, first, i, st);
        }
        o_len[i] = len;
        o_bits[i] = sb;
        o_mode[i] = (uint8_t)md;
        if (Z.I.tid_off) o_tid[i] = (uint8_t)td;
        if (Z.I.crc_off) o_crc[i] = cr;
        sum += len;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) sum += __shfl_xor(sum, d, 64);
    if ((threadIdx.x & 63) == 0 && sum) atomicAdd(Z.total, (unsigned long long)sum);
}

// after k_hbb_dir (status[i] is the directory's): 16 lanes a record as k_hb_lens_pack. The record
// of a segment the encode failed is zeros: the encode never wrote it.
template <bool NYB>
__global__ __launch_bounds__(HB_THREADS) void k_hbb_lens(const uint8_t *__restrict__ lens, uint64_t count,
                                                         const int32_t *__restrict__ enc_status, uint8_t *__restrict__ out,
                                                         int32_t *__restrict__ status, unsigned long long *__restrict__ first)
{
    const uint32_t t = threadIdx.x, part = t % HBL_LANES;
    const uint64_t steps = (count + HBL_RECS - 1) / HBL_RECS;
    const bool wide = ((uintptr_t)lens & 15u) == 0;   // (uniform)
    for (uint64_t g = blockIdx.x; g < steps; g += gridDim.x) {   // (workgroup-uniform: every lane meets the ballot)
        const uint64_t i = g * HBL_RECS + t / HBL_LANES;
        const bool in = i < count;
        uint4 q = make_uint4(0u, 0u, 0u, 0u);
        if (in && enc_status[i] == DC_OK) {
            if (wide) {
                q = reinterpret_cast<const uint4 *>(lens)[i * HBL_LANES + part];
            } else {
                uint32_t d[4];
                const uint8_t *const p = lens + 256 * i + 16 * part;
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    d[j] = (uint32_t)p[4 * j] | ((uint32_t)p[4 * j + 1] << 8) | ((uint32_t)p[4 * j + 2] << 16) |
                           ((uint32_t)p[4 * j + 3] << 24);
                q = make_uint4(d[0], d[1], d[2], d[3]);
            }
        }
        if (!NYB) {
            if (in) reinterpret_cast<uint4 *>(out)[i * HBL_LANES + part] = q;
            continue;
        }
        const uint64_t over = __ballot(((q.x | q.y | q.z | q.w) & 0xF0F0F0F0u) != 0u);
        const bool bad = ((over >> (t & 48u)) & 0xFFFFull) != 0;   // the record's 16 lanes
        if (!in) continue;
        const uint2 o = bad ? make_uint2(0u, 0u)
                            : make_uint2(hbl_pack4(q.x) | (hbl_pack4(q.y) << 16), hbl_pack4(q.z) | (hbl_pack4(q.w) << 16));
        reinterpret_cast<uint2 *>(out)[i * HBL_LANES + part] = o;
        if (part == 0 && bad) hb_fail(status, first, i, DC_E_CODE_TOO_LONG);   // (an encode-failed record is zeros: never bad)
    }
}

// one workgroup of 256: byte s's length in digits; a table of another arity, of a status that is
// no table, or with a code for a symbol at or above 256 cannot be sealed
__global__ __launch_bounds__(HB_THREADS) void k_hbb_table_rec(const dc_dtable *__restrict__ tab, int nary,
                                                              uint8_t *__restrict__ rec, uint64_t *__restrict__ info)
{
    const int t = threadIdx.x;
    const int M = tab->max_symbol_value;
    bool bad = tab->n_ary != nary || M < 0 || M >= DC_MAX_SYMS || (tab->status != DC_OK && tab->status != DC_E_CODE_TOO_LONG);
    int L = 0;
    if (!bad) {
        if (t <= M) L = tab->lengths[t];
        bad = L < 0 || L > 255;
        for (int s = 256 + t; s <= M; s += HB_THREADS) bad |= tab->lengths[s] != 0;
    }
    rec[t] = bad ? (uint8_t)0 : (uint8_t)L;
    if (bad) info[1] = (uint64_t)(int64_t)DC_E_ARG;
}

// WHAT 0: `fixed` bytes src -> blob + dst_off. WHAT 1: the payload, pay_off[count] bytes -> blob +
// payload_off. WHAT 2: the sync index, 2 sync_off[count] bytes -> blob + payload_off +
// pay_off[count]. 1 and 2 return before their first store when the container passes blob_cap.
template <int WHAT>
__global__ __launch_bounds__(256) void k_hbb_move(HbbSeal Z, const uint8_t *__restrict__ src, uint64_t dst_off, uint64_t fixed)
{
    uint64_t bytes = fixed;
    if (WHAT != 0) {
        uint64_t sync_at, bb;
        const uint64_t pt = Z.pay_off[Z.I.count], st = Z.sync_off[Z.I.count];
        if (!Z.dir || pt > Z.pay_cap || st > Z.sync_cap || !hbb_fits(Z.I.payload_off, pt, st, Z.blob_cap, &sync_at, &bb))
            return;   // (uniform)
        dst_off = WHAT == 1 ? Z.I.payload_off : sync_at;
        bytes = WHAT == 1 ? pt : 2 * st;
    }
    uint8_t *const dst = Z.blob + dst_off;   // (16-B aligned: the blob is, and every section starts at a multiple of 16)
    const uint64_t stride = (uint64_t)gridDim.x * 256, g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    uint64_t n16 = ((uintptr_t)src & 15u) == 0 ? bytes / 16 : 0;   // (uniform; a source off 16 goes byte by byte)
    for (uint64_t i = g; i < n16; i += stride)
        st_nt(reinterpret_cast<uint4 *>(dst) + i, ld_nt(reinterpret_cast<const uint4 *>(src) + i));
    for (uint64_t k = 16 * n16 + g; k < bytes; k += stride) dst[k] = src[k];
}

// one wave, after every other kernel of the seal
__global__ __launch_bounds__(64) void k_hbb_header(HbbSeal Z)
{
    const uint32_t t = threadIdx.x;
    const uint64_t n = Z.I.count, pt = n ? Z.pay_off[n] : 0, st = n ? Z.sync_off[n] : 0;
    uint64_t sync_at = 0, bb = 0;
    const bool fits = hbb_fits(Z.I.payload_off, pt, st, Z.blob_cap, &sync_at, &bb);
    int64_t held = (int64_t)Z.info[1];   // DC_E_ARG of the directory or the record kernel
    if (pt > Z.pay_cap || st > Z.sync_cap) held = DC_E_ARG;   // (an encode that ran out of room: k_hbb_dir saw its segments too)
    if (!Z.dir || !fits || held != 0) {
        if (t == 0) {
            Z.info[0] = bb;
            Z.info[1] = (uint64_t)(held != 0 ? held : (int64_t)DC_E_CAPACITY);
        }
        return;
    }
    // the gaps: section k ends at e[k] and is padded with zeros to the next multiple of 16
    // (an absent section: 0, which has no gap; the records and the payload are multiples of 16)
    const uint64_t e[HBB_GAPS] = {Z.I.len_off + 4 * n, Z.I.bits_off + 4 * n, Z.I.mode_off + n,
                                  Z.I.tid_off ? Z.I.tid_off + n : 0, Z.I.crc_off ? Z.I.crc_off + 4 * n : 0,
                                  sync_at + 2 * st};
    if (t < 16) {
#pragma unroll
        for (int k = 0; k < HBB_GAPS; ++k)
            if (e[k] + t < ((e[k] + 15u) & ~15ull)) Z.blob[e[k] + t] = 0;
    }
    if (t == 0) {
        uint8_t h[DC_BB_HEADER];
        dc_bb_header_write(h, Z.I.kind, Z.I.flags, Z.I.K, Z.n_ary, Z.S, n, (uint64_t)*Z.total, st, pt, bb);
        for (uint32_t k = 0; k < DC_BB_HEADER / 4; ++k) reinterpret_cast<uint32_t *>(Z.blob)[k] = dc_bb_get32(h + 4 * k);
        Z.info[0] = bb;
        Z.info[1] = 0;
    }
}

// ---- open -------------------------------------------------------------------------------------
__global__ __launch_bounds__(HB_THREADS) void k_hbb_open_seg(const uint8_t *__restrict__ blob, dc_bb_info I,
                                                             uint64_t *__restrict__ items, int32_t *__restrict__ status,
                                                             unsigned long long *__restrict__ first)
{
    const uint64_t n = I.count, stride = (uint64_t)gridDim.x * HB_THREADS;
    const uint32_t *const len = reinterpret_cast<const uint32_t *>(blob + I.len_off);
    const uint32_t *const bits = reinterpret_cast<const uint32_t *>(blob + I.bits_off);
    for (uint64_t i = (uint64_t)blockIdx.x * HB_THREADS + threadIdx.x; i < n; i += stride) {
        const uint32_t l = len[i], b = bits[i];
        const uint32_t td = I.tid_off ? blob[I.tid_off + i] : 0u;
        items[i] = l;
        items[n + i] = dc_bb_pay_item(b);
        items[2 * n + i] = dc_bb_sync_item(l, I.sync_syms);
        if (dc_bb_seg(l, b, blob[I.mode_off + i], td, I.kind, I.K)) hb_fail(status, first, i, DC_E_STREAM);
        else status[i] = DC_OK;
    }
}

__global__ void k_hbb_open_end(dc_bb_info I, const uint64_t *__restrict__ seg_off, const uint64_t *__restrict__ pay_off,
                               const uint64_t *__restrict__ sync_off, int32_t *__restrict__ cstatus)
{
    if (threadIdx.x == 0 && blockIdx.x == 0)
        *cstatus = dc_bb_totals(seg_off[I.count], pay_off[I.count], sync_off[I.count], &I) ? DC_E_STREAM : DC_OK;
}

__global__ __launch_bounds__(HB_THREADS) void k_hbb_widen(const uint8_t *__restrict__ rec, int32_t *__restrict__ lengths)
{
    const int t = threadIdx.x;
    lengths[t] = rec[t];
    if (t < 3) lengths[256 + t] = 0;
}
