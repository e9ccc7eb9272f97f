// dc_batch_shared_kernels.inc -- the shared-table mode of the batched Huffman codec
// (dc_huff_encode_batch_shared / dc_huff_decode_batch_shared, dc_gpu.h "Huffman batch v1, shared
// table"); included by dc_core.hip after dc_batch_kernels.inc. One dc_dtable codes every segment,
// so no work of a segment is proportional to the table: a persistent workgroup copies what it
// needs of the table into LDS once, before its segment loop. Only what is particular to this
// mode is here: what a segment takes once the table is in LDS (hb_pack_seg, hb_decode_check,
// hb_decode_body, hb_decode_slow) is in dc_batch_kernels.inc, the same code as the own-table mode
// and as the byte ranges of either (dc_batch_range_kernels.inc, which calls hbs_tables_load).
//   k_hbs_plan    nbits[256] in LDS; per segment the sum of nb[byte] and whether a byte has no
//                 code (no histogram, no table build): mode, bits, and the payload bytes and
//                 sync entries for the scans
//   k_scan_u64    twice: pay_off and sync_off
//   k_hbs_pack    code / nbits in LDS; per segment hb_pack_seg: the unit scan, LDS stage and
//                 16-B stores
//   k_hbs_decode  once per workgroup the 12-bit first-level table, filled by code ranges from
//                 code / nbits (the packed codes are prefix-free bit strings at any arity), and
//                 the table's canonical arrays for the longer codes; per segment hb_decode_check
//                 and hb_decode_body: the chunk scan, exactness check and phased output stage.
//                 Segments are dealt four at a time: four short ones (<= 8 KiB) to the four
//                 waves, one each, on a quarter of the stage; otherwise one after the other to
//                 the workgroup
// The table is read, never written; dec_ready and the dlut* arrays are not touched, so one table
// serves any number of contexts and streams at once. A table of another arity, or one whose
// status is neither DC_OK nor DC_E_CODE_TOO_LONG, gives every segment DC_E_ARG.

// (workgroup-uniform)
static __device__ __forceinline__ bool hbs_table_ok(const dc_dtable *__restrict__ T, int nary)
{
    const int st = T->status;
    return T->n_ary == nary && (st == DC_OK || st == DC_E_CODE_TOO_LONG);
}

// a byte's bit length as the kernels use it: 0 (no code) for anything the table kernel does not write
static __device__ __forceinline__ uint32_t hbs_nb(uint32_t nbits) { return nbits <= 32u ? nbits : 0u; }

// ---- plan ---------------------------------------------------------------------------------
struct HbsPlanLds {
    uint8_t nb[256];
    uint32_t red[2][4];   // per wave: the bits of its bytes, bit 31: one of them has no code
};

__global__ __launch_bounds__(HB_THREADS) void k_hbs_plan(const uint8_t *__restrict__ in, const uint64_t *__restrict__ in_off,
                                                         uint64_t count, int nary, uint32_t S,
                                                         const dc_dtable *__restrict__ T, uint8_t *__restrict__ mode,
                                                         uint32_t *__restrict__ bits, uint64_t *__restrict__ psize,
                                                         uint64_t *__restrict__ nchunks, int32_t *__restrict__ status,
                                                         unsigned long long *__restrict__ first)
{
    __shared__ HbsPlanLds L;
    const int t = threadIdx.x;
    const uint32_t slog = (uint32_t)__builtin_ctz(S);
    const bool tok = hbs_table_ok(T, nary);
    L.nb[t] = (uint8_t)hbs_nb(T->nbits[t]);
    __syncthreads();
    uint32_t par = 0;   // red[par]: two segments in a row never share a row, so one barrier a segment
    for (uint64_t i = blockIdx.x; i < count; i += gridDim.x) {
        const uint64_t a = in_off[i], b = in_off[i + 1];
        if (!tok || b < a || b - a > DC_BATCH_SEG_MAX) {   // (workgroup-uniform)
            if (t == 0) { psize[i] = 0; nchunks[i] = 0; hb_fail(status, first, i, DC_E_ARG); }
            continue;
        }
        const uint32_t len = (uint32_t)(b - a);
        if (len == 0) {   // stored, 0 bytes
            if (t == 0) { status[i] = DC_OK; mode[i] = 0; bits[i] = 0; psize[i] = 0; nchunks[i] = 0; }
            continue;
        }
        const uint8_t *p = in + a;
        const uint32_t units = (len + HB_UNIT - 1) / HB_UNIT;
        uint32_t sum = 0, miss = 0;
        for (uint32_t u = t; u < units; u += HB_THREADS) {
            uint32_t q[4];
            hb_load16(p, u * HB_UNIT, len, q);
            const uint32_t cntu = min((uint32_t)HB_UNIT, len - u * HB_UNIT);
#pragma unroll
            for (uint32_t k = 0; k < HB_UNIT; ++k) {
                if (k < cntu) {
                    const uint32_t nb = L.nb[(q[k >> 2] >> (8 * (k & 3))) & 255u];
                    sum += nb;
                    miss |= (uint32_t)(nb == 0u);
                }
            }
        }
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {   // <= 65536 * 32 in the whole workgroup
            sum += __shfl_xor(sum, d, 64);
            miss |= __shfl_xor(miss, d, 64);
        }
        if ((t & 63) == 0) L.red[par][t >> 6] = sum | (miss << 31);
        __syncthreads();
        if (t == 0) {
            const uint32_t r0 = L.red[par][0], r1 = L.red[par][1], r2 = L.red[par][2], r3 = L.red[par][3];
            const uint32_t cb = (r0 & 0x7fffffffu) + (r1 & 0x7fffffffu) + (r2 & 0x7fffffffu) + (r3 & 0x7fffffffu);
            const bool huff = ((r0 | r1 | r2 | r3) >> 31) == 0 && cb < 8u * len;
            const uint32_t sb = huff ? cb : 8u * len;
            status[i] = DC_OK;
            mode[i] = huff ? 1 : 0;
            bits[i] = sb;
            psize[i] = hb_pad16((sb + 7u) >> 3);
            nchunks[i] = (len + S - 1) >> slog;
        }
        par ^= 1u;
    }
}

// ---- pack -------------------------------------------------------------------------------------
struct HbsPackLds {
    HbPackWork P;
    uint32_t code[256];   // the table's, read once
    uint32_t nb[256];
};

__global__ __launch_bounds__(HB_THREADS) void k_hbs_pack(const uint8_t *__restrict__ in, const uint64_t *__restrict__ in_off,
                                                         uint64_t count, uint32_t S, const dc_dtable *__restrict__ T,
                                                         const uint8_t *__restrict__ mode,
                                                         const uint64_t *__restrict__ pay_off, uint8_t *__restrict__ payload,
                                                         uint64_t payload_cap, const uint64_t *__restrict__ sync_off,
                                                         uint16_t *__restrict__ sync_len, uint64_t sync_cap,
                                                         int32_t *__restrict__ status, unsigned long long *__restrict__ first)
{
    __shared__ HbsPackLds L;
    const int t = threadIdx.x;
    {
        const uint32_t nb = hbs_nb(T->nbits[t]);
        L.nb[t] = nb;
        L.code[t] = nb ? T->code[t] : 0u;
    }
    for (uint64_t i = blockIdx.x; i < count; i += gridDim.x) {
        __syncthreads();   // the LDS of the segment before (the first time: the table's copy)
        if (status[i] != DC_OK) continue;   // (DC_E_ARG by the plan; uniform)
        hb_pack_seg(L.P, L.code, L.nb, i, in, in_off, S, mode, pay_off, payload, payload_cap, sync_off, sync_len, sync_cap,
                    status, first);
    }
}

// ---- decode -----------------------------------------------------------------------------------
// the table's canonical arrays (first / count / start / syms), for codes over 12 bits
struct HbsCanon {
    uint32_t cnt[DC_MAX_DIGITS + 1], startv[DC_MAX_DIGITS + 1], starti[DC_MAX_DIGITS + 1];
    uint16_t syms[DC_MAX_SYMS];   // up to 1024 symbols: one >= 256 is never a byte
    int mn, mx;
};

struct HbsDecLds {   // (the members hb_decode_body uses, as HbDecLds)
    __attribute__((aligned(16))) uint8_t out[HB_STAGE_BYTES];
    uint16_t lut[1 << HB_LUT_BITS];   // next 12 bits -> sym | bits << 8; 0: longer, or no code
    HbsCanon C;
    uint32_t scan[4];
    int bad;
};

// The decode tables of *T in L (lut and C), by the whole workgroup (t: threadIdx.x, its lane and
// wave), once for every segment or range it takes: k_hbs_decode and k_hbs_decode_ranges
// (dc_batch_range_kernels.inc). The caller's next barrier ends the fill.
static __device__ __forceinline__ void hbs_tables_load(HbsDecLds &L, const dc_dtable *__restrict__ T, int t, uint32_t lane,
                                                       uint32_t wave)
{
    for (uint32_t e = t; e < (1u << HB_LUT_BITS); e += HB_THREADS) L.lut[e] = 0;
    for (int q = t; q <= DC_MAX_DIGITS; q += HB_THREADS) {
        L.C.cnt[q] = T->count[q];
        L.C.startv[q] = T->first[q];
        L.C.starti[q] = T->start[q];
    }
    for (int q = t; q < DC_MAX_SYMS; q += HB_THREADS) L.C.syms[q] = T->syms[q];
    if (t == 0) {
        L.C.mn = max(T->min_len, 1);
        L.C.mx = min(T->max_len, DC_MAX_DIGITS);
    }
    const uint32_t nbt = hbs_nb(T->nbits[t]), codet = T->code[t];
    __syncthreads();
    // byte s of a code of nb <= 12 bits owns the windows [code << (12 - nb), (code + 1) << (12 - nb)):
    // wave v takes bytes 64 v .. 64 v + 63 in turn, its lanes a range's entries
    for (int j = 0; j < 64; ++j) {
        const uint32_t nb = (uint32_t)__shfl((int)nbt, j, 64), code = (uint32_t)__shfl((int)codet, j, 64);
        if (nb == 0 || nb > HB_LUT_BITS) continue;   // (wave-uniform)
        const uint32_t lo = code << (HB_LUT_BITS - nb), span = 1u << (HB_LUT_BITS - nb);
        const uint32_t ent = (64u * wave + (uint32_t)j) | (nb << 8);
        for (uint32_t e = lane; e < span; e += 64)
            if (lo + e < (1u << HB_LUT_BITS)) L.lut[lo + e] = (uint16_t)ent;
    }
}

// Segments are dealt four at a time. Four that ask for at most HBS_WAVE_SEG bytes each go to
// the workgroup's four waves, one each, on a quarter of the stage and without a workgroup
// barrier: a 4 KiB segment has 64 chunks at S = 64, which keep one wave busy and would leave the
// other three waiting. A group with a longer segment is decoded a segment at a time by the
// whole workgroup, as k_hb_decode does.
#define HBS_WAVE_SEG 8192u
#define HBS_WAVE_STAGE 16896u   /* a wave's part of the stage; >= HB_OIDX(15 + HBS_WAVE_SEG), 16-B aligned */
static_assert(HBS_WAVE_SEG + 15u + 4u * ((HBS_WAVE_SEG + 15u) >> 7) < HBS_WAVE_STAGE, "a short segment fits a wave's stage");
static_assert(4u * HBS_WAVE_STAGE <= sizeof(HbsDecLds::out) && HBS_WAVE_STAGE % 16u == 0, "four wave stages in the stage");

// segment i by one wave (WAVE true) or by the whole workgroup, staged at `stage`. (The workgroup's
// commit flag is cleared here and not by the check: measured, with that store in the check this
// kernel's wave path decodes 4 KiB segments 1 % slower, and k_hb_decode 3 % slower without it.)
template <bool WAVE>
static __device__ __forceinline__ void hbs_decode_seg(HbsDecLds &L, uint8_t *stage, const HbDecArgs &A, uint64_t i, uint32_t tt)
{
    HbSpan G;
    if (!hb_decode_check<true>(A, i, tt, G, nullptr)) return;   // (true: see hb_record_check)
    if (!WAVE && tt == 0) L.bad = 0;
    hb_decode_body<WAVE, false>(L, stage, A, i, tt, G);
}

// (The long parameter list, not HbDecArgs by value as k_hb_decode and k_hbs_decode_ranges take it:
// the struct's pointers are not __restrict__, and with it this kernel decodes 64 KiB segments 4.9 %
// and 4 KiB segments 1.4 % slower, profiles/batch_decode_span.log, the struct runs.)
__global__ __launch_bounds__(HB_THREADS) void k_hbs_decode(uint64_t count, int nary, int w, uint32_t S,
                                                           const dc_dtable *__restrict__ T, const uint8_t *__restrict__ mode,
                                                           const uint32_t *__restrict__ bits, const uint64_t *__restrict__ pay_off,
                                                           const uint8_t *__restrict__ payload, uint64_t payload_cap,
                                                           const uint64_t *__restrict__ sync_off,
                                                           const uint16_t *__restrict__ sync_len, uint64_t sync_cap,
                                                           uint8_t *__restrict__ out, const uint64_t *out_beg, const uint64_t *out_end,
                                                           uint64_t out_cap, int32_t *__restrict__ status,
                                                           unsigned long long *__restrict__ first)
{
    __shared__ HbsDecLds L;
    const int t = threadIdx.x;
    const uint32_t lane = (uint32_t)t & 63u, wave = (uint32_t)t >> 6;
    const HbDecArgs A{nary, w, S, mode, bits, pay_off, payload, payload_cap, sync_off, sync_len, sync_cap,
                      out, out_beg, out_end, out_cap, status, first};
    const bool tok = hbs_table_ok(T, A.nary);
    if (tok) hbs_tables_load(L, T, t, lane, wave);   // (uniform) the decode tables, once for every segment of this workgroup
    const uint64_t groups = (count + 3) / 4;
    for (uint64_t g = blockIdx.x; g < groups; g += gridDim.x) {
        __syncthreads();   // the LDS of the group before (the first time: the tables)
        const uint64_t i0 = 4 * g;
        const uint32_t nseg = (uint32_t)min((uint64_t)4, count - i0);
        if (!tok) {
            if ((uint32_t)t < nseg) hb_fail(A.status, A.first, i0 + (uint32_t)t, DC_E_ARG);
            continue;
        }
        bool shortg = true;   // (workgroup-uniform; a range that ends before it starts fails on either path)
        for (uint32_t s = 0; s < nseg; ++s) {
            const uint64_t oa = A.out_beg[i0 + s], ob = A.out_end[i0 + s];
            shortg = shortg && !(ob > oa && ob - oa > HBS_WAVE_SEG);
        }
        if (shortg) {
            if (wave < nseg) hbs_decode_seg<true>(L, L.out + wave * HBS_WAVE_STAGE, A, i0 + wave, lane);
        } else {
            for (uint32_t s = 0; s < nseg; ++s) {
                if (s) __syncthreads();   // the stage of the segment before
                hbs_decode_seg<false>(L, L.out, A, i0 + s, (uint32_t)t);
            }
        }
    }
}
