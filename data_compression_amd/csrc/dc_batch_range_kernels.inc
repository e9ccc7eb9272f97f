// dc_batch_range_kernels.inc -- byte ranges of the segments of a Huffman batch
// (dc_huff_decode_batch_ranges / dc_huff_decode_batch_shared_ranges, dc_gpu.h "Huffman batch v1:
// byte ranges"); included by dc_core.hip after dc_batch_shared_kernels.inc. Range r is the bytes
// [first[r], first[r] + count[r]) of segment seg[r]; one launch decodes any number of them, and
// of a segment only the chunks a range touches: the u16 entries before them are summed for the
// first chunk's bit position, nothing else of the segment is read.
//   hb_range_check        the tests of a range in the order dc_gpu.h gives them, on a workgroup or
//                         a wave; the arithmetic is dc_batch_range.h's
//   hb_decode_range_body  the entries before c_lo summed (strided reads, a wave or workgroup
//                         reduce), then hb_decode_body's chunk loop over [c_lo, c_hi) alone: every
//                         touched chunk decoded whole and checked to take exactly its bits, only
//                         the symbols of the range staged (at the destination's 16-B phase), the
//                         commit, the phased write
//   k_hbs_decode_ranges   shared table: the tables once per workgroup (hbs_tables_load), ranges
//                         dealt four consecutive at a time as k_hbs_decode deals segments: four of
//                         at most HBS_WAVE_SEG bytes to the four waves, otherwise one after the
//                         other to the workgroup
//   k_hb_decode_ranges    own tables: a workgroup takes a contiguous run of range indices and
//                         rebuilds hb_canonical and the 12-bit table only when seg[r] differs from
//                         the segment whose table it holds
// Statuses go to rstatus[r] (hb_fail: the lowest failing range of the call is kept in *first); the
// batch's d_status is not touched. HbDecArgs' out_beg / out_end are not used here.

struct HbRangeArgs {
    const uint64_t *seg_off;   // nseg + 1: only the differences are used
    const uint64_t *seg, *first, *count, *out_off;
    uint64_t nseg;
};

// a range that passed hb_range_check
struct HbRange {
    uint64_t seg;
    uint32_t len, first, count;   // the segment's bytes; the range (count > 0)
    uint32_t md, sb;              // the segment's mode and bits
    uint32_t c_lo, c_hi;          // the chunks it touches
    uint64_t po, pe, so;          // the segment's payload bytes [po, pe), its first sync entry
    uint8_t *dptr;                // where the range goes
};

// Range r by the threads that call it (tt: the caller's index among them), a workgroup or a wave:
// every test is uniform among them and no barrier is reached. table_st: what a range that comes
// as far as the stream gets when the call's table is unusable (shared mode: DC_E_ARG), else DC_OK.
// Writes the status of a range that fails, or that asks for nothing; true: G is a range for
// hb_decode_range_body, which writes its status. count: count[r] as the caller read it (a kernel
// reads a range's count once: what chose the range's stage also bounds what is staged there).
static __device__ __forceinline__ bool hb_range_check(const HbDecArgs &A, const HbRangeArgs &R, uint64_t r, uint64_t count,
                                                      uint32_t tt, int table_st, HbRange &G)
{
    const uint32_t S = A.S;
    const uint64_t seg = R.seg[r];
    if (seg >= R.nseg) {
        if (tt == 0) hb_fail(A.status, A.first, r, DC_E_ARG);
        return false;
    }
    uint32_t len = 0;
    int st = dc_batch_range_seg_len(R.seg_off[seg], R.seg_off[seg + 1], DC_BATCH_SEG_MAX, &len);
    const uint64_t first = R.first[r], oo = R.out_off[r];
    if (st == DC_OK) st = dc_batch_range_args(len, first, count, oo, A.out_cap);   // (DC_E_ARG, then DC_E_CAPACITY)
    if (st != DC_OK) {
        if (tt == 0) hb_fail(A.status, A.first, r, st);
        return false;
    }
    if (count == 0) {   // nothing further is read
        if (tt == 0) A.status[r] = DC_OK;
        return false;
    }
    if (table_st != DC_OK) {
        if (tt == 0) hb_fail(A.status, A.first, r, table_st);
        return false;
    }
    // the segment's record: hb_decode_check's tests against len
    const uint32_t md = A.mode[seg], sb = A.bits[seg];
    const uint64_t po = A.pay_off[seg], pe = A.pay_off[seg + 1], so = A.sync_off[seg], se = A.sync_off[seg + 1];
    const uint32_t nch = (len + S - 1) >> (uint32_t)__builtin_ctz(S);
    bool ok = md <= 1u && sb <= 8u * len && (md == 1u || sb == 8u * len);
    ok = ok && pe >= po && pe <= A.payload_cap && (po & 15u) == 0 && pe - po == hb_pad16((sb + 7u) >> 3);
    ok = ok && se >= so && se <= A.sync_cap && se - so == nch;
    if (!ok) {
        if (tt == 0) hb_fail(A.status, A.first, r, DC_E_STREAM);
        return false;
    }
    uint64_t c_lo, c_hi;
    dc_batch_range_chunks(first, count, S, &c_lo, &c_hi);   // (c_hi <= nch: first + count <= len)
    G = HbRange{seg, len, (uint32_t)first, (uint32_t)count, md, sb, (uint32_t)c_lo, (uint32_t)c_hi, po, pe, so, A.out + oo};
    return true;
}

// The range G (number r) staged at `stage`, by the NT threads that hb_range_check ran on; for a
// mode-1 segment L.lut and L.C hold its code. The whole workgroup (WAVE false: every barrier below
// is reached by all of it, every test before one is uniform, and the caller has cleared L.bad, the
// commit flag, after the barrier that ended the range before), or one wave (WAVE true:
// wave-uniform tests, no workgroup barrier, L.bad not used). Byte k of the range is staged at
// HB_OIDX(phase + k), as hb_decode_body stages byte k of a segment.
template <bool WAVE, class Lds>
static __device__ __forceinline__ void hb_decode_range_body(Lds &L, uint8_t *stage, const HbDecArgs &A, uint64_t r, uint32_t tt,
                                                            const HbRange &G)
{
    constexpr uint32_t NT = WAVE ? 64u : (uint32_t)HB_THREADS;
    const uint32_t S = A.S, slog = (uint32_t)__builtin_ctz(S);
    const uint32_t md = G.md, lo = G.first, hi = G.first + G.count;
    uint8_t *const dptr = G.dptr;
    const uint32_t phase = (uint32_t)(uintptr_t)dptr & 15u;
    const uint8_t *const pay = A.payload + G.po;
    const uint16_t *const sl = A.sync_len + G.so;
    if (md == 0)   // (lo + k < len <= bits / 8: inside the payload)
        for (uint32_t k = tt; k < G.count; k += NT) stage[HB_OIDX(phase + k)] = pay[lo + k];
    // the bit position of chunk c_lo: the entries before it (<= 4096 of <= 65535 each)
    uint32_t before = 0;
#pragma unroll 4
    for (uint32_t c = tt; c < G.c_lo; c += NT) before += sl[c];
    uint32_t base;
    if (WAVE) {
        base = (uint32_t)__builtin_amdgcn_readlane((int)wave_scan_incl(before), 63);
    } else {
        wg_scan_excl_u32(before, L.scan, &base);
    }
    // chunk c by thread (c - c_lo) % NT, NT chunks at a time: their bit lengths scanned, then decoded
    const uint32_t nw = (uint32_t)(G.pe - G.po) / 4;
    const uint32_t *const pw = reinterpret_cast<const uint32_t *>(pay);
#define HB_WORD(k) ((k) < nw ? bswap32(pw[k]) : 0u)
    int bad = 0;
    for (uint32_t c0 = G.c_lo; c0 < G.c_hi; c0 += NT) {
        const uint32_t c = c0 + tt;
        const uint32_t clen = c < G.c_hi ? sl[c] : 0u;
        uint32_t tot, pos;
        if (WAVE) {   // (all 64 lanes are here: the loop's bounds are wave-uniform)
            const uint32_t incl = wave_scan_incl(clen);
            pos = base + incl - clen;
            tot = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        } else {
            pos = base + wg_scan_excl_u32(clen, L.scan, &tot);
        }
        base += tot;
        if (c >= G.c_hi || bad) continue;
        const uint32_t sym0 = c << slog;
        const uint32_t cnt = min(S, G.len - sym0);
        if (md == 0) {   // stored: 8 bits a symbol
            bad |= clen != 8u * cnt;
            continue;
        }
        uint32_t k = pos >> 5;
        const uint32_t sh = pos & 31u;
        uint64_t win = (((uint64_t)HB_WORD(k) << 32) | HB_WORD(k + 1)) << sh;
        int wbits = 64 - (int)sh;
        k += 2;
        uint32_t used = 0;
        for (uint32_t j = 0; j < cnt; ++j) {
            if (wbits < 32) {
                win |= (uint64_t)HB_WORD(k) << (32 - wbits);
                ++k;
                wbits += 32;
            }
            const uint32_t e = L.lut[win >> (64 - HB_LUT_BITS)];
            uint32_t nb = e >> 8, sym = e & 255u;
            if (!nb) {
                nb = hb_decode_slow((uint32_t)(win >> 32), HB_LUT_BITS + 1u, 32u, L.C, A.nary, A.w, sym);
                if (!nb || sym >= 256u) { bad = 1; break; }   // no code, or the code of no byte
            }
            const uint32_t at = sym0 + j;   // only the first and the last touched chunk hold symbols outside the range
            if (at >= lo && at < hi) stage[HB_OIDX(phase + (at - lo))] = (uint8_t)sym;
            win <<= nb;
            wbits -= (int)nb;
            used += nb;
        }
        if (used != clen) bad = 1;
    }
#undef HB_WORD
    bool fail;   // (base: the end of the last touched chunk must not pass bits)
    if (WAVE) {
        __builtin_amdgcn_wave_barrier();   // the stage is read by other lanes than wrote it
        fail = __any(bad || base > G.sb);
    } else {
        if (bad || base > G.sb) L.bad = 1;
        __syncthreads();
        fail = L.bad != 0;
    }
    if (fail) {   // nothing of a range with a corrupt chunk is written
        if (tt == 0) hb_fail(A.status, A.first, r, DC_E_STREAM);
        return;
    }
    if (tt == 0) A.status[r] = DC_OK;
    // the stage has the destination's 16-B phase: a byte head, aligned 16-B pieces, a byte tail
    const uint32_t len = G.count;
    const uint32_t head = min((16u - phase) & 15u, len);
    if (tt < head) dptr[tt] = stage[HB_OIDX(phase + tt)];
    const uint32_t nbody = (len - head) >> 4;
    for (uint32_t v = tt; v < nbody; v += NT) {   // (a piece never crosses a pad: 16 divides 128)
        const uint32_t *const q = reinterpret_cast<const uint32_t *>(stage + HB_OIDX(phase + head + 16 * v));
        *reinterpret_cast<uint4 *>(dptr + head + 16 * v) = make_uint4(q[0], q[1], q[2], q[3]);
    }
    const uint32_t tail = head + 16 * nbody + tt;
    if (tail < len) dptr[tail] = stage[HB_OIDX(phase + tail)];
}

// ---- shared table -------------------------------------------------------------------------------
template <bool WAVE>
static __device__ __forceinline__ void hbs_decode_range(HbsDecLds &L, uint8_t *stage, const HbDecArgs &A, const HbRangeArgs &R,
                                                        uint64_t r, uint64_t count, uint32_t tt, int table_st)
{
    HbRange G;
    if (!hb_range_check(A, R, r, count, tt, table_st, G)) return;
    if (!WAVE && tt == 0) L.bad = 0;   // (the body's first scan has the barrier that orders this store)
    hb_decode_range_body<WAVE>(L, stage, A, r, tt, G);
}

__global__ __launch_bounds__(HB_THREADS) void k_hbs_decode_ranges(
    HbRangeArgs R, uint64_t nranges, int nary, int w, uint32_t S, const dc_dtable *__restrict__ T,
    const uint8_t *__restrict__ mode, const uint32_t *__restrict__ bits, const uint64_t *__restrict__ pay_off,
    const uint8_t *__restrict__ payload, uint64_t payload_cap, const uint64_t *__restrict__ sync_off,
    const uint16_t *__restrict__ sync_len, uint64_t sync_cap, uint8_t *__restrict__ out, uint64_t out_cap,
    int32_t *__restrict__ rstatus, unsigned long long *__restrict__ first)
{
    __shared__ HbsDecLds L;
    const int t = threadIdx.x;
    const uint32_t lane = (uint32_t)t & 63u, wave = (uint32_t)t >> 6;
    const bool tok = hbs_table_ok(T, nary);
    if (tok) hbs_tables_load(L, T, t, lane, wave);   // (uniform) once for every range of this workgroup
    const int table_st = tok ? DC_OK : DC_E_ARG;
    const HbDecArgs A{nary, w, S, mode, bits, pay_off, payload, payload_cap, sync_off, sync_len, sync_cap,
                      out, nullptr, nullptr, out_cap, rstatus, first};
    const uint64_t groups = (nranges + 3) / 4;
    for (uint64_t g = blockIdx.x; g < groups; g += gridDim.x) {
        __syncthreads();   // the LDS of the group before (the first time: the tables)
        const uint64_t r0 = 4 * g;
        const uint32_t nr = (uint32_t)min((uint64_t)4, nranges - r0);
        // the group's counts, read once (workgroup-uniform; unrolled: cnt stays in registers)
        uint64_t cnt[4];
        bool shortg = true;   // (a count that fits no segment fails on either path)
#pragma unroll
        for (uint32_t s = 0; s < 4; ++s) {
            cnt[s] = s < nr ? R.count[r0 + s] : 0;
            shortg = shortg && cnt[s] <= HBS_WAVE_SEG;
        }
#define HBS_CNT(k) ((k) == 0 ? cnt[0] : (k) == 1 ? cnt[1] : (k) == 2 ? cnt[2] : cnt[3])
        if (shortg) {
            if (wave < nr) hbs_decode_range<true>(L, L.out + wave * HBS_WAVE_STAGE, A, R, r0 + wave, HBS_CNT(wave), lane, table_st);
        } else {
            for (uint32_t s = 0; s < nr; ++s) {
                if (s) __syncthreads();   // the stage of the range before
                hbs_decode_range<false>(L, L.out, A, R, r0 + s, HBS_CNT(s), (uint32_t)t, table_st);
            }
        }
#undef HBS_CNT
    }
}

// ---- own tables ---------------------------------------------------------------------------------
__global__ __launch_bounds__(HB_THREADS) void k_hb_decode_ranges(
    HbRangeArgs R, uint64_t nranges, int nary, int w, uint32_t S, const uint8_t *__restrict__ lens,
    const uint8_t *__restrict__ mode, const uint32_t *__restrict__ bits, const uint64_t *__restrict__ pay_off,
    const uint8_t *__restrict__ payload, uint64_t payload_cap, const uint64_t *__restrict__ sync_off,
    const uint16_t *__restrict__ sync_len, uint64_t sync_cap, uint8_t *__restrict__ out, uint64_t out_cap,
    int32_t *__restrict__ rstatus, unsigned long long *__restrict__ first)
{
    __shared__ HbDecLds L;
    const int t = threadIdx.x;
    const HbDecArgs A{nary, w, S, mode, bits, pay_off, payload, payload_cap, sync_off, sync_len, sync_cap,
                      out, nullptr, nullptr, out_cap, rstatus, first};
    // a contiguous run of ranges: neighbours of a list sorted by segment share a table
    const uint64_t per = (nranges + gridDim.x - 1) / gridDim.x;
    const uint64_t beg = min(per * blockIdx.x, nranges), end = min(beg + per, nranges);
    uint64_t have = ~0ull;   // the segment whose code L.C and L.lut hold (uniform)
    for (uint64_t r = beg; r < end; ++r) {
        __syncthreads();   // the LDS of the range before
        HbRange G;
        if (!hb_range_check(A, R, r, R.count[r], (uint32_t)t, DC_OK, G)) continue;   // (uniform, as every test below)
        if (G.md == 1u) {
            if (G.seg != have) {
                have = G.seg;
                hb_canonical(L.C, lens + G.seg * 256, nary, w);
                if (!L.C.bad) {   // (read after hb_canonical's barrier)
                    for (uint32_t e = t; e < (1u << HB_LUT_BITS); e += HB_THREADS) {
                        uint32_t sym = 0;
                        const uint32_t nb = hb_decode_slow(e << (32 - HB_LUT_BITS), 1u, HB_LUT_BITS, L.C, nary, w, sym);
                        L.lut[e] = (uint16_t)(nb ? (sym | (nb << 8)) : 0u);
                    }
                    __syncthreads();
                }
            }
            if (L.C.bad) {   // (kept with `have`: every range of a segment with bad lens fails)
                if (t == 0) hb_fail(rstatus, first, r, DC_E_STREAM);
                continue;
            }
        }
        if (t == 0) L.bad = 0;   // (the body's first scan has the barrier that orders this store)
        hb_decode_range_body<false>(L, L.out, A, r, (uint32_t)t, G);
    }
}
