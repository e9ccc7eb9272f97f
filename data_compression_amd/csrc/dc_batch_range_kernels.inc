// dc_batch_range_kernels.inc -- byte ranges of the segments of a Huffman batch
// (dc_huff_decode_batch_ranges / dc_huff_decode_batch_shared_ranges, dc_gpu.h "Huffman batch v1:
// byte ranges"); included by dc_core.hip after dc_batch_shared_kernels.inc. Range r is the bytes
// [first[r], first[r] + count[r]) of segment seg[r]; one launch decodes any number of them, and
// of a segment only the chunks a range touches: the u16 entries before them are summed for the
// first chunk's bit position, nothing else of the segment is read.
//   hb_range_check       the tests of a range in the order dc_gpu.h gives them, on a workgroup or
//                        a wave; the arithmetic is dc_batch_range.h's, the tests of the segment's
//                        record are hb_record_check's. It fills the HbSpan that hb_decode_body
//                        <.., RANGE true> (dc_batch_kernels.inc) decodes: the one chunk loop,
//                        commit and phased write of the whole-segment kernels, run over the
//                        touched chunks alone
//   k_hbs_decode_ranges  shared table: the tables once per workgroup (hbs_tables_load), ranges
//                        dealt four consecutive at a time as k_hbs_decode deals segments: four of
//                        at most HBS_WAVE_SEG bytes to the four waves, otherwise one after the
//                        other to the workgroup
//   k_hb_decode_ranges   own tables: a workgroup takes a contiguous run of range indices and
//                        rebuilds its tables (hb_own_tables) only when seg[r] differs from the
//                        segment whose tables it holds
// Statuses go to d_rstatus[r] (A.status here; hb_fail: the lowest failing range of the call is kept
// in *first); the batch's d_status is not touched. HbDecArgs' out_beg / out_end are not used here.

struct HbRangeArgs {
    const uint64_t *seg_off;   // nseg + 1: only the differences are used
    const uint64_t *seg, *first, *count, *out_off;
    uint64_t nseg;
};

// Range r by the threads that call it (tt: the caller's index among them), a workgroup or a wave:
// every test is uniform among them and no barrier is reached. table_st: what a range that comes
// as far as the stream gets when the call's table is unusable (shared mode: DC_E_ARG), else DC_OK.
// Writes the status of a range that fails, or that asks for nothing; true: G is a range for
// hb_decode_body<.., true>, which writes its status. count: count[r] as the caller read it (a
// kernel reads a range's count once: what chose the range's stage also bounds what is staged there).
static __device__ __forceinline__ bool hb_range_check(const HbDecArgs &A, const HbRangeArgs &R, uint64_t r, uint64_t count,
                                                      uint32_t tt, int table_st, HbSpan &G)
{
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
    if (!hb_record_check<false>(A, seg, len, G)) {
        if (tt == 0) hb_fail(A.status, A.first, r, DC_E_STREAM);
        return false;
    }
    uint64_t c_lo, c_hi;
    dc_batch_range_chunks(first, count, A.S, &c_lo, &c_hi);   // (c_hi <= the segment's chunks: first + count <= len)
    G.c_lo = (uint32_t)c_lo;
    G.c_hi = (uint32_t)c_hi;
    G.first = (uint32_t)first;
    G.count = (uint32_t)count;
    G.dptr = A.out + oo;
    return true;
}

// ---- shared table -------------------------------------------------------------------------------
template <bool WAVE>
static __device__ __forceinline__ void hbs_decode_range(HbsDecLds &L, uint8_t *stage, const HbDecArgs &A, const HbRangeArgs &R,
                                                        uint64_t r, uint64_t count, uint32_t tt, int table_st)
{
    HbSpan G;
    if (!hb_range_check(A, R, r, count, tt, table_st, G)) return;
    if (!WAVE && tt == 0) L.bad = 0;   // (the body's first scan has the barrier that orders this store)
    hb_decode_body<WAVE, true>(L, stage, A, r, tt, G);
}

__global__ __launch_bounds__(HB_THREADS) void k_hbs_decode_ranges(HbDecArgs A, HbRangeArgs R, uint64_t nranges,
                                                                  const dc_dtable *__restrict__ T)
{
    __shared__ HbsDecLds L;
    const int t = threadIdx.x;
    const uint32_t lane = (uint32_t)t & 63u, wave = (uint32_t)t >> 6;
    const bool tok = hbs_table_ok(T, A.nary);
    if (tok) hbs_tables_load(L, T, t, lane, wave);   // (uniform) once for every range of this workgroup
    const int table_st = tok ? DC_OK : DC_E_ARG;
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
// (The long parameter list as k_hbs_decode, for the same reason: 2.2 to 3.2 % slower with HbDecArgs by value,
// profiles/batch_decode_span.log, the struct runs.)
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
        HbSpan G;
        if (!hb_range_check(A, R, r, R.count[r], (uint32_t)t, DC_OK, G)) continue;   // (uniform, as every test below)
        if (G.md == 1u) {
            if (G.seg != have) {
                have = G.seg;
                hb_own_tables(L, lens + G.seg * 256, A.nary, A.w, t);
            }
            if (L.C.bad) {   // (kept with `have`: every range of a segment with bad lens fails)
                if (t == 0) hb_fail(A.status, A.first, r, DC_E_STREAM);
                continue;
            }
        }
        if (t == 0) L.bad = 0;   // (the body's first scan has the barrier that orders this store)
        hb_decode_body<false, true>(L, L.out, A, r, (uint32_t)t, G);
    }
}
