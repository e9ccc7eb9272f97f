// dc_batch_set_kernels.inc -- the table-set mode of the batched Huffman codec
// (dc_huff_encode_batch_set / dc_huff_decode_batch_set, dc_gpu.h "Huffman batch v1, table set");
// included by dc_core.hip after dc_batch_range_kernels.inc. A set of K <= DC_BATCH_SET_MAX lens
// records stands where the own-table mode has one record per segment: segment i is coded under
// record tid[i], the cheapest record of the set that has a code for every byte it holds
// (n_ary_huffman.c:1210-1255, "remembering the last 2 or so Huffman tables"). Only where the
// table comes from is here: what a segment takes once its table is in LDS is dc_batch_kernels.inc's
// (hb_canonical, hb_own_tables, hb_pack_seg, hb_decode_check, hb_decode_body) and
// dc_batch_range_kernels.inc's (hb_range_check), called as they are.
//   k_hbm_plan           the set's lengths and their validity (dc_batch_set.h) in LDS once per
//                        workgroup; per segment the histogram in LDS, then K dot products of 256
//                        terms: wave v takes the records k = v (mod 4), a lane four byte values
//                        (one u32 of lengths against four counts), a wave reduce; the least cost
//                        in ascending k per wave, then over the four waves, so equal costs go to
//                        the lowest k. tid, mode, bits; with psize / nchunks the sizes for the
//                        scans (the encode), without them nothing else (dc_huff_batch_set_select)
//   k_scan_u64           twice: pay_off and sync_off
//   k_hbm_pack           hb_canonical(set + 256 tid[i]) then hb_pack_seg
//   k_hbm_decode         hb_own_tables(set + 256 tid[i]) then hb_decode_body; segments dealt four at a
//                        time as k_hbs_decode deals them: four short ones of one record to the four
//                        waves, otherwise one after the other to the workgroup
//   k_hbm_decode_ranges  k_hb_decode_ranges with the table keyed by tid[seg[r]]
//   k_hbm_hist           the byte counts of the segments per record, for the training
// Pack, decode and ranges give a workgroup a contiguous run of indices and keep the table they
// hold (`have`) while the next segment or range names the same record: in data made of regions
// the neighbours do. A failed build resets `have`; nothing else of a segment stays in LDS.

#define HBM_NONE 0xffffffffu   /* `have`: no table held */

// the contiguous run [beg, end) of `n` indices that workgroup blockIdx.x takes
static __device__ __forceinline__ void hbm_run(uint64_t n, uint64_t &beg, uint64_t &end)
{
    const uint64_t per = (n + gridDim.x - 1) / gridDim.x;
    beg = min(per * blockIdx.x, n);
    end = min(beg + per, n);
}

// the bytes p[0 .. len) counted into h[256] (LDS, atomics) by 256 threads, as k_hb_plan counts
// them: a byte head up to 4-B alignment, dwords, a byte tail; no barrier
static __device__ __forceinline__ void hbm_count(uint32_t *h, const uint8_t *__restrict__ p, uint32_t len, int t)
{
    const uint32_t mis = (uint32_t)(-(uintptr_t)p) & 3u;
    const uint32_t head = mis < len ? mis : len;
    if ((uint32_t)t < head) atomicAdd(&h[p[t]], 1u);
    const uint32_t nw = (len - head) >> 2;
    const uint32_t *pw = reinterpret_cast<const uint32_t *>(p + head);
    for (uint32_t k = t; k < nw; k += HB_THREADS) {
        const uint32_t v = pw[k];
        atomicAdd(&h[v & 255u], 1u);
        atomicAdd(&h[(v >> 8) & 255u], 1u);
        atomicAdd(&h[(v >> 16) & 255u], 1u);
        atomicAdd(&h[v >> 24], 1u);
    }
    const uint32_t tail = head + 4 * nw + (uint32_t)t;
    if (tail < len) atomicAdd(&h[p[tail]], 1u);
}

// ---- plan / select ------------------------------------------------------------------------------
struct HbmPlanLds {
    __attribute__((aligned(16))) uint8_t lens[DC_BATCH_SET_MAX * 256];   // the set, in digits
    __attribute__((aligned(16))) uint32_t h[256];
    uint32_t red[4][2];                                                  // per wave: least digit sum, its k
    uint8_t valid[DC_BATCH_SET_MAX];
};
static_assert(8 * sizeof(HbmPlanLds) <= 160 * 1024, "k_hbm_plan: eight workgroups in a CU's 160 KiB of LDS");

// psize / nchunks: both or neither (uniform)
__global__ __launch_bounds__(HB_THREADS) void k_hbm_plan(const uint8_t *__restrict__ in, const uint64_t *__restrict__ in_off,
                                                         uint64_t count, int nary, int w, uint32_t S,
                                                         const uint8_t *__restrict__ set, uint32_t K, uint8_t *__restrict__ tid,
                                                         uint8_t *__restrict__ mode, uint32_t *__restrict__ bits,
                                                         uint64_t *__restrict__ psize, uint64_t *__restrict__ nchunks,
                                                         int32_t *__restrict__ status, unsigned long long *__restrict__ first)
{
    __shared__ HbmPlanLds L;
    const int t = threadIdx.x;
    const uint32_t lane = (uint32_t)t & 63u, wave = (uint32_t)t >> 6;
    const uint32_t slog = (uint32_t)__builtin_ctz(S);
    for (uint32_t e = t; e < 16u * K; e += HB_THREADS)   // (set is 16-B aligned)
        reinterpret_cast<uint4 *>(L.lens)[e] = reinterpret_cast<const uint4 *>(set)[e];
    __syncthreads();
    // record t by lane t, each rotated by a dword of its own: 64 records read 64 banks
    if ((uint32_t)t < K) L.valid[t] = (uint8_t)dc_batch_set_table_ok(L.lens + 256 * t, nary, 4u * (uint32_t)t);
    for (uint64_t i = blockIdx.x; i < count; i += gridDim.x) {
        __syncthreads();   // h and red of the segment before (the first time: valid)
        const uint64_t a = in_off[i], b = in_off[i + 1];
        if (b < a || b - a > DC_BATCH_SEG_MAX) {   // (workgroup-uniform)
            if (t == 0) {
                if (psize) { psize[i] = 0; nchunks[i] = 0; }
                hb_fail(status, first, i, DC_E_ARG);
            }
            continue;
        }
        const uint32_t len = (uint32_t)(b - a);
        if (len == 0) {   // stored, 0 bytes
            if (t == 0) {
                status[i] = DC_OK; tid[i] = 0; mode[i] = 0; bits[i] = 0;
                if (psize) { psize[i] = 0; nchunks[i] = 0; }
            }
            continue;
        }
        L.h[t] = 0;
        __syncthreads();
        hbm_count(L.h, in + a, len, t);
        __syncthreads();
        // the digit sum of the segment under record k: sum h[s] L_k[s] <= 65536 * 32 for a valid record
        const uint4 h4 = reinterpret_cast<const uint4 *>(L.h)[lane];
        uint32_t best = ~0u, bestk = 0;
        for (uint32_t k = wave; k < K; k += 4) {   // ascending, and < below: the lowest k of equal sums
            if (!L.valid[k]) continue;             // (wave-uniform)
            const uint32_t l4 = reinterpret_cast<const uint32_t *>(L.lens + 256 * k)[lane];
            const uint32_t l0 = l4 & 255u, l1 = (l4 >> 8) & 255u, l2 = (l4 >> 16) & 255u, l3 = l4 >> 24;
            uint32_t d = h4.x * l0 + h4.y * l1 + h4.z * l2 + h4.w * l3;
            const bool miss = (h4.x && !l0) || (h4.y && !l1) || (h4.z && !l2) || (h4.w && !l3);
#pragma unroll
            for (int x = 32; x > 0; x >>= 1) d += __shfl_xor(d, x, 64);
            if (__any(miss)) continue;             // a byte of the segment has no code under k
            if (d < best) { best = d; bestk = k; }
        }
        if (lane == 0) { L.red[wave][0] = best; L.red[wave][1] = bestk; }
        __syncthreads();
        if (t == 0) {
            best = L.red[0][0];
            bestk = L.red[0][1];
#pragma unroll
            for (int v = 1; v < 4; ++v) {
                const uint32_t d = L.red[v][0], k = L.red[v][1];
                if (d < best || (d == best && k < bestk)) { best = d; bestk = k; }
            }
            const bool usable = best != ~0u;
            const uint32_t cb = usable ? best * (uint32_t)w : 0u;
            const bool huff = usable && cb < 8u * len;
            const uint32_t sb = huff ? cb : 8u * len;
            status[i] = DC_OK;
            tid[i] = usable ? (uint8_t)bestk : (uint8_t)0;
            mode[i] = huff ? 1 : 0;
            bits[i] = sb;
            if (psize) {
                psize[i] = hb_pad16((sb + 7u) >> 3);
                nchunks[i] = (len + S - 1) >> slog;
            }
        }
    }
}

// ---- pack ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(HB_THREADS) void k_hbm_pack(const uint8_t *__restrict__ in, const uint64_t *__restrict__ in_off,
                                                         uint64_t count, int nary, int w, uint32_t S,
                                                         const uint8_t *__restrict__ set, uint32_t K,
                                                         const uint8_t *__restrict__ tid, const uint8_t *__restrict__ mode,
                                                         const uint64_t *__restrict__ pay_off, uint8_t *__restrict__ payload,
                                                         uint64_t payload_cap, const uint64_t *__restrict__ sync_off,
                                                         uint16_t *__restrict__ sync_len, uint64_t sync_cap,
                                                         int32_t *__restrict__ status, unsigned long long *__restrict__ first)
{
    __shared__ HbPackLds L;
    uint64_t beg, end;
    hbm_run(count, beg, end);
    uint32_t have = HBM_NONE;   // the record whose code L.C holds (uniform)
    for (uint64_t i = beg; i < end; ++i) {
        __syncthreads();   // the LDS of the segment before
        if (status[i] != DC_OK) continue;   // (DC_E_ARG by the plan; uniform)
        if (mode[i] != 0) {                 // (uniform; a stored segment has no use for codes)
            const uint32_t k = tid[i];
            bool ok = k < K;
            if (ok && k != have) {
                hb_canonical(L.C, set + 256 * k, nary, w);
                ok = !L.C.bad;
                have = ok ? k : HBM_NONE;
            }
            if (!ok) {   // (not a plan of k_hbm_plan: it codes a segment under a valid record of the set)
                if (threadIdx.x == 0) hb_fail(status, first, i, DC_E_ARG);
                continue;
            }
        }
        hb_pack_seg(L.P, L.C.code, L.C.nb, i, in, in_off, S, mode, pay_off, payload, payload_cap, sync_off, sync_len, sync_cap,
                    status, first);
    }
}

// ---- decode -------------------------------------------------------------------------------------
// The table of record k in L for a mode-1 segment or range, built only when L does not hold it
// already; by the whole workgroup, uniform. false: tid names no record of the set, or the record
// gives no code (then L holds no table and `have` says so).
static __device__ __forceinline__ bool hbm_table(HbDecLds &L, uint32_t &have, const uint8_t *__restrict__ set, uint32_t K,
                                                 uint32_t k, int nary, int w, int t)
{
    if (k >= K) return false;
    if (k == have) return true;
    const bool ok = hb_own_tables(L, set + 256 * k, nary, w, t);
    have = ok ? k : HBM_NONE;
    return ok;
}

static_assert(4u * HBS_WAVE_STAGE <= sizeof(HbDecLds::out), "four wave stages in the stage");

// Segments are dealt four consecutive at a time, as k_hbs_decode deals them, a workgroup taking a
// contiguous run of such groups. A group of four short segments (<= HBS_WAVE_SEG bytes each) whose
// coded ones all name one record goes to the four waves, one segment each, under that record's
// table: a 4 KiB segment has 64 chunks at S = 64, which keep one wave busy. Any other group (a long
// segment, two records, a tid that names no table) is decoded a segment at a time by the whole
// workgroup, each coded segment under the table of its tid.
__global__ __launch_bounds__(HB_THREADS) void k_hbm_decode(HbDecArgs A, uint64_t count, const uint8_t *__restrict__ set,
                                                           uint32_t K, const uint8_t *__restrict__ tid)
{
    __shared__ HbDecLds L;
    const int t = threadIdx.x;
    const uint32_t lane = (uint32_t)t & 63u, wave = (uint32_t)t >> 6;
    uint64_t gbeg, gend;
    hbm_run((count + 3) / 4, gbeg, gend);
    uint32_t have = HBM_NONE;   // the record whose code L.C and L.lut hold (uniform)
    for (uint64_t g = gbeg; g < gend; ++g) {
        __syncthreads();   // the LDS of the group before
        const uint64_t i0 = 4 * g;
        const uint32_t nseg = (uint32_t)min((uint64_t)4, count - i0);
        // (uniform) one segment a wave? The mode byte and tid are only looked at here: every test of
        // a segment is hb_decode_check's, on either path, and a stored segment's tid is never read
        bool waves = true;
        uint32_t k = HBM_NONE;
#pragma unroll
        for (uint32_t s = 0; s < 4; ++s) {   // (a short group looks at its last segment again: the loads of all four start together)
            const uint64_t i = i0 + min(s, nseg - 1u);
            const uint64_t oa = A.out_beg[i], ob = A.out_end[i];
            const uint32_t md = A.mode[i];
            waves = waves && !(ob > oa && ob - oa > HBS_WAVE_SEG);
            if (waves && md == 1u) {
                const uint32_t ks = tid[i];
                waves = k == HBM_NONE || ks == k;
                k = ks;
            }
        }
        if (waves && k != HBM_NONE) waves = hbm_table(L, have, set, K, k, A.nary, A.w, t);   // (ends with a barrier when it builds)
        if (waves) {
            HbSpan G;
            if (wave < nseg && hb_decode_check<false>(A, i0 + wave, lane, G, nullptr))
                hb_decode_body<true, false>(L, L.out + wave * HBS_WAVE_STAGE, A, i0 + wave, lane, G);
            continue;
        }
        for (uint32_t s = 0; s < nseg; ++s) {
            if (s) __syncthreads();   // the stage of the segment before
            const uint64_t i = i0 + s;
            HbSpan G;
            if (!hb_decode_check<false>(A, i, (uint32_t)t, G, &L.bad)) continue;   // (uniform, as every test below)
            // tid and the set only now, and only for a coded segment
            if (G.md == 1u && !hbm_table(L, have, set, K, tid[i], A.nary, A.w, t)) {
                if (t == 0) hb_fail(A.status, A.first, i, DC_E_STREAM);
                continue;
            }
            hb_decode_body<false, false>(L, L.out, A, i, (uint32_t)t, G);
        }
    }
}

// ---- byte ranges --------------------------------------------------------------------------------
__global__ __launch_bounds__(HB_THREADS) void k_hbm_decode_ranges(HbDecArgs A, HbRangeArgs R, uint64_t nranges,
                                                                  const uint8_t *__restrict__ set, uint32_t K,
                                                                  const uint8_t *__restrict__ tid)
{
    __shared__ HbDecLds L;
    const int t = threadIdx.x;
    uint64_t beg, end;
    hbm_run(nranges, beg, end);   // a list sorted by record pays one build per record
    uint32_t have = HBM_NONE;
    for (uint64_t r = beg; r < end; ++r) {
        __syncthreads();   // the LDS of the range before
        HbSpan G;
        if (!hb_range_check(A, R, r, R.count[r], (uint32_t)t, DC_OK, G)) continue;   // (uniform, as every test below)
        if (G.md == 1u && !hbm_table(L, have, set, K, tid[G.seg], A.nary, A.w, t)) {
            if (t == 0) hb_fail(A.status, A.first, r, DC_E_STREAM);
            continue;
        }
        if (t == 0) L.bad = 0;   // (the body's first scan has the barrier that orders this store)
        hb_decode_body<false, true>(L, L.out, A, r, (uint32_t)t, G);
    }
}

// ---- histograms per record ----------------------------------------------------------------------
struct HbmHistLds {
    uint32_t h[DC_BATCH_SET_MAX * 256];   // 64 KiB: two workgroups a CU
};

// the workgroup's counters added to hist and zeroed; ends with a barrier
static __device__ __forceinline__ void hbm_hist_flush(HbmHistLds &L, uint32_t K, unsigned long long *__restrict__ hist, int t)
{
    __syncthreads();
    for (uint32_t e = t; e < 256u * K; e += HB_THREADS) {
        const uint32_t v = L.h[e];
        if (v) {
            atomicAdd(&hist[e], (unsigned long long)v);
            L.h[e] = 0;
        }
    }
    __syncthreads();
}

// hist (zeroed by the host) += the bytes of the segments of this workgroup's run, under tid[i]
__global__ __launch_bounds__(HB_THREADS) void k_hbm_hist(const uint8_t *__restrict__ in, const uint64_t *__restrict__ in_off,
                                                         uint64_t count, const uint8_t *__restrict__ tid, uint32_t K,
                                                         unsigned long long *__restrict__ hist)
{
    __shared__ HbmHistLds L;
    const int t = threadIdx.x;
    uint64_t beg, end;
    hbm_run(count, beg, end);
    for (uint32_t e = t; e < 256u * K; e += HB_THREADS) L.h[e] = 0;
    __syncthreads();
    uint64_t held = 0;   // the bytes counted since the last flush: a u32 counter holds them (uniform)
    for (uint64_t i = beg; i < end; ++i) {
        const uint64_t a = in_off[i], b = in_off[i + 1];
        if (b < a || b - a > DC_BATCH_SEG_MAX) continue;   // (uniform, as every test here)
        const uint32_t len = (uint32_t)(b - a), k = tid[i];
        if (k >= K || len == 0) continue;
        if (held + len > 0xffffffffull) {
            hbm_hist_flush(L, K, hist, t);
            held = 0;
        }
        held += len;
        hbm_count(L.h + 256 * k, in + a, len, t);   // (atomics: no barrier between segments)
    }
    hbm_hist_flush(L, K, hist, t);
}
