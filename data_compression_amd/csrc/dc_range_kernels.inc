// dc_range_kernels.inc -- random-access decode by the sync index (dc_huff_decode_ranges /
// dc_huff_decode_range, dc_gpu.h (5r)); included by dc_core.hip after the general decoder,
// whose tables (DecLds), readers and chunk decoders it uses unchanged.
//
// The work unit is an item = (range, one group of 64 chunks the range touches): a range over
// the whole stream spreads over the whole grid, a million short ranges are a million items.
//   k_range_items        per range: items (groups touched; 0 for an empty or bad range), and
//                        the bad-range bit of the error slot
//   k_scan_u64           item offsets, the total in off[nranges] (device-resident)
//   k_huff_decode_ranges persistent grid; every wave takes a contiguous run of items (one
//                        binary search of the offsets per wave, then a walk), and per item:
//     1. the lanes up to the last needed chunk read their chunk lengths and prefix-sum them;
//     2. the wave stages only the bits from the first needed chunk's start to the last needed
//        chunk's end (a 100-byte read moves ~100 B of payload, not the group's 4 KiB);
//     3. the lanes whose chunk intersects the range decode it whole (decode_chunk_lds for
//        S <= DEC_OUT_SYMS, the masked HBM variant otherwise);
//     4. S <= DEC_OUT_SYMS: the wanted bytes go from the LDS rows to the (unaligned)
//        destination as a byte head, 16-B pieces and a byte tail. No byte outside
//        [out_off, out_off + count) of a range is written.

#define RNG_BAD_RANGE 2   /* error slot bit: a range outside the stream or the output buffer */

__global__ __launch_bounds__(256) void k_range_items(const uint64_t *__restrict__ first, const uint64_t *__restrict__ count,
                                                     const uint64_t *__restrict__ out_off, uint64_t nranges, uint64_t n,
                                                     uint64_t out_cap, uint32_t S, uint64_t *__restrict__ items,
                                                     int *__restrict__ err)
{
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= nranges) return;
    const uint64_t f = first[r], c = count[r], o = out_off[r];
    const bool bad = f > n || c > n - f || o > out_cap || c > out_cap - o;
    const uint32_t glog = (uint32_t)__builtin_ctz(S) + DC_SYNC_GROUP_LOG;
    items[r] = (bad || c == 0) ? 0ull : ((f + c - 1) >> glog) - (f >> glog) + 1;
    if (bad) atomicOr(err, RNG_BAD_RANGE);
}

// decode_chunk_hbm writing only the symbols [mlo, mhi) of the chunk: symbol p -> out[idx0 + p]
// (idx0 is taken modulo 2^64: it may lie "before" out for the symbols that are not written)
template <class R>
static __device__ __forceinline__ void decode_chunk_masked(R rd, uint32_t sh, uint32_t cnt, uint8_t *__restrict__ out,
                                                           uint64_t idx0, uint32_t mlo, uint32_t mhi, const DecLds &L,
                                                           const dc_dtable *__restrict__ T, int nary, int w, bool pow2,
                                                           int &bad)
{
    rd.init();
    const uint32_t hi = rd.peek();
    rd.advance(true);
    const uint32_t lo = rd.peek();
    rd.advance(true);
    uint64_t win = (((uint64_t)hi << 32) | lo) << sh;
    int wbits = 64 - (int)sh;
    for (uint32_t pos = 0; pos < cnt;) {
        const uint32_t e = decode_step(rd, win, wbits, L, T, nary, w, pow2, bad);
        const bool two = E_COUNT(e) == 2 && pos + 1 < cnt;
        if (pos >= mlo && pos < mhi) out[idx0 + pos] = (uint8_t)e;
        if (two && pos + 1 >= mlo && pos + 1 < mhi) out[idx0 + pos + 1] = (uint8_t)(e >> 16);
        const uint32_t nbt = two ? E_BITS(e) : E_BITS0(e);
        win <<= nbt;
        wbits -= (int)nbt;
        pos += two ? 2 : 1;
    }
}

// d_first == nullptr: the one range (v_first, v_count) -> out[0 ..), checked by the host
__global__ __launch_bounds__(DEC_WAVES * 64) void k_huff_decode_ranges(
    const uint32_t *__restrict__ in, uint64_t bit_base, uint64_t words, const uint64_t *__restrict__ sync_base,
    const uint16_t *__restrict__ sync_len, uint32_t S, uint64_t n, const dc_dtable *__restrict__ T,
    const uint64_t *__restrict__ d_first, const uint64_t *__restrict__ d_count, const uint64_t *__restrict__ d_out_off,
    const uint64_t *__restrict__ item_off, uint64_t nranges, uint64_t v_first, uint64_t v_count,
    uint8_t *__restrict__ out, int *__restrict__ err, int *__restrict__ err_next)
{
    __shared__ DecLds L;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    if (blockIdx.x == 0 && t < 4) err_next[t] = 0;   // the next decode's error slot
    if (!__hip_atomic_load(&T->dec_ready, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {   // tables rebuilt since
        if (threadIdx.x == 0) atomicOr(err, 1);
        return;
    }
    const uint32_t slog = (uint32_t)__builtin_ctz(S);   // S is a power of two (checked by the host)
    const uint32_t glog = slog + DC_SYNC_GROUP_LOG;
    const bool by_value = d_first == nullptr;
    const uint64_t total = by_value ? (v_count ? ((v_first + v_count - 1) >> glog) - (v_first >> glog) + 1 : 0ull)
                                    : item_off[nranges];
    // a contiguous run of items per wave
    const uint64_t nwaves = (uint64_t)gridDim.x * DEC_WAVES;
    const uint64_t per = (total + nwaves - 1) / nwaves;
    if ((uint64_t)blockIdx.x * DEC_WAVES * per >= total) return;   // (workgroup-uniform) nothing for this workgroup
    {
        const uint4 *src = reinterpret_cast<const uint4 *>(T->lut);
        uint4 *dst = reinterpret_cast<uint4 *>(L.lut);
        for (int i = t; i < (1 << DC_LUT_BITS) / 4; i += DEC_WAVES * 64) dst[i] = src[i];
        for (int k = t; k <= DC_MAX_DIGITS; k += DEC_WAVES * 64) {
            L.first[k] = T->first[k]; L.count[k] = T->count[k]; L.start[k] = T->start[k];
        }
        for (int i = t; i < DC_MAX_SYMS; i += DEC_WAVES * 64) L.syms[i] = T->syms[i];
    }
    const int nary = T->n_ary, w = T->w;
    const bool pow2 = (nary & (nary - 1)) == 0;
    __syncthreads();

    const uint64_t word_base = bit_base >> 5;
    uint32_t *stage = L.stage[wv];
    uint8_t *ostage = L.out[wv];
    const bool stage_out = S <= DEC_OUT_SYMS;
    int bad = 0;
    const uint64_t wid = (uint64_t)blockIdx.x * DEC_WAVES + wv;
    const uint64_t i0 = wid * per, i1 = (i0 + per < total) ? i0 + per : total;
    // the range of item i0: the last r with item_off[r] <= i0 (wave-uniform binary search)
    uint64_t r = 0;
    if (!by_value && i0 < i1) {
        uint64_t lo = 0, hi = nranges;   // item_off[lo] <= i0 < item_off[hi] (= total)
        while (hi - lo > 1) {
            const uint64_t mid = lo + ((hi - lo) >> 1);
            if (item_off[mid] <= i0) lo = mid; else hi = mid;
        }
        r = lo;
    }
    for (uint64_t i = i0; i < i1; ++i) {
        uint64_t first = v_first, count = v_count, oo = 0, ibase = 0;
        if (!by_value) {
            while (item_off[r + 1] <= i) ++r;   // (ranges without items are passed over; i < total ends it)
            first = d_first[r]; count = d_count[r]; oo = d_out_off[r]; ibase = item_off[r];
        }
        const uint64_t g = (first >> glog) + (i - ibase);
        const uint64_t gsym = g << glog;                                        // the group's first symbol
        const uint64_t lo = first > gsym ? first : gsym;                        // wanted symbols [lo, hi) of the group
        const uint64_t gend = gsym + ((uint64_t)1 << glog);
        const uint64_t hi = first + count < gend ? first + count : gend;
        const uint32_t la = (uint32_t)((lo - gsym) >> slog), lb = (uint32_t)((hi - 1 - gsym) >> slog);   // lanes la..lb decode
        const uint64_t c = g * DC_SYNC_GROUP + lane;
        const uint32_t len = (uint32_t)lane <= lb ? sync_len[c] : 0u;   // (hi <= n: chunks up to lb exist)
        uint32_t incl = len;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t y = __shfl_up(incl, d, 64);
            if (lane >= d) incl += y;
        }
        const uint32_t off_a = __shfl(incl - len, (int)la, 64);                 // bits of the group before chunk la
        const uint32_t span_bits = __shfl(incl, (int)lb, 64) - off_a;           // chunks la..lb
        const uint64_t rel0 = sync_base[g] - (word_base << 5) + off_a;          // span start, bits from in[0]
        const uint64_t w0 = (rel0 >> 5) & ~3ull;                                // 16-B aligned staging origin
        const uint32_t lead = (uint32_t)(rel0 - (w0 << 5));
        const uint32_t nwords = (lead + span_bits + 31) / 32 + 2;               // + window look-ahead
        // an index that leaves the payload (a valid stream has its slack past the last span: every 16-B staging load stays inside)
        if (sync_base[g] < (word_base << 5) || w0 + 4 * (uint64_t)((nwords + 4) / 4) > words) {
            bad = 1;
            continue;
        }
        const bool act = (uint32_t)lane >= la && (uint32_t)lane <= lb;
        const uint64_t sym0 = c << slog;
        const uint32_t cnt = act ? (uint32_t)((n - sym0 < S) ? (n - sym0) : S) : 0u;
        const uint32_t pos = lead + (incl - len - off_a);                       // lane start, bits into staging
        uint8_t *row = ostage + lane * DEC_OUT_STRIDE;
        // masked HBM writes (S > DEC_OUT_SYMS): symbol p of the chunk -> out[oo + sym0 + p - first]
        const uint64_t idx0 = oo + sym0 - first;
        const uint32_t mlo = lo > sym0 ? (uint32_t)(lo - sym0) : 0u;
        const uint32_t mhi = hi - sym0 < (uint64_t)cnt ? (uint32_t)(hi - sym0) : cnt;   // (act: sym0 < hi)
        if (nwords + 1 <= DEC_STAGE_WORDS) {   // +1: the reader peeks one word ahead
            const uint4 *src = reinterpret_cast<const uint4 *>(in + w0);
            uint4 *dst = reinterpret_cast<uint4 *>(stage);
            const uint32_t nvec = (nwords + 4) / 4;
#define DC_SWZ(v) make_uint4(bswap32(v.x), bswap32(v.y), bswap32(v.z), bswap32(v.w))
            // as k_huff_decode: all loads in flight, indices clamped rather than loads predicated
            // (a short read's clamped loads all fetch its last 16 B)
            const uint32_t j0 = lane, j1 = lane + 64, j2 = lane + 128, j3 = lane + 192, j4 = lane + 256, last = nvec - 1;
            const uint4 v0 = src[min(j0, last)], v1 = src[min(j1, last)], v2 = src[min(j2, last)],
                        v3 = src[min(j3, last)], v4 = src[min(j4, last)];
            if (j0 < nvec) dst[j0] = DC_SWZ(v0);
            if (j1 < nvec) dst[j1] = DC_SWZ(v1);
            if (j2 < nvec) dst[j2] = DC_SWZ(v2);
            if (j3 < nvec) dst[j3] = DC_SWZ(v3);
            if (j4 < nvec) dst[j4] = DC_SWZ(v4);
#undef DC_SWZ
            __builtin_amdgcn_wave_barrier();
            if (act) {
                LdsWords rd{stage + (pos >> 5), 0u};
                if (stage_out) decode_chunk_lds(rd, pos & 31, cnt, row, L, T, nary, w, pow2, bad);
                else decode_chunk_masked(rd, pos & 31, cnt, out, idx0, mlo, mhi, L, T, nary, w, pow2, bad);
            }
        } else if (act) {
            HbmWords rd{in + w0 + (pos >> 5), 0u};
            if (stage_out) decode_chunk_lds(rd, pos & 31, cnt, row, L, T, nary, w, pow2, bad);
            else decode_chunk_masked(rd, pos & 31, cnt, out, idx0, mlo, mhi, L, T, nary, w, pow2, bad);
        }
        if (stage_out) {
            // symbols [lo, hi) of the group: byte k of them is row (s0 + k) / S, column (s0 + k) % S
            __builtin_amdgcn_wave_barrier();
            const uint32_t s0 = (uint32_t)(lo - gsym), m = (uint32_t)(hi - lo);
            uint8_t *const dptr = out + oo + (lo - first);
            const uint32_t mis = (uint32_t)(-(uintptr_t)dptr) & 15u;
            const uint32_t head = mis < m ? mis : m;
            const uint32_t nbody = (m - head) >> 4;
            if ((uint32_t)lane < head) dptr[lane] = ostage[((s0 + lane) >> slog) * DEC_OUT_STRIDE + ((s0 + lane) & (S - 1))];
            if (((s0 + head) & 15u) == 0) {   // pieces aligned in their rows (S is a multiple of 16): two ds_read_b64
                for (uint32_t j = lane; j < nbody; j += 64) {
                    const uint32_t k = s0 + head + 16 * j;
                    const uint64_t *src = reinterpret_cast<const uint64_t *>(ostage + (k >> slog) * DEC_OUT_STRIDE + (k & (S - 1)));
                    const uint64_t a = src[0], b = src[1];
                    *reinterpret_cast<uint4 *>(dptr + head + 16 * j) =
                        make_uint4((uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b, (uint32_t)(b >> 32));
                }
            } else {                          // a piece may straddle two rows: gathered byte by byte
                for (uint32_t j = lane; j < nbody; j += 64) {
                    const uint32_t k = s0 + head + 16 * j;
                    uint32_t v[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        uint32_t x = 0;
#pragma unroll
                        for (int b = 0; b < 4; ++b) {
                            const uint32_t kk = k + 4 * q + b;
                            x |= (uint32_t)ostage[(kk >> slog) * DEC_OUT_STRIDE + (kk & (S - 1))] << (8 * b);
                        }
                        v[q] = x;
                    }
                    *reinterpret_cast<uint4 *>(dptr + head + 16 * j) = make_uint4(v[0], v[1], v[2], v[3]);
                }
            }
            const uint32_t tail0 = head + 16 * nbody;   // < 16 bytes left
            if (tail0 + lane < m) {
                const uint32_t kk = s0 + tail0 + lane;
                dptr[tail0 + lane] = ostage[(kk >> slog) * DEC_OUT_STRIDE + (kk & (S - 1))];
            }
        }
        __builtin_amdgcn_wave_barrier();   // staging areas reused by the next item
    }
    if (bad) atomicOr(err, 1);
}
