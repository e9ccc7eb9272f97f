// dc_batch_shared_kernels.inc -- the shared-table mode of the batched Huffman codec
// (dc_huff_encode_batch_shared / dc_huff_decode_batch_shared, dc_gpu.h "Huffman batch v1, shared
// table"); included by dc_core.hip after dc_batch_kernels.inc, whose helpers it uses. One
// dc_dtable codes every segment, so no work of a segment is proportional to the table: a
// persistent workgroup copies what it needs of the table into LDS once, before its segment loop.
//   k_hbs_plan    nbits[256] in LDS; per segment the sum of nb[byte] and whether a byte has no
//                 code (no histogram, no table build): mode, bits, and the payload bytes and
//                 sync entries for the scans
//   k_scan_u64    twice: pay_off and sync_off
//   k_hbs_pack    code / nbits in LDS; per segment exactly k_hb_pack's unit scan, LDS stage and
//                 16-B stores
//   k_hbs_decode  once per workgroup the 12-bit first-level table, filled by code ranges from
//                 code / nbits (the packed codes are prefix-free bit strings at any arity), and
//                 the table's canonical arrays for the longer codes; per segment exactly
//                 k_hb_decode's chunk scan, exactness check and phased output stage. Segments
//                 are dealt four at a time: four short ones (<= 8 KiB) to the four waves, one
//                 each, on a quarter of the stage; otherwise one after the other to the workgroup
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
    __attribute__((aligned(16))) uint32_t stage[DC_BATCH_SEG_MAX / 4];   // the payload, word bit 31 first
    uint32_t code[256];            // the table's, read once
    uint32_t nb[256];
    uint16_t ulen[HB_UNITS_MAX];   // bits per 16-symbol unit
    uint32_t tbase[HB_THREADS];    // bit offset of unit 16 t
    uint32_t scan[4];
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
    const uint32_t slog = (uint32_t)__builtin_ctz(S);
    {
        const uint32_t nb = hbs_nb(T->nbits[t]);
        L.nb[t] = nb;
        L.code[t] = nb ? T->code[t] : 0u;
    }
    for (uint64_t i = blockIdx.x; i < count; i += gridDim.x) {
        __syncthreads();   // the LDS of the segment before (the first time: the table's copy)
        if (status[i] != DC_OK) continue;   // (DC_E_ARG by the plan; uniform)
        const uint64_t a = in_off[i];
        const uint32_t len = (uint32_t)(in_off[i + 1] - a);
        const uint64_t po = pay_off[i], pe = pay_off[i + 1], so = sync_off[i], se = sync_off[i + 1];
        if (pe > payload_cap || se > sync_cap) {
            if (t == 0) hb_fail(status, first, i, DC_E_CAPACITY);
            continue;
        }
        if (len == 0) continue;
        const uint32_t psz = (uint32_t)(pe - po), nch = (uint32_t)(se - so);
        const uint8_t *p = in + a;
        uint4 *const dst = reinterpret_cast<uint4 *>(payload + po);   // (po and payload 16-B aligned)
        if (mode[i] == 0) {   // stored: the bytes, zero-padded to 16
            for (uint32_t v = t; v < psz / 16; v += HB_THREADS) {
                uint32_t q[4];
                hb_load16(p, 16 * v, len, q);
                const uint32_t left = len - 16 * v;   // (> 0: psz = pad16(len))
#pragma unroll
                for (uint32_t j = 0; j < 4; ++j) {
                    if (left <= 4 * j) q[j] = 0;
                    else if (left < 4 * j + 4) q[j] &= (1u << (8 * (left - 4 * j))) - 1u;
                }
                dst[v] = make_uint4(q[0], q[1], q[2], q[3]);
            }
            for (uint32_t c = t; c < nch; c += HB_THREADS) {
                const uint32_t left = len - (c << slog);
                sync_len[so + c] = (uint16_t)(8u * (left < S ? left : S));
            }
            continue;
        }
        for (uint32_t k = t; k < psz / 4; k += HB_THREADS) L.stage[k] = 0;
        // unit u (16 symbols) by thread u % 256: its bit length, then the scan (thread t sums
        // units 16 t .. 16 t + 15), then its codes OR-ed into the stage at its bit offset
        const uint32_t units = (len + HB_UNIT - 1) / HB_UNIT;
        for (uint32_t u = t; u < units; u += HB_THREADS) {
            uint32_t q[4];
            hb_load16(p, u * HB_UNIT, len, q);
            const uint32_t cntu = min((uint32_t)HB_UNIT, len - u * HB_UNIT);
            uint32_t ub = 0;
#pragma unroll
            for (uint32_t k = 0; k < HB_UNIT; ++k)
                if (k < cntu) ub += L.nb[(q[k >> 2] >> (8 * (k & 3))) & 255u];
            L.ulen[u] = (uint16_t)ub;   // <= 16 * 32
        }
        __syncthreads();
        uint32_t tsum = 0;
        for (uint32_t u = 16 * (uint32_t)t; u < min(16 * (uint32_t)t + 16, units); ++u) tsum += L.ulen[u];
        uint32_t total;
        L.tbase[t] = wg_scan_excl_u32(tsum, L.scan, &total);
        __syncthreads();
        {   // the sync index: chunk c = units [c r, (c + 1) r), r = S / 16
            const uint32_t r = S / HB_UNIT;
            for (uint32_t c = t; c < nch; c += HB_THREADS) {
                const uint32_t e = min((c + 1) * r, units);
                uint32_t cb = 0;
                for (uint32_t u = c * r; u < e; ++u) cb += L.ulen[u];
                sync_len[so + c] = (uint16_t)cb;   // <= 1024 * 32
            }
        }
        for (uint32_t u = t; u < units; u += HB_THREADS) {
            uint32_t pos = L.tbase[u >> 4];
            for (uint32_t k = u & ~15u; k < u; ++k) pos += L.ulen[k];
            uint32_t q[4];
            hb_load16(p, u * HB_UNIT, len, q);
            const uint32_t cntu = min((uint32_t)HB_UNIT, len - u * HB_UNIT);
            // a 64-bit accumulator, whole words OR-ed into the stage (neighbours share words)
            uint32_t wi = pos >> 5, nacc = pos & 31u;
            uint64_t acc = 0;
#pragma unroll
            for (uint32_t k = 0; k < HB_UNIT; ++k) {
                if (k < cntu) {
                    const uint32_t b = (q[k >> 2] >> (8 * (k & 3))) & 255u, nb = L.nb[b];
                    if (nb) acc |= (uint64_t)L.code[b] << (64u - nacc - nb);
                    nacc += nb;
                    if (nacc >= 32u) {
                        if (wi < DC_BATCH_SEG_MAX / 4) atomicOr(&L.stage[wi], (uint32_t)(acc >> 32));
                        ++wi;
                        acc <<= 32;
                        nacc -= 32u;
                    }
                }
            }
            if (nacc && wi < DC_BATCH_SEG_MAX / 4) atomicOr(&L.stage[wi], (uint32_t)(acc >> 32));
        }
        __syncthreads();
        for (uint32_t v = t; v < psz / 16; v += HB_THREADS) {
            const uint4 q = reinterpret_cast<const uint4 *>(L.stage)[v];
            dst[v] = make_uint4(bswap32(q.x), bswap32(q.y), bswap32(q.z), bswap32(q.w));
        }
    }
}

// ---- decode -----------------------------------------------------------------------------------
struct HbsDecLds {
    // byte k of the segment at out[HB_OIDX(phase + k)]: 4 pad bytes after every 128
    __attribute__((aligned(16))) uint8_t out[DC_BATCH_SEG_MAX + 16 + 4 * (DC_BATCH_SEG_MAX / 128 + 1)];
    uint16_t lut[1 << HB_LUT_BITS];   // next 12 bits -> sym | bits << 8; 0: longer, or no code
    // the table's canonical arrays (first / count / start / syms), for codes over 12 bits
    uint32_t cnt[DC_MAX_DIGITS + 1], startv[DC_MAX_DIGITS + 1], starti[DC_MAX_DIGITS + 1];
    uint16_t syms[DC_MAX_SYMS];       // up to 1024 symbols: one >= 256 is never a byte
    uint32_t scan[4];
    int mn, mx, bad;
};

// hb_decode_slow on the table's arrays: the symbol (< DC_MAX_SYMS) whose code leads the 32-bit
// window `win`, its bit length, 0 when no code of lo .. 32 bits matches
static __device__ __forceinline__ uint32_t hbs_decode_slow(uint32_t win, uint32_t lo, const HbsDecLds &C, int nary, int w,
                                                           uint32_t &sym)
{
    const int top = C.mx;
    if ((nary & (nary - 1)) == 0) {   // n = 2^w: the value of the first L digits is the first L w bits
        int L = C.mn;
        while ((uint32_t)(L * w) < lo) ++L;
        for (; L <= top && L * w <= 32; ++L) {
            const uint32_t r = (win >> (32 - L * w)) - C.startv[L];
            if (r < C.cnt[L]) {
                sym = C.syms[(C.starti[L] + r) & (DC_MAX_SYMS - 1)];
                return (uint32_t)(L * w);
            }
        }
        return 0;
    }
    uint32_t v = 0;
    const uint32_t dmask = (1u << w) - 1u;
    for (int L = 1; L <= top && L * w <= 32; ++L) {
        const uint32_t d = (win >> (32 - L * w)) & dmask;
        if (d >= (uint32_t)nary) return 0;
        v = v * (uint32_t)nary + d;
        if (L >= C.mn && (uint32_t)(L * w) >= lo) {
            const uint32_t r = v - C.startv[L];
            if (r < C.cnt[L]) {
                sym = C.syms[(C.starti[L] + r) & (DC_MAX_SYMS - 1)];
                return (uint32_t)(L * w);
            }
        }
    }
    return 0;
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

struct HbsDecArgs {
    int nary, w;
    uint32_t S;
    const uint8_t *mode;
    const uint32_t *bits;
    const uint64_t *pay_off;
    const uint8_t *payload;
    uint64_t payload_cap;
    const uint64_t *sync_off;
    const uint16_t *sync_len;
    uint64_t sync_cap;
    uint8_t *out;
    const uint64_t *out_beg, *out_end;   // (the two may alias: d_out_off, d_out_off + 1)
    uint64_t out_cap;
    int32_t *status;
    unsigned long long *first;
};

// segment i by the NT threads that call it (tt: the caller's index among them), staged at
// `stage`: the whole workgroup (WAVE false: every barrier below is reached by all of it, and every
// test before one is uniform), or one wave (WAVE true: wave-uniform tests, no workgroup barrier)
template <bool WAVE>
static __device__ __forceinline__ void hbs_decode_seg(HbsDecLds &L, uint8_t *stage, const HbsDecArgs &A, uint64_t i, uint32_t tt)
{
    constexpr uint32_t NT = WAVE ? 64u : (uint32_t)HB_THREADS;
    const uint32_t S = A.S, slog = (uint32_t)__builtin_ctz(S);
    const uint64_t oa = A.out_beg[i], ob = A.out_end[i];
    if (ob < oa || ob - oa > DC_BATCH_SEG_MAX) {
        if (tt == 0) hb_fail(A.status, A.first, i, DC_E_ARG);
        return;
    }
    if (ob > A.out_cap) {
        if (tt == 0) hb_fail(A.status, A.first, i, DC_E_CAPACITY);
        return;
    }
    const uint32_t len = (uint32_t)(ob - oa);
    const uint32_t md = A.mode[i], sb = A.bits[i];
    const uint64_t po = A.pay_off[i], pe = A.pay_off[i + 1], so = A.sync_off[i], se = A.sync_off[i + 1];
    const uint32_t nch = (len + S - 1) >> slog;
    bool ok = md <= 1u && sb <= 8u * len && (md == 1u || sb == 8u * len);
    ok = ok && pe >= po && pe <= A.payload_cap && (po & 15u) == 0 && pe - po == hb_pad16((sb + 7u) >> 3);
    ok = ok && se >= so && se <= A.sync_cap && se - so == nch;
    if (!ok) {
        if (tt == 0) hb_fail(A.status, A.first, i, DC_E_STREAM);
        return;
    }
    if (tt == 0) {
        A.status[i] = DC_OK;
        if (!WAVE) L.bad = 0;
    }
    if (len == 0) return;
    uint8_t *const dptr = A.out + oa;
    const uint32_t phase = (uint32_t)(uintptr_t)dptr & 15u;
    const uint8_t *const pay = A.payload + po;
    if (md == 0)
        for (uint32_t k = tt; k < len; k += NT) stage[HB_OIDX(phase + k)] = pay[k];
    // chunk c by thread c % NT, NT chunks at a time: their bit lengths scanned, then decoded
    const uint32_t nw = (uint32_t)(pe - po) / 4;
    const uint32_t *const pw = reinterpret_cast<const uint32_t *>(pay);
#define HBS_WORD(k) ((k) < nw ? bswap32(pw[k]) : 0u)
    uint32_t base = 0;
    int bad = 0;
    for (uint32_t c0 = 0; c0 < nch; c0 += NT) {
        const uint32_t c = c0 + tt;
        const uint32_t clen = c < nch ? A.sync_len[so + c] : 0u;
        uint32_t tot, pos;
        if (WAVE) {   // (all 64 lanes are here: the loop's bounds are wave-uniform)
            const uint32_t incl = wave_scan_incl(clen);
            pos = base + incl - clen;
            tot = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        } else {
            pos = base + wg_scan_excl_u32(clen, L.scan, &tot);
        }
        base += tot;
        if (c >= nch || bad) continue;
        const uint32_t sym0 = c << slog;
        const uint32_t cnt = min(S, len - sym0);
        if (md == 0) {   // stored: 8 bits a symbol
            bad |= clen != 8u * cnt;
            continue;
        }
        uint32_t k = pos >> 5;
        const uint32_t sh = pos & 31u;
        uint64_t win = (((uint64_t)HBS_WORD(k) << 32) | HBS_WORD(k + 1)) << sh;
        int wbits = 64 - (int)sh;
        k += 2;
        uint32_t used = 0;
        const uint32_t row = phase + sym0;
        for (uint32_t j = 0; j < cnt; ++j) {
            if (wbits < 32) {
                win |= (uint64_t)HBS_WORD(k) << (32 - wbits);
                ++k;
                wbits += 32;
            }
            const uint32_t e = L.lut[win >> (64 - HB_LUT_BITS)];
            uint32_t nb = e >> 8, sym = e & 255u;
            if (!nb) {
                nb = hbs_decode_slow((uint32_t)(win >> 32), HB_LUT_BITS + 1u, L, A.nary, A.w, sym);
                if (!nb || sym >= 256u) { bad = 1; break; }   // no code, or the code of no byte
            }
            stage[HB_OIDX(row + j)] = (uint8_t)sym;
            win <<= nb;
            wbits -= (int)nb;
            used += nb;
        }
        if (used != clen) bad = 1;
    }
#undef HBS_WORD
    bad |= base != sb;   // (the chunk lengths must sum to bits)
    if (WAVE) {
        __builtin_amdgcn_wave_barrier();   // the stage is read by other lanes than wrote it
        bad = __any(bad);
    } else {
        if (bad) L.bad = 1;
        __syncthreads();
        bad = L.bad;
    }
    if (bad) {   // nothing of a corrupt segment is written
        if (tt == 0) hb_fail(A.status, A.first, i, DC_E_STREAM);
        return;
    }
    // the stage has the destination's 16-B phase: a byte head, aligned 16-B pieces, a byte tail
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
    const bool tok = hbs_table_ok(T, nary);
    if (tok) {   // (uniform) the decode tables, once for every segment of this workgroup
        for (uint32_t e = t; e < (1u << HB_LUT_BITS); e += HB_THREADS) L.lut[e] = 0;
        for (int q = t; q <= DC_MAX_DIGITS; q += HB_THREADS) {
            L.cnt[q] = T->count[q];
            L.startv[q] = T->first[q];
            L.starti[q] = T->start[q];
        }
        for (int q = t; q < DC_MAX_SYMS; q += HB_THREADS) L.syms[q] = T->syms[q];
        if (t == 0) {
            L.mn = max(T->min_len, 1);
            L.mx = min(T->max_len, DC_MAX_DIGITS);
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
    const HbsDecArgs A{nary, w, S, mode, bits, pay_off, payload, payload_cap, sync_off, sync_len, sync_cap,
                       out, out_beg, out_end, out_cap, status, first};
    const uint64_t groups = (count + 3) / 4;
    for (uint64_t g = blockIdx.x; g < groups; g += gridDim.x) {
        __syncthreads();   // the LDS of the group before (the first time: the tables)
        const uint64_t i0 = 4 * g;
        const uint32_t nseg = (uint32_t)min((uint64_t)4, count - i0);
        if (!tok) {
            if ((uint32_t)t < nseg) hb_fail(status, first, i0 + (uint32_t)t, DC_E_ARG);
            continue;
        }
        bool shortg = true;   // (workgroup-uniform; a range that ends before it starts fails on either path)
        for (uint32_t s = 0; s < nseg; ++s) {
            const uint64_t oa = out_beg[i0 + s], ob = out_end[i0 + s];
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
