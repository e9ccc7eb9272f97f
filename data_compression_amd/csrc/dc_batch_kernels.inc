// dc_batch_kernels.inc -- the batched Huffman codec (dc_huff_encode_batch / dc_huff_decode_batch,
// dc_gpu.h "Huffman batch v1"); included by dc_core.hip after the range decode. Many small
// independent segments, one code table each, a fixed number of launches for any batch:
//   k_hb_plan     one workgroup per segment on a persistent grid: the histogram in LDS, the
//                 lengths and canonical codes by huff_table_body (no dc_dtable written), then the
//                 compact record: lens (u8 x 256), mode, bits, and the segment's payload bytes
//                 and sync entries for the scans
//   k_scan_u64    twice: pay_off and sync_off
//   k_hb_pack     one workgroup per segment: the codes rebuilt from lens, the bit length of
//                 every 16-symbol unit (unit u by thread u % 256: neighbouring lanes read
//                 neighbouring 16 bytes), a workgroup scan, the bits OR-ed into an LDS stage and
//                 stored as whole 16-B pieces (zero pad included); a stored segment is a padded copy
//   k_hb_decode   one workgroup per segment: a 12-bit first-level table and the canonical
//                 arrays from lens; the chunk lengths scanned 256 chunks at a time, chunk c by
//                 thread c % 256, every chunk checked to decode to exactly its bits, into an LDS
//                 stage that has the destination's 16-B phase (4 pad bytes per 128: at S = 64 the
//                 lanes' rows are 16 and 17 dwords apart in turn, two lanes to a bank at worst
//                 where unpadded rows put sixteen), then written as a byte head, 16-B pieces
//                 and a byte tail
// A segment's status goes to status[i]; the lowest failing (index, status) of the call is kept
// in *first (atomicMin) for dc_huff_batch_status.
// What a segment takes once its table is in LDS is here once, for this mode, for the shared-table
// mode (dc_batch_shared_kernels.inc) and for the byte ranges of both (dc_batch_range_kernels.inc):
// hb_pack_seg (the whole of a pack); hb_record_check (the tests of a segment's record) under
// hb_decode_check and hb_range_check; hb_decode_body (the chunk loop, commit and phased write of an
// HbSpan, a whole segment or with RANGE a byte range of one); hb_decode_slow. The kernels differ
// in where the table comes from: k_hb_pack builds it per segment from lens (hb_canonical), k_hb_decode
// and k_hb_decode_ranges likewise (hb_own_tables), the shared kernels copy it once per workgroup.

#define HB_THREADS 256
#define HB_UNIT 16                                   /* symbols per pack work unit (divides S)  */
#define HB_UNITS_MAX (DC_BATCH_SEG_MAX / HB_UNIT)
#define HB_LUT_BITS 12
#define HB_NO_FAIL (~0ull)

static __device__ __forceinline__ void hb_fail(int32_t *__restrict__ status, unsigned long long *__restrict__ first,
                                               uint64_t i, int st)
{
    status[i] = st;
    atomicMin(first, (unsigned long long)((i << 8) | (uint64_t)(uint32_t)(-st)));
}

static __host__ __device__ __forceinline__ uint32_t hb_pad16(uint32_t bytes) { return (bytes + 15u) & ~15u; }

// ---- plan ---------------------------------------------------------------------------------
struct HbPlanLds {
    TblLds tbl;
    uint64_t h64[256];
    uint32_t h[256];
    uint32_t red[4];
};
// three workgroups a CU (hbatch_grid(c, count, 768)): the capped plan's class counts live in
// tbl.startv (huff_table_body's limit stage), so the cap adds nothing here; the 256 B beside the
// struct are what the limit stage's __syncthreads_or takes in the capped kernel
static_assert(sizeof(HbPlanLds) == sizeof(TblLds) + 256 * 12 + 16 && 3 * (sizeof(HbPlanLds) + 256) <= 160 * 1024,
              "k_hb_plan: three workgroups in a CU's 160 KiB of LDS");

// LIMIT (dc_huff_encode_batch_limit): the segment's table is the one capped at max_digits digits
// (huff_table_body<true>); a segment whose distinct bytes outnumber the codes of that length is
// stored under a record of 256 zeros. The unlimited call compiles the body without the stage.
template <bool LIMIT>
__global__ __launch_bounds__(HB_THREADS) void k_hb_plan(const uint8_t *__restrict__ in, const uint64_t *__restrict__ in_off,
                                                        uint64_t count, int nary, uint32_t S, uint8_t *__restrict__ lens,
                                                        uint8_t *__restrict__ mode, uint32_t *__restrict__ bits,
                                                        uint64_t *__restrict__ psize, uint64_t *__restrict__ nchunks,
                                                        int32_t *__restrict__ status, unsigned long long *__restrict__ first,
                                                        int max_digits)
{
    __shared__ HbPlanLds L;
    const int t = threadIdx.x;
    const uint32_t slog = (uint32_t)__builtin_ctz(S);
    for (uint64_t i = blockIdx.x; i < count; i += gridDim.x) {
        __syncthreads();   // the LDS of the segment before
        const uint64_t a = in_off[i], b = in_off[i + 1];
        if (b < a || b - a > DC_BATCH_SEG_MAX) {   // (workgroup-uniform)
            if (t == 0) { psize[i] = 0; nchunks[i] = 0; hb_fail(status, first, i, DC_E_ARG); }
            continue;
        }
        const uint32_t len = (uint32_t)(b - a);
        if (t == 0) status[i] = DC_OK;
        if (len == 0) {   // stored, 0 bytes
            lens[i * 256 + t] = 0;
            if (t == 0) { mode[i] = 0; bits[i] = 0; psize[i] = 0; nchunks[i] = 0; }
            continue;
        }
        L.h[t] = 0;
        __syncthreads();
        {   // the histogram: a byte head up to 4-B alignment, dwords, a byte tail (u32 counters:
            // 65536 equal bytes pass a u16)
            const uint8_t *p = in + a;
            const uint32_t mis = (uint32_t)(-(uintptr_t)p) & 3u;
            const uint32_t head = mis < len ? mis : len;
            if ((uint32_t)t < head) atomicAdd(&L.h[p[t]], 1u);
            const uint32_t nw = (len - head) >> 2;
            const uint32_t *pw = reinterpret_cast<const uint32_t *>(p + head);
            for (uint32_t k = t; k < nw; k += HB_THREADS) {
                const uint32_t v = pw[k];
                atomicAdd(&L.h[v & 255u], 1u);
                atomicAdd(&L.h[(v >> 8) & 255u], 1u);
                atomicAdd(&L.h[(v >> 16) & 255u], 1u);
                atomicAdd(&L.h[v >> 24], 1u);
            }
            const uint32_t tail = head + 4 * nw + (uint32_t)t;
            if (tail < len) atomicAdd(&L.h[p[tail]], 1u);
        }
        __syncthreads();
        L.h64[t] = L.h[t];
        __syncthreads();
        // lengths and canonical codes of symbols 0..258 exactly as k_huff_table (dc_huff_table)
        if constexpr (LIMIT) {
            // inlined as the unlimited body is here (the compiler leaves a body with two callers out of
            // line): the constant arguments drop the dc_dtable, tree and plan halves of it
            [[clang::always_inline]] huff_table_body<true>(L.tbl, L.h64, 1, nullptr, 258, nary, nullptr, nullptr, nullptr,
                                                           nullptr, nullptr, nullptr, max_digits);
        } else {
            huff_table_body(L.tbl, L.h64, 1, nullptr, 258, nary, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
        }
        uint32_t v = L.h[t] * L.tbl.nb[t];   // <= 65536 * 32
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
        if ((t & 63) == 0) L.red[t >> 6] = v;
        // (LIMIT: bad is a failed repair, n^D < k; what the body then left in len is no code)
        lens[i * 256 + t] = (LIMIT && L.tbl.bad) ? (uint8_t)0 : (uint8_t)L.tbl.len[t];
        __syncthreads();
        if (t == 0) {
            const uint32_t cb = L.red[0] + L.red[1] + L.red[2] + L.red[3];
            const bool huff = !L.tbl.bad && L.tbl.maxbits <= 32 && cb < 8u * len;
            const uint32_t sb = huff ? cb : 8u * len;
            mode[i] = huff ? 1 : 0;
            bits[i] = sb;
            psize[i] = hb_pad16((sb + 7u) >> 3);
            nchunks[i] = (len + S - 1) >> slog;
        }
    }
}

// ---- the canonical code of a lens record -----------------------------------------------------
// (convert_lengths_to_encode_table on lengths 0..255, symbols 256..258 at length 0: the first
// value per length is n * (first + count) of the length below, u32 wrapping as the table kernel;
// a symbol's value is its length's first value plus its rank among the symbols of that length)
struct HbCode {
    uint32_t code[256];    // packed MSB-first bits (pack)
    uint32_t nb[256];      // bit length; 0: no code, or a code over 32 bits
    uint32_t cnt[DC_MAX_DIGITS + 2], startv[DC_MAX_DIGITS + 2], starti[DC_MAX_DIGITS + 2];
    uint8_t len[256];
    uint8_t syms[256];     // symbols by (length, value)
    int mn, mx, bad;       // bad: a length over DC_MAX_DIGITS, or a code over 32 bits
};

// 256 threads; ends with a barrier
static __device__ void hb_canonical(HbCode &C, const uint8_t *__restrict__ lens, int nary, int w)
{
    const int t = threadIdx.x;
    const int Lt = lens[t];
    C.len[t] = (uint8_t)Lt;
    if (t < DC_MAX_DIGITS + 2) C.cnt[t] = 0;
    if (t == 0) { C.mn = 300; C.mx = 0; C.bad = 0; }
    __syncthreads();
    const bool coded = Lt > 0 && Lt <= DC_MAX_DIGITS;
    if (Lt > DC_MAX_DIGITS) C.bad = 1;
    if (coded) { atomicAdd(&C.cnt[Lt], 1u); atomicMin(&C.mn, Lt); atomicMax(&C.mx, Lt); }
    __syncthreads();
    if (t == 0) {
        uint32_t v = 0, si = 0;
        for (int L = C.mn; L <= C.mx; ++L) {
            C.startv[L] = v;
            C.starti[L] = si;
            v = (v + C.cnt[L]) * (uint32_t)nary;
            si += C.cnt[L];
        }
    }
    __syncthreads();
    uint32_t code = 0, nb = 0;
    if (coded) {
        uint32_t rank = 0;
        for (int i = 0; i < t; ++i) rank += (C.len[i] == Lt);   // (an LDS broadcast per step)
        const uint32_t val = C.startv[Lt] + rank;
        C.syms[C.starti[Lt] + rank] = (uint8_t)t;
        if (Lt * w <= 32) {
            uint64_t packed = 0;
            if ((nary & (nary - 1)) == 0) {
                packed = (Lt * w >= 32) ? (uint64_t)val : ((uint64_t)val & ((1ull << (Lt * w)) - 1));
            } else {
                uint32_t x = val;
                for (int d = 0; d < Lt; ++d) {
                    packed |= (uint64_t)(x % (uint32_t)nary) << (w * d);
                    x /= (uint32_t)nary;
                }
            }
            code = (uint32_t)packed;
            nb = (uint32_t)(Lt * w);
        } else {
            C.bad = 1;
        }
    }
    C.code[t] = code;
    C.nb[t] = nb;
    __syncthreads();
}

// ---- pack -------------------------------------------------------------------------------------
// the LDS a segment is packed in, beside the code table of the kernel that packs it
struct HbPackWork {
    __attribute__((aligned(16))) uint32_t stage[DC_BATCH_SEG_MAX / 4];   // the payload, word bit 31 first
    uint16_t ulen[HB_UNITS_MAX];   // bits per 16-symbol unit
    uint32_t tbase[HB_THREADS];    // bit offset of unit 16 t
    uint32_t scan[4];
};
static_assert(HB_UNITS_MAX == 16 * HB_THREADS, "the unit scan gives every thread 16 units");

struct HbPackLds {
    HbPackWork P;
    HbCode C;
};

// bytes p[at .. at + 16) of a segment of len bytes (at < len) as 4 little-endian dwords, by
// aligned dword loads: only dwords that hold a byte of the segment are read; the bytes at and
// past len are unspecified
static __device__ __forceinline__ void hb_load16(const uint8_t *__restrict__ p, uint32_t at, uint32_t len, uint32_t q[4])
{
    const uint8_t *const s = p + at, *const end = p + len;
    const uint32_t a = (uint32_t)(uintptr_t)s & 3u;
    const uint32_t *const w = reinterpret_cast<const uint32_t *>(s - a);
    uint32_t d[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) d[j] = reinterpret_cast<const uint8_t *>(w + j) < end ? w[j] : 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) q[j] = __builtin_amdgcn_alignbyte(d[j + 1], d[j], a);
}

// segment i (status DC_OK by its plan) by the whole workgroup, under the byte codes code[] / nb[]
// (nb 0: no code) that the caller has ready in LDS; a stored segment reads neither. Every barrier
// is reached by the whole workgroup: the tests before one are uniform.
static __device__ __forceinline__ void hb_pack_seg(
    HbPackWork &P, const uint32_t (&code)[256], const uint32_t (&nb)[256], uint64_t i, const uint8_t *__restrict__ in,
    const uint64_t *__restrict__ in_off, uint32_t S, const uint8_t *__restrict__ mode, const uint64_t *__restrict__ pay_off,
    uint8_t *__restrict__ payload, uint64_t payload_cap, const uint64_t *__restrict__ sync_off, uint16_t *__restrict__ sync_len,
    uint64_t sync_cap, int32_t *__restrict__ status, unsigned long long *__restrict__ first)
{
    const int t = threadIdx.x;
    const uint32_t slog = (uint32_t)__builtin_ctz(S);
    const uint64_t a = in_off[i];
    const uint32_t len = (uint32_t)(in_off[i + 1] - a);
    const uint64_t po = pay_off[i], pe = pay_off[i + 1], so = sync_off[i], se = sync_off[i + 1];
    if (pe > payload_cap || se > sync_cap) {
        if (t == 0) hb_fail(status, first, i, DC_E_CAPACITY);
        return;
    }
    if (len == 0) return;
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
        return;
    }
    for (uint32_t k = t; k < psz / 4; k += HB_THREADS) P.stage[k] = 0;
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
            if (k < cntu) ub += nb[(q[k >> 2] >> (8 * (k & 3))) & 255u];
        P.ulen[u] = (uint16_t)ub;   // <= 16 * 32
    }
    __syncthreads();
    uint32_t tsum = 0;
    for (uint32_t u = 16 * (uint32_t)t; u < min(16 * (uint32_t)t + 16, units); ++u) tsum += P.ulen[u];
    uint32_t total;
    P.tbase[t] = wg_scan_excl_u32(tsum, P.scan, &total);
    __syncthreads();
    {   // the sync index: chunk c = units [c r, (c + 1) r), r = S / 16
        const uint32_t r = S / HB_UNIT;
        for (uint32_t c = t; c < nch; c += HB_THREADS) {
            const uint32_t e = min((c + 1) * r, units);
            uint32_t cb = 0;
            for (uint32_t u = c * r; u < e; ++u) cb += P.ulen[u];
            sync_len[so + c] = (uint16_t)cb;   // <= 1024 * 32
        }
    }
    for (uint32_t u = t; u < units; u += HB_THREADS) {
        uint32_t pos = P.tbase[u >> 4];
        for (uint32_t k = u & ~15u; k < u; ++k) pos += P.ulen[k];
        uint32_t q[4];
        hb_load16(p, u * HB_UNIT, len, q);
        const uint32_t cntu = min((uint32_t)HB_UNIT, len - u * HB_UNIT);
        // a 64-bit accumulator, whole words OR-ed into the stage (neighbours share words)
        uint32_t wi = pos >> 5, nacc = pos & 31u;
        uint64_t acc = 0;
#pragma unroll
        for (uint32_t k = 0; k < HB_UNIT; ++k) {
            if (k < cntu) {
                const uint32_t b = (q[k >> 2] >> (8 * (k & 3))) & 255u, n = nb[b];
                if (n) acc |= (uint64_t)code[b] << (64u - nacc - n);
                nacc += n;
                if (nacc >= 32u) {
                    if (wi < DC_BATCH_SEG_MAX / 4) atomicOr(&P.stage[wi], (uint32_t)(acc >> 32));
                    ++wi;
                    acc <<= 32;
                    nacc -= 32u;
                }
            }
        }
        if (nacc && wi < DC_BATCH_SEG_MAX / 4) atomicOr(&P.stage[wi], (uint32_t)(acc >> 32));
    }
    __syncthreads();
    for (uint32_t v = t; v < psz / 16; v += HB_THREADS) {
        const uint4 q = reinterpret_cast<const uint4 *>(P.stage)[v];
        dst[v] = make_uint4(bswap32(q.x), bswap32(q.y), bswap32(q.z), bswap32(q.w));
    }
}

__global__ __launch_bounds__(HB_THREADS) void k_hb_pack(const uint8_t *__restrict__ in, const uint64_t *__restrict__ in_off,
                                                        uint64_t count, int nary, int w, uint32_t S,
                                                        const uint8_t *__restrict__ lens, const uint8_t *__restrict__ mode,
                                                        const uint64_t *__restrict__ pay_off, uint8_t *__restrict__ payload,
                                                        uint64_t payload_cap, const uint64_t *__restrict__ sync_off,
                                                        uint16_t *__restrict__ sync_len, uint64_t sync_cap,
                                                        int32_t *__restrict__ status, unsigned long long *__restrict__ first)
{
    __shared__ HbPackLds L;
    for (uint64_t i = blockIdx.x; i < count; i += gridDim.x) {
        __syncthreads();   // the LDS of the segment before
        if (status[i] != DC_OK) continue;   // (DC_E_ARG by the plan; uniform)
        if (mode[i] != 0) hb_canonical(L.C, lens + i * 256, nary, w);   // (uniform; a stored segment has no use for codes)
        hb_pack_seg(L.P, L.C.code, L.C.nb, i, in, in_off, S, mode, pay_off, payload, payload_cap, sync_off, sync_len, sync_cap,
                    status, first);
    }
}

// ---- decode -----------------------------------------------------------------------------------
// byte k of a segment is staged at out[HB_OIDX(phase + k)]: 4 pad bytes after every 128
#define HB_OIDX(pos) ((pos) + 4u * ((pos) >> 7))
#define HB_STAGE_BYTES (DC_BATCH_SEG_MAX + 16 + 4 * (DC_BATCH_SEG_MAX / 128 + 1))

// What hb_decode_body wants of a decode kernel's LDS: lut, scan, bad, and in C
// the canonical arrays cnt / startv / starti / syms / mn / mx of hb_decode_slow.
struct HbDecLds {
    __attribute__((aligned(16))) uint8_t out[HB_STAGE_BYTES];
    uint16_t lut[1 << HB_LUT_BITS];   // next 12 bits -> sym | bits << 8; 0: longer, or no code
    HbCode C;
    uint32_t scan[4];
    int bad;
};

// what every decode kernel takes of the batch, its output and the call
struct HbDecArgs {
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
    const uint64_t *out_beg, *out_end;   // whole segments (the two may alias: d_out_off, d_out_off + 1); ranges: null
    uint64_t out_cap;
    int32_t *status;
    unsigned long long *first;
};

// the symbol whose code leads the 32-bit window `win` (MSB first), by the canonical arrays of C
// (HbCode, or the shared mode's copy of a dc_dtable's): its bit length, 0 when no code of
// lo .. maxbits bits matches (lo: bits the caller has ruled out already are not tested again).
// syms is indexed under a mask of its size: HbCode's starti + r is below 256 by construction, a
// table that another kernel built is not trusted that far.
template <class Canon>
static __device__ __forceinline__ uint32_t hb_decode_slow(uint32_t win, uint32_t lo, uint32_t maxbits, const Canon &C,
                                                          int nary, int w, uint32_t &sym)
{
    constexpr uint32_t smask = sizeof(C.syms) / sizeof(C.syms[0]) - 1u;
    static_assert((smask & (smask + 1u)) == 0, "syms holds a power of two of symbols");
    const int top = C.mx;
    if ((nary & (nary - 1)) == 0) {   // n = 2^w: the value of the first L digits is the first L w bits
        int L = C.mn;
        while ((uint32_t)(L * w) < lo) ++L;
        for (; L <= top && (uint32_t)(L * w) <= maxbits; ++L) {
            const uint32_t r = (win >> (32 - L * w)) - C.startv[L];
            if (r < C.cnt[L]) {
                sym = C.syms[(C.starti[L] + r) & smask];
                return (uint32_t)(L * w);
            }
        }
        return 0;
    }
    uint32_t v = 0;
    const uint32_t dmask = (1u << w) - 1u;
    for (int L = 1; L <= top && (uint32_t)(L * w) <= maxbits; ++L) {
        const uint32_t d = (win >> (32 - L * w)) & dmask;
        if (d >= (uint32_t)nary) return 0;
        v = v * (uint32_t)nary + d;
        if (L >= C.mn && (uint32_t)(L * w) >= lo) {
            const uint32_t r = v - C.startv[L];
            if (r < C.cnt[L]) {
                sym = C.syms[(C.starti[L] + r) & smask];
                return (uint32_t)(L * w);
            }
        }
    }
    return 0;
}

// What hb_decode_body decodes: a segment that passed hb_decode_check, or the byte range of one
// that passed hb_range_check (dc_batch_range_kernels.inc).
struct HbSpan {
    uint64_t seg;            // the segment's number
    uint32_t len, md, sb;    // its output bytes, mode and bits
    uint64_t po, pe, so;     // its payload bytes [po, pe), its first sync entry
    uint32_t c_lo, c_hi;     // the chunks decoded: all of them, or those a range touches
    uint32_t first, count;   // the bytes [first, first + count) staged and written: all len, or a range (count > 0)
    uint8_t *dptr;           // where they go
};

// The record of segment `seg` of len output bytes: its mode and bits, its payload bytes and its sync
// entries against len, as both checks test them. Writes no status; with true, G is the whole
// segment but for dptr. FILL_LATE: G is written only when the tests pass, else before their outcome
// is used. Both give the same G to a caller that reads it only after true; which one the compiler
// sees decides how it lays out the kernel around the call. k_hbs_decode takes true: it then
// compiles to the instructions it had when segments and ranges had a body each. The other three
// kernels take false: they measured 0.5 to 2 % slower with true
// (profiles/batch_decode_span_forms.log, the late_fill runs).
template <bool FILL_LATE>
static __device__ __forceinline__ bool hb_record_check(const HbDecArgs &A, uint64_t seg, uint32_t len, HbSpan &G)
{
    const uint32_t S = A.S, slog = (uint32_t)__builtin_ctz(S);
    const uint32_t md = A.mode[seg], sb = A.bits[seg];
    const uint64_t po = A.pay_off[seg], pe = A.pay_off[seg + 1], so = A.sync_off[seg], se = A.sync_off[seg + 1];
    const uint32_t nch = (len + S - 1) >> slog;
    bool ok = md <= 1u && sb <= 8u * len && (md == 1u || sb == 8u * len);
    ok = ok && pe >= po && pe <= A.payload_cap && (po & 15u) == 0 && pe - po == hb_pad16((sb + 7u) >> 3);
    ok = ok && se >= so && se <= A.sync_cap && se - so == nch;
    if (FILL_LATE && !ok) return false;
    G = HbSpan{seg, len, md, sb, po, pe, so, 0u, nch, 0u, len, nullptr};
    return ok;
}

// Segment i by the threads that call it (tt: the caller's index among them), a workgroup or a
// wave: every test is uniform among them, and no barrier is reached. Validates the output range,
// then the cap, then the stream's record, and writes the segment's status; with DC_OK it clears
// *flag when the caller gives one (a workgroup's commit flag, see hb_decode_body). true: G is a
// segment for hb_decode_body (false: it failed, or has 0 bytes).
template <bool FILL_LATE>
static __device__ __forceinline__ bool hb_decode_check(const HbDecArgs &A, uint64_t i, uint32_t tt, HbSpan &G, int *flag)
{
    const uint64_t oa = A.out_beg[i], ob = A.out_end[i];
    if (ob < oa || ob - oa > DC_BATCH_SEG_MAX) {
        if (tt == 0) hb_fail(A.status, A.first, i, DC_E_ARG);
        return false;
    }
    if (ob > A.out_cap) {
        if (tt == 0) hb_fail(A.status, A.first, i, DC_E_CAPACITY);
        return false;
    }
    if (!hb_record_check<FILL_LATE>(A, i, (uint32_t)(ob - oa), G)) {
        if (tt == 0) hb_fail(A.status, A.first, i, DC_E_STREAM);
        return false;
    }
    if (tt == 0) {
        A.status[i] = DC_OK;
        if (flag) *flag = 0;
    }
    G.dptr = A.out + oa;
    return G.len != 0;
}

// The span G (segment or range number i: where its status goes) staged at `stage`, by the NT
// threads that its check ran on; for a mode-1 segment L.lut and L.C hold its code. The whole
// workgroup (WAVE false: every barrier below is reached by all of it, every test before one is
// uniform, and the caller has cleared L.bad, the commit flag, after the barrier that ended the span
// before), or one wave (WAVE true: wave-uniform tests, no workgroup barrier, L.bad not used).
// Byte k of the span is staged at HB_OIDX(phase + k).
// RANGE false, a whole segment (c_lo, first = 0, count = len; status DC_OK by hb_decode_check):
// every symbol is staged, and the chunk lengths must sum to bits. RANGE true, a byte range: the
// u16 entries before c_lo are summed for its bit position (strided reads, a wave or workgroup
// reduce), every touched chunk is decoded whole and checked to take exactly its bits, only the
// symbols of [first, first + count) are staged, the last touched chunk must end within bits, and
// DC_OK is written at the commit.
template <bool WAVE, bool RANGE, class Lds>
static __device__ __forceinline__ void hb_decode_body(Lds &L, uint8_t *stage, const HbDecArgs &A, uint64_t i, uint32_t tt,
                                                      const HbSpan &G)
{
    constexpr uint32_t NT = WAVE ? 64u : (uint32_t)HB_THREADS;
    const uint32_t S = A.S, slog = (uint32_t)__builtin_ctz(S);
    const uint32_t md = G.md, c_lo = RANGE ? G.c_lo : 0u, c_hi = G.c_hi;
    const uint32_t lo = RANGE ? G.first : 0u, n = RANGE ? G.count : G.len, hi = lo + n;
    uint8_t *const dptr = G.dptr;
    const uint32_t phase = (uint32_t)(uintptr_t)dptr & 15u;
    const uint8_t *const pay = A.payload + G.po;
    const uint16_t *const sl = A.sync_len + G.so;
    if (md == 0)   // (lo + k < len <= bits / 8: inside the payload)
        for (uint32_t k = tt; k < n; k += NT) stage[HB_OIDX(phase + k)] = pay[lo + k];
    uint32_t base = 0;
    if (RANGE) {   // the bit position of chunk c_lo: the entries before it (<= 4096 of <= 65535 each)
        uint32_t before = 0;
#pragma unroll 4
        for (uint32_t c = tt; c < c_lo; c += NT) before += sl[c];
        if (WAVE) {
            base = (uint32_t)__builtin_amdgcn_readlane((int)wave_scan_incl(before), 63);
        } else {
            wg_scan_excl_u32(before, L.scan, &base);
        }
    }
    // chunk c by thread (c - c_lo) % NT, NT chunks at a time: their bit lengths scanned, then decoded
    const uint32_t nw = (uint32_t)(G.pe - G.po) / 4;
    const uint32_t *const pw = reinterpret_cast<const uint32_t *>(pay);
#define HB_WORD(k) ((k) < nw ? bswap32(pw[k]) : 0u)
    int bad = 0;
    for (uint32_t c0 = c_lo; c0 < c_hi; c0 += NT) {
        const uint32_t c = c0 + tt;
        const uint32_t clen = c < c_hi ? sl[c] : 0u;
        uint32_t tot, pos;
        if (WAVE) {   // (all 64 lanes are here: the loop's bounds are wave-uniform)
            const uint32_t incl = wave_scan_incl(clen);
            pos = base + incl - clen;
            tot = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        } else {
            pos = base + wg_scan_excl_u32(clen, L.scan, &tot);
        }
        base += tot;
        if (c >= c_hi || bad) continue;
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
        const uint32_t row = phase + sym0 - lo;   // (a range: only used where sym0 + j >= lo)
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
                if (!nb || sym >= 256u) { bad = 1; break; }   // no code, or the code of no byte (a dc_dtable's symbol >= 256)
            }
            // (a range: only its first and last touched chunk hold symbols outside it)
            if (!RANGE || (sym0 + j >= lo && sym0 + j < hi)) stage[HB_OIDX(row + j)] = (uint8_t)sym;
            win <<= nb;
            wbits -= (int)nb;
            used += nb;
        }
        if (used != clen) bad = 1;
    }
#undef HB_WORD
    // base: a segment's chunk lengths must sum to bits; a range's last touched chunk must end within them
    bool fail;   // (the test is written in each branch: hoisted into one bool before them, k_hbs_decode
                 // no longer compiles to the instructions it had, see hb_record_check)
    if (WAVE) {
        __builtin_amdgcn_wave_barrier();   // the stage is read by other lanes than wrote it
        fail = __any(bad || (RANGE ? base > G.sb : base != G.sb));
    } else {
        if (bad || (RANGE ? base > G.sb : base != G.sb)) L.bad = 1;
        __syncthreads();
        fail = L.bad != 0;
    }
    if (fail) {   // nothing of a corrupt segment, or of a range with a corrupt chunk, is written
        if (tt == 0) hb_fail(A.status, A.first, i, DC_E_STREAM);
        return;
    }
    if (RANGE && tt == 0) A.status[i] = DC_OK;
    // the stage has the destination's 16-B phase: a byte head, aligned 16-B pieces, a byte tail
    const uint32_t head = min((16u - phase) & 15u, n);
    if (tt < head) dptr[tt] = stage[HB_OIDX(phase + tt)];
    const uint32_t nbody = (n - head) >> 4;
    for (uint32_t v = tt; v < nbody; v += NT) {   // (a piece never crosses a pad: 16 divides 128)
        const uint32_t *const q = reinterpret_cast<const uint32_t *>(stage + HB_OIDX(phase + head + 16 * v));
        *reinterpret_cast<uint4 *>(dptr + head + 16 * v) = make_uint4(q[0], q[1], q[2], q[3]);
    }
    const uint32_t tail = head + 16 * nbody + tt;
    if (tail < n) dptr[tail] = stage[HB_OIDX(phase + tail)];
}

// The code of a lens record in L, by the whole workgroup (t: threadIdx.x): the canonical arrays,
// then the 12-bit table; ends with a barrier. false: the lengths are no code (L.C.bad stays set,
// no table is filled).
static __device__ __forceinline__ bool hb_own_tables(HbDecLds &L, const uint8_t *__restrict__ lens, int nary, int w, int t)
{
    hb_canonical(L.C, lens, nary, w);
    if (L.C.bad) return false;   // (uniform: read after hb_canonical's barrier)
    for (uint32_t e = t; e < (1u << HB_LUT_BITS); e += HB_THREADS) {
        uint32_t sym = 0;
        const uint32_t nb = hb_decode_slow(e << (32 - HB_LUT_BITS), 1u, HB_LUT_BITS, L.C, nary, w, sym);
        L.lut[e] = (uint16_t)(nb ? (sym | (nb << 8)) : 0u);
    }
    __syncthreads();
    return true;
}

__global__ __launch_bounds__(HB_THREADS) void k_hb_decode(HbDecArgs A, uint64_t count, const uint8_t *__restrict__ lens)
{
    __shared__ HbDecLds L;
    const int t = threadIdx.x;
    for (uint64_t i = blockIdx.x; i < count; i += gridDim.x) {
        __syncthreads();   // the LDS of the segment before
        HbSpan G;
        if (!hb_decode_check<false>(A, i, (uint32_t)t, G, &L.bad)) continue;   // (uniform, as every test below)
        // the table only now: a segment with a bad range or record has its status already
        if (G.md == 1u && !hb_own_tables(L, lens + i * 256, A.nary, A.w, t)) {
            if (t == 0) hb_fail(A.status, A.first, i, DC_E_STREAM);
            continue;
        }
        hb_decode_body<false, false>(L, L.out, A, i, (uint32_t)t, G);
    }
}
