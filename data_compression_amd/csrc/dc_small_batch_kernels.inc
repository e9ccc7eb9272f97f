// dc_small_batch_kernels.inc -- small batch v1 (dc_gpu.h): many independent buffers, each coded as
// the small front-end's stream of that buffer alone (small_compression.c:582-665), back to back,
// and the asynchronous decode of such a batch. Included by dc_core.hip after
// dc_nyb_batch_kernels.inc (swar_eq / swar_lower, the DPP wave shifts and scans; bs_item /
// bs_report: the per-buffer frame, status[i] and the context's first-failure slot).
//
// Whether position i starts a pair depends on x[i] and x[i + 1] alone (' ' then a..z, i >= 1; a
// letter is never ' ', so pairs cannot overlap): the encode is a stream compaction, the decode a
// stream expansion, and a whole wave works inside one buffer. ONE WAVE PER BUFFER, SB_WAVES waves
// a workgroup on a persistent grid, buffers taken in a fixed stride: 64 unequal buffers do not
// wait for the longest one. A buffer is walked in wave tiles of 64 lanes x 16 B (sb_walk).
//
//   k_small_batch_len   P (pair starts) of every buffer -> its stream's length
//   k_scan_u64          the lengths -> d_out_off
//   k_small_batch_enc   the stream straight to its final place (len + 1 bytes: the LITERAL form)
//   k_small_batch_dec   one launch: the decoded length is counted first, and bytes are written
//                       only when it is the length asked for
//
// Loads: 16-B granules from the aligned address below x[0]; bytes outside the buffer are zeroed
// before any test (sb_load), so the right neighbour of a buffer's last byte and the left neighbour
// of its first are never another buffer's bytes (0 is neither ' ' nor a letter). The neighbour
// bytes of a lane's 16 come from the adjacent lanes (DPP wave shifts); across tiles the left one is
// carried (the last byte of the tile before) and the right one is the first byte of the next
// tile's granules, which are loaded a tile ahead anyway.
// Stores: the kept bytes are compacted into the wave's LDS stage at the destination's 16-B phase
// and leave it as whole 16-B granules where the stream owns the granule, bytes only in a stream's
// first and last partial granule (sb_flush): neighbouring streams are written by other waves at
// the same time, and a read-modify-write of a shared granule would be a race.

#define SB_WAVES 4
#define SB_THREADS (64 * SB_WAVES)
#define SB_TILE 1024u                      /* input bytes per wave tile: 64 lanes x 16 B       */
#define SB_STAGE (2u * SB_TILE + 32u)      /* the decode doubles a tile at most; + carry + phase */
#define SB_PRUNED 8u                       /* EIGHT_BIT_PRUNED, small_compression.c:39           */

// one buffer x[0 .. n) as its wave sees it (wave-uniform)
struct SbBuf {
    const uint4 *g;   // the granule that holds x[0]
    uint32_t sh;      // x[0]'s byte in it
    uint64_t n;
    uint64_t ng;      // granules that hold bytes of x (0 for n = 0)
};
static __device__ __forceinline__ SbBuf sb_buf(const uint8_t *x, uint64_t n)
{
    SbBuf B;
    B.sh = (uint32_t)((uintptr_t)x & 15u);
    B.g = reinterpret_cast<const uint4 *>(x - B.sh);
    B.n = n;
    B.ng = n ? (B.sh + n + 15) / 16 : 0;
    return B;
}

// Bytes k of the dword at byte u with u + k >= lim / < lim, as bit 7 of each byte. The distance
// is clamped as a signed number and the shift is 64 bits wide, so no case needs a select of its
// own. (swar_ge / swar_lt, inlined here with lim = sh + 1 and sh + 2 side by side, were compiled
// without their lim > u test for the second: every dword past the threshold lost its bytes.)
static __device__ __forceinline__ uint32_t sb_ge(uint32_t u, uint32_t lim)
{
    const int a = min(max((int)lim - (int)u, 0), 4);   // leading bytes below lim
    return (uint32_t)(0x80808080ull << (8 * a));
}
static __device__ __forceinline__ uint32_t sb_lt(uint32_t u, uint32_t lim)
{
    const int b = min(max((int)lim - (int)u, 0), 4);   // bytes below lim
    return (uint32_t)(0x80808080ull >> (8 * (4 - b)));
}
// 0xFF in the bytes k of the dword at granule byte u with lo <= u + k < hi
static __device__ __forceinline__ uint32_t sb_inside(uint32_t u, uint32_t lo, uint32_t hi)
{
    const uint32_t m = sb_ge(u, lo) & sb_lt(u, hi);
    return (m - (m >> 7)) | m;   // 0x80 -> 0xFF per byte
}

// granule gi of the buffer, the bytes outside x[0 .. n) zeroed; zeros past the last granule
static __device__ __forceinline__ uint4 sb_load(const SbBuf &B, uint64_t gi)
{
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (gi < B.ng) {
        v = B.g[gi];
        if (gi == 0 || gi + 1 == B.ng) {
            const uint32_t lo = gi == 0 ? B.sh : 0u;
            const uint64_t e = B.sh + B.n - gi * 16;   // (> 0: the granule holds bytes)
            const uint32_t hi = e < 16 ? (uint32_t)e : 16u;
            v.x &= sb_inside(0, lo, hi);
            v.y &= sb_inside(4, lo, hi);
            v.z &= sb_inside(8, lo, hi);
            v.w &= sb_inside(12, lo, hi);
        }
    }
    return v;
}

// a tile's bounds in tile bytes u = 16 lane + k (uniform): buffer byte index = tile * SB_TILE + u - sh
struct SbTile {
    uint32_t lo, hi;    // the buffer's bytes: u in [lo, hi)
    uint32_t one, two;  // u >= one / two <=> byte index >= 1 / 2
    bool interior;      // lo = one = two = 0 and hi = SB_TILE
};

// fn(T, d, p, q, last) per wave tile: d = the lane's 16 bytes, p / q = the bytes before / after
// them (0 outside the buffer). Every lane of the wave calls it; the next tile's granules are in
// flight while fn works on this one.
template <class Fn> static __device__ __forceinline__ void sb_walk(const SbBuf &B, int lane, Fn fn)
{
    const uint64_t ntiles = (B.ng + 63) / 64;
    uint4 cur = sb_load(B, (uint64_t)lane);
    uint32_t left = 0;   // the last byte of the tile before
    for (uint64_t t = 0; t < ntiles; ++t) {
        const uint4 nxt = sb_load(B, (t + 1) * 64 + (uint64_t)lane);
        SbTile T;
        const uint64_t e = B.sh + B.n - t * SB_TILE;
        T.lo = t ? 0u : B.sh;
        T.hi = e < SB_TILE ? (uint32_t)e : SB_TILE;
        T.one = t ? 0u : B.sh + 1u;
        T.two = t ? 0u : B.sh + 2u;
        T.interior = t && T.hi == SB_TILE;
        uint32_t p = dpp_wave_shr1(cur.w) >> 24;    // (statements of their own: every lane active)
        uint32_t q = dpp_wave_shl1(cur.x) & 255u;
        const uint32_t first_next = (uint32_t)__builtin_amdgcn_readlane((int)nxt.x, 0) & 255u;
        if (lane == 0) p = left;
        if (lane == 63) q = first_next;
        fn(T, cur, p, q, t + 1 == ntiles);
        left = (uint32_t)__builtin_amdgcn_readlane((int)cur.w, 63) >> 24;
        cur = nxt;
    }
}

// Encode, the lane's 16 bytes at tile byte u0 = 16 lane: val = the output byte of each position
// (' ' + letter -> 0x80 + letter at the pair's START), keep = the positions that emit one (bit 7
// of each byte; all but a pair's second), *pairs += the pair starts. Returns the bytes kept.
static __device__ __forceinline__ uint32_t sb_classify(const SbTile &T, const uint4 &c, uint32_t p, uint32_t q, int lane,
                                                       uint32_t (&val)[4], uint32_t (&keep)[4], uint32_t &pairs)
{
    const uint32_t d[4] = {c.x, c.y, c.z, c.w};
    uint32_t cnt = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t u = (uint32_t)lane * 16u + 4u * j;
        const uint32_t prev = (d[j] << 8) | (j ? d[j - 1] >> 24 : p);
        const uint32_t next = (d[j] >> 8) | ((j < 3 ? d[j + 1] & 255u : q) << 24);
        uint32_t valid = 0x80808080u;
        uint32_t start = swar_eq(d[j], 0x20202020u) & swar_lower(next);    // (the byte after the buffer is 0: no letter)
        uint32_t second = swar_eq(prev, 0x20202020u) & swar_lower(d[j]);
        if (!T.interior) {
            valid = sb_ge(u, T.lo) & sb_lt(u, T.hi);
            start &= sb_ge(u, T.one);     // no pair starts at byte 0 ...
            second &= sb_ge(u, T.two);    // ... so byte 1 is no pair's second
        }
        const uint32_t m8 = (start - (start >> 7)) | start;   // 0x80 -> 0xFF per byte
        val[j] = (d[j] & ~m8) | ((next | 0x80808080u) & m8);
        keep[j] = valid & ~second;
        cnt += (uint32_t)__popc(keep[j]);
        pairs += (uint32_t)__popc(start);
    }
    return cnt;
}

static __device__ __forceinline__ uint64_t sb_wave_sum(uint64_t v)
{
    v = wave_scan_incl_u64(v);
    return ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), 63) << 32) |
           (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, 63);
}

// A wave's output through its stage. Stage byte s is destination byte G + s (G 16-B aligned);
// [lo, fill) are the stream's bytes not yet sent (lo < 16: the stream's first granule may begin
// inside it), `room` the bytes the stream may still send.
struct SbOut {
    uint8_t *G;
    uint32_t lo, fill;
    uint64_t room;
};
static __device__ __forceinline__ SbOut sb_out(uint8_t *dst, uint64_t room)
{
    SbOut O;
    O.lo = O.fill = (uint32_t)((uintptr_t)dst & 15u);
    O.G = dst - O.lo;
    O.room = room;
    return O;
}

// Sends the stage's whole granules (every byte when `last`) and moves the rest to the stage's
// front. Whole 16-B stores where [lo, hi) covers the granule, bytes elsewhere: never a byte outside
// the stream's own range, never more than `room`.
static __device__ __forceinline__ void sb_flush(uint8_t *stage, SbOut &O, bool last, int lane)
{
    __builtin_amdgcn_wave_barrier();   // the stage is read by other lanes than wrote it
    if (O.fill - O.lo > O.room) O.fill = O.lo + (uint32_t)O.room;
    const uint32_t lo = O.lo, hi = last ? O.fill : O.fill & ~15u;
    if (hi <= lo) return;
    for (uint32_t s = 16u * (uint32_t)lane; s < hi; s += SB_TILE) {
        if (s >= lo && s + 16u <= hi) {
            *reinterpret_cast<uint4 *>(O.G + s) = *reinterpret_cast<const uint4 *>(stage + s);
        } else {
            const uint32_t k1 = min(s + 16u, hi);
            for (uint32_t k = max(s, lo); k < k1; ++k) O.G[k] = stage[k];
        }
    }
    O.room -= hi - lo;
    if (last) return;
    // (hi is a multiple of 16 above lo: the carry, fewer than 16 bytes, goes to the front)
    __builtin_amdgcn_wave_barrier();
    if (lane == 0) {
        const uint4 r = *reinterpret_cast<const uint4 *>(stage + hi);
        *reinterpret_cast<uint4 *>(stage) = r;
    }
    __builtin_amdgcn_wave_barrier();   // the stage is rewritten by the next tile
    O.G += hi;
    O.lo = 0;
    O.fill -= hi;
}

// The stream length of every buffer -> len[i]: n + 1 - P for P >= 2 pair starts, n + 1 (LITERAL)
// otherwise, 1 for n = 0; 0 for offsets that decrease (nothing of such a buffer is read).
__global__ __launch_bounds__(SB_THREADS) void k_small_batch_len(const uint8_t *__restrict__ in,
                                                                const uint64_t *__restrict__ in_off, uint64_t count,
                                                                uint64_t *__restrict__ len)
{
    const int lane = threadIdx.x & 63;
    const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    for (uint64_t i = (uint64_t)blockIdx.x * SB_WAVES + w; i < count; i += (uint64_t)gridDim.x * SB_WAVES) {
        const uint64_t a = in_off[i], b = in_off[i + 1];
        if (b < a) {
            if (lane == 0) len[i] = 0;
            continue;
        }
        const uint64_t n = b - a;
        uint64_t pairs = 0;
        sb_walk(sb_buf(in + a, n), lane, [&](const SbTile &T, const uint4 &c, uint32_t p, uint32_t q, bool) {
            uint32_t val[4], keep[4], pr = 0;
            (void)sb_classify(T, c, p, q, lane, val, keep, pr);
            pairs += pr;
        });
        const uint64_t P = sb_wave_sum(pairs);
        if (lane == 0) len[i] = P >= 2 ? n + 1 - P : n + 1;
    }
}

// buffer i -> out[out_off[i] .. out_off[i + 1]) (the scan of k_small_batch_len's lengths), and its
// status. A buffer whose offsets decrease, or whose stream would end past out_cap, is not read and
// writes no byte. A stream of n + 1 bytes is the LITERAL form (the pruned form has n - 1 at most).
__global__ __launch_bounds__(SB_THREADS) void k_small_batch_enc(const uint8_t *__restrict__ in,
                                                                const uint64_t *__restrict__ in_off,
                                                                const uint64_t *__restrict__ out_off, uint64_t count,
                                                                uint8_t *__restrict__ out, uint64_t out_cap,
                                                                int32_t *__restrict__ status,
                                                                unsigned long long *__restrict__ first)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_stage[SB_WAVES][SB_STAGE];
    const int lane = threadIdx.x & 63;
    const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    uint8_t *const stage = s_stage[w];
    for (uint64_t i = (uint64_t)blockIdx.x * SB_WAVES + w; i < count; i += (uint64_t)gridDim.x * SB_WAVES) {
        const BsItem E = bs_item<false>(in_off, out_off, i, true, out_cap);
        if (!E.good) {
            bs_report(status, first, i, E.st, lane == 0);
            continue;
        }
        const uint64_t n = E.n;
        const bool literal = E.room == n + 1;
        SbOut O = sb_out(out + E.o0, E.room);
        if (lane == 0) stage[O.fill] = literal ? (uint8_t)' ' : (uint8_t)SB_PRUNED;   // the type byte
        O.fill += 1;
        sb_walk(sb_buf(in + E.a, n), lane, [&](const SbTile &T, const uint4 &c, uint32_t p, uint32_t q, bool last) {
            uint32_t val[4], keep[4], pr = 0;
            uint32_t cnt = sb_classify(T, c, p, q, lane, val, keep, pr);
            if (literal) {   // every byte of the buffer as it is
                const uint32_t d[4] = {c.x, c.y, c.z, c.w};
                cnt = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    val[j] = d[j];
                    keep[j] = T.interior ? 0x80808080u : sb_ge((uint32_t)lane * 16u + 4u * j, T.lo) &
                                                             sb_lt((uint32_t)lane * 16u + 4u * j, T.hi);
                    cnt += (uint32_t)__popc(keep[j]);
                }
            }
            const uint32_t incl = wave_scan_incl(cnt);
            const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
            uint32_t pos = O.fill + incl - cnt;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if ((keep[j] >> (8 * k + 7)) & 1u) stage[pos++] = (uint8_t)(val[j] >> (8 * k));
                }
            }
            O.fill += total;
            sb_flush(stage, O, last, lane);
        });
        if (n == 0) sb_flush(stage, O, true, lane);   // (no tile: the type byte alone)
        __builtin_amdgcn_wave_barrier();               // the stage is rewritten by the next buffer
        bs_report(status, first, i, DC_OK, lane == 0);
    }
}

// Decode, the lane's 16 stream bytes: emit = the positions that give output (stream bytes 1 ..),
// two = those that give two bytes (>= 0x80 at stream bytes 2 .., pruned form only). Returns the
// output bytes.
static __device__ __forceinline__ uint32_t sb_dec_classify(const SbTile &T, const uint4 &c, int lane, bool pruned,
                                                           uint32_t (&emit)[4], uint32_t (&two)[4])
{
    const uint32_t d[4] = {c.x, c.y, c.z, c.w};
    uint32_t cnt = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t u = (uint32_t)lane * 16u + 4u * j;
        emit[j] = 0x80808080u;
        two[j] = pruned ? d[j] & 0x80808080u : 0u;
        if (!T.interior) {
            emit[j] = sb_ge(u, T.one) & sb_lt(u, T.hi);
            two[j] &= sb_ge(u, T.two) & emit[j];
        }
        cnt += (uint32_t)__popc(emit[j]) + (uint32_t)__popc(two[j]);
    }
    return cnt;
}

// dc_small_decompress_batch: stream i = in[in_off[i] .. in_off[i + 1]) decoded into
// out[out_off[i] .. out_off[i + 1]), and its status. The decoded length is a count over the stream
// (orc_small_decompress's rules: the pruned form gives m - 1 bytes and one more per byte >= 0x80
// after its first two, the LITERAL form m - 1, anything else 0), so it is counted first and the
// stream is written only when it is the length asked for: a stream of any other status writes no
// byte (the second read of the stream hits cache).
__global__ __launch_bounds__(SB_THREADS) void k_small_batch_dec(const uint8_t *__restrict__ in,
                                                                const uint64_t *__restrict__ in_off,
                                                                const uint64_t *__restrict__ out_off, uint64_t count,
                                                                uint8_t *__restrict__ out, uint64_t out_cap,
                                                                int32_t *__restrict__ status,
                                                                unsigned long long *__restrict__ first)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_stage[SB_WAVES][SB_STAGE];
    const int lane = threadIdx.x & 63;
    const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    uint8_t *const stage = s_stage[w];
    for (uint64_t i = (uint64_t)blockIdx.x * SB_WAVES + w; i < count; i += (uint64_t)gridDim.x * SB_WAVES) {
        const BsItem E = bs_item<true>(in_off, out_off, i, true, out_cap);
        int st = E.st;
        if (E.good) {
            const uint64_t m = E.n, want = E.room;
            const uint32_t type = m ? in[E.a] : 0x100u;
            const bool pruned = type == SB_PRUNED, literal = type == ' ';
            const SbBuf B = sb_buf(in + E.a, m);
            uint64_t have = 0;
            if (literal) have = m - 1;
            else if (pruned) {
                uint64_t mine = 0;
                sb_walk(B, lane, [&](const SbTile &T, const uint4 &c, uint32_t, uint32_t, bool) {
                    uint32_t emit[4], two[4];
                    mine += sb_dec_classify(T, c, lane, true, emit, two);
                });
                have = sb_wave_sum(mine);
            }
            if (have != want) st = DC_E_STREAM;
            else if (want) {
                SbOut O = sb_out(out + E.o0, want);
                sb_walk(B, lane, [&](const SbTile &T, const uint4 &c, uint32_t, uint32_t, bool last) {
                    uint32_t emit[4], two[4];
                    const uint32_t cnt = sb_dec_classify(T, c, lane, pruned, emit, two);
                    const uint32_t d[4] = {c.x, c.y, c.z, c.w};
                    const uint32_t incl = wave_scan_incl(cnt);
                    const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
                    uint32_t pos = O.fill + incl - cnt;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            const uint32_t v = (d[j] >> (8 * k)) & 255u;
                            if ((emit[j] >> (8 * k + 7)) & 1u) {
                                if ((two[j] >> (8 * k + 7)) & 1u) {
                                    stage[pos++] = (uint8_t)' ';
                                    stage[pos++] = (uint8_t)(v - 0x80u);
                                } else {
                                    stage[pos++] = (uint8_t)v;
                                }
                            }
                        }
                    }
                    O.fill += total;
                    sb_flush(stage, O, last, lane);
                });
                __builtin_amdgcn_wave_barrier();   // the stage is rewritten by the next stream
            }
        }
        bs_report(status, first, i, st, lane == 0);
    }
}
