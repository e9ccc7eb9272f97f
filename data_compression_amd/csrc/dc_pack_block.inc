// The pack's block body: what k_huff_pack's fast path, k_fe_pack and the A/B variants of
// dc_ab_kernels.inc share. A block's codes are gathered into runs of at most 64 bits
// (pack_code_piece), OR-ed into the LDS stage (pack_emit), and the stage moves to HBM with the
// two words a block shares with its neighbours OR-ed (pack_store_block). The LDS arrays come as
// pointers: the A/B kernels keep them in a struct.

// OR a right-justified run of nb <= 64 bits into the stage at bit pos (<= 3 words)
// Branch-free: the run left-justified in 64 bits has zeros below it, so the
// words it does not reach receive 0 (a no-op OR; some lane of a wave needs each
// of the 3 ORs anyway, so skipping them per lane saved no LDS cycle and cost
// compares and exec-mask branches). nb == 0 only for an all-zero acc (absent
// symbols have code 0), where the unmasked shift by 64 & 63 = 0 is harmless.
static __device__ __forceinline__ void pack_emit(uint32_t *stage, uint64_t acc, uint32_t nb, uint32_t pos)
{
    const uint64_t al = acc << ((64u - nb) & 63u);
    const uint32_t hi = (uint32_t)(al >> 32), lo = (uint32_t)al, r = pos & 31u, wi = pos >> 5;
    atomicOr(&stage[wi], hi >> r);
    atomicOr(&stage[wi + 1], __builtin_amdgcn_alignbit(hi, lo, r));
    atomicOr(&stage[wi + 2], __builtin_amdgcn_alignbit(lo, 0u, r));
}

// pass A: the bits of a 16-byte piece's two halves of 8 codes, from the byte-length table
static __device__ __forceinline__ void pack_piece_bits(const uint32_t (&w4)[4], const uint8_t *nb8, uint32_t &s0,
                                                       uint32_t &s1)
{
    s0 = 0;
    s1 = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) s0 += nb8[(w4[i >> 2] >> (8 * (i & 3))) & 255u];
#pragma unroll
    for (int i = 8; i < 16; ++i) s1 += nb8[(w4[i >> 2] >> (8 * (i & 3))) & 255u];
}

// Half h of a piece as two quarters of 4 codes from bit pos on, each one run when it has
// <= 64 bits (always, unless codes exceed 16 bits), else code by code. Returns the bit after the
// half. tally(i, l): the length l of the piece's code i, for callers that want them.
template <class Tally>
static __device__ __forceinline__ uint32_t pack_code_quarters(uint32_t *stage, const uint2 *tab, const uint32_t (&w4)[4],
                                                              int h, uint32_t pos, Tally tally)
{
#pragma unroll
    for (int qq = 0; qq < 2; ++qq) {
        uint2 e[4];
        uint32_t nq = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int bi = 8 * h + 4 * qq + i;
            const uint32_t wv = qq ? w4[2 * h + 1] : w4[2 * h];
            e[i] = tab[(wv >> (8 * (bi & 3))) & 255u];
            nq += e[i].y;
            tally(bi, e[i].y);
        }
        if (nq <= 64u) {
            uint64_t acc = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) acc = (acc << e[i].y) | e[i].x;
            pack_emit(stage, acc, nq, pos);
            pos += nq;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) { pack_emit(stage, e[i].x, e[i].y, pos); pos += e[i].y; }
        }
    }
    return pos;
}

// pass B of one piece: its 16 codes (bytes w4 under tab) into the stage from bit rel on, as
// two halves of 8 codes (Hk bits, then Tk - Hk), each gathered into a 64-bit register (no
// per-code flush) and OR-ed in as at most 3 words. A half of more than 64 bits (skewed or
// long codes, e.g. C4's Zipf bytes), or every half in quarter mode, goes as two quarters.
// (k_huff_pack keeps this body as its own text around pack_emit: see there.)
template <class Tally>
static __device__ __forceinline__ void pack_code_piece(uint32_t *stage, const uint2 *tab, const uint32_t (&w4)[4],
                                                       bool qmode, uint32_t Hk, uint32_t Tk, uint32_t rel, Tally tally)
{
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const uint32_t Th = h ? Tk - Hk : Hk;
        const uint32_t pos = h ? rel + Hk : rel;
        if (!qmode && Th <= 64u) {
            // (a packed 32-bit code|length table measured 4% slower: the
            // extraction VALU costs more than the uint2 reads' bank conflicts)
            uint64_t acc = 0;
#pragma unroll
            for (int i = 8 * h; i < 8 * h + 8; ++i) {
                const uint2 e = tab[(w4[i >> 2] >> (8 * (i & 3))) & 255u];
                acc = (acc << e.y) | e.x;
                tally(i, e.y);
            }
            pack_emit(stage, acc, Th, pos);
        } else {
            pack_code_quarters(stage, tab, w4, h, pos, tally);
        }
    }
}

// The plain stores of the store phase: stage words (sh, last_plain) to dst, byte-swapped (the
// stream is MSB-first), as uint4s where whole. Every stage word read is zeroed by the thread
// that read it (the stage is zero at the next block's start; words < sh and past the block's
// last were never written).
static __device__ __forceinline__ void pack_store_plain(uint32_t *stage, uint32_t *dst, uint32_t sh, uint32_t last_plain,
                                                        bool vec_out, int t)
{
    if (vec_out) {
        const uint32_t nq = last_plain >> 2;   // uint4 q covers stage words [4q, 4q+4)
        for (uint32_t q = 1 + t; q < nq; q += 256) {
            uint4 *const sq = reinterpret_cast<uint4 *>(&stage[4 * q]);
            const uint4 v = *sq;
            *sq = make_uint4(0u, 0u, 0u, 0u);
            // streaming (nt) stores: same-box A/B on 1 GiB C2, pack 0.420 -> 0.382 ms
            // (the decode after it reads the payload no slower)
            uint4 *const d4 = reinterpret_cast<uint4 *>(dst + 4 * q);
            __builtin_nontemporal_store(bswap32(v.x), &d4->x);
            __builtin_nontemporal_store(bswap32(v.y), &d4->y);
            __builtin_nontemporal_store(bswap32(v.z), &d4->z);
            __builtin_nontemporal_store(bswap32(v.w), &d4->w);
        }
        // head: words sh+1..3 of uint4 0; tail: words of the last, partial uint4
        const uint32_t hend = last_plain < 4u ? last_plain : 4u;
        if (t < 4 && (uint32_t)t > sh && (uint32_t)t < hend) { dst[t] = bswap32(stage[t]); stage[t] = 0u; }
        const uint32_t tb = nq > 0 ? 4 * nq : 4u;
        if (t >= 8 && t < 12 && tb + (t - 8) < last_plain) {
            dst[tb + (t - 8)] = bswap32(stage[tb + (t - 8)]);
            stage[tb + (t - 8)] = 0u;
        }
    } else {
        for (uint32_t i = t + 1; i < last_plain; i += 256) { dst[i] = bswap32(stage[i]); stage[i] = 0u; }
    }
}

// The store phase of a block of nw_blk words staged from stage word sh on (nwa = sh + nw_blk;
// dst = the output word of stage word 0; run = the absolute bit after the block). Stage word sh
// = the block's first word, shared with the previous block when the block starts inside it; the
// last word is shared with the next one when the block ends inside it: those two are OR-ed into
// HBM, where k_block_final_wide zeroed them, by one lane each (no-return atomics); the rest are
// plain stores.
static __device__ __forceinline__ void pack_store_block(uint32_t *stage, uint32_t *dst, uint32_t sh, uint32_t nw_blk,
                                                        uint32_t nwa, uint64_t run, bool vec_out, int t)
{
    // opaque copy: stops the compiler from hoisting the phase's lane tests (t == 0, t == 64,
    // t < 4 ..) out of the block loop, where each held two SGPRs through every block
    asm volatile("" : "+v"(t));
    const uint32_t last_plain = ((run & 31) != 0) ? nwa - 1 : nwa;   // plain: [sh+1, last_plain)
    pack_store_plain(stage, dst, sh, last_plain, vec_out, t);
    // (nw_blk = 0: a shard's one-byte last block in k_fe_pack, a pair's start, on a word
    // boundary. It has no word: its first word would be the one at index = the stream's words,
    // which words_cap need not hold. k_huff_pack and its variants come here with full blocks
    // only, which always have a word: the condition is always true there.)
    if (t == 0 && nw_blk > 0) {
        atomicOr(&dst[sh], bswap32(stage[sh]));
        stage[sh] = 0u;
    }
    if (t == 64 && last_plain < nwa && nw_blk > 1) {
        atomicOr(&dst[nwa - 1], bswap32(stage[nwa - 1]));
        stage[nwa - 1] = 0u;
    }
}
