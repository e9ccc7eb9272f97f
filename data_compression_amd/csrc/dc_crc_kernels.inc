// dc_crc_kernels.inc -- CRC-32 of device buffers (dc_gpu.h "Checksums"; the arithmetic is
// dc_crc32.h). Included by dc_core.hip after dc_small_batch_kernels.inc, whose buffer view it
// shares (sb_buf / sb_load: 16-B granules from the aligned address below x[0], the bytes outside
// the buffer zeroed; bs_report: status[i] and the context's first-failure slot).
//
//   k_crc_batch    buffer i = in[beg[i] .. end[i]) -> crc[i], status[i]; or, VERIFY, status[i]
//                  against expect[i]
//   k_crc_pieces   one buffer in pieces of DC_CRC_PIECE bytes -> each piece's CRC times the weight
//                  of the bytes after the piece
//   k_crc_fold     the xor of those: crc(A || B) = crc(A) x^(8 |B|) ^ crc(B), piece by piece
//
// ONE WAVE PER BUFFER (or piece), CRC_WAVES waves a workgroup on a persistent grid, buffers taken
// in a fixed stride, as the small batch codec does. The wave walks the buffer in tiles of 64 lanes
// x 16 B (DC_CRC_TILE) in the FOLDING form: lane l takes granule l of every tile, so a wave's load
// is one coalesced KiB, and advances its own register per tile by the constant x^(8 * 1024)
// (crc_mulk: four lookups in the tables of that product) before it adds the raw CRC of its 16
// bytes (slicing by four: sixteen lookups in four dependent rounds). The contiguous form, a slice
// of the buffer per lane, would stride the lanes of one load 64 B or more apart. After the last
// tile lane l's register is multiplied by its place x^(8 * 16 * (63 - l)) (one 32-step product a
// buffer) and the 64 are xored.
//
// Edges. The raw register of a zero start ignores leading zero bytes, so (1) the unaligned head
// is masked to zeros in its aligned granule; (2) the tiles are aligned to the buffer's END: the
// whole granules before the last one fill the last tile up to lane 63, and what is missing in
// front of the first tile is zeros that are never loaded; (3) the start value all ones is 0xFF
// xored into the buffer's first four bytes as they are loaded (a buffer of n < 4 bytes adds the
// constant 0xFFFFFFFF x^(8 n) instead). Trailing zeros are NOT free, so the granule that holds the
// buffer's last byte (1 to 16 bytes of it) is not part of the fold: the folded register is
// advanced through its bytes as a running CRC, dwords then bytes, by every lane alike (one
// address: a broadcast). Empty buffers, buffers inside one granule and buffers shorter than a
// lane's share all take this one path with zero tiles.
//
// Tables (CrcTabs: 8.6 KiB, made on the host by dc_crc32.h's generators, uploaded once per
// context, copied to LDS by every workgroup): a wave's lookups are ds_read_b32 at random indices
// of one 1 KiB table, several lanes to a bank.

#define CRC_WAVES 4
#define CRC_THREADS (64 * CRC_WAVES)
#define CRC_T_SL 0u        /* [4][256] the slicing tables                          */
#define CRC_T_MK 1024u     /* [4][256] the product by x^(8 DC_CRC_TILE)            */
#define CRC_T_WL 2048u     /* [64]     lane l's place: x^(8 * 16 * (63 - l))       */
#define CRC_T_P2 2112u     /* [64]     x^(8 * 2^k)                                 */
#define CRC_T_C 2176u      /* [4]      0xFFFFFFFF x^(8 n), n = 0..3                */
#define CRC_T_WORDS 2192u  /* (a multiple of 4: copied as uint4)                   */
static_assert(DC_CRC_TILE == 64u * 16u, "a wave tile is 64 lanes x 16 B");

static void crc_make_tables(uint32_t *w)
{
    dc_crc32_slice_tables(reinterpret_cast<uint32_t(*)[256]>(w + CRC_T_SL), 4);
    dc_crc32_mul_tables(reinterpret_cast<uint32_t(*)[256]>(w + CRC_T_MK), dc_crc32_xpow8(DC_CRC_TILE));
    for (uint32_t l = 0; l < 64; ++l) w[CRC_T_WL + l] = dc_crc32_xpow8(16u * (63u - l));
    uint32_t sq = DC_CRC_X8;
    for (uint32_t k = 0; k < 64; ++k, sq = dc_crc32_mul(sq, sq)) w[CRC_T_P2 + k] = sq;
    for (uint32_t n = 0; n < 4; ++n) w[CRC_T_C + n] = dc_crc32_mul(0xFFFFFFFFu, dc_crc32_xpow8(n));
    for (uint32_t i = CRC_T_C + 4; i < CRC_T_WORDS; ++i) w[i] = 0;
}

static __device__ __forceinline__ void crc_tables_in(uint32_t *L, const uint32_t *__restrict__ tab)
{
    for (uint32_t i = threadIdx.x; i < CRC_T_WORDS / 4; i += blockDim.x)
        reinterpret_cast<uint4 *>(L)[i] = reinterpret_cast<const uint4 *>(tab)[i];
    __syncthreads();
}

static __device__ __forceinline__ uint32_t crc_slice4(const uint32_t *L, uint32_t c)
{
    return L[CRC_T_SL + 768u + (c & 255u)] ^ L[CRC_T_SL + 512u + ((c >> 8) & 255u)] ^
           L[CRC_T_SL + 256u + ((c >> 16) & 255u)] ^ L[CRC_T_SL + (c >> 24)];
}
// s x^(8 DC_CRC_TILE)
static __device__ __forceinline__ uint32_t crc_mulk(const uint32_t *L, uint32_t s)
{
    return L[CRC_T_MK + (s & 255u)] ^ L[CRC_T_MK + 256u + ((s >> 8) & 255u)] ^
           L[CRC_T_MK + 512u + ((s >> 16) & 255u)] ^ L[CRC_T_MK + 768u + (s >> 24)];
}

// granule gi < ng of the buffer: outside bytes zeroed, the start value in the first four bytes
static __device__ __forceinline__ uint4 crc_gran(const SbBuf &B, uint64_t gi, bool init)
{
    uint4 v = sb_load(B, gi);
    if (init && gi < 2) {   // the buffer's bytes 0..3 are granule bytes sh .. sh + 3 of granules 0 and 1
        const uint32_t u = 16u * (uint32_t)gi;
        v.x ^= sb_inside(u, B.sh, B.sh + 4u);
        v.y ^= sb_inside(u + 4u, B.sh, B.sh + 4u);
        v.z ^= sb_inside(u + 8u, B.sh, B.sh + 4u);
        v.w ^= sb_inside(u + 12u, B.sh, B.sh + 4u);
    }
    return v;
}

// crc32 of x[0 .. n), by a whole wave, the same value in every lane (x and n wave-uniform)
static __device__ __forceinline__ uint32_t crc_wave(const uint32_t *L, const uint8_t *x, uint64_t n, int lane)
{
    if (n == 0) return 0u;
    const SbBuf B = sb_buf(x, n);
    const bool init = n >= 4;
    const uint64_t nga = B.ng - 1;                          // whole granules in front of the last one
    const uint64_t nt = (nga + 63) / 64, pad = nt * 64 - nga;   // tiles; zero granules in front of tile 0
    const uint4 tl = crc_gran(B, B.ng - 1, init);
    const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
    uint32_t c = 0;
    if (nt) {
        uint4 cur = (uint64_t)lane >= pad ? crc_gran(B, (uint64_t)lane - pad, init) : zero;
        uint32_t s = 0;
        for (uint64_t t = 0; t < nt; ++t) {
            const uint64_t gp = (t + 1) * 64 + (uint64_t)lane;   // (>= 64 > pad; past the end after the last tile)
            const uint4 nxt = gp - pad < nga ? crc_gran(B, gp - pad, init) : zero;
            uint32_t r = crc_slice4(L, cur.x);
            r = crc_slice4(L, r ^ cur.y);
            r = crc_slice4(L, r ^ cur.z);
            r = crc_slice4(L, r ^ cur.w);
            s = crc_mulk(L, s) ^ r;
            cur = nxt;
        }
        s = dc_crc32_mul(s, L[CRC_T_WL + (uint32_t)lane]);
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) s ^= __shfl_xor(s, d, 64);
        c = s;
    }
    // the last granule: granule bytes 0 .. e - 1 (those below the buffer's first byte are zeros,
    // met with a zero register when the buffer begins here)
    const uint32_t e = (uint32_t)((B.sh + n - 1) & 15u) + 1u;
    const uint32_t words = e >> 2, rem = e & 3u;
    if (words > 0) c = crc_slice4(L, c ^ tl.x);
    if (words > 1) c = crc_slice4(L, c ^ tl.y);
    if (words > 2) c = crc_slice4(L, c ^ tl.z);
    if (words > 3) c = crc_slice4(L, c ^ tl.w);
    const uint32_t v = words == 0 ? tl.x : words == 1 ? tl.y : words == 2 ? tl.z : tl.w;
    for (uint32_t k = 0; k < rem; ++k) c = L[CRC_T_SL + ((c ^ (v >> (8u * k))) & 255u)] ^ (c >> 8);
    return c ^ (init ? 0u : L[CRC_T_C + (uint32_t)n]) ^ 0xFFFFFFFFu;
}

// Buffer i = in[beg[i] .. end[i]) (beg and end may be one array and the same array shifted by
// one). Its status: DC_E_ARG when end < beg, else DC_E_CAPACITY when end > in_cap (nothing of
// such a buffer is read, and its crc is 0), else DC_OK. VERIFY: an entry whose status is nonzero
// on entry keeps it and is not read; a good buffer whose CRC is not expect[i] is DC_E_CHECKSUM.
template <bool VERIFY>
__global__ __launch_bounds__(CRC_THREADS) void k_crc_batch(const uint8_t *__restrict__ in, uint64_t in_cap,
                                                           const uint64_t *beg, const uint64_t *end, uint64_t count,
                                                           const uint32_t *__restrict__ expect, uint32_t *__restrict__ crc,
                                                           int32_t *status, unsigned long long *__restrict__ first,
                                                           const uint32_t *__restrict__ tab)
{
    __shared__ __attribute__((aligned(16))) uint32_t L[CRC_T_WORDS];
    crc_tables_in(L, tab);
    const int lane = threadIdx.x & 63;
    const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    for (uint64_t i = (uint64_t)blockIdx.x * CRC_WAVES + w; i < count; i += (uint64_t)gridDim.x * CRC_WAVES) {
        int st = VERIFY ? status[i] : DC_OK;
        uint32_t v = 0;
        if (st == DC_OK) {
            const uint64_t a = beg[i], b = end[i];
            st = b < a ? DC_E_ARG : b > in_cap ? DC_E_CAPACITY : DC_OK;
            if (st == DC_OK) {
                v = crc_wave(L, in + a, b - a, lane);
                if (VERIFY && v != expect[i]) st = DC_E_CHECKSUM;
            }
        }
        if (!VERIFY && lane == 0) crc[i] = v;
        bs_report(status, first, i, st, lane == 0);
    }
}

// Piece i = in[i PIECE .. min(n, (i + 1) PIECE)) of one buffer: part[i] = crc(piece) x^(8 r), r the
// bytes of the buffer after the piece. x^(8 r) is the product of x^(8 * 2^k) over the set bits k of
// r: lane k holds its factor (or x^0) and the wave multiplies them in six butterfly steps.
__global__ __launch_bounds__(CRC_THREADS) void k_crc_pieces(const uint8_t *__restrict__ in, uint64_t n, uint64_t npieces,
                                                            uint32_t *__restrict__ part, const uint32_t *__restrict__ tab)
{
    __shared__ __attribute__((aligned(16))) uint32_t L[CRC_T_WORDS];
    crc_tables_in(L, tab);
    const int lane = threadIdx.x & 63;
    const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    for (uint64_t i = (uint64_t)blockIdx.x * CRC_WAVES + w; i < npieces; i += (uint64_t)gridDim.x * CRC_WAVES) {
        const uint64_t a = i * DC_CRC_PIECE;
        const uint64_t len = n - a < DC_CRC_PIECE ? n - a : DC_CRC_PIECE;
        const uint32_t v = crc_wave(L, in + a, len, lane);
        const uint64_t r = n - a - len;
        uint32_t f = ((r >> lane) & 1u) ? L[CRC_T_P2 + (uint32_t)lane] : DC_CRC_X0;
        if (r) {
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) f = dc_crc32_mul(f, (uint32_t)__shfl_xor(f, d, 64));
        }
        if (lane == 0) part[i] = dc_crc32_mul(v, f);
    }
}

// *out = the xor of part[0 .. npieces): one workgroup
__global__ __launch_bounds__(1024) void k_crc_fold(const uint32_t *__restrict__ part, uint64_t npieces,
                                                    uint32_t *__restrict__ out)
{
    __shared__ uint32_t s_w[16];
    uint32_t x = 0;
    for (uint64_t i = threadIdx.x; i < npieces; i += 1024) x ^= part[i];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) x ^= __shfl_xor(x, d, 64);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = x;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t y = 0;
        for (int k = 0; k < 16; ++k) y ^= s_w[k];
        *out = y;
    }
}
