// dc_batch_lens_kernels.inc -- the nybble form of a Huffman batch's lens records
// (dc_huff_batch_lens_pack / dc_huff_batch_lens_unpack, dc_gpu.h "Huffman batch v1: nybble
// records"); included by dc_core.hip after dc_batch_kernels.inc (hb_fail, HB_THREADS). A storage
// form only: the batch kernels read 256-byte records.
// Both kernels move 384 B a record and compute next to nothing, so the lane mapping is the widest
// access on the wide side: a lane takes 16 lengths, one 16-B access (global_load / store_dwordx4)
// of the 256-byte record and one 8-B access (dwordx2) of the 128-byte one. 16 lanes make a record,
// a wave four records (1 KiB and 512 B contiguous per wave instruction), a workgroup sixteen. No LDS.
//   k_hb_lens_pack    byte j of record i = lens[2j] << 4 | lens[2j + 1]; a record holding a length
//                     over 15 is written as 128 zeros with status DC_E_CODE_TOO_LONG (the 16 lanes
//                     of a record learn of it from one wave ballot)
//   k_hb_lens_unpack  the reverse: every one of the 256 bytes of every record is written

#define HBL_LANES 16                                /* lanes per record */
#define HBL_RECS (HB_THREADS / HBL_LANES)           /* records per workgroup step */

// four lengths (a little-endian dword, each <= 15) -> two bytes, the first length in the high nybble
static __device__ __forceinline__ uint32_t hbl_pack4(uint32_t x)
{
    const uint32_t p = ((x & 0x000F000Fu) << 4) | ((x >> 8) & 0x000F000Fu);   // byte 0 and byte 2 hold the pairs
    return (p & 0xFFu) | ((p >> 8) & 0xFF00u);
}

// two bytes (the low 16 bits of h) -> four lengths
static __device__ __forceinline__ uint32_t hbl_unpack2(uint32_t h)
{
    return ((h >> 4) & 0xFu) | ((h & 0xFu) << 8) | (((h >> 12) & 0xFu) << 16) | (((h >> 8) & 0xFu) << 24);
}

__global__ __launch_bounds__(HB_THREADS) void k_hb_lens_pack(const uint8_t *__restrict__ lens, uint64_t count,
                                                             uint8_t *__restrict__ lens4, int32_t *__restrict__ status,
                                                             unsigned long long *__restrict__ first)
{
    const uint32_t t = threadIdx.x, part = t % HBL_LANES;
    const uint64_t steps = (count + HBL_RECS - 1) / HBL_RECS;
    for (uint64_t g = blockIdx.x; g < steps; g += gridDim.x) {   // (workgroup-uniform: every lane meets the ballot)
        const uint64_t i = g * HBL_RECS + t / HBL_LANES;
        const bool in = i < count;
        uint4 q = make_uint4(0u, 0u, 0u, 0u);
        if (in) q = reinterpret_cast<const uint4 *>(lens)[i * HBL_LANES + part];
        const uint64_t over = __ballot(((q.x | q.y | q.z | q.w) & 0xF0F0F0F0u) != 0u);
        const bool bad = ((over >> (t & 48u)) & 0xFFFFull) != 0;   // the record's 16 lanes: bits [16 r, 16 r + 16) of the wave
        if (!in) continue;
        const uint2 o = bad ? make_uint2(0u, 0u)
                            : make_uint2(hbl_pack4(q.x) | (hbl_pack4(q.y) << 16), hbl_pack4(q.z) | (hbl_pack4(q.w) << 16));
        reinterpret_cast<uint2 *>(lens4)[i * HBL_LANES + part] = o;
        if (part == 0) {
            if (bad) hb_fail(status, first, i, DC_E_CODE_TOO_LONG);
            else status[i] = DC_OK;
        }
    }
}

__global__ __launch_bounds__(HB_THREADS) void k_hb_lens_unpack(const uint8_t *__restrict__ lens4, uint64_t count,
                                                               uint8_t *__restrict__ lens)
{
    const uint64_t units = count * HBL_LANES;   // 8 bytes in, 16 bytes out each (count <= DC_RANGES_MAX: no wrap)
    for (uint64_t u = (uint64_t)blockIdx.x * HB_THREADS + threadIdx.x; u < units; u += (uint64_t)gridDim.x * HB_THREADS) {
        const uint2 q = reinterpret_cast<const uint2 *>(lens4)[u];
        reinterpret_cast<uint4 *>(lens)[u] =
            make_uint4(hbl_unpack2(q.x), hbl_unpack2(q.x >> 16), hbl_unpack2(q.y), hbl_unpack2(q.y >> 16));
    }
}
