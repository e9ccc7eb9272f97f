// dc_nyb_batch_kernels.inc -- nybble batch v1 (dc_gpu.h): many independent buffers, each coded as
// the reference stream of that buffer alone (compress_bytestring, nybble_compression.c:887-1038),
// back to back, and the asynchronous decode of such a batch. Included by dc_core.hip after the
// one-lane-per-stream machinery (nl_walk, NlOut, nyb_lane_encode, nyb_wave_decode) and after
// dc_batch_kernels.inc (hb_fail: status[i] and the context's first-failure slot). The three batch
// kernels, and before them the per-buffer frame they share with dc_small_batch_kernels.inc.
//
// Encode is form (b) of the two the layout allows: a length walk (k_nyb_batch_enc_len), the scan
// (k_scan_u64 into d_out_off) and an encode straight to the final place (k_nyb_batch_enc). Form
// (a), DCNK's (scratch slots of len + 2 bytes at in_off[i] - in_off[0] + 2 i, scan, placement),
// walks each buffer once, but it needs two things this call does not have: the scratch size
// (in_off[count] - in_off[0] + 2 count) is on the device and the call makes no host read; and the
// slots are disjoint only while the offsets rise, where this call must code every good buffer
// beside a decreasing pair, and a buffer after such a pair overlaps the one before it. Form (b)
// needs neither, at the price of the second walk; it also knows each stream's form (nybble or
// LITERAL) before the first byte is put, so nothing is ever rewritten after whole lines have left.

// ---- the per-buffer frame of a byte-stream batch kernel (dc_gpu.h "byte-stream batch v1") ----
// Entry i reads in[a .. a + n) and may write out[o0 .. o0 + room). Its status, in this order:
//   in_off[i + 1] < in_off[i]                                   DC_E_ARG
//   DEC and out_off[i + 1] < out_off[i]                         DC_E_ARG
//   out_off[i + 1] > out_cap or out_off[i + 1] < out_off[i]     DC_E_CAPACITY
// On encode out_off is the call's own scan of the stream lengths, so a pair of it decreases only
// when that scan wrapped 2^64: no room either. (k_nyb_batch_enc did not test this before it took
// the frame; no reachable input changes status.) An entry that is not good (failed, or !live: a
// lane past count) hands out zeros: it reads no input byte and writes no output byte.
struct BsItem {
    uint64_t a, n, o0, room;
    int st;
    bool good;
};
template <bool DEC>
static __device__ __forceinline__ BsItem bs_item(const uint64_t *__restrict__ in_off, const uint64_t *__restrict__ out_off,
                                                 uint64_t i, bool live, uint64_t out_cap)
{
    const uint64_t a = live ? in_off[i] : 0, b = live ? in_off[i + 1] : 0;
    const uint64_t o0 = live ? out_off[i] : 0, o1 = live ? out_off[i + 1] : 0;
    BsItem B;
    B.st = (b < a || (DEC && o1 < o0)) ? DC_E_ARG : (o1 > out_cap || o1 < o0) ? DC_E_CAPACITY : DC_OK;
    B.good = live && B.st == DC_OK;
    B.a = B.good ? a : 0;
    B.n = B.good ? b - a : 0;
    B.o0 = B.good ? o0 : 0;
    B.room = B.good ? o1 - o0 : 0;
    return B;
}
// the entry's outcome (st: the frame's, or what the codec found in a good entry), by one lane of it
static __device__ __forceinline__ void bs_report(int32_t *__restrict__ status, unsigned long long *__restrict__ first,
                                                 uint64_t i, int st, bool live)
{
    if (!live) return;
    if (st == DC_OK) status[i] = DC_OK;
    else hb_fail(status, first, i, st);
}

// the length of each buffer's stream -> len[i] (one lane per buffer); 0 for offsets that decrease
__global__ __launch_bounds__(64) void k_nyb_batch_enc_len(const uint8_t *__restrict__ in, const uint64_t *__restrict__ in_off,
                                                          uint64_t count, int modify, uint64_t *__restrict__ len)
{
    __shared__ uint64_t s_L[16][64];
    const int t = threadIdx.x;
    const uint64_t i = (uint64_t)blockIdx.x * 64 + t;
    const bool live = i < count;
    const uint64_t a = live ? in_off[i] : 0, b = live ? in_off[i + 1] : 0;
    const bool good = live && b >= a;
    NlOut o = {};   // (no output in this pass)
    const uint64_t q = nyb_lane_encode<false>(in + (good ? a : 0), good ? b - a : 0, modify, false, 0, o, s_L, t);
    if (live) len[i] = good ? q : 0;
}

// buffer i -> out[out_off[i] .. out_off[i + 1]) (the scan of k_nyb_batch_enc_len's lengths), and
// its status. A lane whose offsets decrease, or whose stream would end past out_cap, reads no
// input byte and writes no output byte. A stream of len + 1 bytes is the LITERAL form.
__global__ __launch_bounds__(64) void k_nyb_batch_enc(const uint8_t *__restrict__ in, const uint64_t *__restrict__ in_off,
                                                      const uint64_t *__restrict__ out_off, uint64_t count, int modify,
                                                      uint8_t *__restrict__ out, uint64_t out_cap,
                                                      int32_t *__restrict__ status, unsigned long long *__restrict__ first)
{
    __shared__ uint64_t s_L[16][64];
    __shared__ __attribute__((aligned(16))) uint8_t s_out[64 * NL_OSTR];
    const int t = threadIdx.x;
    const uint64_t i = (uint64_t)blockIdx.x * 64 + t;
    const bool live = i < count;
    const BsItem B = bs_item<false>(in_off, out_off, i, live, out_cap);
    NlOut o;
    nl_out_init(o, out + B.o0, s_out + t * NL_OSTR);
    (void)nyb_lane_encode<true>(in + B.a, B.n, modify, B.good && B.room == B.n + 1, B.room, o, s_L, t);
    bs_report(status, first, i, B.st, live);
}

// dc_nyb_decompress_batch_async: stream i = in[in_off[i] .. in_off[i + 1]) decoded into
// out[out_off[i] .. out_off[i + 1]) (one lane per stream, nyb_wave_decode), and its status. A lane
// with a decreasing offset pair, or whose range ends past out_cap, reads and writes nothing.
__global__ __launch_bounds__(64) void k_nyb_batch_dec_async(const uint8_t *__restrict__ in, const uint64_t *__restrict__ in_off,
                                                            const uint64_t *__restrict__ out_off, uint64_t count, int modify,
                                                            uint8_t *__restrict__ out, uint64_t out_cap,
                                                            int32_t *__restrict__ status, unsigned long long *__restrict__ first)
{
    __shared__ uint64_t s_L[16][64];
    __shared__ __attribute__((aligned(16))) uint8_t s_in[64 * NL_RSTR];
    __shared__ __attribute__((aligned(16))) uint8_t s_out[64 * NL_OSTR];
    const int t = threadIdx.x;
    const uint64_t i = (uint64_t)blockIdx.x * 64 + t;
    const bool live = i < count;
    const BsItem B = bs_item<true>(in_off, out_off, i, live, out_cap);
    const bool ok = nyb_wave_decode(in + B.a, B.n, B.room, modify, true, out + B.o0, B.good, s_L, s_in + t * NL_RSTR,
                                    s_out + t * NL_OSTR, t);
    bs_report(status, first, i, B.good && !ok ? DC_E_STREAM : B.st, live);
}
