// dc_nyb_batch_kernels.inc -- nybble batch v1 (dc_gpu.h): many independent buffers, each coded as
// the reference stream of that buffer alone (compress_bytestring, nybble_compression.c:887-1038),
// back to back, and the asynchronous decode of such a batch. Included by dc_core.hip after the
// one-lane-per-stream machinery (nl_walk, NlOut, mtf_touch8, nyb_wave_decode) and after
// dc_batch_kernels.inc (hb_fail: status[i] and the context's first-failure slot).
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

// One lane's walk of its buffer x[0 .. len) (every lane of the wave calls it; a lane without a
// buffer passes len = 0, cap = 0, literal = false). STORE = false: returns the stream's length
// (the nybble form's bytes q, or len + 1 when q >= len: the LITERAL form, :1018-1037; 1 for
// len 0) and touches no output. STORE = true: puts the stream (the form given by `literal`)
// through o, of which never more than cap bytes leave for memory, and returns the bytes put.
template <bool STORE>
static __device__ __forceinline__ uint64_t nyb_lane_encode(const uint8_t *__restrict__ x, uint64_t len, int modify,
                                                           bool literal, uint64_t cap, NlOut &o, uint64_t (*sL)[64],
                                                           int t)
{
    for (int c = 0; c < 16; ++c) sL[c][t] = mtf_init_word();
    uint64_t q = 0;   // bytes put
    auto put = [&](uint32_t v) {
        if (STORE) o.ring[(o.sh + q) & (NL_ORING - 1)] = (uint8_t)v;   // (LDS, the index masked)
        ++q;
    };
    // what may leave for memory: the bytes put, never more than cap (tested at the points, not per
    // byte: q == cap at the end whenever the input is what the length walk saw)
    auto sent = [&]() { return o.sh + (q < cap ? q : cap); };
    uint32_t prev = len ? x[0] : 0u;
    if (STORE && literal) put(' ');
    else if (len) put(0xAF);
    if (len) put(prev);
    int half = 0;
    uint32_t hi = 0;   // pending high nybble
    const uintptr_t xa = (uintptr_t)x;
    const uint4 *g = len > 1 ? reinterpret_cast<const uint4 *>(x - (xa & 15)) : nl_zero;
    const uint64_t sh = len > 1 ? xa & 15 : 0;
    nl_walk(g, len > 1 ? sh + 1 : 0, len > 1 ? sh + len : 0,
        [&](uint32_t v, bool valid) {
            if (valid) {
                const uint32_t c = (prev >> 3) & 15u;
                uint32_t pb;
                bool hit;
                // compress_byte_index :833-839 (rank before the touch), update_context :665-687
                const uint64_t L = mtf_touch8(sL[c][t], v, pb, hit);
                if (modify) sL[c][t] = L;
                if (STORE && literal) hit = false;   // the LITERAL form: every byte goes as a miss does, raw
                if (!hit) {
                    if (half) { put(prev); half = 0; }   // miss at offset 1 (:855-857)
                    put(v);
                } else if (!half) {
                    hi = (8u | (pb >> 3)) << 4;
                    half = 1;
                } else {
                    put(hi | 8u | (pb >> 3));
                    half = 0;
                }
                prev = v;
            }
        },
        [&]() { if (STORE) nl_out_point(o, sent()); });
    if (half) put(prev);   // odd tail (:1000-1009): the last byte raw
    if (!STORE) return q >= len ? len + 1 : q;
    nl_out_point(o, sent());
    nl_out_finish(o, sent());
    return q;
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
    const uint64_t a = live ? in_off[i] : 0, b = live ? in_off[i + 1] : 0;
    const uint64_t o0 = live ? out_off[i] : 0, o1 = live ? out_off[i + 1] : 0;
    int st = DC_OK;
    if (b < a) st = DC_E_ARG;
    else if (o1 > out_cap) st = DC_E_CAPACITY;
    const bool good = live && st == DC_OK;
    const uint64_t len = good ? b - a : 0, cap = good ? o1 - o0 : 0;
    NlOut o;
    nl_out_init(o, out + (good ? o0 : 0), s_out + t * NL_OSTR);
    (void)nyb_lane_encode<true>(in + (good ? a : 0), len, modify, good && cap == len + 1, cap, o, s_L, t);
    if (live) {
        if (st == DC_OK) status[i] = DC_OK;
        else hb_fail(status, first, i, st);
    }
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
    const uint64_t a = live ? in_off[i] : 0, b = live ? in_off[i + 1] : 0;
    const uint64_t o0 = live ? out_off[i] : 0, o1 = live ? out_off[i + 1] : 0;
    int st = DC_OK;
    if (b < a || o1 < o0) st = DC_E_ARG;
    else if (o1 > out_cap) st = DC_E_CAPACITY;
    const bool good = live && st == DC_OK;
    const bool ok = nyb_wave_decode(in + (good ? a : 0), good ? b - a : 0, good ? o1 - o0 : 0, modify, true,
                                    out + (good ? o0 : 0), good, s_L, s_in + t * NL_RSTR, s_out + t * NL_OSTR, t);
    if (good && !ok) st = DC_E_STREAM;
    if (live) {
        if (st == DC_OK) status[i] = DC_OK;
        else hb_fail(status, first, i, st);
    }
}
