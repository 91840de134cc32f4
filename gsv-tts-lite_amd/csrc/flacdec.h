// flacdec: one FLAC frame -> its integers.  flac_decode_frame is ONE routine for the device kernel below, for the host
// entry point gsv_flac_decode_host and for the stand-alone checker tools/flac_host_check.cpp: the same text compiled
// three times, so the CPU tests and the sanitizer run exercise what the GPU runs.
//
// Read: 1-2 channels at 4..24 bits per sample, both blocking strategies, every block-size code, the sample-rate codes
// (parsed and skipped), the UTF-8-style frame / sample number (1-7 bytes), CRC-8; CONSTANT, VERBATIM, FIXED 0-4 and LPC
// 1-32 subframes (precision 1-15, shift 0-15, sums in int64), wasted bits, the side channel one bit wider; both residual
// methods, escape partitions (raw width 0 included), partition orders 0-15; independent, left/side, right/side and
// mid/side channels; CRC-16 over the whole frame.
//
// Total on arbitrary bytes: every bit comes through FlacBits, which never loads at or past its length (`len - 2`; the
// CRC-16 is loaded once, at len - 2 and len - 1, after `len >= 6` is known; an open-ended frame: `len`, and the CRC-16
// at e and e + 1 after e + 2 <= len is known) and turns a read past the end into FLAC_E_OVERRUN; a
// unary run ends at the last bit; every store goes to out[i * channels + c] with i < block_size, the size the CALLER
// allotted (a header that names another size is FLAC_E_MISMATCH before any store).  Every failure zero-fills the
// frame's output and returns a distinct nonzero status.  No assert, trap or printf; no recursion; no table in memory
// (the CRC-16 byte step is arithmetic); predictor history and coefficients live in registers (constant indices only).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FLAC_HD __host__ __device__ __forceinline__
#else
#define FLAC_HD inline
#endif

namespace gsv {

enum FlacStatus {
    FLAC_OK = 0,
    FLAC_E_OVERRUN = 1,     // the frame's structure needs more bits than byte_len holds
    FLAC_E_SYNC = 2,        // no frame sync code, or a reserved header bit set
    FLAC_E_RESERVED = 3,    // a reserved code: block size, sample rate, channel assignment, sample size, subframe type,
                            // residual method, LPC precision 16, negative LPC shift, malformed coded number
    FLAC_E_CRC8 = 4,        // header CRC-8 mismatch
    FLAC_E_MISMATCH = 5,    // the header's block size, channels or sample size differ from the caller's
    FLAC_E_ORDER = 6,       // predictor order larger than the block
    FLAC_E_PARTITION = 7,   // the partition count does not divide the block, or a partition is shorter than the order
    FLAC_E_RESIDUAL = 8,    // a Rice-coded residual outside 32 bits
    FLAC_E_RANGE = 9,       // a decoded sample outside the stream's bits per sample
    FLAC_E_LENGTH = 10,     // the frame's structure ends before byte_len - 2: bytes left in front of the CRC-16
    FLAC_E_CRC16 = 11,      // frame CRC-16 mismatch
    FLAC_E_WASTED = 12,     // wasted bits leave no bit of the sample
    FLAC_N_STATUS = 13
};

// CRC-16 (polynomial 0x8005, init 0, unreflected) over one more byte.  The table entry T[x] = x(t) t^16 mod P has the closed
// form parity(x) << 15 ^ y << 2 ^ y with y = x ^ x >> 1 ^ ... ^ x >> 7, since t^16 = t^15 + t^2 + 1 (mod P).
FLAC_HD unsigned flac_crc16_byte(unsigned crc, unsigned b) {
    unsigned x = ((crc >> 8) ^ b) & 0xFFu;
    unsigned y = x ^ (x >> 1);
    y ^= y >> 2;
    y ^= y >> 4;                    // y = prefix XOR; its bit 0 is the parity of x
    return ((crc << 8) ^ ((y & 1u) << 15) ^ (y << 2) ^ y) & 0xFFFFu;
}

// CRC-8 (polynomial 0x07, init 0) over one more byte; headers are at most 16 bytes
FLAC_HD unsigned flac_crc8_byte(unsigned crc, unsigned b) {
    crc ^= b;
    for (int i = 0; i < 8; ++i) crc = (crc & 0x80u) ? ((crc << 1) ^ 0x07u) & 0xFFu : (crc << 1);
    return crc;
}

// MSB-first bit reader over p[0, len): byte loads only (a frame starts anywhere), 64-bit window, sticky error.  The
// CRC-16 runs over every byte as it is loaded; the window only ever loads bytes in front of `len`, so once `bp == len`
// and `cnt == 0` the CRC covers exactly p[0, len).
struct FlacBits {
    const unsigned char* p;
    uint32_t len, bp;       // bytes in all, bytes loaded
    uint64_t acc;           // the next cnt bits, left-justified; the bits below them are zero
    int cnt;
    unsigned crc;
    int err;
};

FLAC_HD void flac_bits_init(FlacBits& b, const unsigned char* p, uint32_t len) {
    b.p = p; b.len = len; b.bp = 0; b.acc = 0; b.cnt = 0; b.crc = 0; b.err = 0;
}

FLAC_HD void flac_bits_fill(FlacBits& b) {
    while (b.cnt <= 56 && b.bp < b.len) {
        const unsigned v = b.p[b.bp++];
        b.crc = flac_crc16_byte(b.crc, v);
        b.acc |= (uint64_t)v << (56 - b.cnt);
        b.cnt += 8;
    }
}

// n in 0..32
FLAC_HD uint32_t flac_bits_read(FlacBits& b, int n) {
    if (n == 0) return 0;
    if (b.cnt < n) flac_bits_fill(b);
    if (b.cnt < n) {
        b.err = FLAC_E_OVERRUN;
        b.acc = 0; b.cnt = 0; b.bp = b.len;
        return 0;
    }
    const uint32_t v = (uint32_t)(b.acc >> (64 - n));
    b.acc <<= n;
    b.cnt -= n;
    return v;
}

// n in 1..32, two's complement
FLAC_HD int32_t flac_bits_read_signed(FlacBits& b, int n) {
    const uint32_t v = flac_bits_read(b, n);
    return (int32_t)(v << (32 - n)) >> (32 - n);
}

// zeros in front of the next 1 bit, which is consumed; the run ends with the frame (FLAC_E_OVERRUN)
FLAC_HD uint32_t flac_bits_unary(FlacBits& b) {
    uint32_t q = 0;
    for (;;) {
        if (b.cnt == 0 || b.acc == 0) {
            q += (uint32_t)b.cnt;
            b.acc = 0; b.cnt = 0;
            flac_bits_fill(b);
            if (b.cnt == 0) {
                b.err = FLAC_E_OVERRUN;
                return 0;
            }
            if (b.acc == 0) continue;       // at least 8 fresh zero bits were consumed: the loop ends with the bytes
        }
        const int z = __builtin_clzll(b.acc);       // < cnt: the bits below the window are zero and acc != 0
        q += (uint32_t)z;
        b.acc = (b.acc << z) << 1;
        b.cnt -= z + 1;
        return q;
    }
}

FLAC_HD uint32_t flac_bits_consumed_bytes(const FlacBits& b) { return b.bp - (uint32_t)(b.cnt >> 3); }

// what a frame header says, for callers that look (the host indexer has its own parser)
struct FlacHeader {
    int variable, block_size, channels, assignment, bps, header_bytes;
    uint64_t number;        // frame number (fixed blocking) or first sample (variable blocking)
};

// parses the frame header; bps_stream stands in for sample-size code 0.  The CRC-8 is checked here.
FLAC_HD int flac_read_header(FlacBits& br, int bps_stream, FlacHeader& h) {
    const uint32_t sync = flac_bits_read(br, 16);
    if (br.err) return br.err;
    if ((sync & 0xFFFEu) != 0xFFF8u) return FLAC_E_SYNC;
    h.variable = (int)(sync & 1u);
    const uint32_t bs_code = flac_bits_read(br, 4), sr_code = flac_bits_read(br, 4);
    const uint32_t ch_code = flac_bits_read(br, 4), ss_code = flac_bits_read(br, 3);
    const uint32_t resv = flac_bits_read(br, 1);
    if (br.err) return br.err;
    if (resv) return FLAC_E_SYNC;
    if (bs_code == 0 || sr_code == 15 || ch_code > 10 || ss_code == 3 || ss_code == 7) return FLAC_E_RESERVED;
    // the coded number: 0xxxxxxx, or 110xxxxx .. 11111110 followed by 1-6 bytes 10xxxxxx
    const uint32_t b0 = flac_bits_read(br, 8);
    if (br.err) return br.err;
    int extra = 0;
    uint64_t num = b0;
    if (b0 & 0x80u) {
        int ones = 0;
        for (uint32_t m = 0x80u; m && (b0 & m); m >>= 1) ++ones;
        if (ones < 2 || ones > 7) return FLAC_E_RESERVED;
        extra = ones - 1;
        num = ones == 7 ? 0 : (b0 & (0x7Fu >> ones));
    }
    for (int i = 0; i < extra; ++i) {
        const uint32_t c = flac_bits_read(br, 8);
        if (br.err) return br.err;
        if ((c & 0xC0u) != 0x80u) return FLAC_E_RESERVED;
        num = (num << 6) | (c & 0x3Fu);
    }
    h.number = num;
    if (!h.variable && extra > 5) return FLAC_E_RESERVED;      // a frame number has at most 31 bits
    int bs;
    if (bs_code == 1) bs = 192;
    else if (bs_code <= 5) bs = 576 << (bs_code - 2);
    else if (bs_code == 6) bs = (int)flac_bits_read(br, 8) + 1;
    else if (bs_code == 7) bs = (int)flac_bits_read(br, 16) + 1;
    else bs = 256 << (bs_code - 8);
    if (sr_code == 12) (void)flac_bits_read(br, 8);
    else if (sr_code == 13 || sr_code == 14) (void)flac_bits_read(br, 16);
    const uint32_t crc8 = flac_bits_read(br, 8);
    if (br.err) return br.err;
    h.block_size = bs;
    h.assignment = ch_code < 8 ? 0 : (int)ch_code - 7;      // 0 independent, 1 left/side, 2 right/side, 3 mid/side
    h.channels = ch_code < 8 ? (int)ch_code + 1 : 2;
    h.bps = ss_code == 0 ? bps_stream : ss_code == 1 ? 8 : ss_code == 2 ? 12 : ss_code == 4 ? 16 : ss_code == 5 ? 20 : 24;
    h.header_bytes = (int)flac_bits_consumed_bytes(br);     // byte-aligned here; <= 16, all in front of len
    unsigned c8 = 0;
    for (int i = 0; i + 1 < h.header_bytes; ++i) c8 = flac_crc8_byte(c8, br.p[i]);
    if (c8 != crc8) return FLAC_E_CRC8;
    return FLAC_OK;
}

// one subframe's samples, as they are decoded: range check against the subframe's width, then the store
struct FlacEmit {
    int32_t* out;       // this channel's first sample
    int stride, shift, lo, hi, bad;
};

FLAC_HD void flac_emit(FlacEmit& e, int i, int64_t v) {
    if (v < e.lo || v > e.hi) e.bad = 1;
    e.out[(int64_t)i * e.stride] = (int32_t)((uint32_t)(int32_t)v << e.shift);
}

// A FIXED or LPC subframe of order <= M: warm-up samples, the LPC header when `lpc`, then residual and prediction.
// c[j] multiplies sample i - 1 - j.  M is a compile-time bucket so that history and coefficients stay in registers
// (constant indices only); FIXED order k is the LPC predictor of the k-th difference with shift 0.
template <int M>
FLAC_HD int flac_predicted(FlacBits& br, FlacEmit& e, int order, bool lpc, int sbps, int bs) {
    int c[M], h[M];
#pragma unroll
    for (int j = 0; j < M; ++j) c[j] = h[j] = 0;
    for (int i = 0; i < order; ++i) {
        const int32_t v = flac_bits_read_signed(br, sbps);
        if (br.err) return br.err;
        flac_emit(e, i, v);
#pragma unroll
        for (int j = M - 1; j > 0; --j) h[j] = h[j - 1];
        h[0] = v;
    }
    int shift = 0;
    if (lpc) {
        const int prec = (int)flac_bits_read(br, 4) + 1;
        shift = flac_bits_read_signed(br, 5);
        if (br.err) return br.err;
        if (prec == 16 || shift < 0) return FLAC_E_RESERVED;
#pragma unroll
        for (int j = 0; j < M; ++j)
            if (j < order) c[j] = flac_bits_read_signed(br, prec);
        if (br.err) return br.err;
    } else if (M == 4) {
        if (order == 1) { c[0] = 1; }
        else if (order == 2) { c[0] = 2; c[1] = -1; }
        else if (order == 3) { c[0] = 3; c[1] = -3; c[2] = 1; }
        else if (order == 4) { c[0] = 4; c[1] = -6; c[2] = 4; c[3] = -1; }
    }
    const uint32_t method = flac_bits_read(br, 2);
    const int po = (int)flac_bits_read(br, 4);
    if (br.err) return br.err;
    if (method > 1) return FLAC_E_RESERVED;
    if (po > 0 && (bs & ((1 << po) - 1))) return FLAC_E_PARTITION;
    const int psz = bs >> po;
    if (psz < order) return FLAC_E_PARTITION;
    const int pbits = method ? 5 : 4, esc_code = method ? 31 : 15;
    int i = order;
    for (int part = 0; part < (1 << po); ++part) {
        int k = (int)flac_bits_read(br, pbits);
        const bool esc = k == esc_code;
        if (esc) k = (int)flac_bits_read(br, 5);
        if (br.err) return br.err;
        const int n = psz - (part == 0 ? order : 0);
        for (int t = 0; t < n; ++t, ++i) {
            int64_t r;
            if (esc) {
                r = k ? flac_bits_read_signed(br, k) : 0;
            } else {
                const uint64_t q = flac_bits_unary(br);
                const uint64_t u = (q << k) | flac_bits_read(br, k);
                if (u > 0xFFFFFFFFull) return FLAC_E_RESIDUAL;
                r = (int64_t)(u >> 1) ^ -(int64_t)(u & 1);
            }
            if (br.err) return br.err;
            int64_t sum = 0;
#pragma unroll
            for (int j = 0; j < M; ++j) sum += (int64_t)c[j] * h[j];
            const int64_t v = r + (sum >> shift);
            flac_emit(e, i, v);
            if (e.bad) return FLAC_E_RANGE;
#pragma unroll
            for (int j = M - 1; j > 0; --j) h[j] = h[j - 1];
            h[0] = (int32_t)v;
        }
    }
    return FLAC_OK;
}

// one subframe of sbps bits per sample into out[i * stride], i < bs; out_shift is added to the wasted bits
FLAC_HD int flac_subframe(FlacBits& br, int sbps, int bs, int32_t* out, int stride, int out_shift) {
    const uint32_t head = flac_bits_read(br, 8);
    if (br.err) return br.err;
    if (head & 0x80u) return FLAC_E_RESERVED;
    const int type = (int)(head >> 1) & 0x3F;
    int wasted = 0;
    if (head & 1u) {
        wasted = (int)flac_bits_unary(br) + 1;
        if (br.err) return br.err;
        if (wasted >= sbps) return FLAC_E_WASTED;
    }
    sbps -= wasted;
    FlacEmit e;
    e.out = out; e.stride = stride; e.shift = wasted + out_shift; e.bad = 0;
    e.lo = -(1 << (sbps - 1)); e.hi = (1 << (sbps - 1)) - 1;
    if (type == 0) {                                            // CONSTANT
        const int32_t v = flac_bits_read_signed(br, sbps);
        if (br.err) return br.err;
        for (int i = 0; i < bs; ++i) flac_emit(e, i, v);
        return FLAC_OK;
    }
    if (type == 1) {                                            // VERBATIM
        for (int i = 0; i < bs; ++i) {
            const int32_t v = flac_bits_read_signed(br, sbps);
            if (br.err) return br.err;
            flac_emit(e, i, v);
        }
        return FLAC_OK;
    }
    int order;
    const bool lpc = type >= 32;
    if (lpc) order = type - 31;
    else if (type >= 8 && type <= 12) order = type - 8;
    else return FLAC_E_RESERVED;
    if (order > bs) return FLAC_E_ORDER;
    if (order <= 4) return flac_predicted<4>(br, e, order, lpc, sbps, bs);
    if (order <= 8) return flac_predicted<8>(br, e, order, lpc, sbps, bs);
    if (order <= 12) return flac_predicted<12>(br, e, order, lpc, sbps, bs);
    return flac_predicted<32>(br, e, order, lpc, sbps, bs);
}

// One frame: p[0, len) -> out[i * channels + c] for i < block_size, c < channels, each sample (after the inter-channel
// decorrelation) shifted left by out_shift: 0 for the integers as they were encoded, 32 - bps for left-justified s32.
// channels (1 or 2) and bps (4..24) are the stream's, block_size is what the caller allotted in `out`; a header that
// disagrees is FLAC_E_MISMATCH.  open_end: `len` is an upper bound (a file's last frame, which no header follows): the
// CRC-16 is the two bytes behind the structure, wherever inside `len` that ends, and is computed in a second pass.
// Returns a FlacStatus; on any failure the block_size * channels outputs are zero.
FLAC_HD int flac_decode_frame(const unsigned char* p, uint32_t len, int channels, int bps, int block_size, int32_t* out,
                              int out_shift, bool open_end) {
    int st = FLAC_OK;
    if (channels < 1 || channels > 2 || bps < 4 || bps > 24 || block_size < 1 || block_size > 65536 || out_shift < 0 ||
        out_shift > 32 - bps)
        st = FLAC_E_MISMATCH;
    else if (len < 6)
        st = FLAC_E_OVERRUN;
    if (st == FLAC_OK) {
        FlacBits br;
        flac_bits_init(br, p, open_end ? len : len - 2);    // closed: the CRC-16 itself is never part of the structure
        FlacHeader h;
        st = flac_read_header(br, bps, h);
        if (st == FLAC_OK && (h.block_size != block_size || h.channels != channels || h.bps != bps)) st = FLAC_E_MISMATCH;
        if (st == FLAC_OK) {
            const bool indep = h.assignment == 0;
            for (int c = 0; c < channels && st == FLAC_OK; ++c) {
                const bool side = (h.assignment == 1 && c == 1) || (h.assignment == 2 && c == 0) || (h.assignment == 3 && c == 1);
                st = flac_subframe(br, bps + (side ? 1 : 0), block_size, out + c, channels, indep ? out_shift : 0);
            }
            if (st == FLAC_OK && !indep) {
                const int lo = -(1 << (bps - 1)), hi = (1 << (bps - 1)) - 1;
                int bad = 0;
                for (int i = 0; i < block_size; ++i) {
                    const int32_t a = out[2 * (int64_t)i], b = out[2 * (int64_t)i + 1];   // at most 25 bits each
                    int32_t l, r;
                    if (h.assignment == 1) { l = a; r = a - b; }
                    else if (h.assignment == 2) { l = a + b; r = b; }
                    else {
                        const int32_t m = (int32_t)((uint32_t)a << 1) | (b & 1);
                        l = (m + b) >> 1;
                        r = (m - b) >> 1;
                    }
                    if (l < lo || l > hi || r < lo || r > hi) bad = 1;
                    out[2 * (int64_t)i] = (int32_t)((uint32_t)l << out_shift);
                    out[2 * (int64_t)i + 1] = (int32_t)((uint32_t)r << out_shift);
                }
                if (bad) st = FLAC_E_RANGE;
            }
        }
        if (st == FLAC_OK) {
            (void)flac_bits_read(br, br.cnt & 7);                       // zero padding to the byte boundary
            if (open_end) {
                const uint32_t e = flac_bits_consumed_bytes(br);        // byte-aligned; e <= len
                if (len - e < 2) {
                    st = FLAC_E_OVERRUN;
                } else {
                    unsigned crc = 0;
                    for (uint32_t i = 0; i < e; ++i) crc = flac_crc16_byte(crc, p[i]);
                    if (crc != (((unsigned)p[e] << 8) | p[e + 1])) st = FLAC_E_CRC16;
                }
            } else if (br.cnt != 0 || br.bp != br.len) {
                st = FLAC_E_LENGTH;
            } else {
                const unsigned want = ((unsigned)p[len - 2] << 8) | p[len - 1];
                if (br.crc != want) st = FLAC_E_CRC16;
            }
        }
    }
    if (st != FLAC_OK && channels >= 1 && channels <= 2 && block_size >= 1 && block_size <= 65536)
        for (int64_t i = 0; i < (int64_t)block_size * channels; ++i) out[i] = 0;
    return st;
}

#if defined(__HIPCC__) && !defined(GSV_FLACDEC_NO_KERNEL)   // flacenc.h wants the scalar pieces only
// one frame of the device table (built by gsv_flac_decode from the caller's host tables, 32 bytes)
struct FlacFrameDev {
    long long byte_off;     // of the frame in the packed byte buffer
    long long out_off;      // int32 elements into the staging area: the clip's base + first_sample * channels
    unsigned byte_len;
    int block_size;
    short channels, bps;
    int open_end;
};

// One lane per frame.  Block b's first `fpb` lanes (1..64) decode frames [b * fpb, b * fpb + fpb): a small batch puts
// one frame in each wave (no divergence between frames, more CUs at work), a large one fills the waves.  Staging is
// interleaved s32, left-justified (x << (32 - bps)): the input format WAV_S32 of wav_to_mono_kernel.
static __global__ __launch_bounds__(64) void flac_frames_kernel(const unsigned char* __restrict__ bytes,
                                                                const FlacFrameDev* __restrict__ tab, int n_frames, int fpb,
                                                                int32_t* __restrict__ staging, int32_t* __restrict__ status) {
    if ((int)threadIdx.x >= fpb) return;
    const long long f = (long long)blockIdx.x * fpb + threadIdx.x;
    if (f >= n_frames) return;
    const FlacFrameDev t = tab[f];
    status[f] = flac_decode_frame(bytes + t.byte_off, t.byte_len, t.channels, t.bps, t.block_size, staging + t.out_off,
                                  32 - t.bps, t.open_end != 0);
}
#endif

}  // namespace gsv
