// flacenc: mono fp32 samples -> FLAC frames (fixed blocking, 16 or 24 bits, CONSTANT / FIXED 0-4 / VERBATIM subframes,
// Rice partitions of order 0-6, no escapes).  Everything is integer arithmetic once the samples are quantised, so a
// frame has ONE right encoding: the scalar pieces below -- quantiser, k-th difference, zig-zag, a
// partition's cost, the total order of the candidates, the CRC-16 steps -- are one text for the device kernel, for the
// serial host encoder flac_encode_frame_host (gsv_flac_encode_host: the CPU path and the device's oracle) and for the
// stand-alone checker tools/flac_enc_host_check.cpp.  Device bytes equal host bytes.
//
// The frame header is built by the caller (flacio.build_header: the inverse of flacio._header, CRC-8 included) and
// copied in front of the subframe; the CRC-16 runs over header and subframe.
#pragma once
#include <math.h>
#include <stdint.h>

#include "flacdec.h"

namespace gsv {

enum FlacEncKind { FLAC_ENC_CONSTANT = 0, FLAC_ENC_VERBATIM = 1, FLAC_ENC_FIXED = 2 };

constexpr int FLAC_ENC_MAX_BLOCK = 4608;
constexpr int FLAC_ENC_MIN_HEADER = 6, FLAC_ENC_MAX_HEADER = 16;
constexpr int FLAC_ENC_MAX_PORDER = 6;      // at most 64 partitions: one per lane

// what a frame was coded with (the ABI's gsv_flac_enc_choice): k[j] is partition j's Rice parameter, j < 2^porder
struct FlacEncChoice {
    uint8_t kind, order, porder, method;
    uint8_t k[64];
};

// q = clamp(rint(x * 2^(bits-1))): round half to even, NaN (by its bit pattern) -> 0, +-inf clamp.  The scaling is a power
// of two, so the only rounding is rintf's; the inverse of the reader's q / 2^(bits-1).
FLAC_HD int32_t flac_enc_quantise(float x, int bits) {
    uint32_t b;
    __builtin_memcpy(&b, &x, 4);
    if ((b & 0x7FFFFFFFu) > 0x7F800000u) return 0;
    const float full = (float)(1 << (bits - 1));
    float s = rintf(x * full);
    if (s < -full) s = -full;
    if (s > full - 1.0f) s = full - 1.0f;       // 2^23 - 1 is an fp32 value
    return (int32_t)s;
}

// the o-th difference at sample i >= o: FIXED order o's residual.  At 24 bits |r| <= 16 * 2^23: int32 holds it.  Q is
// anything indexed by the sample number: a plain array on the host, the kernel's padded LDS view on the device.
template <typename Q>
FLAC_HD int32_t flac_enc_diff(const Q& q, int i, int o) {
    switch (o) {
        case 0: return q[i];
        case 1: return q[i] - q[i - 1];
        case 2: return q[i] - 2 * q[i - 1] + q[i - 2];
        case 3: return q[i] - 3 * q[i - 1] + 3 * q[i - 2] - q[i - 3];
        default: return q[i] - 4 * q[i - 1] + 6 * q[i - 2] - 4 * q[i - 3] + q[i - 4];
    }
}

FLAC_HD uint32_t flac_enc_zigzag(int32_t r) { return ((uint32_t)r << 1) ^ (uint32_t)(r >> 31); }

// bits of a partition of `len` residuals under Rice parameter k, given sum(u >> k): the unary parts, the stop bits and
// the k low bits.  64 bits: at 24 bits and k = 0 a partition's sum passes 2^32.
FLAC_HD uint64_t flac_enc_cost(uint64_t sum_shifted, uint32_t len, int k) { return sum_shifted + (uint64_t)len * (uint32_t)(1 + k); }

// the finest partition order a block of n samples admits: the largest p <= 6 with n % 2^p == 0
FLAC_HD int flac_enc_finest(int n) {
    int p = 0;
    while (p < FLAC_ENC_MAX_PORDER && (n & ((2 << p) - 1)) == 0) ++p;
    return p;
}

// FIXED order o with partition order p <= flac_enc_finest(n) is a candidate
FLAC_HD bool flac_enc_valid(int n, int o, int p) { return p == 0 || (n >> p) > o; }

// the total order of FIXED candidates: fewer bits, then the lower order, then the lower partition order
FLAC_HD bool flac_enc_better(uint64_t bits, int o, int p, uint64_t best_bits, int best_o, int best_p) {
    if (bits != best_bits) return bits < best_bits;
    if (o != best_o) return o < best_o;
    return p < best_p;
}

// a * b in GF(2)[x] modulo the CRC-16 polynomial: the CRC of A || B is crc(A) * x^(8 |B|) + crc(B), and feeding a zero
// byte (flac_crc16_byte(c, 0)) is the multiplication by x^8
FLAC_HD unsigned flac_crc16_mulmod(unsigned a, unsigned b) {
    unsigned r = 0;
    for (int i = 15; i >= 0; --i) {
        r = (r & 0x8000u) ? ((r << 1) ^ 0x18005u) : (r << 1);
        if ((b >> i) & 1u) r ^= a;
    }
    return r & 0xFFFFu;
}

// the most bytes a frame of n samples takes: the subframe is never longer than VERBATIM
FLAC_HD uint32_t flac_enc_worst_bytes(int header_len, int n, int bits) {
    return (uint32_t)header_len + (uint32_t)((8 + n * bits + 7) >> 3) + 2u;
}

// ------------------------------------------------------------------------------------------------------------------
// the serial encoder
// ------------------------------------------------------------------------------------------------------------------
struct FlacEncWriter {
    uint8_t* p;
    uint32_t at;        // bytes written
    uint64_t acc;
    int cnt;            // bits waiting in acc (< 8 between calls)
};

// v < 2^w, w in 0..32
inline void flac_enc_put(FlacEncWriter& b, uint32_t v, int w) {
    b.acc = (b.acc << w) | v;
    b.cnt += w;
    while (b.cnt >= 8) {
        b.p[b.at++] = (uint8_t)(b.acc >> (b.cnt - 8));
        b.cnt -= 8;
    }
    b.acc &= 0xFFu;
}

inline void flac_enc_zeros(FlacEncWriter& b, uint32_t n) {
    for (; n >= 32; n -= 32) flac_enc_put(b, 0, 32);
    flac_enc_put(b, 0, (int)n);
}

// One frame: x[0, n) -> out[0, length), length <= flac_enc_worst_bytes(header_len, n, bits), which is what the caller
// allotted.  n in 1..4608, bits 16 or 24, header_len in 6..16 (checked by the callers).  -> the frame's length.
inline uint32_t flac_encode_frame_host(const float* x, int n, int bits, const uint8_t* header, int header_len, uint8_t* out,
                                       FlacEncChoice* choice) {
    int32_t q[FLAC_ENC_MAX_BLOCK];
    for (int i = 0; i < n; ++i) q[i] = flac_enc_quantise(x[i], bits);
    bool same = true;
    for (int i = 1; i < n; ++i) same = same && q[i] == q[0];
    const int kmax = bits == 24 ? 31 : 15, pbits = bits == 24 ? 5 : 4;
    FlacEncChoice ch;
    for (int j = 0; j < 64; ++j) ch.k[j] = 0;
    ch.kind = FLAC_ENC_CONSTANT; ch.order = 0; ch.porder = 0; ch.method = 0;
    if (!same) {
        const int pstar = flac_enc_finest(n), cells = 1 << pstar, cell_len = n >> pstar;
        uint64_t best_bits = ~0ull;
        int best_o = 0, best_p = 0;
        static thread_local uint64_t cell[31][64];
        for (int o = 0; o <= 4 && o < n; ++o) {
            for (int k = 0; k < kmax; ++k)
                for (int c = 0; c < cells; ++c) cell[k][c] = 0;
            for (int i = o; i < n; ++i) {
                const uint32_t u = flac_enc_zigzag(flac_enc_diff(q, i, o));
                const int c = i / cell_len;
                for (int k = 0; k < kmax; ++k) cell[k][c] += u >> k;
            }
            for (int p = 0; p <= pstar; ++p) {
                if (!flac_enc_valid(n, o, p)) continue;
                uint64_t total = 8u + (uint64_t)o * bits + 6u;
                uint8_t ks[64];
                const int per = cells >> p;         // cells in a partition
                for (int j = 0; j < (1 << p); ++j) {
                    const uint32_t len = (uint32_t)(n >> p) - (j == 0 ? o : 0);
                    uint64_t bc = ~0ull;
                    int bk = 0;
                    for (int k = 0; k < kmax; ++k) {
                        uint64_t s = 0;
                        for (int c = j * per; c < (j + 1) * per; ++c) s += cell[k][c];
                        const uint64_t cost = flac_enc_cost(s, len, k);
                        if (cost < bc) { bc = cost; bk = k; }
                    }
                    ks[j] = (uint8_t)bk;
                    total += pbits + bc;
                }
                if (flac_enc_better(total, o, p, best_bits, best_o, best_p)) {
                    best_bits = total; best_o = o; best_p = p;
                    for (int j = 0; j < 64; ++j) ch.k[j] = j < (1 << p) ? ks[j] : 0;
                }
            }
        }
        if (8u + (uint64_t)n * bits < best_bits) {
            ch.kind = FLAC_ENC_VERBATIM;
            for (int j = 0; j < 64; ++j) ch.k[j] = 0;
        } else {
            ch.kind = FLAC_ENC_FIXED; ch.order = (uint8_t)best_o; ch.porder = (uint8_t)best_p; ch.method = bits == 24 ? 1 : 0;
        }
    }
    FlacEncWriter w;
    w.p = out; w.at = 0; w.acc = 0; w.cnt = 0;
    const uint32_t mask = (1u << bits) - 1u;
    for (int i = 0; i < header_len; ++i) flac_enc_put(w, header[i], 8);
    if (ch.kind == FLAC_ENC_CONSTANT) {
        flac_enc_put(w, 0x00, 8);
        flac_enc_put(w, (uint32_t)q[0] & mask, bits);
    } else if (ch.kind == FLAC_ENC_VERBATIM) {
        flac_enc_put(w, 0x02, 8);
        for (int i = 0; i < n; ++i) flac_enc_put(w, (uint32_t)q[i] & mask, bits);
    } else {
        const int o = ch.order, p = ch.porder, psz = n >> p;
        flac_enc_put(w, (uint32_t)(8 + o) << 1, 8);
        for (int i = 0; i < o; ++i) flac_enc_put(w, (uint32_t)q[i] & mask, bits);
        flac_enc_put(w, ch.method, 2);
        flac_enc_put(w, (uint32_t)p, 4);
        for (int j = 0; j < (1 << p); ++j) {
            const int k = ch.k[j];
            flac_enc_put(w, (uint32_t)k, pbits);
            for (int i = j == 0 ? o : j * psz; i < (j + 1) * psz; ++i) {
                const uint32_t u = flac_enc_zigzag(flac_enc_diff(q, i, o));
                flac_enc_zeros(w, u >> k);
                flac_enc_put(w, (1u << k) | (u & ((1u << k) - 1u)), k + 1);
            }
        }
    }
    if (w.cnt) flac_enc_put(w, 0, 8 - w.cnt);
    unsigned crc = 0;
    for (uint32_t i = 0; i < w.at; ++i) crc = flac_crc16_byte(crc, out[i]);
    out[w.at] = (uint8_t)(crc >> 8);
    out[w.at + 1] = (uint8_t)crc;
    if (choice) *choice = ch;
    return w.at + 2;
}

#if defined(__HIPCC__) && !defined(GSV_FLACENC_NO_KERNEL)   // track.h wants the scalar pieces only
// ------------------------------------------------------------------------------------------------------------------
// the device encoder: one wave of 64 lanes per frame, one frame per block
// ------------------------------------------------------------------------------------------------------------------
// one frame of the device table (built by gsv_flac_encode from the caller's host tables, 40 bytes)
struct FlacEncFrameDev {
    long long in_off;       // of the frame's first sample in the packed fp32 input
    int block_size, bits, header_len, reserved;
    unsigned char header[FLAC_ENC_MAX_HEADER];
};

// The quantised samples in LDS.  A lane walks a contiguous run, and at B = 4096 the runs start 64 words apart: every lane
// of a half-wave on one bank.  One pad word per 64 samples moves neighbouring runs to neighbouring banks.
constexpr int kFlacEncPcmWords = FLAC_ENC_MAX_BLOCK + FLAC_ENC_MAX_BLOCK / 64;
struct FlacEncPcm {
    int32_t* p;
    __device__ __forceinline__ int32_t& operator[](int i) const { return p[i + (i >> 6)]; }
};

// the frame's bits in LDS, as big-endian 32-bit words: header 16 B + subframe header 1 B + 4608 * 3 B, a spare word
constexpr int kFlacEncWords = 3472;

// ORs v (< 2^width, width 1..32) in at bit `pos`: the buffer was zeroed once, neighbouring lanes share a boundary word
__device__ __forceinline__ void flac_enc_or(uint32_t* w, uint32_t pos, uint32_t v, int width) {
    const uint32_t i = pos >> 5;
    const int end = (int)(pos & 31u) + width;
    if (i + 1 >= (uint32_t)kFlacEncWords) return;       // never taken: a frame is at most its VERBATIM length
    if (end <= 32) {
        atomicOr(&w[i], v << (32 - end));
    } else {
        atomicOr(&w[i], v >> (end - 32));
        atomicOr(&w[i + 1], v << (64 - end));
    }
}

__device__ __forceinline__ unsigned flac_enc_byte(const uint32_t* w, uint32_t j) { return (w[j >> 2] >> (24 - 8 * (j & 3u))) & 0xFFu; }

__device__ __forceinline__ unsigned long long flac_enc_wave_sum(unsigned long long v) {
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) v += __shfl_xor(v, s);
    return v;
}

// FIXED order o over this lane's run [i0, i1): sum(u >> k) for every k, then a butterfly over the wave.  After t stages
// a lane holds the sums of its aligned group of 2^t lanes, which is one partition at order 6 - t when that order is at
// most `pstar` (lanes below a cell are pieces of it).  Every valid (o, p) is weighed against the best so far; best_k is
// the parameter of THIS lane's partition under the best candidate.
template <int KMAX>
__device__ __forceinline__ void flac_enc_order(const FlacEncPcm& q, int n, int bits, int o, int lane, int i0, int i1, int pstar,
                                               unsigned long long& best_bits, int& best_o, int& best_p, int& best_k) {
    constexpr int PBITS = KMAX == 15 ? 4 : 5;
    unsigned long long acc[KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) acc[k] = 0;
    for (int i = i0 > o ? i0 : o; i < i1; ++i) {
        const uint32_t u = flac_enc_zigzag(flac_enc_diff(q, i, o));
#pragma unroll
        for (int k = 0; k < KMAX; ++k) acc[k] += u >> k;
    }
    unsigned long long tot[7];
    int kb[7];
#pragma unroll
    for (int t = 0; t < 7; ++t) {
        const int p = 6 - t;
        tot[t] = 0;
        kb[t] = 0;
        if (p <= pstar && flac_enc_valid(n, o, p)) {        // the same in every lane
            const uint32_t len = (uint32_t)(n >> p) - ((lane >> t) == 0 ? (uint32_t)o : 0u);
            unsigned long long bc = ~0ull;
            int bk = 0;
#pragma unroll
            for (int k = 0; k < KMAX; ++k) {
                const unsigned long long c = flac_enc_cost(acc[k], len, k);
                if (c < bc) { bc = c; bk = k; }
            }
            tot[t] = flac_enc_wave_sum((lane & ((1 << t) - 1)) == 0 ? PBITS + bc : 0ull);
            kb[t] = bk;
        }
        if (t < 6) {
#pragma unroll
            for (int k = 0; k < KMAX; ++k) acc[k] += __shfl_xor(acc[k], 1 << t);
        }
    }
#pragma unroll
    for (int p = 0; p <= 6; ++p) {
        const int t = 6 - p;
        if (p <= pstar && flac_enc_valid(n, o, p)) {
            const unsigned long long total = 8ull + (unsigned long long)(o * bits) + 6ull + tot[t];
            if (flac_enc_better(total, o, p, best_bits, best_o, best_p)) {
                best_bits = total; best_o = o; best_p = p; best_k = kb[t];
            }
        }
    }
}

// SPLIT_CRC: the CRC-16 split across the lanes (what gsv_flac_encode launches); false: one lane walks the frame's bytes,
// kept as the yardstick the split is measured against (tools/flac_encode_time.py).  Same bytes either way.
template <bool SPLIT_CRC>
static __global__ __launch_bounds__(64) void flac_enc_frames_kernel(const float* __restrict__ samples,
                                                                    const FlacEncFrameDev* __restrict__ tab, int n_frames,
                                                                    unsigned char* __restrict__ slots, uint32_t stride,
                                                                    int32_t* __restrict__ lengths, FlacEncChoice* __restrict__ choices) {
    __shared__ int32_t pcm[kFlacEncPcmWords];
    const FlacEncPcm q{pcm};
    __shared__ uint32_t w[kFlacEncWords];
    const int f = blockIdx.x, lane = threadIdx.x;
    if (f >= n_frames) return;
    const int n = tab[f].block_size, bits = tab[f].bits, header_len = tab[f].header_len;
    const long long in_off = tab[f].in_off;
    // 1. quantise; all equal?
    for (int i = lane; i < n; i += 64) q[i] = flac_enc_quantise(samples[in_off + i], bits);
    __syncthreads();
    bool same = true;
    const int32_t q0 = q[0];
    for (int i = lane; i < n; i += 64) same = same && q[i] == q0;
    const bool constant = __all(same) != 0;
    // this lane's run: a cell is one partition at the finest order; 64 >> pstar lanes share a cell
    const int pstar = flac_enc_finest(n), lpc = 64 >> pstar, cell_len = n >> pstar;
    const int chunk = (cell_len + lpc - 1) / lpc, cell0 = (lane / lpc) * cell_len, sub = lane % lpc;
    const int i0 = cell0 + min(sub * chunk, cell_len), i1 = cell0 + min((sub + 1) * chunk, cell_len);
    // 2, 3. costs and choice
    int kind = FLAC_ENC_CONSTANT, bo = 0, bp = 0, bk = 0;
    unsigned long long sub_bits = 8ull + (unsigned long long)bits;
    if (!constant) {
        unsigned long long best = ~0ull;
#pragma unroll 1
        for (int o = 0; o <= 4 && o < n; ++o) {
            if (bits == 24) flac_enc_order<31>(q, n, bits, o, lane, i0, i1, pstar, best, bo, bp, bk);
            else flac_enc_order<15>(q, n, bits, o, lane, i0, i1, pstar, best, bo, bp, bk);
        }
        const unsigned long long verbatim = 8ull + (unsigned long long)(n * bits);
        if (verbatim < best) { kind = FLAC_ENC_VERBATIM; sub_bits = verbatim; bo = bp = bk = 0; }
        else { kind = FLAC_ENC_FIXED; sub_bits = best; }
    }
    // 4. emit
    const uint32_t hbits = (uint32_t)header_len * 8u, nbytes = (hbits + (uint32_t)sub_bits + 7u) >> 3;
    for (uint32_t i = lane; i <= (nbytes + 3u) >> 2 && i < (uint32_t)kFlacEncWords; i += 64) w[i] = 0;
    __syncthreads();
    const uint32_t mask = (1u << bits) - 1u, pos0 = hbits + 8u;
    const int pbits = bits == 24 ? 5 : 4;
    if (lane < header_len) flac_enc_or(w, (uint32_t)lane * 8u, tab[f].header[lane], 8);
    if (kind == FLAC_ENC_CONSTANT) {
        if (lane == 0) flac_enc_or(w, pos0, (uint32_t)q0 & mask, bits);     // the subframe header byte is 0
    } else if (kind == FLAC_ENC_VERBATIM) {
        if (lane == 0) flac_enc_or(w, hbits, 0x02u, 8);
        for (int i = lane; i < n; i += 64) flac_enc_or(w, pos0 + (uint32_t)(i * bits), (uint32_t)q[i] & mask, bits);
    } else {
        if (lane < bo) flac_enc_or(w, pos0 + (uint32_t)(lane * bits), (uint32_t)q[lane] & mask, bits);
        if (lane == 0) {
            flac_enc_or(w, hbits, (uint32_t)(8 + bo) << 1, 8);
            if (bits == 24) flac_enc_or(w, pos0 + (uint32_t)(bo * bits), 1u, 2);
            if (bp) flac_enc_or(w, pos0 + (uint32_t)(bo * bits) + 2u, (uint32_t)bp, 4);
        }
        const bool first = (lane & ((64 >> bp) - 1)) == 0;      // of its partition: it writes the parameter
        const int lo = i0 > bo ? i0 : bo;
        uint32_t len = first ? (uint32_t)pbits : 0u;
        for (int i = lo; i < i1; ++i) len += (flac_enc_zigzag(flac_enc_diff(q, i, bo)) >> bk) + 1u + (uint32_t)bk;
        uint32_t incl = len;
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {
            const uint32_t up = __shfl_up(incl, s);
            if (lane >= s) incl += up;
        }
        uint32_t pos = pos0 + (uint32_t)(bo * bits) + 6u + incl - len;
        if (first) {
            if (bk) flac_enc_or(w, pos, (uint32_t)bk, pbits);
            pos += (uint32_t)pbits;
        }
        for (int i = lo; i < i1; ++i) {
            const uint32_t u = flac_enc_zigzag(flac_enc_diff(q, i, bo));
            pos += u >> bk;                                     // the unary zeros are already there
            flac_enc_or(w, pos, (1u << bk) | (u & ((1u << bk) - 1u)), bk + 1);
            pos += (uint32_t)bk + 1u;
        }
    }
    __syncthreads();
    // 5. CRC-16, split across the lanes: zero bytes IN FRONT leave a CRC at 0, so the bytes are right-aligned in 64 equal
    // chunks; lane l's CRC then moves up by whole chunks: crc(A || B) = crc(A) * x^(8 |B|) + crc(B)
    unsigned crc = 0;
    if (SPLIT_CRC) {
        const uint32_t cb = (nbytes + 63u) >> 6, pad = 64u * cb - nbytes;
        unsigned xp = 1;                // x^(8 * cb), squared at every stage
        for (uint32_t j = (uint32_t)lane * cb; j < ((uint32_t)lane + 1u) * cb; ++j) {
            crc = flac_crc16_byte(crc, j < pad ? 0u : flac_enc_byte(w, j - pad));
            xp = flac_crc16_byte(xp, 0u);
        }
#pragma unroll
        for (int s = 0; s < 6; ++s) {
            const unsigned right = __shfl_down(crc, 1u << s);
            if ((lane & ((2 << s) - 1)) == 0) crc = flac_crc16_mulmod(crc, xp) ^ right;
            xp = flac_crc16_mulmod(xp, xp);
        }
    } else if (lane == 0) {
        for (uint32_t j = 0; j < nbytes; ++j) crc = flac_crc16_byte(crc, flac_enc_byte(w, j));
    }
    // 6. store: the slot is 16-byte aligned and at least flac_enc_worst_bytes long
    if (nbytes + 2u <= stride) {
        unsigned char* dst = slots + (size_t)f * stride;
        const uint32_t full = nbytes >> 2;
        for (uint32_t i = lane; i < full; i += 64) reinterpret_cast<uint32_t*>(dst)[i] = __builtin_bswap32(w[i]);
        if (lane == 0) {
            for (uint32_t j = full * 4u; j < nbytes; ++j) dst[j] = (unsigned char)flac_enc_byte(w, j);
            dst[nbytes] = (unsigned char)(crc >> 8);
            dst[nbytes + 1] = (unsigned char)crc;
            lengths[f] = (int32_t)(nbytes + 2u);
        }
    } else if (lane == 0) {
        lengths[f] = 0;
    }
    if (choices) {
        const int kj = __shfl(bk, (lane << (6 - bp)) & 63);
        choices[f].k[lane] = (unsigned char)(kind == FLAC_ENC_FIXED && lane < (1 << bp) ? kj : 0);
        if (lane == 0) {
            choices[f].kind = (unsigned char)kind;
            choices[f].order = (unsigned char)bo;
            choices[f].porder = (unsigned char)bp;
            choices[f].method = (unsigned char)(kind == FLAC_ENC_FIXED && bits == 24 ? 1 : 0);
        }
    }
}

// lengths [n] -> offsets [n + 1] (exclusive scan, the total last): one block
static __global__ __launch_bounds__(256) void flac_enc_scan_kernel(const int32_t* __restrict__ lengths, int n,
                                                                   long long* __restrict__ offsets) {
    __shared__ long long part[256];
    const int tid = threadIdx.x, per = (n + 255) / 256;
    const int a = min(tid * per, n), b = min(a + per, n);
    long long s = 0;
    for (int i = a; i < b; ++i) s += lengths[i];
    part[tid] = s;
    __syncthreads();
    if (tid == 0) {
        long long run = 0;
        for (int i = 0; i < 256; ++i) { const long long v = part[i]; part[i] = run; run += v; }
        offsets[n] = run;
    }
    __syncthreads();
    s = part[tid];
    for (int i = a; i < b; ++i) { offsets[i] = s; s += lengths[i]; }
}

// frame f: its slot -> out[offsets[f], offsets[f + 1])
static __global__ __launch_bounds__(256) void flac_enc_copy_kernel(const unsigned char* __restrict__ slots, uint32_t stride,
                                                                   const int32_t* __restrict__ lengths,
                                                                   const long long* __restrict__ offsets, int n_frames,
                                                                   unsigned char* __restrict__ out, unsigned long long out_bytes) {
    const int f = blockIdx.x;
    if (f >= n_frames) return;
    const long long at = offsets[f];
    const uint32_t len = (uint32_t)lengths[f];
    if (len > stride || (unsigned long long)at + len > out_bytes) return;      // never taken: out_bytes holds the worst case
    const unsigned char* src = slots + (size_t)f * stride;
    for (uint32_t i = threadIdx.x; i < len; i += 256) out[at + i] = src[i];
}
#endif

}  // namespace gsv
