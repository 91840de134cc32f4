// loudness: ITU-R BS.1770 integrated loudness of B packed fp32 clips and the gain to a target level.  The
// K-filter (a high shelf and a high pass in series, two transposed direct form II biquads), the 400 ms blocks that overlap
// by 75 %, the absolute gate at -70 LUFS, the relative gate 10 LU under the mean of what passed, the gain and its peak limit.
//
// Everything that decides a bit -- the filter step, the combine of the scan, the block bounds, the summation trees, the gates,
// the gain -- is one __host__ __device__ text for the four kernels, for the host twin loud_run_host (gsv_loudness_host: the CPU
// path and the device's oracle) and for the stand-alone checker tools/loudness_host_check.cpp.  All arithmetic is fp64 with
// every multiply-add an explicit fma, every other sum behind an exact product, and every order fixed, so contraction has
// nothing to change and device records and samples equal the host's bit for bit.  The device takes no sin, cos, pow or log:
// the coefficients, the powers of the transition matrix and the gate constants are built on the host in fp64 (loud_params)
// and passed down as a kernel argument; Python computes L = -0.691 + 10 log10(zbar) from the record.
//
// Why fp64 state: the high pass has a double pole (0.9926 at 32 kHz, closer to 1 the higher the rate) and a double root moves
// by the square root of a coefficient's rounding.  Measured on the filter's response with fp32-rounded coefficients against
// fp64: 1.1e-4 LU at 60 Hz and 3e-4 LU at 20 Hz at 32 kHz, 1e-3 LU at 20 Hz at 44.1 kHz -- and 0.018 LU at 96 kHz, 0.13 LU at
// 192 kHz, 0.95 LU at 768 kHz, rates this ABI accepts.  In fp64 the twin sits within 1e-6 LU of the plain serial
// filter from 8 to 192 kHz (tools/loudness_host_check.cpp), and the filter is not what the meter's time goes to.
//
// The scan.  The two biquads are one affine map of a 4-element state: s' = M s + f(x).  A block of LOUD_T threads takes a span of
// LOUD_T * LOUD_R samples; thread t runs its LOUD_R consecutive samples from zero state (thread 0: from the state the last span
// left), a Hillis-Steele scan with the matrices P_k = M^(LOUD_R 2^k) turns the end states into true end states, and every
// thread reruns its samples from the true state of its left neighbour and writes y.  A block carries the state from span to
// span over a chunk of LOUD_CHUNK_SPANS spans.  The chunks of a clip run side by side, chained the same way one level up:
// every chunk but the last first finds its end state from zero state (the first half of the work above, nothing written),
// one thread per clip walks the chunks with M^(chunk) and leaves every chunk's true start state, and the full pass starts
// from it.  So one long clip costs the time of one chunk, about one and a half times the arithmetic.
//
// Workspace: [LoudRow rows[B] | y fp32 [sum of n, each clip 4-float aligned] | z fp64 [sum of blocks] | chunk end states,
// chunk start states, 4 fp64 each [sum of chunks] | peak bits u32 [B]].
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define LOUD_HD __host__ __device__ inline
#else
#define LOUD_HD inline
#endif

namespace gsv {

constexpr int LOUD_T = 512;                     // threads of the filter block
constexpr int LOUD_LOG_T = 9;
constexpr int LOUD_R = 16;                      // consecutive samples per thread and span
constexpr int LOUD_SPAN = LOUD_T * LOUD_R;
constexpr int LOUD_LOG_CH = 1;                  // a chunk is 2^LOUD_LOG_CH spans
constexpr int LOUD_CHUNK = LOUD_SPAN << LOUD_LOG_CH;
constexpr int LOUD_NP = LOUD_LOG_T + LOUD_LOG_CH + 1;      // the scan's matrices, then M^(2 spans) ... M^(chunk)
constexpr int LOUD_LANES = 64;                  // lanes of the block-sum and decide waves
constexpr int LOUD_MIN_RATE = 4000, LOUD_MAX_RATE = 768000;     // the shelf sits at 1500 Hz
constexpr int LOUD_MAX_CLIPS = 65535;
constexpr int LOUD_LIMITED = 1, LOUD_MEASURED = 2, LOUD_NONFINITE = 4;      // record flags
static_assert(LOUD_T == 1 << LOUD_LOG_T, "scan steps");

struct LoudClip {           // gsv_loudness_clip
    long long offset;       // first sample in the packed buffer
    int32_t n;
    float target;           // LUFS; NaN: measure only
};
static_assert(sizeof(LoudClip) == 16, "clip");

struct LoudRecord {         // gsv_loudness_record
    double zbar;            // mean square of the blocks past both gates; 0 without a measurement
    float gain;             // the factor applied (1 without a measurement or a target)
    float peak;             // max |x|
    int32_t blocks, above_abs, kept, flags;
};
static_assert(sizeof(LoudRecord) == 32, "record");

struct LoudRow {            // one clip as the kernels see it (built on the host, first part of the workspace)
    long long offset, yoff, zoff, soff;     // soff: the clip's first chunk state
    double k;               // 10^((target + 0.691) / 10); NaN: measure only
    int32_t n, nb, nch, pad;
};
static_assert(sizeof(LoudRow) == 56, "row");

struct LoudParams {
    double b[2][3], na[2][2];           // per biquad: b0 b1 b2, -a1 -a2 (normalised by a0)
    double P[LOUD_NP][16];              // M^(LOUD_R 2^k), row-major; the last is M^LOUD_CHUNK
    double rate, gate_len, abs_thr;     // Tg * rate; 10^((-70 + 0.691) / 10)
    float peak_limit;
    int32_t pad;
};

struct LoudState { double s[4]; };

// one sample through both biquads; the order of every operation is this text
LOUD_HD double loud_step(const LoudParams& p, LoudState& st, double x) {
    const double y1 = fma(p.b[0][0], x, st.s[0]);
    st.s[0] = fma(p.na[0][0], y1, fma(p.b[0][1], x, st.s[1]));
    st.s[1] = fma(p.na[0][1], y1, p.b[0][2] * x);
    const double y2 = fma(p.b[1][0], y1, st.s[2]);
    st.s[2] = fma(p.na[1][0], y2, fma(p.b[1][1], y1, st.s[3]));
    st.s[3] = fma(p.na[1][1], y2, p.b[1][2] * y1);
    return y2;
}

// own + P left: the state after two adjacent runs from the end state of each run alone
LOUD_HD LoudState loud_combine(const double* P, const LoudState& left, const LoudState& own) {
    LoudState r;
    for (int i = 0; i < 4; ++i)
        r.s[i] = fma(P[4 * i], left.s[0], fma(P[4 * i + 1], left.s[1], fma(P[4 * i + 2], left.s[2], fma(P[4 * i + 3], left.s[3], own.s[i]))));
    return r;
}

// blocks of a clip of n samples (0: too short to measure); every expression in fp64 in this order
LOUD_HD int loud_blocks(int n, double rate) {
    const double Tg = 0.4, step = 0.25;
    if (n < (int)(Tg * rate)) return 0;
    const double T = (double)n / rate;
    return (int)nearbyint((T - Tg) / (Tg * step)) + 1;
}

LOUD_HD void loud_block_bounds(int j, int n, double rate, int* lo, int* hi) {
    const double Tg = 0.4, step = 0.25;
    const double a = (double)j * step;          // exact
    int l = (int)(Tg * a * rate);
    int u = (int)(Tg * (a + 1.0) * rate);       // a + 1 is exact
    if (u > n) u = n;
    if (l > u) l = u;
    *lo = l; *hi = u;
}

// v[0] <- the sum of v[0, 64) by halving: the order both sides take
LOUD_HD void loud_tree_host(double* v) {
    for (int d = LOUD_LANES / 2; d >= 1; d >>= 1)
        for (int i = 0; i < d; ++i) v[i] += v[i + d];
}

LOUD_HD uint32_t loud_abs_bits(float x) {
    uint32_t u;
    memcpy(&u, &x, 4);
    return u & 0x7FFFFFFFu;
}
LOUD_HD float loud_from_bits(uint32_t u) {
    float f;
    memcpy(&f, &u, 4);
    return f;
}

// the filtered sample as it is stored: fp32, saturating -- the shelf lifts a finite |x| near FLT_MAX past the fp32 range, and
// an infinity there would leave a measured clip with zbar = inf
LOUD_HD float loud_store(double v) {
    const double m = 3.4028234663852886e38;     // FLT_MAX
    return (float)fmin(fmax(v, -m), m);
}

// the gain of a measured clip: sqrt(k / zbar), at most peak_limit / peak, as fp32; the product gain * peak never rounds
// above the limit
LOUD_HD float loud_gain(double k, double zbar, float peak, float peak_limit, int* limited) {
    const double g = sqrt(k / zbar);
    const double lim = (double)peak_limit / (double)peak;
    *limited = lim < g;
    float gain = (float)(*limited ? lim : g);
    if (*limited && gain * peak > peak_limit) gain = loud_from_bits(loud_abs_bits(gain) - 1);
    return gain;
}

LOUD_HD bool loud_keep_abs(double z, double abs_thr) { return z >= abs_thr; }
LOUD_HD bool loud_keep_both(double z, double abs_thr, double rel_thr) { return z > rel_thr && z > abs_thr; }

LOUD_HD LoudRecord loud_finish(const LoudRow& row, const LoudParams& p, uint32_t peak_bits, int above_abs, int kept, double sum_kept) {
    LoudRecord r;
    r.blocks = row.nb;
    r.peak = loud_from_bits(peak_bits);
    r.flags = 0;
    const bool nonfinite = peak_bits >= 0x7F800000u;
    if (nonfinite) { r.flags |= LOUD_NONFINITE; above_abs = 0; kept = 0; }
    r.above_abs = above_abs;
    r.kept = kept;
    r.zbar = 0.0;
    r.gain = 1.f;
    if (kept > 0) {
        r.flags |= LOUD_MEASURED;
        r.zbar = sum_kept / (double)kept;
        if (row.k == row.k) {
            int limited;
            r.gain = loud_gain(row.k, r.zbar, r.peak, p.peak_limit, &limited);
            if (limited) r.flags |= LOUD_LIMITED;
        }
    }
    return r;
}

// the parts of every workspace and caller-owned state here (level.h, eq.h, eqstream.h too) start 16-byte aligned
LOUD_HD size_t loud_align16(size_t v) { return (v + 15) & ~(size_t)15; }

// ------------------------------------------------------------------------------------------------------------------
// host only: the constants, the workspace layout, the serial twin
// ------------------------------------------------------------------------------------------------------------------
struct LoudLayout {
    size_t rows_off, y_off, z_off, ends_off, starts_off, peak_off, bytes;
    long long y_total, z_total, s_total;
    int max_n, max_nb, max_nch;
};

// false on arguments the entries refuse; fills the rows when `rows` is given
inline bool loud_layout(const LoudClip* clips, int n_clips, int rate, size_t n_x, bool check_x, LoudLayout* L, LoudRow* rows) {
    if (!clips || n_clips < 1 || n_clips > LOUD_MAX_CLIPS || rate < LOUD_MIN_RATE || rate > LOUD_MAX_RATE) return false;
    long long y = 0, z = 0, sc = 0;
    int max_n = 0, max_nb = 0, max_nch = 0;
    for (int c = 0; c < n_clips; ++c) {
        const LoudClip& cl = clips[c];
        if (cl.n < 0 || cl.offset < 0) return false;
        if (check_x && (unsigned long long)cl.offset + (unsigned long long)cl.n > (unsigned long long)n_x) return false;
        const int nb = loud_blocks(cl.n, (double)rate);
        const int nch = (int)(((long long)cl.n + LOUD_CHUNK - 1) / LOUD_CHUNK);
        if (rows) {
            LoudRow& r = rows[c];
            r.offset = cl.offset; r.yoff = y; r.zoff = z; r.soff = sc;
            r.k = cl.target == cl.target ? pow(10.0, ((double)cl.target + 0.691) / 10.0) : (double)NAN;
            r.n = cl.n; r.nb = nb; r.nch = nch; r.pad = 0;
        }
        y += ((long long)cl.n + 3) & ~3LL;
        z += nb;
        sc += nch;
        if (cl.n > max_n) max_n = cl.n;
        if (nb > max_nb) max_nb = nb;
        if (nch > max_nch) max_nch = nch;
    }
    L->rows_off = 0;
    L->y_off = loud_align16((size_t)n_clips * sizeof(LoudRow));
    L->z_off = L->y_off + loud_align16((size_t)y * sizeof(float));
    L->ends_off = L->z_off + loud_align16((size_t)z * sizeof(double));
    L->starts_off = L->ends_off + (size_t)sc * sizeof(LoudState);
    L->peak_off = L->starts_off + (size_t)sc * sizeof(LoudState);
    L->bytes = L->peak_off + loud_align16((size_t)n_clips * sizeof(uint32_t));
    L->y_total = y; L->z_total = z; L->s_total = sc; L->max_n = max_n; L->max_nb = max_nb; L->max_nch = max_nch;
    return true;
}

inline void loud_matmul4(const double* a, const double* b, double* out) {
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            double s = 0.0;
            for (int k = 0; k < 4; ++k) s += a[4 * i + k] * b[4 * k + j];
            out[4 * i + j] = s;
        }
}

// the K-filter of the definition at `rate`, the scan's matrices and the gate constants
inline LoudParams loud_params(int rate, float peak_limit) {
    LoudParams p;
    memset(&p, 0, sizeof p);
    const double kPi = 3.14159265358979323846;
    {   // high shelf: G = 4 dB, Q = 1 / sqrt 2, fc = 1500 Hz
        const double A = pow(10.0, 4.0 / 40.0), w0 = 2.0 * kPi * 1500.0 / rate, Q = 1.0 / sqrt(2.0);
        const double al = sin(w0) / (2.0 * Q), c = cos(w0), sA = sqrt(A);
        const double a0 = (A + 1) - (A - 1) * c + 2 * sA * al;
        p.b[0][0] = A * ((A + 1) + (A - 1) * c + 2 * sA * al) / a0;
        p.b[0][1] = -2 * A * ((A - 1) + (A + 1) * c) / a0;
        p.b[0][2] = A * ((A + 1) + (A - 1) * c - 2 * sA * al) / a0;
        p.na[0][0] = -(2 * ((A - 1) - (A + 1) * c) / a0);
        p.na[0][1] = -(((A + 1) - (A - 1) * c - 2 * sA * al) / a0);
    }
    {   // high pass: Q = 0.5, fc = 38 Hz
        const double w0 = 2.0 * kPi * 38.0 / rate, al = sin(w0) / (2.0 * 0.5), c = cos(w0);
        const double a0 = 1 + al;
        p.b[1][0] = (1 + c) / 2 / a0;
        p.b[1][1] = -(1 + c) / a0;
        p.b[1][2] = (1 + c) / 2 / a0;
        p.na[1][0] = -(-2 * c / a0);
        p.na[1][1] = -((1 - al) / a0);
    }
    // M: column i is one step with x = 0 from the unit state e_i
    double M[16], A[16], B[16];
    for (int i = 0; i < 4; ++i) {
        LoudState s = {{0, 0, 0, 0}};
        s.s[i] = 1.0;
        loud_step(p, s, 0.0);
        for (int r = 0; r < 4; ++r) M[4 * r + i] = s.s[r];
    }
    memcpy(A, M, sizeof A);
    for (int r = LOUD_R; r > 1; r >>= 1) {      // LOUD_R is a power of two: M^R by squaring
        loud_matmul4(A, A, B);
        memcpy(A, B, sizeof A);
    }
    static_assert((LOUD_R & (LOUD_R - 1)) == 0, "run length");
    for (int k = 0; k < LOUD_NP; ++k) {
        memcpy(p.P[k], A, sizeof A);
        loud_matmul4(A, A, B);
        memcpy(A, B, sizeof A);
    }
    p.rate = (double)rate;
    p.gate_len = 0.4 * (double)rate;
    p.abs_thr = pow(10.0, (-70.0 + 0.691) / 10.0);
    p.peak_limit = peak_limit;
    return p;
}

// the samples [lo, hi) of a clip span by span from the state `carry`, as one block walks them -> the state behind them.  y null:
// the first half only (the end states of the chunks); else y and the peak bits too
inline LoudState loud_chunk_host(const float* x, int lo, int hi, const LoudParams& p, LoudState carry, float* y, uint32_t* peak_bits) {
    static thread_local LoudState st[LOUD_T], nx[LOUD_T];
    for (int s0 = lo; s0 < hi; s0 += LOUD_SPAN) {
        const int cnt = hi - s0 < LOUD_SPAN ? hi - s0 : LOUD_SPAN;
        auto at = [&](int k) { return k < cnt ? (double)x[s0 + k] : 0.0; };
        if (y)
            for (int k = 0; k < cnt; ++k) {
                const uint32_t a = loud_abs_bits(x[s0 + k]);
                if (a > *peak_bits) *peak_bits = a;
            }
        for (int t = 0; t < LOUD_T; ++t) {
            LoudState s = {{0, 0, 0, 0}};
            if (t == 0) s = carry;
            for (int i = 0; i < LOUD_R; ++i) loud_step(p, s, at(t * LOUD_R + i));
            st[t] = s;
        }
        for (int k = 0; k < LOUD_LOG_T; ++k) {
            const int d = 1 << k;
            for (int t = 0; t < LOUD_T; ++t) nx[t] = t >= d ? loud_combine(p.P[k], st[t - d], st[t]) : st[t];
            memcpy(st, nx, sizeof st);
        }
        for (int t = 0; y && t < LOUD_T && t * LOUD_R < cnt; ++t) {
            LoudState s = t == 0 ? carry : st[t - 1];
            for (int i = 0; i < LOUD_R; ++i) {
                const double v = loud_step(p, s, at(t * LOUD_R + i));
                if (t * LOUD_R + i < cnt) y[s0 + t * LOUD_R + i] = loud_store(v);
            }
        }
        carry = st[LOUD_T - 1];
    }
    return carry;
}

// the true start state of every chunk of a clip from the chunks' end states: what one thread of loud_chain_kernel does
LOUD_HD void loud_chain(const LoudParams& p, int nch, const LoudState* ends, LoudState* starts) {
    LoudState s = {{0, 0, 0, 0}};
    for (int c = 0; c < nch; ++c) {
        starts[c] = s;
        if (c + 1 < nch) s = loud_combine(p.P[LOUD_NP - 1], s, ends[c]);
    }
}

// stage 1 of one clip over host memory: y and the peak bits, chunk by chunk as the three launches do it
inline void loud_filter_host(const float* x, const LoudRow& r, const LoudParams& p, float* y, LoudState* ends, LoudState* starts,
                             uint32_t* peak_bits) {
    const LoudState zero = {{0, 0, 0, 0}};
    for (int c = 0; c + 1 < r.nch; ++c) ends[c] = loud_chunk_host(x, c * LOUD_CHUNK, (c + 1) * LOUD_CHUNK, p, zero, nullptr, nullptr);
    loud_chain(p, r.nch, ends, starts);
    *peak_bits = 0;
    for (int c = 0; c < r.nch; ++c) {
        const long long hi = (long long)(c + 1) * LOUD_CHUNK;
        loud_chunk_host(x, c * LOUD_CHUNK, hi < r.n ? (int)hi : r.n, p, starts[c], y, peak_bits);
    }
}

// stage 2: block j of a clip
inline double loud_block_host(const float* y, int j, int n, const LoudParams& p) {
    int lo, hi;
    loud_block_bounds(j, n, p.rate, &lo, &hi);
    double v[LOUD_LANES];
    for (int lane = 0; lane < LOUD_LANES; ++lane) {
        double acc = 0.0;
        for (int i = lo + lane; i < hi; i += LOUD_LANES) acc = fma((double)y[i], (double)y[i], acc);
        v[lane] = acc;
    }
    loud_tree_host(v);
    return v[0] / p.gate_len;
}

// stage 3: both gates over the clip's block values
inline LoudRecord loud_decide_host(const LoudRow& row, const LoudParams& p, const double* z, uint32_t peak_bits) {
    double v[LOUD_LANES];
    int above = 0, kept = 0;
    for (int lane = 0; lane < LOUD_LANES; ++lane) {
        double acc = 0.0;
        for (int j = lane; j < row.nb; j += LOUD_LANES)
            if (loud_keep_abs(z[j], p.abs_thr)) { acc += z[j]; ++above; }
        v[lane] = acc;
    }
    loud_tree_host(v);
    double sum = 0.0;
    if (above > 0) {
        const double rel = 0.1 * (v[0] / (double)above);
        for (int lane = 0; lane < LOUD_LANES; ++lane) {
            double acc = 0.0;
            for (int j = lane; j < row.nb; j += LOUD_LANES)
                if (loud_keep_both(z[j], p.abs_thr, rel)) { acc += z[j]; ++kept; }
            v[lane] = acc;
        }
        loud_tree_host(v);
        sum = v[0];
    }
    return loud_finish(row, p, peak_bits, above, kept, sum);
}

// the whole call over host memory.  work holds loud_layout's bytes; out may be null (measure only) or x (in place).
inline void loud_run_host(const float* x, const LoudClip* clips, int n_clips, int rate, float peak_limit, float* out, LoudRecord* records,
                          unsigned char* work) {
    LoudLayout L;
    LoudRow* rows = reinterpret_cast<LoudRow*>(work);
    if (!loud_layout(clips, n_clips, rate, 0, false, &L, rows)) return;
    const LoudParams p = loud_params(rate, peak_limit);
    float* y = reinterpret_cast<float*>(work + L.y_off);
    double* z = reinterpret_cast<double*>(work + L.z_off);
    uint32_t* peaks = reinterpret_cast<uint32_t*>(work + L.peak_off);
    LoudState* ends = reinterpret_cast<LoudState*>(work + L.ends_off);
    LoudState* starts = reinterpret_cast<LoudState*>(work + L.starts_off);
    for (int c = 0; c < n_clips; ++c) {
        const LoudRow& r = rows[c];
        loud_filter_host(x + r.offset, r, p, y + r.yoff, ends + r.soff, starts + r.soff, &peaks[c]);
        for (int j = 0; j < r.nb; ++j) z[r.zoff + j] = loud_block_host(y + r.yoff, j, r.n, p);
        records[c] = loud_decide_host(r, p, z + r.zoff, peaks[c]);
        if (!out) continue;
        const float g = records[c].gain;
        if (g == 1.f) {
            if (out != x) memcpy(out + r.offset, x + r.offset, (size_t)r.n * sizeof(float));
        } else {
            for (int i = 0; i < r.n; ++i) out[r.offset + i] = x[r.offset + i] * g;
        }
    }
}

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------------------------------
// the device kernels
// ------------------------------------------------------------------------------------------------------------------
// Stage 1, one block per chunk of a clip.  ENDS: the first half over the chunks that have a successor -- from zero state to the
// chunk's end state, nothing else written.  Else the full pass from the chunk's true start state: y and the peak.  The span is
// staged in LDS by coalesced loads, each thread's run padded by one float so the runs start in different banks; y goes back
// through the same slots.
template <bool ENDS>
static __global__ __launch_bounds__(LOUD_T) void loud_filter_kernel(const float* __restrict__ x, const LoudRow* __restrict__ rows,
                                                                    const LoudParams p, float* __restrict__ yws,
                                                                    LoudState* __restrict__ ends, const LoudState* __restrict__ starts,
                                                                    uint32_t* __restrict__ peaks) {
    __shared__ float xs[LOUD_T * (LOUD_R + 1)];
    __shared__ double st[4][LOUD_T];
    __shared__ uint32_t peak_s;
    const LoudRow row = rows[blockIdx.y];
    const int tid = threadIdx.x, chunk = blockIdx.x;
    if (chunk >= (ENDS ? row.nch - 1 : row.nch)) return;       // block-uniform
    const long long chunk_hi = (long long)(chunk + 1) * LOUD_CHUNK;
    const int lo = chunk * LOUD_CHUNK, hi = chunk_hi < row.n ? (int)chunk_hi : row.n;
    const float* __restrict__ xc = x + row.offset;
    float* __restrict__ yc = yws + row.yoff;
    if (tid == 0) peak_s = 0;
    uint32_t peak = 0;
    LoudState carry = {{0, 0, 0, 0}};
    if (!ENDS) carry = starts[row.soff + chunk];
    float* mine = xs + tid * (LOUD_R + 1);
    for (int s0 = lo; s0 < hi; s0 += LOUD_SPAN) {
        const int cnt = hi - s0 < LOUD_SPAN ? hi - s0 : LOUD_SPAN;
        for (int k = tid; k < LOUD_SPAN; k += LOUD_T) {
            float v = 0.f;
            if (k < cnt) {
                v = xc[s0 + k];
                const uint32_t a = loud_abs_bits(v);
                peak = a > peak ? a : peak;
            }
            xs[(k / LOUD_R) * (LOUD_R + 1) + k % LOUD_R] = v;
        }
        __syncthreads();
        LoudState s = {{0, 0, 0, 0}};
        if (tid == 0) s = carry;
        for (int i = 0; i < LOUD_R; ++i) loud_step(p, s, (double)mine[i]);
        for (int k = 0; k < LOUD_LOG_T; ++k) {
            const int d = 1 << k;
            for (int i = 0; i < 4; ++i) st[i][tid] = s.s[i];
            __syncthreads();
            if (tid >= d) {
                LoudState left;
                for (int i = 0; i < 4; ++i) left.s[i] = st[i][tid - d];
                s = loud_combine(p.P[k], left, s);
            }
            __syncthreads();
        }
        for (int i = 0; i < 4; ++i) st[i][tid] = s.s[i];
        __syncthreads();
        LoudState start = carry;
        if (tid > 0)
            for (int i = 0; i < 4; ++i) start.s[i] = st[i][tid - 1];
        for (int i = 0; i < 4; ++i) carry.s[i] = st[i][LOUD_T - 1];
        if (!ENDS) {
            if (tid * LOUD_R < cnt)
                for (int i = 0; i < LOUD_R; ++i) mine[i] = loud_store(loud_step(p, start, (double)mine[i]));
            __syncthreads();
            for (int k = tid; k < cnt; k += LOUD_T) yc[s0 + k] = xs[(k / LOUD_R) * (LOUD_R + 1) + k % LOUD_R];
        }
        __syncthreads();        // the next span stages over xs and st
    }
    if (ENDS) {
        if (tid == 0) ends[row.soff + chunk] = carry;
        return;
    }
    __syncthreads();
    atomicMax(&peak_s, peak);
    __syncthreads();
    if (tid == 0) atomicMax(&peaks[blockIdx.y], peak_s);        // an integer maximum: the order of the chunks does not show
}

// between the two: one thread per clip chains its chunks and clears the clip's peak
static __global__ __launch_bounds__(LOUD_LANES) void loud_chain_kernel(const LoudRow* __restrict__ rows, int n_clips, const LoudParams p,
                                                                       const LoudState* __restrict__ ends, LoudState* __restrict__ starts,
                                                                       uint32_t* __restrict__ peaks) {
    const int c = blockIdx.x * LOUD_LANES + threadIdx.x;
    if (c >= n_clips) return;
    const LoudRow row = rows[c];
    peaks[c] = 0;
    loud_chain(p, row.nch, ends + row.soff, starts + row.soff);
}

// the sum of the 64 lanes' values in loud_tree_host's order; every lane calls, lane 0's return is the sum
__device__ __forceinline__ double loud_tree_dev(double* red, double v, int lane) {
    red[lane] = v;
    for (int d = LOUD_LANES / 2; d >= 1; d >>= 1) {
        __syncthreads();
        if (lane < d) red[lane] += red[lane + d];
    }
    __syncthreads();
    const double r = red[0];
    __syncthreads();
    return r;
}

// Stage 2, one wave per (block j, clip)
static __global__ __launch_bounds__(LOUD_LANES) void loud_blocks_kernel(const LoudRow* __restrict__ rows, const LoudParams p,
                                                                        const float* __restrict__ yws, double* __restrict__ zws) {
    __shared__ double red[LOUD_LANES];
    const LoudRow row = rows[blockIdx.y];
    const int j = blockIdx.x, lane = threadIdx.x;
    if (j >= row.nb) return;
    int lo, hi;
    loud_block_bounds(j, row.n, p.rate, &lo, &hi);
    const float* __restrict__ y = yws + row.yoff;
    double acc = 0.0;
    for (int i = lo + lane; i < hi; i += LOUD_LANES) {
        const double v = (double)y[i];
        acc = fma(v, v, acc);
    }
    const double sum = loud_tree_dev(red, acc, lane);
    if (lane == 0) zws[row.zoff + j] = sum / p.gate_len;
}

// Stage 3, one wave per clip
static __global__ __launch_bounds__(LOUD_LANES) void loud_decide_kernel(const LoudRow* __restrict__ rows, const LoudParams p,
                                                                        const double* __restrict__ zws, const uint32_t* __restrict__ peaks,
                                                                        LoudRecord* __restrict__ records) {
    __shared__ double red[LOUD_LANES];
    __shared__ int cnt_s[2];
    const LoudRow row = rows[blockIdx.x];
    const int lane = threadIdx.x;
    const double* __restrict__ z = zws + row.zoff;
    if (lane < 2) cnt_s[lane] = 0;
    __syncthreads();
    double acc = 0.0;
    int c = 0;
    for (int j = lane; j < row.nb; j += LOUD_LANES) {
        const double v = z[j];
        if (loud_keep_abs(v, p.abs_thr)) { acc += v; ++c; }
    }
    atomicAdd(&cnt_s[0], c);
    const double sum_a = loud_tree_dev(red, acc, lane);
    const int above = cnt_s[0];
    double sum = 0.0;
    if (above > 0) {            // block-uniform
        const double rel = 0.1 * (sum_a / (double)above);
        acc = 0.0; c = 0;
        for (int j = lane; j < row.nb; j += LOUD_LANES) {
            const double v = z[j];
            if (loud_keep_both(v, p.abs_thr, rel)) { acc += v; ++c; }
        }
        atomicAdd(&cnt_s[1], c);
        sum = loud_tree_dev(red, acc, lane);
    }
    if (lane == 0) records[blockIdx.x] = loud_finish(row, p, peaks[blockIdx.x], above, cnt_s[1], sum);
}

// Stage 4: out = x * gain inside [offset, offset + n) of every clip.  In place a gain of 1 writes nothing.
static __global__ __launch_bounds__(256) void loud_scale_kernel(const float* x, const LoudRow* __restrict__ rows,
                                                                const LoudRecord* __restrict__ records, float* out) {
    const LoudRow row = rows[blockIdx.y];
    const float g = records[blockIdx.y].gain;
    const bool copy = g == 1.f;
    if (copy && out == x) return;
    const float* xc = x + row.offset;        // out may be x: no restrict
    float* oc = out + row.offset;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < row.n; i += gridDim.x * 256) oc[i] = copy ? xc[i] : xc[i] * g;
}
#endif

}  // namespace gsv
