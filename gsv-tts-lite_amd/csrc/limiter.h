// limiter: the true peak of B packed fp32 clips and a look-ahead limiter that holds each under its ceiling.
// Seven stages, every one a FIR, a sliding minimum, a min-plus prefix scan or a moving average:
//   1  e[n] = max |u[4n-3 .. 4n+3]|, u the clip oversampled 4x by a 49-tap windowed sinc (12 taps per phase, phase 0 the
//      identity, zeros outside the clip); the clip's true peak in = max e
//   2  c[n] = min(1, T / e[n])                               the gain every sample needs
//   3  h[n] = min c[n .. n+L-1]                              hold over the look-ahead, c = 1 behind the clip's end
//   4  r[n] = min(h[n], min_{k<=n} (h[k] + (n-k) s))         release: the gain rises by at most s = 1/R per sample
//   5  g[n] = min(c[n], (sum_{i<L} r[n-i]) (1/L))            attack: the moving average over the look-ahead, r[m<0] = r[0]
//   6  y1 = g x
//   7  t = min(1, T / truepeak(y1)), y = t y1                the trim: smoothing moves the peaks between the samples a little
//
// Everything that decides a bit is one __host__ __device__ text for the kernels, for the host twin lim_run_host
// (gsv_limiter_host: the CPU path and the device's oracle) and for the stand-alone checker tools/limiter_host_check.cpp.  All
// arithmetic is fp32.  Every multiply-add is an explicit fmaf, every other product stands alone (g x, t y1, sum * (1/L)) or
// is formed on the host (the scan's offsets d s), and every order is fixed, so contraction has nothing to change and device
// samples and records equal the host's bit for bit.  Maxima and minima are exact in any order; the peaks are kept as the
// maximum of the floats' bits, as loud_filter_kernel keeps its peak.  The device takes no sin, pow or division by a table:
// the taps are built on the host in fp64 and cast to fp32 (lim_params), as loudness.h and track.h build theirs.
//
// The release scan.  A tile is LIM_TILE samples, one per thread.  Inside a tile a Hillis-Steele scan takes
// v[n] = min(v[n], v[n-d] + d s) for d = 1, 2, .. LIM_TILE/2 from v = h, the offsets d s exact products of a power of two;
// the tile's last v goes to `ends`.  One thread per clip chains the tiles: starts[t] is r at the last sample before tile t
// (1 before the first), starts[t+1] = min(ends[t], starts[t] + LIM_TILE s).  Then r[n] = min(v[n], starts[t] + (n - lo + 1) s),
// one fmaf.  No offset is formed from a distance longer than a tile.  Rounding: at most LIM_LOG_TILE additions inside the
// tile, one fmaf per chained tile and one at the end, each at most 2^-24 (half an ulp of a value below 2; a value above 1 never
// wins a minimum against h <= 1); a chained value that has risen to 1 is replaced by the exact value of the next tile's own
// samples, and it rises to 1 within R samples, so the chain carries rounding over ceil(R / LIM_TILE) + 1 tiles at the most:
// |r - exact| <= (LIM_LOG_TILE + ceil(R / LIM_TILE) + 3) 2^-24, the rounding of s = fl(1 / R) included.
//
// Workspace: [LimRow rows[B] | LimStat stats[B] | c | h | v | r | g fp32, each [sum of n] | ends | starts fp32, each [sum of
// tiles]], every part 16-byte aligned.  Clip k's part of a stage array starts at the sum of the lengths before it.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define LIM_HD __host__ __device__ inline
#else
#define LIM_HD inline
#endif

namespace gsv {

constexpr int LIM_TILE = 1024;                  // samples of a scan tile: one per thread
constexpr int LIM_LOG_TILE = 10;
constexpr int LIM_ENV_T = 256;                  // samples of one round of an envelope block
constexpr int LIM_ENV_SPAN = 8 * LIM_ENV_T;     // samples an envelope block walks: one atomic on the clip's peak for all of them
constexpr int LIM_PHASES = 3, LIM_TAPS = 12;    // the phases between two samples; taps of each
constexpr int LIM_MAX_L = 4096;                 // longest look-ahead: the halo of a tile in LDS
constexpr int LIM_MAX_R = 1 << 24;
constexpr int LIM_MAX_CLIPS = 65535;
constexpr int LIM_LIMITED = 1, LIM_NONFINITE = 4;       // record flags
static_assert(LIM_TILE == 1 << LIM_LOG_TILE, "scan steps");

struct LimClip {            // gsv_limiter_clip
    long long offset;       // first sample in the packed buffer
    int32_t n;
    float ceiling_db;       // dBTP; NaN: measure only
};
static_assert(sizeof(LimClip) == 16, "clip");

struct LimRecord {          // gsv_limiter_record
    float true_peak_in;     // max e of the clip as it came
    float true_peak_out;    // trim * the true peak of y1
    float min_gain;         // min g (1 when nothing was limited)
    float trim;
    int32_t flags, lookahead, release, pad;
};
static_assert(sizeof(LimRecord) == 32, "record");

struct LimRow {             // one clip as the kernels see it (built on the host, first part of the workspace)
    long long offset, soff, toff;       // in x; in the stage arrays; in ends / starts
    float T;                // 10^(ceiling_db / 20); NaN: measure only
    int32_t n, nt, pad;
};
static_assert(sizeof(LimRow) == 40, "row");

struct LimStat { uint32_t peak_in, peak_out, min_gain, pad; };      // the bits of floats >= 0: their order is the integers'

struct LimParams {
    float tab[LIM_PHASES][LIM_TAPS];    // tab[p-1][j]: the tap of sample g - 5 + j for u[4g + p]
    float ds[LIM_LOG_TILE];             // (1 << k) * s
    float s, inv_L;
    int32_t L, R;
};

LIM_HD uint32_t lim_abs_bits(float x) {
    uint32_t u;
    memcpy(&u, &x, 4);
    return u & 0x7FFFFFFFu;
}
LIM_HD float lim_from_bits(uint32_t u) {
    float f;
    memcpy(&f, &u, 4);
    return f;
}
LIM_HD float lim_min(float a, float b) { return b < a ? b : a; }
LIM_HD uint32_t lim_umax(uint32_t a, uint32_t b) { return b > a ? b : a; }

// the largest |u| between samples g and g + 1 as bits; w[j] is sample g - 5 + j (zero outside the clip).  fp32, tap order, fused
LIM_HD uint32_t lim_gap(const LimParams& p, const float* w) {
    uint32_t m = 0;
    for (int ph = 0; ph < LIM_PHASES; ++ph) {
        float acc = 0.f;
        for (int j = 0; j < LIM_TAPS; ++j) acc = fmaf(w[j], p.tab[ph][j], acc);
        m = lim_umax(m, lim_abs_bits(acc));
    }
    return m;
}

LIM_HD float lim_need(float e, float T) { return e > T ? T / e : 1.f; }     // c; 1 for a NaN of either

// whether stages 2 - 7 touch the clip: a ceiling, finite samples, a true peak above it
LIM_HD bool lim_active(float T, uint32_t peak_bits) { return T == T && peak_bits < 0x7F800000u && lim_from_bits(peak_bits) > T; }

// r of sample m of a clip from the tile scans and the chained starts
LIM_HD float lim_release(const LimParams& p, const float* v, const float* starts, int m) {
    return lim_min(v[m], fmaf((float)(m % LIM_TILE + 1), p.s, starts[m / LIM_TILE]));
}

// the chain over a clip's tiles: what one thread of lim_chain_kernel does
LIM_HD void lim_chain(const LimParams& p, int nt, const float* ends, float* starts) {
    float e = 1.f;
    for (int t = 0; t < nt; ++t) {
        starts[t] = e;
        e = lim_min(ends[t], fmaf((float)LIM_TILE, p.s, e));
    }
}

// the moving average behind sample n: newest[-i] = r[n - i]; fp32, i = 0 .. L-1
LIM_HD float lim_attack(const LimParams& p, float c, const float* newest) {
    float acc = 0.f;
    for (int i = 0; i < p.L; ++i) acc += newest[-i];
    return lim_min(c, acc * p.inv_L);
}

LIM_HD float lim_trim(float T, uint32_t peak_out) {
    const float tp = lim_from_bits(peak_out);
    return tp > T ? T / tp : 1.f;
}

LIM_HD LimRecord lim_finish(const LimRow& row, const LimParams& p, const LimStat& st) {
    LimRecord r;
    r.flags = 0; r.lookahead = p.L; r.release = p.R; r.pad = 0;
    r.min_gain = 1.f; r.trim = 1.f;
    if (st.peak_in >= 0x7F800000u) {            // the bits of a NaN differ from machine to machine: one NaN for all
        r.flags = LIM_NONFINITE;
        r.true_peak_in = r.true_peak_out = lim_from_bits(st.peak_in > 0x7F800000u ? 0x7FC00000u : 0x7F800000u);
        return r;
    }
    r.true_peak_in = r.true_peak_out = lim_from_bits(st.peak_in);
    if (!lim_active(row.T, st.peak_in)) return r;
    r.flags = LIM_LIMITED;
    r.min_gain = lim_from_bits(st.min_gain);
    r.trim = lim_trim(row.T, st.peak_out);
    const float tp = lim_from_bits(st.peak_out);
    r.true_peak_out = r.trim == 1.f ? tp : r.trim * tp;
    return r;
}

// ------------------------------------------------------------------------------------------------------------------
// host only: the constants, the workspace layout, the serial twin
// ------------------------------------------------------------------------------------------------------------------
inline size_t lim_align16(size_t v) { return (v + 15) & ~(size_t)15; }

struct LimLayout {
    size_t rows_off, stats_off, c_off, h_off, v_off, r_off, g_off, ends_off, starts_off, bytes;
    long long s_total, t_total;
    int max_n, max_nt;
};

// false on arguments the entries refuse; fills the rows when `rows` is given
inline bool lim_layout(const LimClip* clips, int n_clips, size_t n_x, bool check_x, LimLayout* L, LimRow* rows) {
    if (!clips || n_clips < 1 || n_clips > LIM_MAX_CLIPS) return false;
    long long s = 0, t = 0;
    int max_n = 0, max_nt = 0;
    for (int c = 0; c < n_clips; ++c) {
        const LimClip& cl = clips[c];
        if (cl.n < 0 || cl.offset < 0) return false;
        if (cl.ceiling_db == cl.ceiling_db && !(cl.ceiling_db <= 0.f && cl.ceiling_db >= -200.f)) return false;
        if (check_x && (unsigned long long)cl.offset + (unsigned long long)cl.n > (unsigned long long)n_x) return false;
        const int nt = (int)(((long long)cl.n + LIM_TILE - 1) / LIM_TILE);
        if (rows) {
            LimRow& r = rows[c];
            r.offset = cl.offset; r.soff = s; r.toff = t;
            r.T = cl.ceiling_db == cl.ceiling_db ? (float)pow(10.0, (double)cl.ceiling_db / 20.0) : NAN;
            r.n = cl.n; r.nt = nt; r.pad = 0;
        }
        s += cl.n;
        t += nt;
        if (cl.n > max_n) max_n = cl.n;
        if (nt > max_nt) max_nt = nt;
    }
    const size_t stage = lim_align16((size_t)s * sizeof(float)), tiles = lim_align16((size_t)t * sizeof(float));
    L->rows_off = 0;
    L->stats_off = lim_align16((size_t)n_clips * sizeof(LimRow));
    L->c_off = L->stats_off + lim_align16((size_t)n_clips * sizeof(LimStat));
    L->h_off = L->c_off + stage;
    L->v_off = L->h_off + stage;
    L->r_off = L->v_off + stage;
    L->g_off = L->r_off + stage;
    L->ends_off = L->g_off + stage;
    L->starts_off = L->ends_off + tiles;
    L->bytes = L->starts_off + tiles;
    L->s_total = s; L->t_total = t; L->max_n = max_n; L->max_nt = max_nt;
    return true;
}

inline bool lim_times_ok(int lookahead, int release) {
    return lookahead >= 1 && lookahead <= LIM_MAX_L && release >= 1 && release <= LIM_MAX_R;
}

inline double lim_bessel_i0(double x) {
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 200; ++k) {
        term *= (x / 2.0) / k * ((x / 2.0) / k);
        sum += term;
        if (term < 1e-18 * sum) break;
    }
    return sum;
}

// tap k (-24 .. 24) of the 49-tap table: sinc(k / 4) * kaiser(49, beta = 8), fp64
inline double lim_tap(int k) {
    const double kPi = 3.14159265358979323846, beta = 8.0;
    const double t = (double)k / 4.0, a = (double)k / 24.0;
    const double sinc = k == 0 ? 1.0 : sin(kPi * t) / (kPi * t);
    return sinc * (lim_bessel_i0(beta * sqrt(1.0 - a * a)) / lim_bessel_i0(beta));
}

inline LimParams lim_params(int lookahead, int release) {
    LimParams p;
    memset(&p, 0, sizeof p);
    // u[4g + ph] = sum_m x[m] tap(4 (g - m) + ph): sample g - 5 + j meets tap 4 (5 - j) + ph
    for (int ph = 1; ph <= LIM_PHASES; ++ph)
        for (int j = 0; j < LIM_TAPS; ++j) p.tab[ph - 1][j] = (float)lim_tap(4 * (5 - j) + ph);
    p.L = lookahead; p.R = release;
    p.s = 1.f / (float)release;
    p.inv_L = 1.f / (float)lookahead;
    for (int k = 0; k < LIM_LOG_TILE; ++k) p.ds[k] = (float)(1 << k) * p.s;
    return p;
}

// stage 1 of one clip: e's bits into peak; c when given (T as the clip's row says)
inline void lim_envelope_host(const float* x, int n, float T, const LimParams& p, float* c, uint32_t* peak) {
    auto at = [&](long long i) { return i >= 0 && i < n ? x[i] : 0.f; };
    uint32_t left = 0;
    {
        float w[LIM_TAPS];
        for (int j = 0; j < LIM_TAPS; ++j) w[j] = at(-1 - 5 + j);
        left = lim_gap(p, w);
    }
    for (int i = 0; i < n; ++i) {
        float w[LIM_TAPS];
        for (int j = 0; j < LIM_TAPS; ++j) w[j] = at((long long)i - 5 + j);
        const uint32_t right = lim_gap(p, w);
        const uint32_t e = lim_umax(lim_abs_bits(x[i]), lim_umax(left, right));
        *peak = lim_umax(*peak, e);
        if (c) c[i] = lim_need(lim_from_bits(e), T);
        left = right;
    }
}

// stages 3 and 4 of one tile as one block of lim_hold_kernel runs it
inline float lim_hold_tile_host(const float* c, int n, int lo, const LimParams& p, float* h, float* v) {
    static thread_local float st[LIM_TILE], nx[LIM_TILE];
    for (int t = 0; t < LIM_TILE; ++t) {
        float m = 1.f;
        const int i = lo + t;
        for (int k = 0; k < p.L && i + k < n; ++k) m = lim_min(m, c[i + k]);
        st[t] = m;
        if (i < n) h[i] = m;
    }
    for (int k = 0; k < LIM_LOG_TILE; ++k) {
        const int d = 1 << k;
        for (int t = 0; t < LIM_TILE; ++t) nx[t] = t >= d ? lim_min(st[t], st[t - d] + p.ds[k]) : st[t];
        memcpy(st, nx, sizeof st);
    }
    for (int t = 0; t < LIM_TILE && lo + t < n; ++t) v[lo + t] = st[t];
    return st[LIM_TILE - 1];
}

// the whole call over host memory.  work holds lim_layout's bytes; out may be null (measure only) or x (in place).
inline void lim_run_host(const float* x, const LimClip* clips, int n_clips, int lookahead, int release, float* out, LimRecord* records,
                         unsigned char* work) {
    LimLayout L;
    LimRow* rows = reinterpret_cast<LimRow*>(work);
    if (!lim_layout(clips, n_clips, 0, false, &L, rows)) return;
    const LimParams p = lim_params(lookahead, release);
    LimStat* stats = reinterpret_cast<LimStat*>(work + L.stats_off);
    auto arr = [&](size_t off) { return reinterpret_cast<float*>(work + off); };
    for (int k = 0; k < n_clips; ++k) {
        const LimRow& row = rows[k];
        const float* xc = x + row.offset;
        float *c = arr(L.c_off) + row.soff, *h = arr(L.h_off) + row.soff, *v = arr(L.v_off) + row.soff, *r = arr(L.r_off) + row.soff,
              *g = arr(L.g_off) + row.soff, *ends = arr(L.ends_off) + row.toff, *starts = arr(L.starts_off) + row.toff;
        LimStat& st = stats[k];
        st.peak_in = 0; st.peak_out = 0; st.min_gain = 0x3F800000u; st.pad = 0;
        lim_envelope_host(xc, row.n, row.T, p, c, &st.peak_in);
        if (out) {
            float* oc = out + row.offset;
            for (int t = 0; t < row.nt; ++t) ends[t] = lim_hold_tile_host(c, row.n, t * LIM_TILE, p, h, v);
            lim_chain(p, row.nt, ends, starts);
            const bool active = lim_active(row.T, st.peak_in);
            static thread_local float win[LIM_MAX_L];
            for (int i = 0; i < row.n; ++i) {
                r[i] = lim_release(p, v, starts, i);
                if (!active) { g[i] = 1.f; continue; }
                for (int j = 0; j < p.L; ++j) win[p.L - 1 - j] = r[i - j > 0 ? i - j : 0];
                g[i] = lim_attack(p, c[i], win + p.L - 1);
                st.min_gain = g[i] < lim_from_bits(st.min_gain) ? lim_abs_bits(g[i]) : st.min_gain;
            }
            if (active)
                for (int i = 0; i < row.n; ++i) oc[i] = g[i] * xc[i];
            else if (oc != xc && row.n > 0)
                memcpy(oc, xc, (size_t)row.n * sizeof(float));
            lim_envelope_host(oc, row.n, row.T, p, nullptr, &st.peak_out);
            const float t = lim_trim(row.T, st.peak_out);
            if (active && t != 1.f)
                for (int i = 0; i < row.n; ++i) oc[i] = t * oc[i];
        } else {
            st.peak_out = st.peak_in;
        }
        LimRow measured = row;
        if (!out) measured.T = NAN;
        records[k] = lim_finish(measured, p, st);
    }
}

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------------------------------
// the device kernels
// ------------------------------------------------------------------------------------------------------------------
// Stages 1 and 2 (NEED), or the envelope alone: one block per LIM_ENV_SPAN samples of a clip, LIM_ENV_T at a time.  The samples
// of a round and a halo of six on each side are staged in LDS; thread q takes the gap in front of sample lo + q (the block's
// first thread one more, behind the round's last sample), then every sample takes the larger of itself and its two gaps.
template <bool NEED>
static __global__ __launch_bounds__(LIM_ENV_T) void lim_envelope_kernel(const float* __restrict__ x, const LimRow* __restrict__ rows,
                                                                        const LimParams p, float* __restrict__ cws,
                                                                        LimStat* __restrict__ stats) {
    __shared__ float xs[LIM_ENV_T + LIM_TAPS + 1];      // sample lo - 6 + k
    __shared__ uint32_t gap[LIM_ENV_T + 1];             // the gap behind sample lo - 1 + q
    __shared__ uint32_t peak_s;
    const LimRow row = rows[blockIdx.y];
    const int tid = threadIdx.x;
    const long long first = (long long)blockIdx.x * LIM_ENV_SPAN;
    if (first >= row.n) return;                         // block-uniform
    const float* __restrict__ xc = x + row.offset;
    if (tid == 0) peak_s = 0;
    uint32_t e = 0;
    for (long long lo = first; lo < first + LIM_ENV_SPAN && lo < row.n; lo += LIM_ENV_T) {     // block-uniform
        for (int k = tid; k < LIM_ENV_T + LIM_TAPS + 1; k += LIM_ENV_T) {
            const long long i = lo - 6 + k;
            xs[k] = i >= 0 && i < row.n ? xc[i] : 0.f;
        }
        __syncthreads();
        for (int q = tid; q < LIM_ENV_T + 1; q += LIM_ENV_T) gap[q] = lim_gap(p, xs + q);
        __syncthreads();
        if (lo + tid < row.n) {
            const uint32_t en = lim_umax(lim_abs_bits(xs[tid + 6]), lim_umax(gap[tid], gap[tid + 1]));
            if (NEED) cws[row.soff + lo + tid] = lim_need(lim_from_bits(en), row.T);
            e = lim_umax(e, en);
        }
        __syncthreads();                                // the next round stages over xs and gap
    }
    for (int d = 32; d >= 1; d >>= 1) e = lim_umax(e, (uint32_t)__shfl_xor((int)e, d));
    if ((tid & 63) == 0) atomicMax(&peak_s, e);
    __syncthreads();
    if (tid == 0) atomicMax(NEED ? &stats[blockIdx.y].peak_in : &stats[blockIdx.y].peak_out, peak_s);
}

// Stages 3 and 4 inside a tile: c with its look-ahead halo in LDS, the sliding minimum, the Hillis-Steele min-plus scan
static __global__ __launch_bounds__(LIM_TILE) void lim_hold_kernel(const LimRow* __restrict__ rows, const LimParams p,
                                                                   const float* __restrict__ cws, float* __restrict__ hws,
                                                                   float* __restrict__ vws, float* __restrict__ ends) {
    __shared__ float cs[LIM_TILE + LIM_MAX_L - 1];
    __shared__ float sv[LIM_TILE];
    const LimRow row = rows[blockIdx.y];
    const int tid = threadIdx.x, tile = blockIdx.x;
    if (tile >= row.nt) return;                         // block-uniform
    const int lo = tile * LIM_TILE;                     // < n <= INT_MAX
    const float* __restrict__ c = cws + row.soff;
    for (int k = tid; k < LIM_TILE + p.L - 1; k += LIM_TILE) cs[k] = (long long)lo + k < row.n ? c[lo + k] : 1.f;
    __syncthreads();
    float v = 1.f;
    for (int k = 0; k < p.L; ++k) v = lim_min(v, cs[tid + k]);
    const bool inside = (long long)lo + tid < row.n;
    if (inside) hws[row.soff + lo + tid] = v;
    for (int k = 0; k < LIM_LOG_TILE; ++k) {
        const int d = 1 << k;
        sv[tid] = v;
        __syncthreads();
        if (tid >= d) v = lim_min(v, sv[tid - d] + p.ds[k]);
        __syncthreads();
    }
    if (inside) vws[row.soff + lo + tid] = v;
    if (tid == LIM_TILE - 1) ends[row.toff + tile] = v;
}

// between the two: one thread per clip chains its tiles
static __global__ __launch_bounds__(64) void lim_chain_kernel(const LimRow* __restrict__ rows, int n_clips, const LimParams p,
                                                              const float* __restrict__ ends, float* __restrict__ starts) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= n_clips) return;
    const LimRow row = rows[c];
    lim_chain(p, row.nt, ends + row.toff, starts + row.toff);
}

// Stages 4 (the chained starts folded in), 5 and 6: r with its look-ahead halo in LDS, the moving average, y1 = g x.  A clip
// that is not limited is copied (in place: left alone).
static __global__ __launch_bounds__(LIM_TILE) void lim_attack_kernel(const float* x, const LimRow* __restrict__ rows, const LimParams p,
                                                                     const float* __restrict__ cws, const float* __restrict__ vws,
                                                                     const float* __restrict__ starts, float* __restrict__ rws,
                                                                     float* __restrict__ gws, LimStat* stats, float* out) {
    __shared__ float rs[LIM_TILE + LIM_MAX_L - 1];      // r of sample lo - (L - 1) + k
    __shared__ uint32_t min_s;
    const LimRow row = rows[blockIdx.y];
    const int tid = threadIdx.x, tile = blockIdx.x;
    if (tile >= row.nt) return;                         // block-uniform
    const int lo = tile * LIM_TILE;
    const bool active = lim_active(row.T, stats[blockIdx.y].peak_in);      // written two launches ago
    const float* __restrict__ v = vws + row.soff;
    const float* __restrict__ st = starts + row.toff;
    const float* xc = x + row.offset;                   // out may be x: no restrict
    float* oc = out + row.offset;
    if (tid == 0) min_s = 0x3F800000u;
    for (int k = tid; k < LIM_TILE + p.L - 1; k += LIM_TILE) {
        long long m = (long long)lo - (p.L - 1) + k;
        if (m < 0) m = 0;
        rs[k] = m < row.n ? lim_release(p, v, st, (int)m) : 1.f;
    }
    __syncthreads();
    const bool inside = (long long)lo + tid < row.n;
    float g = 1.f;
    if (inside) {
        const long long i = row.soff + lo + tid;
        rws[i] = rs[tid + p.L - 1];
        if (active) g = lim_attack(p, cws[i], rs + tid + p.L - 1);
        gws[i] = g;
        if (active) oc[lo + tid] = g * xc[lo + tid];
        else if (oc != xc) oc[lo + tid] = xc[lo + tid];
    }
    if (!active) return;                                // block-uniform
    uint32_t gb = lim_abs_bits(g);
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)gb, d);
        gb = o < gb ? o : gb;
    }
    if ((tid & 63) == 0) atomicMin(&min_s, gb);
    __syncthreads();
    if (tid == 0) atomicMin(&stats[blockIdx.y].min_gain, min_s);
}

// Stage 7 and the record
static __global__ __launch_bounds__(256) void lim_trim_kernel(const LimRow* __restrict__ rows, const LimParams p,
                                                              const LimStat* __restrict__ stats, float* out,
                                                              LimRecord* __restrict__ records) {
    LimRow row = rows[blockIdx.y];
    const LimStat st = stats[blockIdx.y];
    if (!out) { row.T = NAN; }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        LimStat s = st;
        if (!out) s.peak_out = s.peak_in;
        records[blockIdx.y] = lim_finish(row, p, s);
    }
    if (!out || !lim_active(row.T, st.peak_in)) return;
    const float t = lim_trim(row.T, st.peak_out);
    if (t == 1.f) return;
    float* oc = out + row.offset;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < row.n; i += gridDim.x * 256) oc[i] = t * oc[i];
}
#endif

}  // namespace gsv
