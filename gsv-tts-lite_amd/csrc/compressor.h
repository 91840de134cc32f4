// compressor: a feed-forward dynamic range compressor over B packed fp32 clips, each clip with one of a few parameter sets
// (DESIGN 4.26).  The level detector is the smooth decoupled peak detector of Giannoulis, Massberg and Reiss (JAES 2012), from
// zero state, everything in fp64, one rounding to fp32 at the end (saturating, loud_store's rule); same length out as in:
//
//   p[n] = max(|x[n]|, aR p[n-1] + (1 - aR) |x[n]|)        the release: a max-affine recurrence
//   e[n] = aA e[n-1] + (1 - aA) p[n]                       the attack: a one-pole recurrence
//   g[n] = e[n] <= T ? 1 : exp2(s log2(e[n] (1/T)))        hard knee, s = 1/ratio - 1
//   y[n] = fp32((M g[n]) x[n])
//
// Everything that decides a bit -- the steps, the combines of the two scans, the chains of the chunks, log2 and exp2, the record
// -- is one __host__ __device__ text for the kernels, for the host twin cmp_run_host (gsv_compressor_host: the CPU path and the
// device's oracle) and for the stand-alone checker tools/compressor_host_check.cpp.  Every multiply-add is an explicit fma, every
// other product stands alone and every order is fixed, so contraction has nothing to change and device samples and records equal
// the host's bit for bit.  The device takes no exp, log or pow from a library: the caller hands in aA, aR, T, s and M, the powers
// of aR and aA are built on the host (cmp_design), and cmp_log2 / cmp_exp2 below are bits and fma polynomials.
//
// Why this detector scans.  As a map of the state, one step of p is y -> max(c, a y + b) with a >= 0, and such maps compose
// within the family: max(c2, a2 max(c1, a1 y + b1) + b2) = max(max(c2, a2 c1 + b2), a2 a1 y + (a2 b1 + b2)).  Over y >= 0 the
// map of a run is held by (B, C) -- B the affine recurrence from 0, C the max recurrence from 0, which is max(c, b) -- and its
// slope aR^length, which is known ahead.  (A detector that picks its coefficient by comparing the input with its own state is a
// maximum of two affine maps of the state, and compositions of those do not stay in a family of fixed size.)
//
// The scans.  A block of CMP_T threads takes a span of CMP_T * CMP_R samples; thread t holds its CMP_R consecutive samples in
// fp64 registers.  Stage p: the thread runs its |x| from zero state (thread 0: from the state the last span left) to (B, C), a
// Hillis-Steele scan with PR[k] = aR^(CMP_R 2^k) -- C <- max(C, A C_left + B), B <- A B_left + B -- gives every run's true end
// state, and the thread reruns its samples from the true end state of its left neighbour, which replaces them by p.  Stage e: the
// same with a linear scan of one value over the p the thread now holds, PA[k] = aA^(CMP_R 2^k); the rerun gives e, the gain and
// the product per sample.  A span shorter than CMP_T * CMP_R is padded with zeros behind the clip; what the padding turns into is
// never written, and a prefix of a scan depends on the runs to its left alone.
//
// A block carries the states from span to span over a chunk of CMP_CHUNK samples and the chunks of a clip run side by side.  The
// chain is not linear, so a chunk's end state of e needs the chunk's true p; three passes:
//   0  every chunk but the last: (B, C) of the chunk from zero state; one wave per clip then walks the chunks with aR^CMP_CHUNK
//      and leaves each chunk's start p;
//   1  every chunk but the last: from its true start p, the end e from zero state; the wave walks again with aA^CMP_CHUNK;
//   2  the full pass from both start states: y, both peaks, the smallest gain.
// p is recomputed in passes 1 and 2 and not parked: parking it is 8 bytes written and 16 read per sample of workspace traffic
// against 4 bytes of x read again and one more scan of two values in LDS, and the passes are bound by their barriers, not by x.
//
// y goes to the workspace, not to `out`: whether a clip holds a NaN or an infinity is known from the integer maximum of its |x|
// bit patterns only when the full pass is over, and such a clip comes back bit for bit.  The commit launch then writes the record
// and, per clip, y or x into `out` (in place and copied: nothing).  At most six launches, whatever the batch and the lengths.
//
// One text for clip and stream: cmpstream.h is the second caller of each of these.  On the device a block is cmp_open, per span
// cmp_body -- cmp_span and, in pass 2, the products and the run's statistics under a mask of the samples that count -- and
// cmp_close, around the kernel's own staging and write-back (cmp_slot: the padded runs); lane 0 of a chain wave calls
// cmp_chain_walk, which steps with cmp_link.  On the host cmp_walk_host is a chunk span by span (the caller says how a sample is
// loaded and what becomes of its gain) and cmp_drive_host the passes 0 and 1 with both chains, through cmp_chain_walk too.
//
// Workspace: [CmpRow rows[B] | CmpDesign designs[D] | y fp32 [sum of n, each clip 4-float aligned] | CmpChunk [sum of chunks] |
// stats u32 [3 B]: max |x| bits, max |y| bits, min gain bits].  Rows and designs are one upload.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "loudness.h"

namespace gsv {

constexpr int CMP_T = 512;                      // threads of the block
constexpr int CMP_LOG_T = 9;
constexpr int CMP_R = 16;                       // consecutive samples per thread and span
constexpr int CMP_SPAN = CMP_T * CMP_R;
constexpr int CMP_LOG_CH = 1;                   // a chunk is 2^CMP_LOG_CH spans
constexpr int CMP_CHUNK = CMP_SPAN << CMP_LOG_CH;
constexpr int CMP_LANES = 64;                   // lanes of the chain wave
constexpr int CMP_MAX_CLIPS = 65535, CMP_MAX_DESIGNS = 65535;
constexpr int CMP_COMPRESSED = 1, CMP_NONFINITE = 4;    // record flags
constexpr uint32_t CMP_ONE_BITS = 0x3F800000u;          // 1.0f
static_assert(CMP_T == 1 << CMP_LOG_T, "scan steps");
static_assert((CMP_R & (CMP_R - 1)) == 0 && (CMP_CHUNK & (CMP_CHUNK - 1)) == 0, "powers by squaring");

struct CmpClip {            // gsv_compressor_clip
    long long offset;       // first sample in the packed buffer
    int32_t n;
    int32_t design;         // index into the parameter sets of the call; -1: measure the peaks, copy
};
static_assert(sizeof(CmpClip) == 16, "clip");

struct CmpParams {          // gsv_compressor_params
    double attack, release; // aA, aR: the one-pole coefficients, in (0, 1)
    double threshold;       // T, linear
    double slope;           // s = 1 / ratio - 1, in [-1, 0]
    double makeup;          // M, linear
};
static_assert(sizeof(CmpParams) == 40, "params");

struct CmpRecord {          // gsv_compressor_record
    float peak_in, peak_out;            // max |x|, max |y|
    float min_gain;                     // the smallest g (makeup excluded) as fp32; 1 for a clip that was copied
    int32_t flags;
};
static_assert(sizeof(CmpRecord) == 16, "record");

struct CmpRow {             // one clip as the kernels see it (built on the host, first part of the workspace)
    long long offset, yoff, soff;       // soff: the clip's first chunk
    int32_t n, nch, design, pad;
};
static_assert(sizeof(CmpRow) == 40, "row");

struct CmpDesign {          // one parameter set as the kernels see it (built on the host, behind the rows)
    double aR, omR, aA, omA;            // the coefficients and 1 - them
    double T, invT, s, M;
    double PR[CMP_LOG_T], PA[CMP_LOG_T];        // aR^(CMP_R 2^k), aA^(CMP_R 2^k)
    double JR, JA;                              // aR^CMP_CHUNK, aA^CMP_CHUNK
};
static_assert(sizeof(CmpDesign) % 8 == 0, "design");

struct CmpChunk {           // what the passes leave per chunk
    double B, C;            // pass 0: the chunk's p map from zero state
    double pstart;          // chain 0: p in front of the chunk
    double eend;            // pass 1: e behind the chunk from zero state of e and the true p
    double estart;          // chain 1: e in front of the chunk
};

// no product of the routines below may melt into a neighbouring sum, here or where they are inlined
#if defined(__clang__)
#define CMP_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define CMP_NO_CONTRACT
#endif

LOUD_HD double cmp_from_bits(uint64_t u) {
    double d;
    memcpy(&d, &u, 8);
    return d;
}

// log2 of a positive, finite, normal v: the exponent by bits, the mantissa to m in (sqrt 1/2, sqrt 2], and with z = (m - 1) /
// (m + 1): ln m = 2 z (1 + z^2/3 + z^4/5 + ... + z^18/19); z^2 <= 0.0295, so the series is cut below 1e-16 of its sum.  Relative
// error a few 2^-53 (m - 1 is exact, so there is no cancellation next to 1); tests/test_compressor_cpu.py holds it to 2^-40.
LOUD_HD double cmp_log2(double v) {
    CMP_NO_CONTRACT
    uint64_t u;
    memcpy(&u, &v, 8);
    int k = (int)((u >> 52) & 0x7FFu) - 1023;
    double m = cmp_from_bits((u & 0x000FFFFFFFFFFFFFull) | 0x3FF0000000000000ull);
    if (m > 1.4142135623730951) { m = m * 0.5; k += 1; }
    const double f = m - 1.0;
    const double z = f / (2.0 + f);
    const double w = z * z;
    double q = 1.0 / 19.0;
    q = fma(w, q, 1.0 / 17.0);
    q = fma(w, q, 1.0 / 15.0);
    q = fma(w, q, 1.0 / 13.0);
    q = fma(w, q, 1.0 / 11.0);
    q = fma(w, q, 1.0 / 9.0);
    q = fma(w, q, 1.0 / 7.0);
    q = fma(w, q, 1.0 / 5.0);
    q = fma(w, q, 1.0 / 3.0);
    const double z2 = 2.0 * z;
    const double ln = fma(z2, w * q, z2);
    return fma(ln, 1.4426950408889634, (double)k);
}

// 2^t for t in [-1000, 1000] (clamped to it; a NaN gives 2^-1000): t = k + r with |r| <= 1/2, exp(r ln 2) by its series to the
// 13th power (|r ln 2| <= 0.347: cut below 1e-17), the scale by bits.  Relative error a few 2^-53.
LOUD_HD double cmp_exp2(double t) {
    CMP_NO_CONTRACT
    if (!(t > -1000.0)) t = -1000.0;
    if (t > 1000.0) t = 1000.0;
    const double kf = floor(t + 0.5);
    const double u = (t - kf) * 0.6931471805599453;
    double q = 1.0 / 6227020800.0;
    q = fma(u, q, 1.0 / 479001600.0);
    q = fma(u, q, 1.0 / 39916800.0);
    q = fma(u, q, 1.0 / 3628800.0);
    q = fma(u, q, 1.0 / 362880.0);
    q = fma(u, q, 1.0 / 40320.0);
    q = fma(u, q, 1.0 / 5040.0);
    q = fma(u, q, 1.0 / 720.0);
    q = fma(u, q, 1.0 / 120.0);
    q = fma(u, q, 1.0 / 24.0);
    q = fma(u, q, 1.0 / 6.0);
    q = fma(u, q, 0.5);
    q = fma(u, q, 1.0);
    q = fma(u, q, 1.0);
    return q * cmp_from_bits((uint64_t)((int)kf + 1023) << 52);
}

// one sample of the release: p behind |x| = ax; a NaN among the two gives ax
LOUD_HD double cmp_p_step(double aR, double omR, double p, double ax) {
    const double t = fma(aR, p, omR * ax);
    return t > ax ? t : ax;
}

// one sample of a one-pole recurrence: the affine part of the release (v = |x|) and the attack (v = p)
LOUD_HD double cmp_lin_step(double a, double om, double st, double v) { return fma(a, st, om * v); }

// own after left for the release: (B, C) of two adjacent stretches from (B, C) of each alone; A the slope of `own`
LOUD_HD void cmp_combine(double A, double Bl, double Cl, double& B, double& C) {
    const double t = fma(A, Cl, B);
    C = t > C ? t : C;
    B = fma(A, Bl, B);
}

LOUD_HD double cmp_gain(double T, double invT, double s, double e) {
    CMP_NO_CONTRACT
    return e <= T ? 1.0 : cmp_exp2(s * cmp_log2(e * invT));
}

LOUD_HD float cmp_out(double M, double g, float x) {
    CMP_NO_CONTRACT
    return loud_store((M * g) * (double)x);
}

LOUD_HD CmpRecord cmp_finish(const CmpRow& row, uint32_t peak_in, uint32_t peak_out, uint32_t gmin) {
    CmpRecord r;
    const bool nonfinite = peak_in >= 0x7F800000u, copied = nonfinite || row.design < 0;
    r.peak_in = loud_from_bits(peak_in);
    r.peak_out = loud_from_bits(copied ? peak_in : peak_out);
    r.min_gain = copied ? 1.f : loud_from_bits(gmin);
    r.flags = nonfinite ? CMP_NONFINITE : (r.min_gain < 1.f ? CMP_COMPRESSED : 0);
    return r;
}

// the samples of such a clip come from x, not from y
LOUD_HD bool cmp_copied(const CmpRow& row, const CmpRecord& r) { return row.design < 0 || (r.flags & CMP_NONFINITE); }

// one link of a chain: the state in front of the next chunk from the state `st` in front of chunk c.  stage 0: p, from the chunk's
// (B, C) with J = aR^CMP_CHUNK; 1: e, from its eend with J = aA^CMP_CHUNK
LOUD_HD double cmp_link(double J, int stage, double st, const CmpChunk& c) {
    if (stage == 0) {
        double B = c.B, C = c.C;
        cmp_combine(J, 0.0, st, B, C);
        return C;
    }
    return fma(J, st, c.eend);
}

// the chain: from the state `st` in front of the first of cnt chunks, of which the first `links` have a successor, out(c, state in
// front of chunk c) for every chunk -> the state behind the last link.  in(c) gives chunk c's (B, C) or eend and is asked for
// chunks that have a successor alone: the fields of the others were never written
template <class In, class Out>
LOUD_HD double cmp_chain_walk(double J, int stage, double st, int cnt, int links, In in, Out out) {
    for (int c = 0; c < cnt; ++c) {
        out(c, st);
        if (c < links) st = cmp_link(J, stage, st, in(c));
    }
    return st;
}

// a run's samples [0, n) as bits, n clamped to the run: which of its CMP_R samples count
LOUD_HD uint32_t cmp_run_bits(long long n) { return n >= CMP_R ? (1u << CMP_R) - 1u : n > 0 ? (1u << n) - 1u : 0u; }

// ------------------------------------------------------------------------------------------------------------------
// host only: the checks, the workspace layout, the powers, the serial twin
// ------------------------------------------------------------------------------------------------------------------
inline bool cmp_params_ok(const CmpParams& d) {
    if (!(d.attack > 0.0 && d.attack < 1.0) || !(d.release > 0.0 && d.release < 1.0)) return false;
    if (!(d.threshold > 0.0) || !isfinite(d.threshold) || !isfinite(1.0 / d.threshold)) return false;
    if (!(d.slope >= -1.0 && d.slope <= 0.0)) return false;
    return d.makeup > 0.0 && isfinite(d.makeup);
}

struct CmpLayout {
    size_t rows_off, designs_off, y_off, chunks_off, stats_off, bytes;
    long long y_total, s_total;
    int max_n, max_nch;
};

// false on arguments the entries refuse; fills the rows when `rows` is given
inline bool cmp_layout(const CmpClip* clips, int n_clips, int n_designs, size_t n_x, bool check_x, CmpLayout* L, CmpRow* rows) {
    if (!clips || n_clips < 1 || n_clips > CMP_MAX_CLIPS || n_designs < 0 || n_designs > CMP_MAX_DESIGNS) return false;
    long long y = 0, sc = 0;
    int max_n = 0, max_nch = 0;
    for (int c = 0; c < n_clips; ++c) {
        const CmpClip& cl = clips[c];
        if (cl.n < 0 || cl.offset < 0 || cl.design < -1 || cl.design >= n_designs) return false;
        if (check_x && (unsigned long long)cl.offset + (unsigned long long)cl.n > (unsigned long long)n_x) return false;
        const int nch = (int)(((long long)cl.n + CMP_CHUNK - 1) / CMP_CHUNK);
        if (rows) {
            CmpRow& r = rows[c];
            r.offset = cl.offset; r.yoff = y; r.soff = sc;
            r.n = cl.n; r.nch = nch; r.design = cl.design; r.pad = 0;
        }
        y += ((long long)cl.n + 3) & ~3LL;
        sc += nch;
        if (cl.n > max_n) max_n = cl.n;
        if (nch > max_nch) max_nch = nch;
    }
    L->rows_off = 0;
    L->designs_off = loud_align16((size_t)n_clips * sizeof(CmpRow));
    L->y_off = L->designs_off + loud_align16((size_t)n_designs * sizeof(CmpDesign));
    L->chunks_off = L->y_off + loud_align16((size_t)y * sizeof(float));
    L->stats_off = L->chunks_off + loud_align16((size_t)sc * sizeof(CmpChunk));
    L->bytes = L->stats_off + loud_align16((size_t)n_clips * 3 * sizeof(uint32_t));
    L->y_total = y; L->s_total = sc; L->max_n = max_n; L->max_nch = max_nch;
    return true;
}

// a^(CMP_R 2^k) for the scan and a^CMP_CHUNK for the chain, squared in long double and rounded to fp64 once
inline void cmp_powers(double a, double* P, double* J) {
    long double v = a;
    for (int r = CMP_R; r > 1; r >>= 1) v = v * v;
    long double w = v;
    for (int k = 0; k < CMP_LOG_T; ++k) {
        P[k] = (double)w;
        w = w * w;
    }
    for (int r = CMP_CHUNK / CMP_R; r > 1; r >>= 1) v = v * v;
    *J = (double)v;
}

inline void cmp_design(const CmpParams& d, CmpDesign* out) {
    CmpDesign& D = *out;
    memset(&D, 0, sizeof D);
    D.aR = d.release; D.omR = 1.0 - d.release;
    D.aA = d.attack; D.omA = 1.0 - d.attack;
    D.T = d.threshold; D.invT = 1.0 / d.threshold;
    D.s = d.slope; D.M = d.makeup;
    cmp_powers(D.aR, D.PR, &D.JR);
    cmp_powers(D.aA, D.PA, &D.JA);
}

// one span as the block's threads run it (cmp_span below), over the runs v[0 .. CMP_T - 1] of x from carry = {B, p, e}: carry
// becomes the state behind the span.  pass 0: the release alone; 1: and the attack's end state; 2: v becomes the gains.
inline void cmp_span_host(const CmpDesign& D, int pass, double (*v)[CMP_R], double* carry) {
    static thread_local double st[2][CMP_T], nx[2][CMP_T];
    const int nt = CMP_T;
    const double b_in = carry[0], p_in = carry[1], e_in = carry[2];
    for (int t = 0; t < nt; ++t) {
        double B = t == 0 ? b_in : 0.0, C = t == 0 ? p_in : 0.0;
        for (int i = 0; i < CMP_R; ++i) {
            v[t][i] = fabs(v[t][i]);
            B = cmp_lin_step(D.aR, D.omR, B, v[t][i]);
            C = cmp_p_step(D.aR, D.omR, C, v[t][i]);
        }
        st[0][t] = B; st[1][t] = C;
    }
    for (int k = 0; k < CMP_LOG_T; ++k) {
        const int d = 1 << k;
        for (int t = 0; t < nt; ++t) {
            double B = st[0][t], C = st[1][t];
            if (t >= d) cmp_combine(D.PR[k], st[0][t - d], st[1][t - d], B, C);
            nx[0][t] = B; nx[1][t] = C;
        }
        memcpy(st, nx, sizeof st);
    }
    carry[0] = st[0][nt - 1];
    carry[1] = st[1][nt - 1];
    if (pass == 0) return;
    for (int t = 0; t < nt; ++t) {
        double p = t == 0 ? p_in : st[1][t - 1];
        for (int i = 0; i < CMP_R; ++i) v[t][i] = p = cmp_p_step(D.aR, D.omR, p, v[t][i]);
    }
    for (int t = 0; t < nt; ++t) {
        double E = t == 0 ? e_in : 0.0;
        for (int i = 0; i < CMP_R; ++i) E = cmp_lin_step(D.aA, D.omA, E, v[t][i]);
        st[0][t] = E;
    }
    for (int k = 0; k < CMP_LOG_T; ++k) {
        const int d = 1 << k;
        for (int t = 0; t < nt; ++t) nx[0][t] = t >= d ? fma(D.PA[k], st[0][t - d], st[0][t]) : st[0][t];
        memcpy(st[0], nx[0], sizeof st[0]);
    }
    carry[2] = st[0][nt - 1];
    if (pass == 1) return;
    for (int t = 0; t < nt; ++t) {
        double e = t == 0 ? e_in : st[0][t - 1];
        for (int i = 0; i < CMP_R; ++i) {
            e = cmp_lin_step(D.aA, D.omA, e, v[t][i]);
            v[t][i] = cmp_gain(D.T, D.invT, D.s, e);
        }
    }
}

// the runs of a span for cmp_walk_host: one buffer for all its forms
inline double (*cmp_runs_host())[CMP_R] {
    static thread_local double v[CMP_T][CMP_R];
    return v;
}

// the samples [lo, hi) of a signal span by span as one block walks them (inside one chunk, lo a span's first sample), from
// carry = {B, p, e} -> carry behind them.  load(s) gives sample s as it enters the detector; in pass 2, gain(s, g) takes its
// gain, after every load of the span
template <class Load, class Gain>
inline void cmp_walk_host(const CmpDesign& D, int pass, long long lo, long long hi, double* carry, Load load, Gain gain) {
    double(*v)[CMP_R] = cmp_runs_host();
    for (long long s0 = lo; s0 < hi; s0 += CMP_SPAN) {
        const int cnt = hi - s0 < CMP_SPAN ? (int)(hi - s0) : CMP_SPAN;
        for (int k = 0; k < CMP_SPAN; ++k) v[k / CMP_R][k % CMP_R] = k < cnt ? (double)load(s0 + k) : 0.0;
        cmp_span_host(D, pass, v, carry);
        for (int k = 0; pass == 2 && k < cnt; ++k) gain(s0 + k, v[k / CMP_R][k % CMP_R]);
    }
}

// what the passes 0 and 1 and the chain waves do over `done` whole chunks, the first one at sample lo, from the states (p0, e0)
// in front of it: ch[0 .. done - 1] get (B, C) and eend, ch[0 .. done] pstart and estart.  Pass 2 is the caller's.
template <class Load>
inline void cmp_drive_host(const CmpDesign& D, long long lo, int done, double p0, double e0, CmpChunk* ch, Load load) {
    for (int stage = 0; stage < 2; ++stage) {
        for (int b = 0; b < done; ++b) {
            double carry[3] = {0.0, stage == 0 ? 0.0 : ch[b].pstart, 0.0};
            cmp_walk_host(D, stage, lo + (long long)b * CMP_CHUNK, lo + (long long)(b + 1) * CMP_CHUNK, carry, load, [](long long, double) {});
            if (stage == 0) { ch[b].B = carry[0]; ch[b].C = carry[1]; }
            else ch[b].eend = carry[2];
        }
        cmp_chain_walk(stage == 0 ? D.JR : D.JA, stage, stage == 0 ? p0 : e0, done + 1, done,
                       [&](int c) -> const CmpChunk& { return ch[c]; },
                       [&](int c, double st) { (stage == 0 ? ch[c].pstart : ch[c].estart) = st; });
    }
}

// the whole call over host memory.  work holds cmp_layout's bytes; out may be x (in place).
inline void cmp_run_host(const float* x, const CmpClip* clips, int n_clips, const CmpParams* designs, int n_designs, float* out, CmpRecord* records,
                         unsigned char* work) {
    CmpLayout L;
    CmpRow* rows = reinterpret_cast<CmpRow*>(work);
    if (!cmp_layout(clips, n_clips, n_designs, 0, false, &L, rows)) return;
    CmpDesign* D = reinterpret_cast<CmpDesign*>(work + L.designs_off);
    for (int d = 0; d < n_designs; ++d) cmp_design(designs[d], &D[d]);
    float* yws = reinterpret_cast<float*>(work + L.y_off);
    CmpChunk* chunks = reinterpret_cast<CmpChunk*>(work + L.chunks_off);
    uint32_t* stats = reinterpret_cast<uint32_t*>(work + L.stats_off);
    for (int c = 0; c < n_clips; ++c) {
        const CmpRow& r = rows[c];
        const float* xc = x + r.offset;
        uint32_t* st = stats + 3 * c;
        st[0] = 0; st[1] = 0; st[2] = CMP_ONE_BITS;
        if (r.design >= 0) {
            const CmpDesign& Dd = D[r.design];
            CmpChunk* ch = chunks + r.soff;
            float* yc = yws + r.yoff;
            cmp_drive_host(Dd, 0, r.nch - 1, 0.0, 0.0, ch, [&](long long s) { return xc[s]; });
            const auto load = [&](long long s) {
                const uint32_t a = loud_abs_bits(xc[s]);
                if (a > st[0]) st[0] = a;
                return xc[s];
            };
            const auto gain = [&](long long s, double g) {
                const float o = cmp_out(Dd.M, g, xc[s]);
                const uint32_t a = loud_abs_bits(o), gb = loud_abs_bits((float)g);
                if (a > st[1]) st[1] = a;
                if (gb < st[2]) st[2] = gb;
                yc[s] = o;
            };
            for (int k = 0; k < r.nch; ++k) {
                const long long hi = (long long)(k + 1) * CMP_CHUNK;
                double carry[3] = {0.0, ch[k].pstart, ch[k].estart};
                cmp_walk_host(Dd, 2, (long long)k * CMP_CHUNK, hi < r.n ? hi : r.n, carry, load, gain);
            }
        } else {
            for (int i = 0; i < r.n; ++i) {
                const uint32_t a = loud_abs_bits(xc[i]);
                if (a > st[0]) st[0] = a;
            }
        }
        records[c] = cmp_finish(r, st[0], st[1], st[2]);
        if (r.n == 0) continue;
        if (!cmp_copied(r, records[c]))
            memcpy(out + r.offset, yws + r.yoff, (size_t)r.n * sizeof(float));
        else if (out != x)
            memcpy(out + r.offset, xc, (size_t)r.n * sizeof(float));
    }
}

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------------------------------
// the device kernels
// ------------------------------------------------------------------------------------------------------------------
// One span.  Thread tid's run of x is staged at `mine` (CMP_R floats of LDS); carry_s = {B, p, e} (LDS) goes from the state in
// front of the span to the state behind it.  PASS 0: the release alone; 1: and the attack's end state; 2: v becomes the gains of
// the run.  The scans' exchange sc is double-buffered: one barrier per step.
// Barriers: entered by all CMP_T threads of the block behind a barrier that follows the staging of the runs, the last write of
// carry_s and the last span's reads of sc.  It returns without one: the caller owes a barrier before carry_s is read, sc or
// carry_s is written again, or a run is read by another thread.
template <int PASS>
__device__ __forceinline__ void cmp_span(const CmpDesign* __restrict__ D, const float* mine, double (*sc)[2][CMP_T], double* carry_s,
                                         double (&v)[CMP_R]) {
    const int tid = threadIdx.x;
    constexpr int LAST = CMP_LOG_T & 1;
    const double aR = D->aR, omR = D->omR;
    double B = 0.0, C = 0.0, e_in = 0.0;
    if (tid == 0) { B = carry_s[0]; C = carry_s[1]; e_in = carry_s[2]; }
    const double p_in = C;
#pragma unroll
    for (int i = 0; i < CMP_R; ++i) {
        v[i] = fabs((double)mine[i]);
        B = cmp_lin_step(aR, omR, B, v[i]);
        C = cmp_p_step(aR, omR, C, v[i]);
    }
#pragma unroll 1
    for (int k = 0; k < CMP_LOG_T; ++k) {
        const int d = 1 << k, buf = k & 1;
        sc[buf][0][tid] = B;
        sc[buf][1][tid] = C;
        __syncthreads();
        if (tid >= d) cmp_combine(D->PR[k], sc[buf][0][tid - d], sc[buf][1][tid - d], B, C);
    }
    sc[LAST][1][tid] = C;
    if (tid == CMP_T - 1) { carry_s[0] = B; carry_s[1] = C; }       // thread 0 read its carry before the scan
    if (PASS == 0) return;
    __syncthreads();
    double p = tid > 0 ? sc[LAST][1][tid - 1] : p_in;
#pragma unroll
    for (int i = 0; i < CMP_R; ++i) v[i] = p = cmp_p_step(aR, omR, p, v[i]);
    const double aA = D->aA, omA = D->omA;
    double E = e_in;
#pragma unroll
    for (int i = 0; i < CMP_R; ++i) E = cmp_lin_step(aA, omA, E, v[i]);
#pragma unroll 1
    for (int k = 0; k < CMP_LOG_T; ++k) {
        const int d = 1 << k, buf = k & 1;
        sc[buf][0][tid] = E;            // plane 0: the reads of plane 1 above may still be under way
        __syncthreads();
        if (tid >= d) E = fma(D->PA[k], sc[buf][0][tid - d], E);
    }
    sc[LAST][0][tid] = E;
    if (tid == CMP_T - 1) carry_s[2] = E;
    if (PASS == 1) return;
    __syncthreads();
    double e = tid > 0 ? sc[LAST][0][tid - 1] : e_in;
    const double T = D->T, invT = D->invT, s = D->s;
#pragma unroll
    for (int i = 0; i < CMP_R; ++i) {
        e = cmp_lin_step(aA, omA, e, v[i]);
        v[i] = cmp_gain(T, invT, s, e);
    }
}

// the slot of sample k of a span in LDS: each thread's run is padded by one float so the runs start in different banks
__device__ __forceinline__ int cmp_slot(int k) { return (k / CMP_R) * (CMP_R + 1) + k % CMP_R; }

// in front of a block's first span: the block's statistics and the carry in front of the chunk -- zero, but in PASS 1 and 2 the
// pstart and in PASS 2 the estart of `from`, when there is one.  The barrier in front of the first cmp_body publishes them.
template <int PASS>
__device__ __forceinline__ void cmp_open(uint32_t* stat_s, double* carry_s, const CmpChunk* from) {
    const int tid = threadIdx.x;
    if (tid < 3) stat_s[tid] = tid == 2 ? CMP_ONE_BITS : 0u;
    if (tid == 0) {
        carry_s[0] = 0.0;
        carry_s[1] = PASS > 0 && from ? from->pstart : 0.0;
        carry_s[2] = PASS == 2 && from ? from->estart : 0.0;
    }
}

// One span of a block, between "the runs are staged" and "the products stand in the runs": cmp_span, and in PASS 2 the run at
// `mine` becomes the products and the samples whose bit is set in `counts` (bit i: sample i of the run) enter the thread's
// peak_out and gmin (the bits of max |y| and min g).  A run with no bit set is left as it is: nothing of it is written or counted.
// Barriers: cmp_span's, on entry and on return.
template <int PASS>
__device__ __forceinline__ void cmp_body(const CmpDesign* __restrict__ D, float* mine, double (*sc)[2][CMP_T], double* carry_s, uint32_t counts,
                                         uint32_t& peak_out, uint32_t& gmin) {
    double v[CMP_R];
    cmp_span<PASS>(D, mine, sc, carry_s, v);
    if (PASS < 2 || !counts) return;
    const double M = D->M;
#pragma unroll
    for (int i = 0; i < CMP_R; ++i) {
        const float o = cmp_out(M, v[i], mine[i]);
        mine[i] = o;
        const bool on = counts >> i & 1u;       // selects, no branch: the run's LDS reads and writes stay paired
        const uint32_t a = on ? loud_abs_bits(o) : 0u, gb = on ? loud_abs_bits((float)v[i]) : CMP_ONE_BITS;
        peak_out = a > peak_out ? a : peak_out;
        gmin = gb < gmin ? gb : gmin;
    }
}

// behind a block's last span and its barrier.  PASS 0 and 1 park what the carry holds in the chunk's fields -- (B, C), eend -- and
// give false: the block is done.  PASS 2 folds the threads' statistics (the bits of max |x|, max |y|, min g) into stat_s, passes a
// barrier and gives true: stat_s is the block's, for the kernel's own atomics.
template <int PASS>
__device__ __forceinline__ bool cmp_close(const double* carry_s, CmpChunk* ch, uint32_t* stat_s, uint32_t peak_in, uint32_t peak_out,
                                          uint32_t gmin) {
    if (PASS < 2) {
        if (threadIdx.x == 0) {
            if (PASS == 0) { ch->B = carry_s[0]; ch->C = carry_s[1]; }
            else ch->eend = carry_s[2];
        }
        return false;
    }
    atomicMax(&stat_s[0], peak_in);
    atomicMax(&stat_s[1], peak_out);
    atomicMin(&stat_s[2], gmin);
    __syncthreads();
    return true;
}

// One block per chunk of a clip.  PASS 0 and 1 run over the chunks that have a successor and write their CmpChunk fields alone;
// PASS 2 runs over all of them from the true start states: y, both peaks, the smallest gain.  The span is staged in LDS by
// coalesced loads (cmp_slot); y goes back through the same slots.
template <int PASS>
static __global__ __launch_bounds__(CMP_T) void cmp_kernel(const float* __restrict__ x, const CmpRow* __restrict__ rows,
                                                           const CmpDesign* __restrict__ designs, float* __restrict__ yws,
                                                           CmpChunk* __restrict__ chunks, uint32_t* __restrict__ stats) {
    __shared__ float xs[CMP_T * (CMP_R + 1)];
    __shared__ double sc[2][2][CMP_T];
    __shared__ double carry_s[3];
    __shared__ uint32_t stat_s[3];
    const CmpRow row = rows[blockIdx.y];
    const int tid = threadIdx.x, chunk = blockIdx.x;
    if (chunk >= (PASS < 2 ? row.nch - 1 : row.nch)) return;   // block-uniform
    const long long chunk_hi = (long long)(chunk + 1) * CMP_CHUNK;
    const int lo = chunk * CMP_CHUNK, hi = chunk_hi < row.n ? (int)chunk_hi : row.n;
    const float* __restrict__ xc = x + row.offset;
    if (row.design < 0) {                                       // measure only: the peak of x
        if (PASS < 2) return;
        uint32_t peak = 0;
        for (int k = lo + tid; k < hi; k += CMP_T) {
            const uint32_t a = loud_abs_bits(xc[k]);
            peak = a > peak ? a : peak;
        }
        if (tid == 0) stat_s[0] = 0;
        __syncthreads();
        atomicMax(&stat_s[0], peak);
        __syncthreads();
        if (tid == 0) atomicMax(&stats[3 * blockIdx.y], stat_s[0]);
        return;
    }
    const CmpDesign* __restrict__ D = designs + row.design;
    CmpChunk* __restrict__ ch = chunks + row.soff + chunk;
    float* __restrict__ yc = yws + row.yoff;
    cmp_open<PASS>(stat_s, carry_s, chunk > 0 ? ch : nullptr);     // a clip of one chunk was never walked
    uint32_t peak_in = 0, peak_out = 0, gmin = CMP_ONE_BITS;
    float* mine = xs + tid * (CMP_R + 1);
    for (int s0 = lo; s0 < hi; s0 += CMP_SPAN) {
        const int cnt = hi - s0 < CMP_SPAN ? hi - s0 : CMP_SPAN;
        for (int k = tid; k < CMP_SPAN; k += CMP_T) {
            float xv = 0.f;
            if (k < cnt) {
                xv = xc[s0 + k];
                const uint32_t a = loud_abs_bits(xv);
                peak_in = a > peak_in ? a : peak_in;
            }
            xs[cmp_slot(k)] = xv;
        }
        __syncthreads();                // xs, and carry_s of the last span (or of cmp_open)
        cmp_body<PASS>(D, mine, sc, carry_s, cmp_run_bits(cnt - tid * CMP_R), peak_out, gmin);
        if (PASS == 2) {
            __syncthreads();
            for (int k = tid; k < cnt; k += CMP_T) yc[s0 + k] = xs[cmp_slot(k)];
        }
        __syncthreads();        // the next span stages over xs and sc; carry_s is whole
    }
    if (!cmp_close<PASS>(carry_s, ch, stat_s, peak_in, peak_out, gmin)) return;
    if (tid < 2) atomicMax(&stats[3 * blockIdx.y + tid], stat_s[tid]);      // integer extrema: the order of the chunks does not show
    if (tid == 2) atomicMin(&stats[3 * blockIdx.y + 2], stat_s[2]);
}

// between the passes: one wave per clip walks its chunks (cmp_chain_walk), CMP_LANES at a time through LDS.  STAGE 0: pstart from
// (B, C); STAGE 1: estart from eend, and the clip's statistics are cleared for pass 2.
template <int STAGE>
static __global__ __launch_bounds__(CMP_LANES) void cmp_chain_kernel(const CmpRow* __restrict__ rows, const CmpDesign* __restrict__ designs,
                                                                     CmpChunk* __restrict__ chunks, uint32_t* __restrict__ stats) {
    __shared__ double in_s[2][CMP_LANES], out_s[CMP_LANES];
    const CmpRow row = rows[blockIdx.x];
    const int lane = threadIdx.x;
    if (STAGE == 1 && lane < 3) stats[3 * blockIdx.x + lane] = lane == 2 ? CMP_ONE_BITS : 0u;
    if (row.design < 0) return;                 // block-uniform
    const double J = STAGE == 0 ? designs[row.design].JR : designs[row.design].JA;
    CmpChunk* __restrict__ ch = chunks + row.soff;
    double st = 0.0;                            // lane 0's: the state in front of chunk `base`
    for (int base = 0; base < row.nch; base += CMP_LANES) {
        const int cnt = row.nch - base < CMP_LANES ? row.nch - base : CMP_LANES;
        if (lane < cnt && base + lane + 1 < row.nch) {      // the last chunk's fields were never written
            in_s[0][lane] = STAGE == 0 ? ch[base + lane].B : ch[base + lane].eend;
            if (STAGE == 0) in_s[1][lane] = ch[base + lane].C;
        }
        __syncthreads();
        if (lane == 0) {
            st = cmp_chain_walk(J, STAGE, st, cnt, row.nch - 1 - base,
                                [&](int c) {
                                    CmpChunk k = {};
                                    k.B = k.eend = in_s[0][c];
                                    if (STAGE == 0) k.C = in_s[1][c];
                                    return k;
                                },
                                [&](int c, double v) { out_s[c] = v; });
        }
        __syncthreads();
        if (lane < cnt) {
            if (STAGE == 0) ch[base + lane].pstart = out_s[lane];
            else ch[base + lane].estart = out_s[lane];
        }
        __syncthreads();        // the next round writes in_s and out_s
    }
}

// last: the record, and out = y (a clip that went through the compressor) or x (measure only, or a NaN or an infinity among the
// samples: in place nothing is written) inside [offset, offset + n) of every clip
static __global__ __launch_bounds__(256) void cmp_commit_kernel(const float* x, const CmpRow* __restrict__ rows, const float* __restrict__ yws,
                                                                const uint32_t* __restrict__ stats, CmpRecord* __restrict__ records, float* out) {
    const CmpRow row = rows[blockIdx.y];
    const CmpRecord rec = cmp_finish(row, stats[3 * blockIdx.y], stats[3 * blockIdx.y + 1], stats[3 * blockIdx.y + 2]);
    if (blockIdx.x == 0 && threadIdx.x == 0) records[blockIdx.y] = rec;
    const bool copy = cmp_copied(row, rec);
    if (copy && out == x) return;
    const float* src = copy ? x + row.offset : yws + row.yoff;      // out may be x: no restrict
    float* oc = out + row.offset;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < row.n; i += gridDim.x * 256) oc[i] = src[i];
}
#endif

}  // namespace gsv
