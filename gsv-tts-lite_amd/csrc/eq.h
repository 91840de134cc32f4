// eq: a cascade of 1 to 6 second-order sections over B packed fp32 clips, each clip with one of a few coefficient sets
// (DESIGN 4.24).  Zero initial state, every section in transposed direct form II in fp64, fp64 between the sections, the last
// section's output rounded once to fp32 (saturating, loud_store's rule); same length out as in.
//
// Everything that decides a bit -- the section step, the combine of the scan, the chain of the chunks, the record -- is one
// __host__ __device__ text for the kernels, for the host twin eq_run_host (gsv_eq_host: the CPU path and the device's oracle)
// and for the stand-alone checker tools/eq_host_check.cpp.  Every multiply-add is an explicit fma and every order is fixed, so
// contraction has nothing to change and device samples and records equal the host's bit for bit.  The device takes no sin, cos
// or pow: the caller hands in normalised coefficients, and the powers of the state matrices are built on the host (eq_design).
// The stream form (eqstream.h) owes the clip's bytes, so the sections of a span and the chain of the chunks are each one
// function on the device (eq_sections, eq_chain_walk) and one on the host (eq_sections_host, eq_chain_host) that both forms call.
//
// The scan, section after section.  A block of EQ_T threads takes a span of EQ_T * EQ_R samples; thread t holds its EQ_R
// consecutive samples in fp64 registers.  For section s = 0, 1, ...: the thread runs its samples from zero state (thread 0:
// from the state the last span left in this section), a Hillis-Steele scan with the 2x2 matrices P[s][k] = M_s^(EQ_R 2^k)
// turns the end states into true end states, and the thread reruns its samples from the true end state of its left neighbour,
// which replaces them by the section's output: the input of section s + 1.  So S sections cost S scans of 2x2 work, 4 S fmas
// per scan step where one joint 2S-state scan takes 4 S^2.  A span shorter than EQ_T * EQ_R is padded with zeros behind the
// clip, so every run is full length and the same matrices hold everywhere; what the padding turns into is never written, and a
// prefix of the scan depends on the runs to its left alone.
//
// A block carries the states from span to span over a chunk of EQ_CHUNK samples.  The chunks of a clip run side by side,
// chained one level up with the joint state of all sections (2 per section, EQ_NS doubles, unused ones 0): every chunk but the
// last first finds its end state from zero state (the work above without the last rerun, nothing written), one wave per clip
// walks the chunks with J = Mjoint^EQ_CHUNK and leaves every chunk's true start state, and the full pass starts from it.
//
// The filtered samples go to the workspace, not to `out`: whether a clip holds a NaN or an infinity is known from the integer
// maximum of its |x| bit patterns only when the full pass is over, and such a clip comes back bit for bit.  The commit launch
// then writes the record and, per clip, y or x into `out` (in place and copied: nothing).
//
// Workspace: [EqRow rows[B] | EqDesign designs[D] | y fp32 [sum of n, each clip 4-float aligned] | chunk end states, chunk
// start states, EQ_NS fp64 each [sum of chunks] | peak bits u32 [2 B]: max |x|, max |y|].  Rows and designs are one upload.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "loudness.h"

namespace gsv {

constexpr int EQ_T = 512;                       // threads of the filter block
constexpr int EQ_LOG_T = 9;
constexpr int EQ_R = 16;                        // consecutive samples per thread and span
constexpr int EQ_SPAN = EQ_T * EQ_R;
constexpr int EQ_LOG_CH = 1;                    // a chunk is 2^EQ_LOG_CH spans
constexpr int EQ_CHUNK = EQ_SPAN << EQ_LOG_CH;
constexpr int EQ_MAX_SECTIONS = 6;
constexpr int EQ_NS = 2 * EQ_MAX_SECTIONS;      // doubles of the joint state
constexpr int EQ_LANES = 64;                    // lanes of the chain wave
constexpr int EQ_MAX_CLIPS = 65535, EQ_MAX_DESIGNS = 65535;
constexpr int EQ_EQUALISED = 1, EQ_NONFINITE = 4;      // record flags
static_assert(EQ_T == 1 << EQ_LOG_T, "scan steps");
static_assert((EQ_R & (EQ_R - 1)) == 0 && (EQ_CHUNK & (EQ_CHUNK - 1)) == 0, "powers by squaring");

struct EqClip {             // gsv_eq_clip
    long long offset;       // first sample in the packed buffer
    int32_t n;
    int32_t design;         // index into the designs of the call; -1: measure the peaks, copy
};
static_assert(sizeof(EqClip) == 16, "clip");

struct EqCoefs {            // gsv_eq_design
    int32_t n_sections, reserved;
    double c[EQ_MAX_SECTIONS][5];       // b0 b1 b2 a1 a2, normalised by a0
};
static_assert(sizeof(EqCoefs) == 8 + 240, "design");

struct EqRecord {           // gsv_eq_record
    float peak_in, peak_out;            // max |x|, max |y|
    int32_t sections, flags;            // sections run over the clip (0 for a clip that was copied)
};
static_assert(sizeof(EqRecord) == 16, "record");

struct EqRow {              // one clip as the kernels see it (built on the host, first part of the workspace)
    long long offset, yoff, soff;       // soff: the clip's first chunk state
    int32_t n, nch, design, pad;
};
static_assert(sizeof(EqRow) == 40, "row");

struct EqDesign {           // one coefficient set as the kernels see it (built on the host, behind the rows)
    double b[EQ_MAX_SECTIONS][3], na[EQ_MAX_SECTIONS][2];       // b0 b1 b2, -a1 -a2
    double P[EQ_MAX_SECTIONS][EQ_LOG_T][4];                     // M_s^(EQ_R 2^k), row-major
    double J[EQ_NS * EQ_NS];                                    // Mjoint^EQ_CHUNK, row-major
    int32_t ns, pad;
};
static_assert(sizeof(EqDesign) % 8 == 0, "design");

struct EqState { double s[EQ_NS]; };

// one sample through one section (b0 b1 b2, -a1 -a2; state z0 z1); the order of every operation is this text
LOUD_HD double eq_step(const double* b, const double* na, double& z0, double& z1, double x) {
    const double y = fma(b[0], x, z0);
    z0 = fma(na[0], y, fma(b[1], x, z1));
    z1 = fma(na[1], y, b[2] * x);
    return y;
}

// own + P left: the state of one section after two adjacent runs from the end state of each run alone
LOUD_HD void eq_combine(const double* P, double l0, double l1, double& e0, double& e1) {
    e0 = fma(P[0], l0, fma(P[1], l1, e0));
    e1 = fma(P[2], l0, fma(P[3], l1, e1));
}

// row i of own + J left over the joint state
LOUD_HD double eq_chain_row(const double* Jrow, const double* left, double own) {
    double acc = own;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = EQ_NS - 1; j >= 0; --j) acc = fma(Jrow[j], left[j], acc);
    return acc;
}

LOUD_HD EqRecord eq_finish(const EqRow& row, int ns, uint32_t peak_in, uint32_t peak_out) {
    EqRecord r;
    const bool nonfinite = peak_in >= 0x7F800000u, copied = nonfinite || row.design < 0;
    r.peak_in = loud_from_bits(peak_in);
    r.peak_out = loud_from_bits(copied ? peak_in : peak_out);
    r.sections = copied ? 0 : ns;
    r.flags = nonfinite ? EQ_NONFINITE : (row.design < 0 ? 0 : EQ_EQUALISED);
    return r;
}

// ------------------------------------------------------------------------------------------------------------------
// host only: the checks, the workspace layout, the matrices, the serial twin
// ------------------------------------------------------------------------------------------------------------------
// finite coefficients and both poles inside the unit circle
inline bool eq_coefs_ok(const EqCoefs& d) {
    if (d.n_sections < 1 || d.n_sections > EQ_MAX_SECTIONS) return false;
    for (int s = 0; s < d.n_sections; ++s) {
        for (int i = 0; i < 5; ++i)
            if (!isfinite(d.c[s][i])) return false;
        const double a1 = d.c[s][3], a2 = d.c[s][4];
        if (!(fabs(a2) < 1.0) || !(fabs(a1) < 1.0 + a2)) return false;
    }
    return true;
}

struct EqLayout {
    size_t rows_off, designs_off, y_off, ends_off, starts_off, peak_off, bytes;
    long long y_total, s_total;
    int max_n, max_nch;
};

// false on arguments the entries refuse; fills the rows when `rows` is given
inline bool eq_layout(const EqClip* clips, int n_clips, int n_designs, size_t n_x, bool check_x, EqLayout* L, EqRow* rows) {
    if (!clips || n_clips < 1 || n_clips > EQ_MAX_CLIPS || n_designs < 0 || n_designs > EQ_MAX_DESIGNS) return false;
    long long y = 0, sc = 0;
    int max_n = 0, max_nch = 0;
    for (int c = 0; c < n_clips; ++c) {
        const EqClip& cl = clips[c];
        if (cl.n < 0 || cl.offset < 0 || cl.design < -1 || cl.design >= n_designs) return false;
        if (check_x && (unsigned long long)cl.offset + (unsigned long long)cl.n > (unsigned long long)n_x) return false;
        const int nch = (int)(((long long)cl.n + EQ_CHUNK - 1) / EQ_CHUNK);
        if (rows) {
            EqRow& r = rows[c];
            r.offset = cl.offset; r.yoff = y; r.soff = sc;
            r.n = cl.n; r.nch = nch; r.design = cl.design; r.pad = 0;
        }
        y += ((long long)cl.n + 3) & ~3LL;
        sc += nch;
        if (cl.n > max_n) max_n = cl.n;
        if (nch > max_nch) max_nch = nch;
    }
    L->rows_off = 0;
    L->designs_off = loud_align16((size_t)n_clips * sizeof(EqRow));
    L->y_off = L->designs_off + loud_align16((size_t)n_designs * sizeof(EqDesign));
    L->ends_off = L->y_off + loud_align16((size_t)y * sizeof(float));
    L->starts_off = L->ends_off + (size_t)sc * sizeof(EqState);
    L->peak_off = L->starts_off + (size_t)sc * sizeof(EqState);
    L->bytes = L->peak_off + loud_align16((size_t)n_clips * 2 * sizeof(uint32_t));
    L->y_total = y; L->s_total = sc; L->max_n = max_n; L->max_nch = max_nch;
    return true;
}

inline void eq_matmul(const long double* a, const long double* b, long double* out, int n) {
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            long double s = 0.0L;
            for (int k = 0; k < n; ++k) s += a[n * i + k] * b[n * k + j];
            out[n * i + j] = s;
        }
}

// the device form of one coefficient set: the negated feedback, the scan's matrices of every section, the chunk matrix.  The
// powers are squared in long double and rounded to fp64 once: a section with both poles next to z = 1 (a 20 Hz high pass at
// 192 kHz) has a state matrix so far from normal that fp64 squaring leaves the twin 1e-8 of the clip's peak from the serial
// cascade; with x87's 64-bit significand it is 5e-11 (tools/eq_host_check.cpp).  Where long double is fp64 the call still holds
// its bit equality between device and twin, which share these matrices.
inline void eq_design(const EqCoefs& d, EqDesign* out) {
    EqDesign& D = *out;
    memset(&D, 0, sizeof D);
    D.ns = d.n_sections;
    for (int s = 0; s < D.ns; ++s) {
        for (int i = 0; i < 3; ++i) D.b[s][i] = d.c[s][i];
        D.na[s][0] = -d.c[s][3];
        D.na[s][1] = -d.c[s][4];
        // M_s: column i is one step with x = 0 from the unit state e_i
        long double A[4], B[4];
        for (int i = 0; i < 2; ++i) {
            double z[2] = {0.0, 0.0};
            z[i] = 1.0;
            eq_step(D.b[s], D.na[s], z[0], z[1], 0.0);
            A[i] = z[0]; A[2 + i] = z[1];
        }
        for (int r = EQ_R; r > 1; r >>= 1) { eq_matmul(A, A, B, 2); memcpy(A, B, sizeof A); }
        for (int k = 0; k < EQ_LOG_T; ++k) {
            for (int i = 0; i < 4; ++i) D.P[s][k][i] = (double)A[i];
            eq_matmul(A, A, B, 2);
            memcpy(A, B, sizeof A);
        }
    }
    // Mjoint over (z0, z1) of every section: column i is one step of the cascade with x = 0 from the unit state e_i
    static thread_local long double A[EQ_NS * EQ_NS], B[EQ_NS * EQ_NS];
    for (int i = 0; i < EQ_NS * EQ_NS; ++i) A[i] = 0.0L;
    for (int i = 0; i < 2 * D.ns; ++i) {
        double z[EQ_NS] = {0};
        z[i] = 1.0;
        double v = 0.0;
        for (int s = 0; s < D.ns; ++s) v = eq_step(D.b[s], D.na[s], z[2 * s], z[2 * s + 1], v);
        for (int r = 0; r < EQ_NS; ++r) A[EQ_NS * r + i] = z[r];
    }
    for (int r = EQ_CHUNK; r > 1; r >>= 1) { eq_matmul(A, A, B, EQ_NS); memcpy(A, B, sizeof A); }
    for (int i = 0; i < EQ_NS * EQ_NS; ++i) D.J[i] = (double)A[i];
}

// the sections of one span as the block's threads run them (eq_sections below), over the runs v[0 .. nt - 1] from the joint
// state `carry`: v becomes the last section's output and carry the state behind run nt - 1.  ends: the end state alone -- the
// last section's rerun is left out and v is then not its output.
inline void eq_sections_host(const EqDesign& D, int nt, bool ends, double (*v)[EQ_R], EqState& carry) {
    static thread_local double st[2][EQ_T], nx[2][EQ_T];
    for (int s = 0; s < D.ns; ++s) {
        const double* b = D.b[s];
        const double* na = D.na[s];
        const double c0 = carry.s[2 * s], c1 = carry.s[2 * s + 1];
        for (int t = 0; t < nt; ++t) {
            double z0 = t == 0 ? c0 : 0.0, z1 = t == 0 ? c1 : 0.0;
            for (int i = 0; i < EQ_R; ++i) eq_step(b, na, z0, z1, v[t][i]);
            st[0][t] = z0; st[1][t] = z1;
        }
        for (int k = 0; k < EQ_LOG_T; ++k) {
            const int d = 1 << k;
            for (int t = 0; t < nt; ++t) {
                double e0 = st[0][t], e1 = st[1][t];
                if (t >= d) eq_combine(D.P[s][k], st[0][t - d], st[1][t - d], e0, e1);
                nx[0][t] = e0; nx[1][t] = e1;
            }
            memcpy(st, nx, sizeof st);
        }
        carry.s[2 * s] = st[0][nt - 1];
        carry.s[2 * s + 1] = st[1][nt - 1];
        if (ends && s == D.ns - 1) break;
        for (int t = 0; t < nt; ++t) {
            double z0 = t == 0 ? c0 : st[0][t - 1], z1 = t == 0 ? c1 : st[1][t - 1];
            for (int i = 0; i < EQ_R; ++i) v[t][i] = eq_step(b, na, z0, z1, v[t][i]);
        }
    }
}

// the samples [lo, hi) of a clip span by span from the joint state `carry`, as one block walks them -> the state behind them.
// y null: the first half only (the end states of the chunks); else y and both peaks' bits too
inline EqState eq_chunk_host(const float* x, int lo, int hi, const EqDesign& D, EqState carry, float* y, uint32_t* peak_in, uint32_t* peak_out) {
    static thread_local double v[EQ_T][EQ_R];
    for (int s0 = lo; s0 < hi; s0 += EQ_SPAN) {
        const int cnt = hi - s0 < EQ_SPAN ? hi - s0 : EQ_SPAN;
        for (int k = 0; k < EQ_SPAN; ++k) {
            float xv = 0.f;
            if (k < cnt) {
                xv = x[s0 + k];
                const uint32_t a = loud_abs_bits(xv);
                if (y && a > *peak_in) *peak_in = a;
            }
            v[k / EQ_R][k % EQ_R] = (double)xv;
        }
        eq_sections_host(D, EQ_T, !y, v, carry);
        for (int k = 0; y && k < cnt; ++k) {
            const float o = loud_store(v[k / EQ_R][k % EQ_R]);
            const uint32_t a = loud_abs_bits(o);
            if (a > *peak_out) *peak_out = a;
            y[s0 + k] = o;
        }
    }
    return carry;
}

// what the chain wave does (eq_chain_walk below): from the start state `first` of a chunk over `links` chunks with their end
// states from zero state -> starts[0 .. links], the true start state of each and of the chunk behind them.  links < 0 (a clip
// of no chunks): nothing written
inline void eq_chain_host(const EqDesign& D, const EqState& first, int links, const EqState* ends, EqState* starts) {
    if (links < 0) return;
    starts[0] = first;
    for (int c = 0; c < links; ++c)
        for (int i = 0; i < EQ_NS; ++i) starts[c + 1].s[i] = eq_chain_row(D.J + EQ_NS * i, starts[c].s, ends[c].s[i]);
}

// the whole call over host memory.  work holds eq_layout's bytes; out may be x (in place).
inline void eq_run_host(const float* x, const EqClip* clips, int n_clips, const EqCoefs* designs, int n_designs, float* out, EqRecord* records,
                        unsigned char* work) {
    EqLayout L;
    EqRow* rows = reinterpret_cast<EqRow*>(work);
    if (!eq_layout(clips, n_clips, n_designs, 0, false, &L, rows)) return;
    EqDesign* D = reinterpret_cast<EqDesign*>(work + L.designs_off);
    for (int d = 0; d < n_designs; ++d) eq_design(designs[d], &D[d]);
    float* yws = reinterpret_cast<float*>(work + L.y_off);
    EqState* ends = reinterpret_cast<EqState*>(work + L.ends_off);
    EqState* starts = reinterpret_cast<EqState*>(work + L.starts_off);
    uint32_t* peaks = reinterpret_cast<uint32_t*>(work + L.peak_off);
    EqState zero;
    memset(&zero, 0, sizeof zero);
    for (int c = 0; c < n_clips; ++c) {
        const EqRow& r = rows[c];
        const float* xc = x + r.offset;
        uint32_t pin = 0, pout = 0;
        int ns = 0;
        if (r.design >= 0) {
            const EqDesign& Dd = D[r.design];
            ns = Dd.ns;
            for (int k = 0; k + 1 < r.nch; ++k)
                ends[r.soff + k] = eq_chunk_host(xc, k * EQ_CHUNK, (k + 1) * EQ_CHUNK, Dd, zero, nullptr, nullptr, nullptr);
            eq_chain_host(Dd, zero, r.nch - 1, ends + r.soff, starts + r.soff);
            for (int k = 0; k < r.nch; ++k) {
                const long long hi = (long long)(k + 1) * EQ_CHUNK;
                eq_chunk_host(xc, k * EQ_CHUNK, hi < r.n ? (int)hi : r.n, Dd, starts[r.soff + k], yws + r.yoff, &pin, &pout);
            }
        } else {
            for (int i = 0; i < r.n; ++i) {
                const uint32_t a = loud_abs_bits(xc[i]);
                if (a > pin) pin = a;
            }
        }
        peaks[2 * c] = pin; peaks[2 * c + 1] = pout;
        records[c] = eq_finish(r, ns, pin, pout);
        if (r.n == 0) continue;
        if (records[c].flags & EQ_EQUALISED)
            memcpy(out + r.offset, yws + r.yoff, (size_t)r.n * sizeof(float));
        else if (out != x)
            memcpy(out + r.offset, xc, (size_t)r.n * sizeof(float));
    }
}

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------------------------------
// the device kernels
// ------------------------------------------------------------------------------------------------------------------
// The sections of one span: the one text of eq_filter_kernel and of eqs_filter_kernel (eqstream.h).  Thread tid's run is staged
// at `mine` (EQ_R floats of LDS); v becomes the last section's output for the run and carry_s (EQ_NS doubles of LDS) goes from
// the joint state in front of the span to the state behind it.  ENDS: the end state alone -- the last section's rerun is left
// out, and v is then not its output.  The scan's exchange sc is double-buffered: one barrier per step.  The section loop is not
// unrolled and indexes no register array (the carried states live in LDS), so the section count costs neither registers nor
// scratch.
// Barriers: entered by all EQ_T threads of the block (ns is block-uniform, and so is the ENDS exit) behind a barrier that
// follows the staging of the runs, the last write of carry_s and the last span's reads of sc.  It returns without one: the
// caller owes a barrier before carry_s is read, sc or carry_s is written again, or a run is read by another thread.
template <bool ENDS>
__device__ __forceinline__ void eq_sections(const EqDesign* __restrict__ D, int ns, const float* mine, double (*sc)[2][EQ_T], double* carry_s,
                                            double (&v)[EQ_R]) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int i = 0; i < EQ_R; ++i) v[i] = (double)mine[i];
#pragma unroll 1
    for (int s = 0; s < ns; ++s) {
        const double b[3] = {D->b[s][0], D->b[s][1], D->b[s][2]};
        const double na[2] = {D->na[s][0], D->na[s][1]};
        double c0 = 0.0, c1 = 0.0;
        if (tid == 0) { c0 = carry_s[2 * s]; c1 = carry_s[2 * s + 1]; }
        double e0 = c0, e1 = c1;
#pragma unroll
        for (int i = 0; i < EQ_R; ++i) eq_step(b, na, e0, e1, v[i]);
#pragma unroll 1
        for (int k = 0; k < EQ_LOG_T; ++k) {
            const int d = 1 << k, buf = k & 1;
            sc[buf][0][tid] = e0;
            sc[buf][1][tid] = e1;
            __syncthreads();
            if (tid >= d) {
                const double P[4] = {D->P[s][k][0], D->P[s][k][1], D->P[s][k][2], D->P[s][k][3]};
                eq_combine(P, sc[buf][0][tid - d], sc[buf][1][tid - d], e0, e1);
            }
        }
        sc[EQ_LOG_T & 1][0][tid] = e0;
        sc[EQ_LOG_T & 1][1][tid] = e1;
        if (tid == EQ_T - 1) { carry_s[2 * s] = e0; carry_s[2 * s + 1] = e1; }      // thread 0 read its carry before the scan
        if (ENDS && s == ns - 1) break;
        __syncthreads();
        if (tid > 0) { c0 = sc[EQ_LOG_T & 1][0][tid - 1]; c1 = sc[EQ_LOG_T & 1][1][tid - 1]; }
#pragma unroll
        for (int i = 0; i < EQ_R; ++i) v[i] = eq_step(b, na, c0, c1, v[i]);
    }
}

// The chain of one wave, the one text of eq_chain_kernel and of eqs_chain_kernel (eqstream.h): lane i keeps row i of J and
// element i (`mine`) of the joint start state of a chunk, and walks `links` chunks with their end states from zero state:
// starts[0 .. links] are written, ends[0 .. links - 1] read; links < 0: nothing.  Entered by all EQ_LANES lanes with one
// `links`; two barriers per link.
__device__ __forceinline__ void eq_chain_walk(const double* __restrict__ J, double mine, int links, const EqState* __restrict__ ends,
                                              EqState* __restrict__ starts) {
    __shared__ double s[EQ_NS];
    const int lane = threadIdx.x;
    const bool on = lane < EQ_NS;
    double Jrow[EQ_NS];
#pragma unroll
    for (int j = 0; j < EQ_NS; ++j) Jrow[j] = on ? J[EQ_NS * lane + j] : 0.0;
    for (int c = 0; c <= links; ++c) {
        if (on) {
            starts[c].s[lane] = mine;
            s[lane] = mine;
        }
        if (c == links) break;
        __syncthreads();
        double left[EQ_NS];
#pragma unroll
        for (int j = 0; j < EQ_NS; ++j) left[j] = s[j];
        if (on) mine = eq_chain_row(Jrow, left, ends[c].s[lane]);
        __syncthreads();
    }
}

// One block per chunk of a clip.  ENDS: the first half over the chunks that have a successor -- from zero state to the chunk's
// end state, nothing else written.  Else the full pass from the chunk's true start state: y and both peaks.  The span is staged in
// LDS by coalesced loads, each thread's run padded by one float so the runs start in different banks; y goes back through the
// same slots.
template <bool ENDS>
static __global__ __launch_bounds__(EQ_T) void eq_filter_kernel(const float* __restrict__ x, const EqRow* __restrict__ rows,
                                                                const EqDesign* __restrict__ designs, float* __restrict__ yws,
                                                                EqState* __restrict__ ends, const EqState* __restrict__ starts,
                                                                uint32_t* __restrict__ peaks) {
    __shared__ float xs[EQ_T * (EQ_R + 1)];
    __shared__ double sc[2][2][EQ_T];
    __shared__ double carry_s[EQ_NS];
    __shared__ uint32_t peak_s[2];
    const EqRow row = rows[blockIdx.y];
    const int tid = threadIdx.x, chunk = blockIdx.x;
    if (chunk >= (ENDS ? row.nch - 1 : row.nch)) return;       // block-uniform
    if (row.design < 0) {                                       // measure only: the peak of x
        uint32_t peak = 0;
        const float* __restrict__ xc = x + row.offset;
        const long long hi = (long long)(chunk + 1) * EQ_CHUNK;
        const int end = hi < row.n ? (int)hi : row.n;
        if (ENDS) return;
        for (int k = chunk * EQ_CHUNK + tid; k < end; k += EQ_T) {
            const uint32_t a = loud_abs_bits(xc[k]);
            peak = a > peak ? a : peak;
        }
        if (tid == 0) peak_s[0] = 0;
        __syncthreads();
        atomicMax(&peak_s[0], peak);
        __syncthreads();
        if (tid == 0) atomicMax(&peaks[2 * blockIdx.y], peak_s[0]);
        return;
    }
    const EqDesign* __restrict__ D = designs + row.design;
    const int ns = D->ns;
    const long long chunk_hi = (long long)(chunk + 1) * EQ_CHUNK;
    const int lo = chunk * EQ_CHUNK, hi = chunk_hi < row.n ? (int)chunk_hi : row.n;
    const float* __restrict__ xc = x + row.offset;
    float* __restrict__ yc = yws + row.yoff;
    if (tid < 2) peak_s[tid] = 0;
    if (tid < EQ_NS) carry_s[tid] = ENDS ? 0.0 : starts[row.soff + chunk].s[tid];
    uint32_t peak_in = 0, peak_out = 0;
    float* mine = xs + tid * (EQ_R + 1);
    for (int s0 = lo; s0 < hi; s0 += EQ_SPAN) {
        const int cnt = hi - s0 < EQ_SPAN ? hi - s0 : EQ_SPAN;
        for (int k = tid; k < EQ_SPAN; k += EQ_T) {
            float xv = 0.f;
            if (k < cnt) {
                xv = xc[s0 + k];
                const uint32_t a = loud_abs_bits(xv);
                peak_in = a > peak_in ? a : peak_in;
            }
            xs[(k / EQ_R) * (EQ_R + 1) + k % EQ_R] = xv;
        }
        __syncthreads();                // xs, and carry_s of the last span (or of the prologue)
        double v[EQ_R];
        eq_sections<ENDS>(D, ns, mine, sc, carry_s, v);
        if (!ENDS) {
            if (tid * EQ_R < cnt) {
#pragma unroll
                for (int i = 0; i < EQ_R; ++i) {
                    const float o = loud_store(v[i]);
                    mine[i] = o;
                    if (tid * EQ_R + i < cnt) {
                        const uint32_t a = loud_abs_bits(o);
                        peak_out = a > peak_out ? a : peak_out;
                    }
                }
            }
            __syncthreads();
            for (int k = tid; k < cnt; k += EQ_T) yc[s0 + k] = xs[(k / EQ_R) * (EQ_R + 1) + k % EQ_R];
        }
        __syncthreads();        // the next span stages over xs and sc
    }
    if (ENDS) {
        if (tid < EQ_NS) ends[row.soff + chunk].s[tid] = carry_s[tid];
        return;
    }
    atomicMax(&peak_s[0], peak_in);
    atomicMax(&peak_s[1], peak_out);
    __syncthreads();
    if (tid < 2) atomicMax(&peaks[2 * blockIdx.y + tid], peak_s[tid]);      // integer maxima: the order of the chunks does not show
}

// between the two: one wave per clip chains its chunks from zero state and clears the clip's peaks
static __global__ __launch_bounds__(EQ_LANES) void eq_chain_kernel(const EqRow* __restrict__ rows, const EqDesign* __restrict__ designs,
                                                                   const EqState* __restrict__ ends, EqState* __restrict__ starts,
                                                                   uint32_t* __restrict__ peaks) {
    const EqRow row = rows[blockIdx.x];
    if (threadIdx.x < 2) peaks[2 * blockIdx.x + threadIdx.x] = 0;
    if (row.design < 0) return;                 // block-uniform
    eq_chain_walk(designs[row.design].J, 0.0, row.nch - 1, ends + row.soff, starts + row.soff);
}

// last: the record, and out = y (a clip that was equalised) or x (measure only, or a NaN or an infinity among the samples: in
// place nothing is written) inside [offset, offset + n) of every clip
static __global__ __launch_bounds__(256) void eq_commit_kernel(const float* x, const EqRow* __restrict__ rows, const EqDesign* __restrict__ designs,
                                                               const float* __restrict__ yws, const uint32_t* __restrict__ peaks,
                                                               EqRecord* __restrict__ records, float* out) {
    const EqRow row = rows[blockIdx.y];
    const EqRecord rec = eq_finish(row, row.design < 0 ? 0 : designs[row.design].ns, peaks[2 * blockIdx.y], peaks[2 * blockIdx.y + 1]);
    if (blockIdx.x == 0 && threadIdx.x == 0) records[blockIdx.y] = rec;
    const bool copy = !(rec.flags & EQ_EQUALISED);
    if (copy && out == x) return;
    const float* src = copy ? x + row.offset : yws + row.yoff;      // out may be x: no restrict
    float* oc = out + row.offset;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < row.n; i += gridDim.x * 256) oc[i] = src[i];
}
#endif

}  // namespace gsv
