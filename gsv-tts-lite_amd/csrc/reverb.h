// reverb: Freeverb -- eight parallel damped comb filters, their sum through four all-pass filters in series -- over B packed fp32
// clips, each clip with one of a few parameter sets.  From zero state, everything in fp64, one rounding to fp32 at
// the end (saturating, loud_store's rule); same length out as in, the tail behind the clip is cut.  Per sample, v = (double)x[n]:
//
//   u = gin v
//   comb k (delay Dk):      o_k = b_k[n - Dk];   l_k = (1 - d) o_k + d l_k;   b_k[n] = u + fb l_k
//   s = ((((((o_0 + o_1) + o_2) + o_3) + o_4) + o_5) + o_6) + o_7
//   all-pass j (delay Ej):  t = a_j[n - Ej];   a_j[n] = s + 0.5 t;   s = t - s
//   y = fp32(gw s + gd v)
//
// Everything that decides a bit -- the steps, the combine of the scan, the order of the sum, the mix, the record -- is one
// __host__ __device__ text for the kernels, for the host twin rvb_run_host (gsv_reverb_host: the CPU path and the device's oracle)
// and for the stand-alone checker tools/reverb_host_check.cpp.  Every multiply-add is an explicit fma, every other product stands
// alone and every order is fixed, so contraction has nothing to change and device samples and records equal the host's bit for
// bit.  No long double anywhere: the scan's powers of d are squared in fp64.
//
// The parallel form.  Every feedback path goes through a delay line, so nothing inside a block of D consecutive samples depends
// on the block itself but through the damping filter:
//
//   combs     b_k is kept for the whole clip (a plane of n doubles in the workspace), so o_k[n] is b_k[n - Dk] and there is no
//             ring.  One wave per (clip, comb) walks the clip in blocks of Dk samples, each block in spans of RVB_SPAN; lane t
//             holds RVB_R consecutive samples.  Over a span the o are known (written one block earlier), l is a one-pole scan
//             over them -- each lane runs its o from zero state (lane 0: from the l the last span left), a Hillis-Steele scan
//             with P[k] = d^(RVB_R 2^k) gives every run's true end state, and the lane reruns its samples from the true end state
//             of its left neighbour -- and b is elementwise.  A sample's place in its block decides its lane, the same in every
//             block, and every lane loads and stores its own run of the plane.  So the b a lane needs are the b that same lane
//             stored one block earlier -- one thread's program order, no other lane's store is ever read: with Dk <= RVB_SPAN
//             (every rate up to 55 kHz) a block is one span and they stay in the lane's registers, longer lines are read back
//             from the plane at the addresses the lane wrote.  Whoever changes which lane stores a sample (coalesced rows, say)
//             makes that read cross lanes, and then owes it a barrier between the store and the read-back.
//             A span shorter than RVB_SPAN is padded with zeros; what the padding turns into is never written, and a prefix of
//             a scan depends on the runs to its left.
//   sum       o_0 .. o_7 are read from the planes at n - Dk in the fixed order above, one thread per sample.
//   all-pass  the recurrence a[n] = s[n] + 0.5 a[n - E] couples samples E apart and nothing else: thread p < E runs the phase
//             n = p, p + E, p + 2E, ... serially with a in a register, RVB_U loads ahead.  This is the serial loop's own
//             arithmetic, in another order of n.  One launch per all-pass; the last one mixes, rounds, stores and takes the peak.
//
// The stages meet at kernel boundaries alone: no workgroup waits for another, and every loop is bounded by the clip's length.
// Launches: the combs (with max |x|), the sum, four all-passes, the records: seven, whatever the batch and the lengths.
//
// A clip holding a NaN or an infinity is known from the integer maximum of its |x| bit patterns when the comb launch is over;
// the last all-pass launch copies such a clip (in place: writes nothing), as it does a clip with params -1.
//
// Workspace: [RvbRow rows[B] | RvbDesign designs[P] | stats u32 [2 B]: max |x| bits, max |y| bits] -- one upload, the stats as
// zeros -- then [b fp64, 8 planes of W | s fp64 [W]], W the samples of the clips that have a parameter set: 72 bytes per sample.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <type_traits>
#include <vector>

#include "loudness.h"

namespace gsv {

constexpr int RVB_COMBS = 8, RVB_APS = 4;
constexpr int RVB_T = 64;                       // lanes of the comb wave
constexpr int RVB_LOG_T = 6;
constexpr int RVB_R = 32;                       // consecutive samples per lane and span
constexpr int RVB_SPAN = RVB_T * RVB_R;
constexpr int RVB_AT = 256;                     // threads of an all-pass block
constexpr int RVB_U = 32;                       // loads ahead in a phase
constexpr int RVB_MAX_DELAY = 32768;
constexpr int RVB_MAX_CLIPS = 65535, RVB_MAX_DESIGNS = 65535;
constexpr int RVB_REVERBED = 1, RVB_NONFINITE = 4;      // record flags
static_assert(RVB_T == 1 << RVB_LOG_T && (RVB_R & (RVB_R - 1)) == 0, "scan steps, powers by squaring");

struct RvbClip {            // gsv_reverb_clip
    long long offset;       // first sample in the packed buffer
    int32_t n;
    int32_t design;         // index into the parameter sets of the call; -1: measure the peaks, copy
};
static_assert(sizeof(RvbClip) == 16, "clip");

struct RvbParams {          // gsv_reverb_params
    int32_t comb[RVB_COMBS], allpass[RVB_APS];  // the delays in samples, each 1 .. RVB_MAX_DELAY
    double d, fb;           // damping and feedback, each in [0, 1)
    double gin, gw, gd;     // input, wet and dry gains
};
static_assert(sizeof(RvbParams) == 88, "params");

struct RvbRecord {          // gsv_reverb_record
    float peak_in, peak_out;            // max |x|, max |y|
    int32_t flags, pad;
};
static_assert(sizeof(RvbRecord) == 16, "record");

struct RvbRow {             // one clip as the kernels see it (built on the host, first part of the workspace)
    long long offset, woff; // woff: the clip's first double in a plane
    int32_t n, design;
};
static_assert(sizeof(RvbRow) == 24, "row");

struct RvbDesign {          // one parameter set as the kernels see it (built on the host, behind the rows)
    int32_t comb[RVB_COMBS], allpass[RVB_APS];
    double d, omd, fb, gin, gw, gd;     // omd = 1 - d
    double P[RVB_LOG_T];                // d^(RVB_R 2^k)
};
static_assert(sizeof(RvbDesign) % 8 == 0, "design");

// no product of the routines below may melt into a neighbouring sum, here or where they are inlined
#if defined(__clang__)
#define RVB_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define RVB_NO_CONTRACT
#endif

// one sample of a comb's damping filter: l behind the line's output o
LOUD_HD double rvb_damp(double d, double omd, double l, double o) {
    RVB_NO_CONTRACT
    return fma(d, l, omd * o);
}

// what a comb writes into its line: the scaled input plus the damped feedback
LOUD_HD double rvb_line(double gin, double fb, double l, float x) {
    RVB_NO_CONTRACT
    return fma(l, fb, gin * (double)x);
}

// the scan: own after left, A = d^(length of own)
LOUD_HD double rvb_combine(double A, double left, double own) { return fma(A, left, own); }

// the eight comb outputs at sample i of a clip, summed in the definition's order; b: the clip's first plane
LOUD_HD double rvb_sum(const double* b, long long plane, const int32_t* D, long long i) {
    RVB_NO_CONTRACT
    double s = 0.0;
    for (int k = 0; k < RVB_COMBS; ++k) {
        const double o = i >= D[k] ? b[k * plane + (i - D[k])] : 0.0;
        s = k == 0 ? o : s + o;
    }
    return s;
}

// one sample of an all-pass: a is the line's output going in, what the line takes coming out -> the filter's output
LOUD_HD double rvb_ap_step(double& a, double s) {
    RVB_NO_CONTRACT
    const double t = a;
    a = fma(0.5, t, s);
    return t - s;
}

LOUD_HD float rvb_mix(double gw, double gd, double s, float x) {
    RVB_NO_CONTRACT
    return loud_store(fma(s, gw, (double)x * gd));
}

LOUD_HD bool rvb_nonfinite(uint32_t peak_in) { return peak_in >= 0x7F800000u; }

// the samples of such a clip come from x
LOUD_HD bool rvb_copied(const RvbRow& row, uint32_t peak_in) { return row.design < 0 || rvb_nonfinite(peak_in); }

LOUD_HD RvbRecord rvb_finish(const RvbRow& row, uint32_t peak_in, uint32_t peak_out) {
    RvbRecord r;
    const bool copied = rvb_copied(row, peak_in);
    r.peak_in = loud_from_bits(peak_in);
    r.peak_out = loud_from_bits(copied ? peak_in : peak_out);
    r.flags = rvb_nonfinite(peak_in) ? RVB_NONFINITE : (copied ? 0 : RVB_REVERBED);
    r.pad = 0;
    return r;
}

// ------------------------------------------------------------------------------------------------------------------
// host only: the checks, the workspace layout, the powers, the serial twin
// ------------------------------------------------------------------------------------------------------------------
// 0: fine; 1: a delay outside 1 .. RVB_MAX_DELAY; 2: d or fb outside [0, 1); 3: a gain that is not finite
inline int rvb_params_bad(const RvbParams& p) {
    for (int k = 0; k < RVB_COMBS; ++k)
        if (p.comb[k] < 1 || p.comb[k] > RVB_MAX_DELAY) return 1;
    for (int j = 0; j < RVB_APS; ++j)
        if (p.allpass[j] < 1 || p.allpass[j] > RVB_MAX_DELAY) return 1;
    if (!(p.d >= 0.0 && p.d < 1.0) || !(p.fb >= 0.0 && p.fb < 1.0)) return 2;
    if (!isfinite(p.gin) || !isfinite(p.gw) || !isfinite(p.gd)) return 3;
    return 0;
}

struct RvbLayout {
    size_t rows_off, designs_off, stats_off, head_bytes, b_off, s_off, bytes;
    long long plane;        // W: doubles of one plane
    int max_n;
    bool any_copy;          // a clip with params -1
};

// false on arguments the entries refuse; fills the rows when `rows` is given
inline bool rvb_layout(const RvbClip* clips, int n_clips, int n_designs, size_t n_x, bool check_x, RvbLayout* L, RvbRow* rows) {
    if (!clips || n_clips < 1 || n_clips > RVB_MAX_CLIPS || n_designs < 0 || n_designs > RVB_MAX_DESIGNS) return false;
    long long w = 0;
    int max_n = 0;
    bool any_copy = false;
    for (int c = 0; c < n_clips; ++c) {
        const RvbClip& cl = clips[c];
        if (cl.n < 0 || cl.offset < 0 || cl.design < -1 || cl.design >= n_designs) return false;
        if (check_x && (unsigned long long)cl.offset + (unsigned long long)cl.n > (unsigned long long)n_x) return false;
        if (rows) {
            RvbRow& r = rows[c];
            r.offset = cl.offset; r.woff = w; r.n = cl.n; r.design = cl.design;
        }
        if (cl.design >= 0) w += cl.n;
        else any_copy = true;
        if (cl.n > max_n) max_n = cl.n;
    }
    L->rows_off = 0;
    L->designs_off = loud_align16((size_t)n_clips * sizeof(RvbRow));
    L->stats_off = L->designs_off + loud_align16((size_t)n_designs * sizeof(RvbDesign));
    L->head_bytes = L->stats_off + loud_align16((size_t)n_clips * 2 * sizeof(uint32_t));
    L->b_off = L->head_bytes;
    L->s_off = L->b_off + (size_t)RVB_COMBS * loud_align16((size_t)w * sizeof(double));
    L->bytes = L->s_off + loud_align16((size_t)w * sizeof(double));
    L->plane = (long long)(loud_align16((size_t)w * sizeof(double)) / sizeof(double));
    L->max_n = max_n;
    L->any_copy = any_copy;
    return true;
}

inline void rvb_design(const RvbParams& p, RvbDesign* out) {
    RvbDesign& D = *out;
    memset(&D, 0, sizeof D);
    memcpy(D.comb, p.comb, sizeof D.comb);
    memcpy(D.allpass, p.allpass, sizeof D.allpass);
    D.d = p.d; D.omd = 1.0 - p.d; D.fb = p.fb;
    D.gin = p.gin; D.gw = p.gw; D.gd = p.gd;
    double v = p.d;                     // d^RVB_R, then its squares: each product is rounded to fp64, the same wherever it runs
    for (int r = RVB_R; r > 1; r >>= 1) v = v * v;
    for (int k = 0; k < RVB_LOG_T; ++k) {
        D.P[k] = v;
        v = v * v;
    }
}

// comb k of a clip as its wave runs it (rvb_comb_kernel below): the plane bk [n] from the clip's samples
inline void rvb_comb_host(const float* xc, int n, const RvbDesign& D, int k, double* bk) {
    static thread_local double o[RVB_T][RVB_R], st[RVB_T], nx[RVB_T];
    const int Dk = D.comb[k];
    double carry = 0.0;
    for (long long b0 = 0; b0 < n; b0 += Dk) {
        const int blen = n - b0 < Dk ? (int)(n - b0) : Dk;
        for (int s0 = 0; s0 < blen; s0 += RVB_SPAN) {
            const int cnt = blen - s0 < RVB_SPAN ? blen - s0 : RVB_SPAN;
            const long long at = b0 + s0;
            const int nl = (cnt + RVB_R - 1) / RVB_R;   // the lanes that hold a sample: a prefix of the scan needs no lane to its right
            for (int i = 0; i < nl * RVB_R; ++i) o[i / RVB_R][i % RVB_R] = i < cnt && b0 > 0 ? bk[at + i - Dk] : 0.0;
            for (int t = 0; t < nl; ++t) {
                double l = t == 0 ? carry : 0.0;
                for (int j = 0; j < RVB_R; ++j) l = rvb_damp(D.d, D.omd, l, o[t][j]);
                st[t] = l;
            }
            for (int s = 0; s < RVB_LOG_T; ++s) {
                const int dd = 1 << s;
                for (int t = 0; t < nl; ++t) nx[t] = t >= dd ? rvb_combine(D.P[s], st[t - dd], st[t]) : st[t];
                memcpy(st, nx, sizeof(double) * nl);
            }
            double next = carry;
            for (int t = 0; t < nl; ++t) {
                double l = t == 0 ? carry : st[t - 1];
                for (int j = 0; j < RVB_R && t * RVB_R + j < cnt; ++j) {
                    const int i = t * RVB_R + j;
                    l = rvb_damp(D.d, D.omd, l, o[t][j]);
                    bk[at + i] = rvb_line(D.gin, D.fb, l, xc[at + i]);
                    if (i == cnt - 1) next = l;
                }
            }
            carry = next;
        }
    }
}

// the whole call over host memory.  work holds rvb_layout's bytes; out may be x (in place).
inline void rvb_run_host(const float* x, const RvbClip* clips, int n_clips, const RvbParams* designs, int n_designs, float* out, RvbRecord* records,
                         unsigned char* work) {
    RvbLayout L;
    RvbRow* rows = reinterpret_cast<RvbRow*>(work);
    if (!rvb_layout(clips, n_clips, n_designs, 0, false, &L, rows)) return;
    RvbDesign* D = reinterpret_cast<RvbDesign*>(work + L.designs_off);
    for (int d = 0; d < n_designs; ++d) rvb_design(designs[d], &D[d]);
    double* b = reinterpret_cast<double*>(work + L.b_off);
    double* s = reinterpret_cast<double*>(work + L.s_off);
    std::vector<double> line;
    for (int c = 0; c < n_clips; ++c) {
        const RvbRow& r = rows[c];
        const float* xc = x + r.offset;
        float* oc = out + r.offset;
        uint32_t peak_in = 0, peak_out = 0;
        for (int i = 0; i < r.n; ++i) {
            const uint32_t a = loud_abs_bits(xc[i]);
            if (a > peak_in) peak_in = a;
        }
        records[c] = rvb_finish(r, peak_in, 0);
        if (rvb_copied(r, peak_in)) {
            if (out != x && r.n > 0) memcpy(oc, xc, (size_t)r.n * sizeof(float));
            continue;
        }
        const RvbDesign& Dd = D[r.design];
        double* bc = b + r.woff;
        double* sc = s + r.woff;
        for (int k = 0; k < RVB_COMBS; ++k) rvb_comb_host(xc, r.n, Dd, k, bc + k * L.plane);
        for (int i = 0; i < r.n; ++i) sc[i] = rvb_sum(bc, L.plane, Dd.comb, i);
        for (int j = 0; j < RVB_APS; ++j) {
            const int E = Dd.allpass[j];
            line.assign((size_t)E, 0.0);
            for (int i = 0; i < r.n; ++i) sc[i] = rvb_ap_step(line[(size_t)(i % E)], sc[i]);
        }
        for (int i = 0; i < r.n; ++i) {
            const float y = rvb_mix(Dd.gw, Dd.gd, sc[i], xc[i]);
            const uint32_t a = loud_abs_bits(y);
            if (a > peak_out) peak_out = a;
            oc[i] = y;
        }
        records[c] = rvb_finish(r, peak_in, peak_out);
    }
}

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------------------------------
// the device kernels
// ------------------------------------------------------------------------------------------------------------------
// One wave per (comb, clip): blockIdx.x the comb, blockIdx.y the clip.  Comb 0's wave also takes max |x| of the clip from the
// samples it loads; the eight waves of a clip with params -1 share that maximum among them.  Lane t owns the samples
// [t RVB_R, (t + 1) RVB_R) of every span of every block, loads and stores included.  b of the block before is `keep`
// (Dk <= RVB_SPAN: one span per block) or is read back from the plane at the addresses this same lane stored one block earlier.
static __global__ __launch_bounds__(RVB_T) void rvb_comb_kernel(const float* __restrict__ x, const RvbRow* __restrict__ rows,
                                                                const RvbDesign* __restrict__ designs, double* __restrict__ b, long long plane,
                                                                uint32_t* __restrict__ stats) {
    __shared__ double sc[2][RVB_T];
    __shared__ double carry_s;
    __shared__ uint32_t peak_s;
    const RvbRow row = rows[blockIdx.y];
    const int tid = threadIdx.x, k = blockIdx.x, n = row.n;
    const float* __restrict__ xc = x + row.offset;
    uint32_t peak = 0;
    if (row.design < 0) {                       // block-uniform: measure only, the eight waves share the clip, four loads in flight each
        for (long long i0 = (long long)(k * RVB_T + tid) * 4; i0 < n; i0 += (long long)RVB_COMBS * RVB_T * 4) {
            uint32_t a[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) a[u] = i0 + u < n ? loud_abs_bits(xc[i0 + u]) : 0u;
#pragma unroll
            for (int u = 0; u < 4; ++u) peak = a[u] > peak ? a[u] : peak;
        }
        if (tid == 0) peak_s = 0;
        __syncthreads();
        atomicMax(&peak_s, peak);
        __syncthreads();
        if (tid == 0) atomicMax(&stats[2 * blockIdx.y], peak_s);       // an integer maximum over statistics that were uploaded as zeros
        return;
    }
    const RvbDesign* __restrict__ D = designs + row.design;
    const int Dk = D->comb[k];
    const double d = D->d, omd = D->omd, fb = D->fb, gin = D->gin;
    double P[RVB_LOG_T];
#pragma unroll
    for (int s = 0; s < RVB_LOG_T; ++s) P[s] = D->P[s];
    double* __restrict__ bk = b + k * plane + row.woff;
    const bool in_regs = Dk <= RVB_SPAN;        // block-uniform
    constexpr int LAST = RVB_LOG_T & 1;
    double keep[RVB_R];
#pragma unroll
    for (int j = 0; j < RVB_R; ++j) keep[j] = 0.0;
    if (tid == 0) carry_s = 0.0;
    __syncthreads();
    const int base = tid * RVB_R;
    // the spans of the blocks in order, (b0, s0) the block's and the span's first sample.  Each lane loads and stores its own run
    // (turning coalesced rows into runs through LDS was measured and lost: the wave is bound by the instructions it issues, not
    // by memory); x of the span to come is requested before this span's scan, so that its latency hides behind the arithmetic.
    long long b0 = 0;
    int s0 = 0;
    float xv[RVB_R];
    {
        const int cnt = n < Dk ? (n < RVB_SPAN ? n : RVB_SPAN) : (Dk < RVB_SPAN ? Dk : RVB_SPAN);
#pragma unroll
        for (int j = 0; j < RVB_R; ++j) xv[j] = base + j < cnt ? xc[base + j] : 0.f;
    }
    while (b0 < n) {
        const int blen = n - b0 < Dk ? (int)(n - b0) : Dk;
        const int cnt = blen - s0 < RVB_SPAN ? blen - s0 : RVB_SPAN;
        const long long at = b0 + s0 + base;            // this lane's first sample
#pragma unroll
        for (int j = 0; j < RVB_R; ++j) {
            const uint32_t a = loud_abs_bits(xv[j]);    // every sample of the clip passes here once; the padding is +0
            peak = a > peak ? a : peak;
        }
        long long nb0 = b0;
        int ns0 = s0 + RVB_SPAN;
        if (ns0 >= blen) { nb0 = b0 + Dk; ns0 = 0; }
        float xn[RVB_R];
        {
            const int nblen = nb0 >= n ? 0 : (n - nb0 < Dk ? (int)(n - nb0) : Dk);
            const int ncnt = nblen - ns0 < RVB_SPAN ? nblen - ns0 : RVB_SPAN;      // <= 0 behind the clip's last span
            const long long nat = nb0 + ns0 + base;
#pragma unroll
            for (int j = 0; j < RVB_R; ++j) xn[j] = base + j < ncnt ? xc[nat + j] : 0.f;
        }
        if (!in_regs) {
#pragma unroll
            for (int j = 0; j < RVB_R; ++j) keep[j] = base + j < cnt && b0 > 0 ? bk[at + j - Dk] : 0.0;
        } else {
#pragma unroll
            for (int j = 0; j < RVB_R; ++j) keep[j] = base + j < cnt ? keep[j] : 0.0;
        }
        const double carry = carry_s;           // lane 0's start; behind the barrier that follows its last write
        double l = tid == 0 ? carry : 0.0;
#pragma unroll
        for (int j = 0; j < RVB_R; ++j) l = rvb_damp(d, omd, l, keep[j]);
#pragma unroll
        for (int s = 0; s < RVB_LOG_T; ++s) {
            const int dd = 1 << s, buf = s & 1;
            sc[buf][tid] = l;
            __syncthreads();
            if (tid >= dd) l = rvb_combine(P[s], sc[buf][tid - dd], l);
        }
        sc[LAST][tid] = l;                      // the reads of this plane are behind the last step's barrier
        __syncthreads();
        l = tid > 0 ? sc[LAST][tid - 1] : carry;
        double last = 0.0;                      // l behind the span's last sample, in the lane that holds it
#pragma unroll
        for (int j = 0; j < RVB_R; ++j) {
            l = rvb_damp(d, omd, l, keep[j]);
            if (base + j < cnt) {
                keep[j] = rvb_line(gin, fb, l, xv[j]);
                bk[at + j] = keep[j];
            }
            last = base + j == cnt - 1 ? l : last;
        }
        if (base < cnt && cnt <= base + RVB_R) carry_s = last;
#pragma unroll
        for (int j = 0; j < RVB_R; ++j) xv[j] = xn[j];
        b0 = nb0;
        s0 = ns0;
        __syncthreads();                        // carry_s; the next span writes sc
    }
    if (k == 0) {                               // block-uniform
        if (tid == 0) peak_s = 0;
        __syncthreads();
        atomicMax(&peak_s, peak);
        __syncthreads();
        if (tid == 0) stats[2 * blockIdx.y] = peak_s;
    }
}

// s of every clip from its comb planes: one thread per sample
static __global__ __launch_bounds__(RVB_AT) void rvb_sum_kernel(const RvbRow* __restrict__ rows, const RvbDesign* __restrict__ designs,
                                                                const double* __restrict__ b, long long plane, double* __restrict__ s) {
    const RvbRow row = rows[blockIdx.y];
    if (row.design < 0) return;
    const int32_t* __restrict__ Dk = designs[row.design].comb;
    const double* __restrict__ bc = b + row.woff;
    double* __restrict__ sc = s + row.woff;
    for (long long i = (long long)blockIdx.x * RVB_AT + threadIdx.x; i < row.n; i += (long long)gridDim.x * RVB_AT) sc[i] = rvb_sum(bc, plane, Dk, i);
}

// All-pass J of every clip: thread p of a clip runs the phase p, p + E, p + 2E, ...  J 0, 1 and 2 run s in place, 3 reads s and
// writes the clip -- or copies it (params -1, a NaN or an infinity among the samples).
template <int J>
static __global__ __launch_bounds__(RVB_AT) void rvb_ap_kernel(const float* x, const RvbRow* __restrict__ rows, const RvbDesign* __restrict__ designs,
                                                               double* __restrict__ s, uint32_t* __restrict__ stats, float* out) {
    __shared__ uint32_t peak_s;
    const RvbRow row = rows[blockIdx.y];
    const int tid = threadIdx.x, n = row.n;
    const float* xc = x + row.offset;           // out may be x: no restrict
    float* oc = out + row.offset;
    if (J == 3) {
        if (rvb_copied(row, stats[2 * blockIdx.y])) {           // block-uniform
            if (out != x)
                for (long long i = (long long)blockIdx.x * RVB_AT + tid; i < n; i += (long long)gridDim.x * RVB_AT) oc[i] = xc[i];
            return;
        }
    } else if (row.design < 0) {
        return;
    }
    const RvbDesign* __restrict__ D = designs + row.design;
    const int E = D->allpass[J];
    const long long p = (long long)blockIdx.x * RVB_AT + tid;
    double* __restrict__ sc = s + row.woff;
    const double gw = D->gw, gd = D->gd;
    uint32_t peak = 0;
    double a = 0.0;
    if (p < E) {
        // RVB_U samples of the phase at a time: all loads first, then the chain.  A group that lies inside the clip runs unguarded.
        auto group = [&](long long i0, auto guarded) {
            double* at = sc + i0;               // read, then written in place: one pointer
            const float* xsrc = xc + i0;
            float* ydst = oc + i0;
            double v[RVB_U];
            float xv[RVB_U];
#pragma unroll
            for (int u = 0; u < RVB_U; ++u) {
                const bool in = !decltype(guarded)::value || i0 + (long long)u * E < n;
                v[u] = in ? at[u * E] : 0.0;
                xv[u] = J == 3 && in ? xsrc[u * E] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < RVB_U; ++u) {
                if (decltype(guarded)::value && i0 + (long long)u * E >= n) break;
                const double o = rvb_ap_step(a, v[u]);
                if (J < 3) {
                    at[u * E] = o;
                } else {
                    const float y = rvb_mix(gw, gd, o, xv[u]);
                    const uint32_t ab = loud_abs_bits(y);
                    peak = ab > peak ? ab : peak;
                    ydst[u * E] = y;
                }
            }
        };
        long long i0 = p;
        for (; i0 + (long long)(RVB_U - 1) * E < n; i0 += (long long)E * RVB_U) group(i0, std::false_type());
        if (i0 < n) group(i0, std::true_type());
    }
    if (J == 3) {
        if (tid == 0) peak_s = 0;
        __syncthreads();
        atomicMax(&peak_s, peak);
        __syncthreads();
        if (tid == 0) atomicMax(&stats[2 * blockIdx.y + 1], peak_s);       // an integer maximum: the order of the blocks does not show
    }
}

// last: the records
static __global__ __launch_bounds__(RVB_AT) void rvb_record_kernel(const RvbRow* __restrict__ rows, const uint32_t* __restrict__ stats,
                                                                   RvbRecord* __restrict__ records, int n_clips) {
    const int c = blockIdx.x * RVB_AT + threadIdx.x;
    if (c < n_clips) records[c] = rvb_finish(rows[c], stats[2 * c], stats[2 * c + 1]);
}
#endif

}  // namespace gsv
