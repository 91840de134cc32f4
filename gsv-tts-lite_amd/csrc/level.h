// level: a running BS.1770 gain for a stream of fp32 samples.  The clip meter of loudness.h needs the whole
// programme; a stream has handed out its first packets before that exists.  Here the same K-weighting, 400 ms blocks and two
// gates are measured over the stream so far, hop by hop (a hop is a quarter block), and a gain moves towards the target along
// knots at the hop boundaries: decided from complete hops only, so everything a sample needs is known before it arrives and
// the leveller adds no delay.
//
// Everything that decides a bit -- the knot grid, the filter step and the scan's combine (loudness.h), the summation trees, the
// gates, the desired gain with its clamps and slew, the gain of a sample -- is one __host__ __device__ text for the two kernels,
// for the host twin level_push_host (gsv_level_push_host: the CPU path and the device's oracle) and for the stand-alone checker
// tools/level_host_check.cpp.  All decisions are fp64 with every multiply-add an explicit fma and every order fixed; the device
// takes no pow, log, sin or cos: the constants that need them are built on the host (level_init_host) and live in the state.
//
// A hop is filtered once, when its last sample has arrived, in a shape that depends only on the hop's place in the stream:
// LEVEL_T threads take runs of R consecutive samples (R from the rate, so that a hop up to 81.9 kHz is one span of LEVEL_T * R
// samples; a longer hop takes further spans, the state carried from span to span), thread t from zero state (thread 0: from the
// carried state), a Hillis-Steele scan with P_k = M^(R 2^k) turns the end states into true end states, every thread reruns its
// samples from its left neighbour's and sums y^2, and one halving tree over the LEVEL_T sums gives the hop sum S_h.  Every run
// of a span but the FIRST has R samples -- what the scan's algebra needs (level_run_off) --; the end state is read where the last
// run ends.
// No filtered signal is stored: the hop sums are the history.
//
// The caller-owned state: [LevelHeader | knots fp64 [cap_hops + 2] | hop sums fp64 [cap_hops] | blocks fp64 [cap_blocks] |
// ring fp32 [ring]], each part 16-byte aligned.  The ring holds the newest samples of the stream, sample s at ring[s % ring]:
// longer than a hop, so the samples of the incomplete hop wait there whatever the pushes were.  From a state as init left it, the
// state after N samples does not depend on how they were cut into pushes, byte for byte.  A flush does not wipe the state: it sets
// `ended`, and the next push restarts the moving part of the header; the knots, hop sums, blocks and ring of the stream before
// stay where the new stream has not yet overwritten them (nothing reads them), so the bytes of a second stream on one buffer
// depend on the first, while its samples and records do not.
#pragma once
#include <cmath>

#include "loudness.h"

namespace gsv {

constexpr int32_t LEVEL_MAGIC = 0x4C56454C;        // "LEVL"
constexpr int LEVEL_T = 512;                       // threads of the measure block
constexpr int LEVEL_LOG_T = 9;
constexpr int LEVEL_R_MAX = 16;                    // the longest run of one thread
constexpr int LEVEL_APPLY_T = 256;
constexpr int LEVEL_MIN_RATE = 4000, LEVEL_MAX_RATE = 192000;      // the shelf sits at 1500 Hz; a hop at 192 kHz is three spans
constexpr int LEVEL_MAX_SECONDS = 3600;            // the block history; (seconds + 1) * rate stays an int
constexpr int LEVEL_MEASURED = 2, LEVEL_NONFINITE = 4, LEVEL_FULL = 8;     // record flags (MEASURED, NONFINITE as LOUD_*)
static_assert(LEVEL_T == 1 << LEVEL_LOG_T, "scan steps");

struct LevelRecord {        // gsv_level_record
    double zbar;            // the running measure of the unlevelled stream: mean square of the blocks past both gates, 0 without
    float gain_first, gain_last;        // the gain of the push's first and last sample (an empty push: of the next sample)
    long long clamped;      // samples of the stream so far set to +-peak_limit
    int32_t blocks, above_abs, kept, flags;
};
static_assert(sizeof(LevelRecord) == 40, "record");

struct LevelHeader {
    int32_t magic, rate, cap_hops, cap_blocks, ring, R, ended, pad0;
    // the moving part
    long long n_in;         // samples of the stream so far
    long long clamped;
    int32_t hops, K;        // complete hops measured; the last knot decided (K = hops + 1 until the measure freezes)
    int32_t flags, blocks, above, kept;
    uint32_t peak_bits;     // the largest |x| bit pattern of the measured hops
    int32_t pad1;
    double zbar;
    LoudState filt;         // the K-filter's state behind the last measured hop
    // constants (built on the host)
    double k, w, seed_z, G, invG, r, A0, hop_len;      // hop_len: 0.1 * rate, for the first guess of a sample's hop
    LoudParams lp;          // b, na, rate, gate_len, abs_thr, peak_limit (its P is loudness.h's own and not used here)
    double P[LEVEL_LOG_T][16];      // M^(R 2^k), row-major
    double pad2;
};
static_assert(sizeof(LevelHeader) == 2864 && sizeof(LevelHeader) % 16 == 0 && offsetof(LevelHeader, K) == 52, "state header (level.py reads K and the knots)");

LOUD_HD size_t level_knots_off() { return sizeof(LevelHeader); }
LOUD_HD size_t level_sums_off(int cap_hops) { return level_knots_off() + loud_align16((size_t)(cap_hops + 2) * sizeof(double)); }
LOUD_HD size_t level_blocks_off(int cap_hops) { return level_sums_off(cap_hops) + loud_align16((size_t)cap_hops * sizeof(double)); }
LOUD_HD size_t level_ring_off(int cap_hops, int cap_blocks) { return level_blocks_off(cap_hops) + loud_align16((size_t)cap_blocks * sizeof(double)); }
LOUD_HD size_t level_state_bytes(int cap_hops, int cap_blocks, int ring) {
    return level_ring_off(cap_hops, cap_blocks) + loud_align16((size_t)ring * sizeof(float));
}

// knot h of the grid: the lower bound of loud_block_bounds, every expression in fp64 in this order
LOUD_HD long long level_knot(long long h, double rate) {
    const double Tg = 0.4, step = 0.25;
    const double a = (double)h * step;          // exact
    return (long long)(Tg * a * rate);
}

// v[0] <- the sum of v[0, LEVEL_T) by halving: the order both sides take
LOUD_HD void level_tree_host(double* v) {
    for (int d = LEVEL_T / 2; d >= 1; d >>= 1)
        for (int i = 0; i < d; ++i) v[i] += v[i + d];
}

// Where run t of a span starts.  The scan multiplies a left neighbour's state by M^(R 2^k): the length of the runs t - 2^k + 1 .. t,
// right as long as each of them has R samples.  Run 0 is never among them (it has no left neighbour), so it is the one that takes
// what is left over: `first` samples, 1 .. R.
LOUD_HD int level_run_off(int t, int first, int R) { return t == 0 ? 0 : first + (t - 1) * R; }

// block j from its four hop sums
LOUD_HD double level_block(const double* S, int j, double gate_len) { return (((S[j] + S[j + 1]) + S[j + 2]) + S[j + 3]) / gate_len; }

// the gain at the next knot from the gain at this one, the running measure and the running peak: desired gain, the clamp to
// [1 / G, G], the peak limit, the slew
LOUD_HD double level_next_gain(const LevelHeader& c, double A, int kept, double zbar, uint32_t peak_bits) {
    double d = 1.0;
    const double wk = c.w + (double)kept;
    if (wk > 0.0) {
        const double z_eff = fma(c.w, c.seed_z, (double)kept * zbar) / wk;
        d = sqrt(c.k / z_eff);
    }
    d = d < c.invG ? c.invG : d;
    d = d > c.G ? c.G : d;
    if (peak_bits) {
        const double lim = (double)c.lp.peak_limit / (double)loud_from_bits(peak_bits);
        d = lim < d ? lim : d;
    }
    const double lo = A / c.r, hi = A * c.r;
    d = d < lo ? lo : d;
    d = d > hi ? hi : d;
    return d;
}

// the gain of sample s of the stream: linear between the knots around it, the last knot's gain behind it
LOUD_HD float level_gain_at(long long s, int K, const double* A, double rate, double hop_len) {
    if (s >= level_knot(K, rate)) return (float)A[K];
    long long h = (long long)((double)s / hop_len);
    if (h > K - 1) h = K - 1;
    while (level_knot(h + 1, rate) <= s) ++h;
    while (level_knot(h, rate) > s) --h;
    const long long lo = level_knot(h, rate), hi = level_knot(h + 1, rate);
    const double frac = (double)(s - lo) / (double)(hi - lo);
    return (float)fma(A[h + 1] - A[h], frac, A[h]);
}

// one sample: the fp32 product, +-peak_limit beyond the limit (counted); a NaN stays a NaN
LOUD_HD float level_apply(float x, float a, float peak_limit, int* clamped) {
    float y = x * a;
    if (y > peak_limit) { y = peak_limit; ++*clamped; }
    else if (y < -peak_limit) { y = -peak_limit; ++*clamped; }
    return y;
}

// the moving part as init leaves it: what a push finds after a flush
LOUD_HD void level_restart(LevelHeader& h) {
    h.ended = 0;
    h.n_in = 0; h.clamped = 0;
    h.hops = 0; h.K = 1;
    h.flags = 0; h.blocks = 0; h.above = 0; h.kept = 0;
    h.peak_bits = 0;
    h.zbar = 0.0;
    for (int i = 0; i < 4; ++i) h.filt.s[i] = 0.0;
}

LOUD_HD LevelRecord level_record(const LevelHeader& h, float g0, float g1) {
    LevelRecord r;
    r.zbar = h.zbar; r.gain_first = g0; r.gain_last = g1; r.clamped = h.clamped;
    r.blocks = h.blocks; r.above_abs = h.above; r.kept = h.kept;
    r.flags = h.flags | (h.kept > 0 ? LEVEL_MEASURED : 0);
    return r;
}

// ------------------------------------------------------------------------------------------------------------------
// host only: the constants, a fresh state, the serial twin
// ------------------------------------------------------------------------------------------------------------------
inline int level_cap_blocks(int rate, int max_seconds) { return loud_blocks(max_seconds * rate, (double)rate); }
inline int level_ring_len(int rate) { return ((int)(0.1 * (double)rate) + 2 + 3) & ~3; }
inline int level_run_len(int rate) {
    const int r = ((int)(0.1 * (double)rate) + 1 + LEVEL_T - 1) / LEVEL_T;
    return r < 1 ? 1 : r > LEVEL_R_MAX ? LEVEL_R_MAX : r;
}

inline bool level_rate_ok(int rate, int max_seconds) {
    return rate >= LEVEL_MIN_RATE && rate <= LEVEL_MAX_RATE && max_seconds >= 1 && max_seconds <= LEVEL_MAX_SECONDS;
}

// seed_lufs NaN: no seed
inline bool level_config_ok(double target, double seed_lufs, double seed_blocks, double slew_db_s, double max_gain_db, float peak_limit) {
    return std::isfinite(target) && !std::isinf(seed_lufs) && std::isfinite(seed_blocks) && seed_blocks > 0.0 &&
           std::isfinite(slew_db_s) && slew_db_s >= 0.0 && std::isfinite(max_gain_db) && max_gain_db >= 0.0 && peak_limit > 0.f;
}

// a fresh state in host memory (`state` holds level_state_bytes): header with every constant, A_0 and A_1, zeros behind
inline void level_init_host(unsigned char* state, int rate, double target, double seed_lufs, double seed_blocks, double slew_db_s,
                            double max_gain_db, float peak_limit, int max_seconds) {
    const int cap_blocks = level_cap_blocks(rate, max_seconds), cap_hops = cap_blocks + 3, ring = level_ring_len(rate);
    memset(state, 0, level_state_bytes(cap_hops, cap_blocks, ring));
    LevelHeader h;
    memset(&h, 0, sizeof h);
    h.magic = LEVEL_MAGIC; h.rate = rate; h.cap_hops = cap_hops; h.cap_blocks = cap_blocks; h.ring = ring; h.R = level_run_len(rate);
    level_restart(h);
    h.lp = loud_params(rate, peak_limit);
    const bool seeded = seed_lufs == seed_lufs;
    h.k = pow(10.0, (target + 0.691) / 10.0);
    h.w = seeded ? seed_blocks : 0.0;
    h.seed_z = seeded ? pow(10.0, (seed_lufs + 0.691) / 10.0) : 0.0;
    h.G = pow(10.0, max_gain_db / 20.0);
    h.invG = 1.0 / h.G;
    h.r = pow(10.0, slew_db_s * 0.1 / 20.0);
    h.hop_len = 0.1 * (double)rate;
    double A0 = 1.0;
    if (seeded) {
        A0 = sqrt(h.k / h.seed_z);
        A0 = A0 < h.invG ? h.invG : A0;
        A0 = A0 > h.G ? h.G : A0;
    }
    h.A0 = A0;
    // M: column i is one step with x = 0 from the unit state e_i; P_0 = M^R, P_k = P_(k-1)^2
    double M[16], A[16], B[16];
    for (int i = 0; i < 4; ++i) {
        LoudState s = {{0, 0, 0, 0}};
        s.s[i] = 1.0;
        loud_step(h.lp, s, 0.0);
        for (int r = 0; r < 4; ++r) M[4 * r + i] = s.s[r];
    }
    memcpy(A, M, sizeof A);
    for (int i = 1; i < h.R; ++i) {
        loud_matmul4(A, M, B);
        memcpy(A, B, sizeof A);
    }
    for (int k = 0; k < LEVEL_LOG_T; ++k) {
        memcpy(h.P[k], A, sizeof A);
        loud_matmul4(A, A, B);
        memcpy(A, B, sizeof A);
    }
    memcpy(state, &h, sizeof h);
    double* knots = reinterpret_cast<double*>(state + level_knots_off());
    knots[0] = A0;
    knots[1] = level_next_gain(h, A0, 0, 0.0, 0);      // decided from no hop at all
}

// hop [lo, hi) of the stream as the measure block walks it: false (nothing changed) when it holds a NaN or an infinity, else
// the state behind it, its sum of y^2 and its peak bits.  X maps a stream index to its sample.
template <typename X>
inline bool level_hop_host(const LevelHeader& h, const X& x, long long lo, long long hi, LoudState* carry, double* S, uint32_t* peak_bits) {
    static thread_local LoudState st[LEVEL_T], nx[LEVEL_T];
    static thread_local double acc[LEVEL_T];
    uint32_t pk = 0;
    for (long long s = lo; s < hi; ++s) {
        const uint32_t a = loud_abs_bits(x(s));
        pk = a > pk ? a : pk;
    }
    if (pk >= 0x7F800000u) return false;
    const int R = h.R, span = LEVEL_T * R;
    LoudState c = *carry;
    for (int t = 0; t < LEVEL_T; ++t) acc[t] = 0.0;
    for (long long s0 = lo; s0 < hi; s0 += span) {
        const int cnt = hi - s0 < span ? (int)(hi - s0) : span;
        const int t_last = (cnt + R - 1) / R - 1, first = cnt - t_last * R;        // run 0 has `first` samples, every other run R
        for (int t = 0; t < LEVEL_T; ++t) {
            LoudState s = {{0, 0, 0, 0}};
            if (t == 0) s = c;
            const int off = level_run_off(t, first, R), len = t > t_last ? 0 : t == 0 ? first : R;
            for (int i = 0; i < len; ++i) loud_step(h.lp, s, (double)x(s0 + off + i));
            st[t] = s;
        }
        for (int k = 0; k < LEVEL_LOG_T; ++k) {
            const int d = 1 << k;
            for (int t = 0; t < LEVEL_T; ++t) nx[t] = t >= d ? loud_combine(h.P[k], st[t - d], st[t]) : st[t];
            memcpy(st, nx, sizeof st);
        }
        for (int t = 0; t <= t_last; ++t) {
            LoudState s = t == 0 ? c : st[t - 1];
            const int off = level_run_off(t, first, R), len = t == 0 ? first : R;
            for (int i = 0; i < len; ++i) {
                const double y = loud_step(h.lp, s, (double)x(s0 + off + i));
                acc[t] = fma(y, y, acc[t]);
            }
        }
        c = st[t_last];
    }
    level_tree_host(acc);
    *carry = c;
    *S = acc[0];
    *peak_bits = pk;
    return true;
}

// both gates over the blocks [0, nb): what the measure block does before every knot
inline void level_gates_host(const LevelHeader& h, const double* z, int nb, int* above, int* kept, double* zbar) {
    static thread_local double v[LEVEL_T];
    *above = 0; *kept = 0; *zbar = 0.0;
    for (int lane = 0; lane < LEVEL_T; ++lane) {
        double a = 0.0;
        for (int j = lane; j < nb; j += LEVEL_T)
            if (loud_keep_abs(z[j], h.lp.abs_thr)) { a += z[j]; ++*above; }
        v[lane] = a;
    }
    level_tree_host(v);
    if (*above == 0) return;
    const double rel = 0.1 * (v[0] / (double)*above);
    for (int lane = 0; lane < LEVEL_T; ++lane) {
        double a = 0.0;
        for (int j = lane; j < nb; j += LEVEL_T)
            if (loud_keep_both(z[j], h.lp.abs_thr, rel)) { a += z[j]; ++*kept; }
        v[lane] = a;
    }
    level_tree_host(v);
    if (*kept > 0) *zbar = v[0] / (double)*kept;
}

// one push over host memory: the serial twin of the two launches.  out may be chunk.
inline void level_push_host(unsigned char* state, const float* chunk, long long n, bool flush, float* out, LevelRecord* rec) {
    LevelHeader h;
    memcpy(&h, state, sizeof h);
    double* knots = reinterpret_cast<double*>(state + level_knots_off());
    double* S = reinterpret_cast<double*>(state + level_sums_off(h.cap_hops));
    double* z = reinterpret_cast<double*>(state + level_blocks_off(h.cap_hops));
    float* ring = reinterpret_cast<float*>(state + level_ring_off(h.cap_hops, h.cap_blocks));
    if (h.ended) level_restart(h);
    const long long N0 = h.n_in, N1 = N0 + n;
    const int C = h.ring;
    const double rate = h.lp.rate;
    auto x = [=](long long s) { return s >= N0 ? chunk[s - N0] : ring[s % C]; };
    while (!(h.flags & (LEVEL_NONFINITE | LEVEL_FULL))) {
        const long long lo = level_knot(h.hops, rate), hi = level_knot(h.hops + 1, rate);
        if (hi > N1) break;
        double sum;
        uint32_t pk;
        if (!level_hop_host(h, x, lo, hi, &h.filt, &sum, &pk)) {
            h.flags |= LEVEL_NONFINITE;
            break;
        }
        S[h.hops] = sum;
        h.peak_bits = pk > h.peak_bits ? pk : h.peak_bits;
        const int hops = ++h.hops;
        if (hops >= 4) z[hops - 4] = level_block(S, hops - 4, h.lp.gate_len);
        h.blocks = hops >= 4 ? hops - 3 : 0;
        level_gates_host(h, z, h.blocks, &h.above, &h.kept, &h.zbar);
        knots[hops + 1] = level_next_gain(h, knots[hops], h.kept, h.zbar, h.peak_bits);
        h.K = hops + 1;
        if (hops == h.cap_hops) h.flags |= LEVEL_FULL;
    }
    const float g0 = level_gain_at(N0, h.K, knots, rate, h.hop_len);
    const float g1 = n > 0 ? level_gain_at(N1 - 1, h.K, knots, rate, h.hop_len) : g0;
    int clamped = 0;
    for (long long i = 0; i < n; ++i) {
        const float xi = chunk[i];
        ring[(N0 + i) % C] = xi;        // all but the newest `ring` samples are overwritten again: the ring holds the newest
        out[i] = level_apply(xi, level_gain_at(N0 + i, h.K, knots, rate, h.hop_len), h.lp.peak_limit, &clamped);
    }
    h.n_in = N1;
    h.clamped += clamped;
    h.ended = flush ? 1 : 0;
    *rec = level_record(h, g0, g1);
    memcpy(state, &h, sizeof h);
}

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------------------------------
// the device kernels
// ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ long long level_len_dev(const int32_t* __restrict__ n_dev, int n_cap) {
    if (!n_dev) return n_cap;
    const int v = *n_dev;
    return v < 0 ? 0 : v > n_cap ? n_cap : v;
}

// the sum of the block's LEVEL_T values in level_tree_host's order; every thread calls, every thread gets the sum
// The steps that pair values of different waves go through LDS; from 64 values on the pairs lie inside wave 0, which adds them
// by shuffles -- the same pairs in the same order, without a barrier.
__device__ __forceinline__ double level_tree_dev(double* red, double v, int tid) {
    red[tid] = v;
    for (int d = LEVEL_T / 2; d >= 128; d >>= 1) {
        __syncthreads();
        if (tid < d) red[tid] += red[tid + d];
    }
    __syncthreads();
    if (tid < 64) {
        double r = red[tid] + red[tid + 64];
        for (int d = 32; d >= 1; d >>= 1) r += __shfl_down(r, d, 64);
        if (tid == 0) red[0] = r;
    }
    __syncthreads();
    const double r = red[0];
    __syncthreads();
    return r;
}

// Launch 1, one block: every hop that the ring plus this push completes is filtered and summed, and behind each the gates run
// over the block history and the next knot is decided; then the push's samples go into the ring, the header and rec are written.
// The moving part of the header lives in LDS while the block runs; thread 0 alone changes it, between barriers.
static __global__ __launch_bounds__(LEVEL_T) void level_measure_kernel(unsigned char* __restrict__ state, const float* __restrict__ chunk,
                                                                       int n_cap, const int32_t* __restrict__ n_dev, int flush,
                                                                       LevelRecord* __restrict__ rec) {
    __shared__ float xs[LEVEL_T * (LEVEL_R_MAX + 1)];
    __shared__ double st[4][LEVEL_T];
    __shared__ double red[LEVEL_T];
    __shared__ long long run_n_in, run_clamped;
    __shared__ int run_hops, run_K, run_flags, run_blocks, run_above, run_kept;
    __shared__ uint32_t run_peak, peak_s;
    __shared__ double run_zbar, run_filt[4];
    __shared__ int cnt_s[2];
    __shared__ double znew_s;
    __shared__ double Ps[LEVEL_LOG_T][16];
    LevelHeader* __restrict__ hd = reinterpret_cast<LevelHeader*>(state);
    const int tid = threadIdx.x;
    if (hd->magic != LEVEL_MAGIC) {         // not a state gsv_level_init made: nothing is read through it
        if (tid == 0) {
            LevelRecord r;
            r.zbar = 0.0; r.gain_first = 1.f; r.gain_last = 1.f; r.clamped = 0; r.blocks = 0; r.above_abs = 0; r.kept = 0; r.flags = -1;
            *rec = r;
        }
        return;
    }
    const int cap_hops = hd->cap_hops, C = hd->ring, R = hd->R;
    // the constants of the walk, read once: the filter's coefficients and the gate constants into registers, the scan's matrices
    // into LDS -- the state they come from is written further down, so the compiler would fetch them again behind every barrier
    LoudParams lp;
    for (int i = 0; i < 2; ++i) {
        for (int j = 0; j < 3; ++j) lp.b[i][j] = hd->lp.b[i][j];
        for (int j = 0; j < 2; ++j) lp.na[i][j] = hd->lp.na[i][j];
    }
    lp.rate = hd->lp.rate; lp.gate_len = hd->lp.gate_len; lp.abs_thr = hd->lp.abs_thr;
    for (int i = tid; i < LEVEL_LOG_T * 16; i += LEVEL_T) Ps[i / 16][i % 16] = hd->P[i / 16][i % 16];
    const double rate = lp.rate;
    double* __restrict__ knots = reinterpret_cast<double*>(state + level_knots_off());
    double* __restrict__ S = reinterpret_cast<double*>(state + level_sums_off(cap_hops));
    double* __restrict__ z = reinterpret_cast<double*>(state + level_blocks_off(cap_hops));
    float* __restrict__ ring = reinterpret_cast<float*>(state + level_ring_off(cap_hops, hd->cap_blocks));
    if (tid == 0) {
        const bool fresh = hd->ended != 0;
        run_n_in = fresh ? 0 : hd->n_in; run_clamped = fresh ? 0 : hd->clamped;
        run_hops = fresh ? 0 : hd->hops; run_K = fresh ? 1 : hd->K;
        run_flags = fresh ? 0 : hd->flags; run_blocks = fresh ? 0 : hd->blocks; run_above = fresh ? 0 : hd->above; run_kept = fresh ? 0 : hd->kept;
        run_peak = fresh ? 0u : hd->peak_bits;
        run_zbar = fresh ? 0.0 : hd->zbar;
        for (int i = 0; i < 4; ++i) run_filt[i] = fresh ? 0.0 : hd->filt.s[i];
    }
    __syncthreads();
    const long long n = level_len_dev(n_dev, n_cap);
    const long long N0 = run_n_in, N1 = N0 + n;
    const int span = LEVEL_T * R;
    int hops = run_hops;
    bool frozen = (run_flags & (LEVEL_NONFINITE | LEVEL_FULL)) != 0;
    LoudState carry;
    for (int i = 0; i < 4; ++i) carry.s[i] = run_filt[i];
    // what the walk would otherwise fetch from memory hop after hop: the last three hop sums and the newest knot (thread 0), and
    // block `tid` of the history (every thread; a history past LEVEL_T blocks reads the rest from memory)
    double s1 = 0.0, s2 = 0.0, s3 = 0.0, A_cur = 0.0;
    LevelHeader gc;                 // the constants of level_next_gain, read once
    gc.w = hd->w; gc.seed_z = hd->seed_z; gc.k = hd->k; gc.G = hd->G; gc.invG = hd->invG; gc.r = hd->r;
    gc.lp.peak_limit = hd->lp.peak_limit;
    if (tid == 0) {
        if (hops >= 3) s1 = S[hops - 3];
        if (hops >= 2) s2 = S[hops - 2];
        if (hops >= 1) s3 = S[hops - 1];
        A_cur = knots[run_K];
    }
    double z0 = tid < run_blocks ? z[tid] : 0.0;
    while (!frozen) {
        const long long lo = level_knot(hops, rate), hi = level_knot(hops + 1, rate);
        if (hi > N1) break;                 // block-uniform, as every branch around a barrier below
        if (tid == 0) peak_s = 0;
        const int ring_lo = (int)(lo % C);
        LoudState c = carry;
        double acc = 0.0;
        bool bad = false;
        for (long long s0 = lo; s0 < hi; s0 += span) {
            const int cnt = hi - s0 < span ? (int)(hi - s0) : span;
            __syncthreads();                // xs and st are free; peak_s is cleared
            uint32_t pk = 0;
            const int t_last = (cnt + R - 1) / R - 1, first = cnt - t_last * R;
            float v[LEVEL_R_MAX];           // every load of the thread is under way before the first is used
#pragma unroll
            for (int m = 0; m < LEVEL_R_MAX; ++m) {
                const int k = tid + m * LEVEL_T;
                v[m] = 0.f;
                if (k < cnt) {
                    const long long sk = s0 + k;
                    const int at = ring_lo + (int)(sk - lo);        // sk mod C for a sample of this hop: at < 2 C
                    v[m] = sk >= N0 ? chunk[sk - N0] : ring[at >= C ? at - C : at];
                }
            }
#pragma unroll
            for (int m = 0; m < LEVEL_R_MAX; ++m) {
                const int k = tid + m * LEVEL_T;
                if (k < cnt) {
                    const uint32_t a = loud_abs_bits(v[m]);
                    pk = a > pk ? a : pk;
                    xs[k < first ? k : (1 + (k - first) / R) * (R + 1) + (k - first) % R] = v[m];     // run t lies at xs + t (R + 1)
                }
            }
            atomicMax(&peak_s, pk);
            __syncthreads();
            if (peak_s >= 0x7F800000u) { bad = true; break; }
            const float* mine = xs + tid * (R + 1);
            const int len = tid > t_last ? 0 : tid == 0 ? first : R;
            LoudState s = {{0, 0, 0, 0}};
            if (tid == 0) s = c;
            for (int i = 0; i < len; ++i) loud_step(lp, s, (double)mine[i]);
            for (int k = 0; k < LEVEL_LOG_T; ++k) {
                const int d = 1 << k;
                for (int i = 0; i < 4; ++i) st[i][tid] = s.s[i];
                __syncthreads();
                if (tid >= d) {
                    LoudState l;
                    for (int i = 0; i < 4; ++i) l.s[i] = st[i][tid - d];
                    s = loud_combine(Ps[k], l, s);
                }
                __syncthreads();
            }
            for (int i = 0; i < 4; ++i) st[i][tid] = s.s[i];
            __syncthreads();
            LoudState start = c;
            if (tid > 0)
                for (int i = 0; i < 4; ++i) start.s[i] = st[i][tid - 1];
            for (int i = 0; i < 4; ++i) c.s[i] = st[i][t_last];
            for (int i = 0; i < len; ++i) {
                const double y = loud_step(lp, start, (double)mine[i]);
                acc = fma(y, y, acc);
            }
        }
        if (bad) {
            if (tid == 0) run_flags |= LEVEL_NONFINITE;
            break;
        }
        const double sum = level_tree_dev(red, acc, tid);
        carry = c;
        ++hops;
        const int nb = hops >= 4 ? hops - 3 : 0;
        if (tid == 0) {
            S[hops - 1] = sum;
            run_peak = peak_s > run_peak ? peak_s : run_peak;
            if (hops >= 4) {
                const double four[4] = {s1, s2, s3, sum};
                znew_s = level_block(four, 0, lp.gate_len);
                z[hops - 4] = znew_s;
            }
            s1 = s2; s2 = s3; s3 = sum;
            cnt_s[0] = 0; cnt_s[1] = 0;
        }
        __syncthreads();                    // the new block is visible to the block's threads
        if (nb > 0 && tid == nb - 1) z0 = znew_s;
        double a = 0.0;
        int cn = 0;
        for (int j = tid; j < nb; j += LEVEL_T) {
            const double v = j < LEVEL_T ? z0 : z[j];
            if (loud_keep_abs(v, lp.abs_thr)) { a += v; ++cn; }
        }
        if (cn) atomicAdd(&cnt_s[0], cn);
        const double sum_a = level_tree_dev(red, a, tid);
        const int above = cnt_s[0];
        double zbar = 0.0;
        if (above > 0) {
            const double rel = 0.1 * (sum_a / (double)above);
            a = 0.0; cn = 0;
            for (int j = tid; j < nb; j += LEVEL_T) {
                const double v = j < LEVEL_T ? z0 : z[j];
                if (loud_keep_both(v, lp.abs_thr, rel)) { a += v; ++cn; }
            }
            if (cn) atomicAdd(&cnt_s[1], cn);
            const double sum_k = level_tree_dev(red, a, tid);
            if (cnt_s[1] > 0) zbar = sum_k / (double)cnt_s[1];
        }
        if (tid == 0) {
            run_hops = hops; run_blocks = nb; run_above = above; run_kept = cnt_s[1]; run_zbar = zbar;
            A_cur = level_next_gain(gc, A_cur, cnt_s[1], zbar, run_peak);
            knots[hops + 1] = A_cur;
            run_K = hops + 1;
            if (hops == cap_hops) run_flags |= LEVEL_FULL;
        }
        frozen = hops == cap_hops;
        __syncthreads();                    // cnt_s and peak_s have been read before the next hop clears them
    }
    __syncthreads();                        // every read of the ring lies before this
    for (long long i = (n > C ? n - C : 0) + tid; i < n; i += LEVEL_T) ring[(N0 + i) % C] = chunk[i];
    if (tid == 0) {
        hd->ended = flush ? 1 : 0;
        hd->n_in = N1; hd->clamped = run_clamped;
        hd->hops = run_hops; hd->K = run_K;
        hd->flags = run_flags; hd->blocks = run_blocks; hd->above = run_above; hd->kept = run_kept;
        hd->peak_bits = run_peak;
        hd->zbar = run_zbar;
        for (int i = 0; i < 4; ++i) hd->filt.s[i] = carry.s[i];
        const float g0 = level_gain_at(N0, run_K, knots, rate, hd->hop_len);
        const float g1 = n > 0 ? level_gain_at(N1 - 1, run_K, knots, rate, hd->hop_len) : g0;
        LevelRecord r;
        r.zbar = run_zbar; r.gain_first = g0; r.gain_last = g1; r.clamped = run_clamped;
        r.blocks = run_blocks; r.above_abs = run_above; r.kept = run_kept;
        r.flags = run_flags | (run_kept > 0 ? LEVEL_MEASURED : 0);
        *rec = r;
    }
}

// Launch 2: out = chunk * gain, sample by sample from the knots the first launch left, grid-stride; the samples set to
// +-peak_limit are counted into the header and the record (integer sums: their order does not show).  out may be chunk.
static __global__ __launch_bounds__(LEVEL_APPLY_T) void level_apply_kernel(unsigned char* state, const float* chunk, int n_cap,
                                                                           const int32_t* __restrict__ n_dev, float* out,
                                                                           LevelRecord* rec) {
    __shared__ int cnt_s;
    LevelHeader* hd = reinterpret_cast<LevelHeader*>(state);
    if (hd->magic != LEVEL_MAGIC) return;
    const double* __restrict__ knots = reinterpret_cast<const double*>(state + level_knots_off());
    const long long n = level_len_dev(n_dev, n_cap);
    const long long N0 = hd->n_in - n;
    const int K = hd->K;
    const double rate = hd->lp.rate, hop_len = hd->hop_len;
    const float peak_limit = hd->lp.peak_limit;
    if (threadIdx.x == 0) cnt_s = 0;
    __syncthreads();
    int clamped = 0;
    for (long long i = (long long)blockIdx.x * LEVEL_APPLY_T + threadIdx.x; i < n; i += (long long)gridDim.x * LEVEL_APPLY_T)
        out[i] = level_apply(chunk[i], level_gain_at(N0 + i, K, knots, rate, hop_len), peak_limit, &clamped);
    if (clamped) atomicAdd(&cnt_s, clamped);
    __syncthreads();
    if (threadIdx.x == 0 && cnt_s) {
        atomicAdd(reinterpret_cast<unsigned long long*>(&hd->clamped), (unsigned long long)cnt_s);
        atomicAdd(reinterpret_cast<unsigned long long*>(&rec->clamped), (unsigned long long)cnt_s);
    }
}
#endif

}  // namespace gsv
