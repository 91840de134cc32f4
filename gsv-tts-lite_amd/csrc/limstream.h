// limstream: the look-ahead limiter of limiter.h for a stream that arrives in pushes.  The output is stages 1 - 6
// of limiter.h applied to the whole stream as one clip, y[n] = g[n] x[n]: no trim, no clip-wide "under the ceiling: not touched",
// and one local rule instead -- a window whose L values of r are all exactly 1 gives g = 1 and the sample is copied.  y[n] is
// final once x[n + L + 5] has arrived (e reads x up to n + 6, h reads c up to n + L - 1), so the limiter delays the stream by
// D = L + 5 samples: after N samples max(0, N - D) outputs exist, and a flush emits the rest with zeros behind the end of x and
// c = 1 behind the end, as the clip has them.
//
// The emitted bytes never depend on how the stream was cut.  That fixes the rounding of the release: it is computed on LIM_TILE
// tiles aligned to the STREAM index with the operations of lim_hold_kernel, lim_chain_kernel and lim_attack_kernel -- the
// Hillis-Steele steps inside a tile (causal: v[n] reads h of its tile up to n only), one fmaf per chained tile from starts[0] = 1,
// one fmaf at the end.  A tile that a push leaves unfinished is redone from its h, kept in the state; nothing is continued by a
// serial recurrence.  So for a stream that is limited somewhere the output is fl(g x) with g the clip limiter's stage array, bit
// for bit (at a look-ahead with fl(L fl(1 / L)) == 1, which every default look-ahead is).
//
// A sample whose envelope is not finite needs gain 1 (c = 1) and is copied; the push's record says LIMS_NONFINITE, and such an
// envelope is kept out of the record's peaks.  Finite neighbours outside the FIR's reach are limited as usual.
//
// The scalar routines are limiter.h's (lim_gap, lim_need, lim_release, lim_attack, lim_min); what is new here -- the plan of a
// push, one chain step, the all-ones rule -- is one __host__ __device__ text for the kernels, for the host twin lims_push_host
// (gsv_limstream_push_host: the CPU path and the device's oracle) and for tools/limstream_host_check.cpp.
//
// The caller-owned state, every part 16-byte aligned:
//   [LimsHeader | LimParams | xhist fp32 [HX] | hopen fp32 [2][LIM_TILE] | rhist fp32 [2][L - 1] | ends fp32 [LIMS_MAX_TILES]]
//   xhist  a ring, sample s of the stream at xhist[s % HX], HX = L + 11: an output that is still owed reads x no further back than
//          D + 6 samples behind the newest (its own sample D behind, the envelope's taps 6 more).  The c values the hold still
//          needs are not kept: they are recomputed from these samples by the same lim_gap, so they are the same bits.
//   hopen  h of the open tile's samples that were emitted, [parity] the valid copy
//   rhist  r of the last L - 1 emitted samples, slot j sample E - (L - 1) + j (E the samples emitted; a slot of a sample before
//          the stream's start is never read: the reader clamps the index to 0 first, as the clip does); [parity] the valid copy
//   ends   v at the last sample of every tile this push completes: scratch between the launches of one push
// The header holds the chain's start for the open tile.  The two copies let the kernels of a push read the old one while they
// write the new one; the last launch turns `parity` over.  A push of more than LIMS_MAX_CHUNK samples is refused: `ends` is sized
// for it (callers cut longer input into several pushes, which changes no byte).
#pragma once
#include "limiter.h"

namespace gsv {

constexpr int32_t LIMS_MAGIC = 0x534D4C47;          // "GLMS"
constexpr int LIMS_MAX_CHUNK = 1 << 20;             // samples of one push
constexpr int LIMS_MAX_TILES = (LIMS_MAX_CHUNK + LIM_MAX_L + 5) / LIM_TILE + 2;
constexpr int LIMS_LIMITED = 1, LIMS_LIMITED_EVER = 2, LIMS_NONFINITE = 4;      // record flags
constexpr int LIMS_SPAN = LIM_TILE + LIM_MAX_L - 1; // the most samples of c behind a tile's hold
constexpr int LIMS_C_PER_THREAD = (LIMS_SPAN + LIM_TILE - 1) / LIM_TILE;

struct LimsHeader {
    long long n_in, n_out;          // samples pushed / emitted since the last flush
    float T, start;                 // the ceiling, linear; starts[] of the open tile
    uint32_t peak_run;              // bits of the largest finite e among the emitted samples of the stream
    int32_t ever;                   // the limiter has acted on this stream
    uint32_t acc_peak, acc_min;     // this push: max e / min g over the emitted samples as bits; reset by the last launch
    int32_t acc_flags;
    int32_t parity;
    int32_t L, R, magic, pad;
};
static_assert(sizeof(LimsHeader) == 64, "state header");

struct LimsRecord {                 // gsv_limstream_record
    int32_t emitted;                // samples this push wrote to `out`: the next stage's n_dev
    int16_t flags, lookahead;
    float peak_in;                  // max finite e over the emitted samples of this push (0 for none)
    float peak_run;                 // ... of the stream so far
    float min_gain;                 // min g over the emitted samples of this push (1 for none)
    int32_t release;
    long long total;                // samples emitted so far (this push included; a flush reports the stream's length)
};
static_assert(sizeof(LimsRecord) == 32, "record");

LIM_HD int lims_delay(int L) { return L + 5; }
LIM_HD int lims_hx(int L) { return L + 11; }
LIM_HD size_t lims_params_off() { return sizeof(LimsHeader); }
LIM_HD size_t lims_a16(size_t v) { return (v + 15) & ~(size_t)15; }
LIM_HD size_t lims_xhist_off() { return lims_params_off() + lims_a16(sizeof(LimParams)); }
LIM_HD size_t lims_hopen_off(int L) { return lims_xhist_off() + lims_a16((size_t)lims_hx(L) * sizeof(float)); }
LIM_HD size_t lims_rstride(int L) { return lims_a16((size_t)(L - 1) * sizeof(float)) / sizeof(float); }
LIM_HD size_t lims_rhist_off(int L) { return lims_hopen_off(L) + 2 * (size_t)LIM_TILE * sizeof(float); }
LIM_HD size_t lims_ends_off(int L) { return lims_rhist_off(L) + 2 * lims_rstride(L) * sizeof(float); }
LIM_HD size_t lims_state_bytes(int L) { return lims_ends_off(L) + lims_a16((size_t)LIMS_MAX_TILES * sizeof(float)); }

struct LimsPlan {
    long long N0, E0, N1, E1;       // samples in / emitted before and after this push
    long long t0, nt;               // the first tile that holds an emitted sample of this push; how many do
};

LIM_HD LimsPlan lims_plan(const LimsHeader& h, long long n, bool flush) {
    LimsPlan p;
    const int D = lims_delay(h.L);
    p.N0 = h.n_in; p.E0 = h.n_out;
    p.N1 = p.N0 + n;
    p.E1 = flush ? p.N1 : (p.N1 > D ? p.N1 - D : 0);
    p.t0 = p.E0 / LIM_TILE;
    p.nt = p.E1 > p.E0 ? (p.E1 - 1) / LIM_TILE - p.t0 + 1 : 0;
    return p;
}

// one step of lim_chain: starts of the next tile from this tile's last v
LIM_HD float lims_chain_step(const LimParams& p, float end, float start) { return lim_min(end, fmaf((float)LIM_TILE, p.s, start)); }

// e of a sample from the staged samples: w[0] is the sample six before it, w[12] the one six behind
LIM_HD uint32_t lims_env(const LimParams& p, const float* w) {
    return lim_umax(lim_abs_bits(w[6]), lim_umax(lim_gap(p, w), lim_gap(p, w + 1)));
}
LIM_HD bool lims_finite(uint32_t e) { return e < 0x7F800000u; }
LIM_HD float lims_need(uint32_t e, float T) { return lims_finite(e) ? lim_need(lim_from_bits(e), T) : 1.f; }

// stage 5 with the local rule: newest[-i] = r[n - i]
LIM_HD float lims_attack(const LimParams& p, float c, const float* newest) {
    bool ones = true;
    for (int i = 0; i < p.L; ++i) ones = ones && newest[-i] == 1.f;
    return ones ? 1.f : lim_attack(p, c, newest);
}

LIM_HD LimsRecord lims_record(const LimsHeader& h, const LimsPlan& pl, uint32_t peak_run, bool ever) {
    LimsRecord r;
    r.emitted = (int32_t)(pl.E1 - pl.E0);
    const bool limited = h.acc_min < 0x3F800000u;
    r.flags = (int16_t)((limited ? LIMS_LIMITED : 0) | (ever ? LIMS_LIMITED_EVER : 0) | (h.acc_flags & LIMS_NONFINITE));
    r.lookahead = (int16_t)h.L;
    r.peak_in = lim_from_bits(h.acc_peak);
    r.peak_run = lim_from_bits(peak_run);
    r.min_gain = lim_from_bits(h.acc_min);
    r.release = h.R;
    r.total = pl.E1;
    return r;
}

// ------------------------------------------------------------------------------------------------------------------
// host only
// ------------------------------------------------------------------------------------------------------------------
inline void lims_init_host(unsigned char* state, float ceiling_db, int L, int R) {
    const size_t bytes = lims_state_bytes(L);
    memset(state, 0, bytes);
    LimsHeader h;
    memset(&h, 0, sizeof h);
    h.T = (float)pow(10.0, (double)ceiling_db / 20.0);
    h.start = 1.f;
    h.acc_min = 0x3F800000u;
    h.L = L; h.R = R; h.magic = LIMS_MAGIC;
    memcpy(state, &h, sizeof h);
    const LimParams p = lim_params(L, R);
    memcpy(state + lims_params_off(), &p, sizeof p);
}

// the min-plus scan of one tile as lim_hold_kernel runs it: st holds h on entry and v on return
inline void lims_scan_tile_host(const LimParams& p, float* st) {
    float nx[LIM_TILE];
    for (int k = 0; k < LIM_LOG_TILE; ++k) {
        const int d = 1 << k;
        for (int t = 0; t < LIM_TILE; ++t) nx[t] = t >= d ? lim_min(st[t], st[t - d] + p.ds[k]) : st[t];
        memcpy(st, nx, sizeof nx);
    }
}

// one push over host memory: the serial twin of the three launches.  out holds n + D floats.
inline void lims_push_host(unsigned char* state, const float* chunk, long long n, bool flush, float* out, LimsRecord* rec) {
    LimsHeader h;
    memcpy(&h, state, sizeof h);
    LimParams p;
    memcpy(&p, state + lims_params_off(), sizeof p);
    const int L = h.L, HX = lims_hx(L);
    float* xhist = reinterpret_cast<float*>(state + lims_xhist_off());
    float* hopen = reinterpret_cast<float*>(state + lims_hopen_off(L));
    float* rhist = reinterpret_cast<float*>(state + lims_rhist_off(L));
    const size_t rstride = lims_rstride(L);
    const float* hold_old = hopen + (size_t)h.parity * LIM_TILE;
    float* hold_new = hopen + (size_t)(1 - h.parity) * LIM_TILE;
    const float* r_old = rhist + (size_t)h.parity * rstride;
    float* r_new = rhist + (size_t)(1 - h.parity) * rstride;
    const LimsPlan pl = lims_plan(h, n, flush);
    const long long N0 = pl.N0, N1 = pl.N1, E0 = pl.E0, E1 = pl.E1;
    auto X = [&](long long s) { return s < 0 || s >= N1 ? 0.f : s >= N0 ? chunk[s - N0] : xhist[s % HX]; };
    float start = h.start;
    uint32_t peak_run = h.peak_run;
    if (E1 > E0) {
        const long long m = E1 - E0;
        // stages 1 and 2 for [E0, E1 + L - 1): c = 1 behind the end
        float* c = new float[(size_t)(m + L - 1)];
        unsigned char* nf = new unsigned char[(size_t)m];
        float* r = new float[(size_t)(m + L - 1)];         // r of sample E0 - (L - 1) + k
        for (long long k = 0; k < m + L - 1; ++k) {
            const long long i = E0 + k;
            float w[13];
            for (int j = 0; j < 13; ++j) w[j] = X(i - 6 + j);
            const uint32_t e = i < N1 ? lims_env(p, w) : 0u;
            c[k] = i < N1 ? lims_need(e, h.T) : 1.f;
            if (k < m) {
                nf[k] = !lims_finite(e);
                if (nf[k]) h.acc_flags |= LIMS_NONFINITE;
                else h.acc_peak = lim_umax(h.acc_peak, e);
            }
        }
        for (int k = 0; k < L - 1; ++k) {
            long long s = E0 - (L - 1) + k;
            if (s < 0) s = 0;
            r[k] = s < E0 ? r_old[s - (E0 - (L - 1))] : 0.f;       // a sample of this push: filled below
        }
        // stages 3 and 4, tile by tile
        float st[LIM_TILE], hh[LIM_TILE];
        for (long long t = pl.t0; t < pl.t0 + pl.nt; ++t) {
            const long long lo = t * LIM_TILE;
            for (int q = 0; q < LIM_TILE; ++q) {
                const long long i = lo + q;
                float v = 1.f;
                if (i < E0) v = hold_old[q];
                else if (i < E1)
                    for (int k = 0; k < L; ++k) v = lim_min(v, c[i - E0 + k]);
                st[q] = hh[q] = v;
            }
            lims_scan_tile_host(p, st);
            for (int q = 0; q < LIM_TILE; ++q) {
                const long long i = lo + q;
                if (i >= E0 && i < E1) r[i - E0 + L - 1] = lim_release(p, st, &start, q);
            }
            if (lo + LIM_TILE <= E1) start = lims_chain_step(p, st[LIM_TILE - 1], start);
            else if (!flush)
                for (int q = 0; lo + q < E1; ++q) hold_new[q] = hh[q];
        }
        if (E0 == 0)
            for (int k = 0; k < L - 1; ++k) r[k] = r[L - 1];       // r[m < 0] = r[0]
        // stages 5 and 6
        for (long long k = 0; k < m; ++k) {
            const float g = nf[k] ? 1.f : lims_attack(p, c[k], r + k + L - 1);
            const float x = X(E0 + k);
            out[k] = g == 1.f ? x : g * x;
            if (g < lim_from_bits(h.acc_min)) h.acc_min = lim_abs_bits(g);
        }
        if (!flush)
            for (int j = 0; j < L - 1; ++j) {
                long long s = E1 - (L - 1) + j;
                if (s >= 0) r_new[j] = r[s - (E0 - (L - 1))];
            }
        delete[] c; delete[] nf; delete[] r;
        h.parity = 1 - h.parity;
    }
    for (long long i = n > HX ? n - HX : 0; i < n; ++i) xhist[(N0 + i) % HX] = chunk[i];
    peak_run = lim_umax(peak_run, h.acc_peak);
    const bool ever = h.ever || h.acc_min < 0x3F800000u;
    *rec = lims_record(h, pl, peak_run, ever);
    h.n_in = flush ? 0 : N1;
    h.n_out = flush ? 0 : E1;
    h.start = flush ? 1.f : start;
    h.peak_run = flush ? 0u : peak_run;
    h.ever = flush ? 0 : (int32_t)ever;
    h.acc_peak = 0; h.acc_min = 0x3F800000u; h.acc_flags = 0;
    memcpy(state, &h, sizeof h);
}

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------------------------------
// the device kernels
// ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ long long lims_len_dev(const int32_t* __restrict__ n_dev, int n_cap) {
    if (!n_dev) return n_cap;
    const int v = *n_dev;
    return v < 0 ? 0 : v > n_cap ? n_cap : v;
}

struct LimsView {       // what every kernel of a push reads first
    LimsHeader h;
    LimsPlan pl;
    const float* xhist;
    const float* chunk;
    int HX;
    __device__ __forceinline__ float X(long long s) const {
        return s < 0 || s >= pl.N1 ? 0.f : s >= pl.N0 ? chunk[s - pl.N0] : xhist[s % HX];
    }
};

// Stages 1 - 4 inside tile `t` of the stream for the samples [E0, E1) of it, by a block of LIM_TILE threads.  buf (LIMS_SPAN + 12
// floats) takes the samples behind the tile's c -- history ring, chunk, zeros behind the end -- and then c itself; sv (LIM_TILE)
// the scan.  A sample of the tile in front of E0 takes its h from the state, one behind E1 takes 1: the scan is causal, so no
// emitted sample reads it.  Returns this thread's v and leaves it in sv[tid], c of sample a + k in buf[k] (a the first emitted
// sample of the tile) and h in *h_out.  OWN: also the statistics of e and the non-finite marks of the tile's samples, nf[k].
template <bool OWN>
__device__ __forceinline__ float lims_tile(const LimsView& s, const LimParams& p, const float* __restrict__ hold_old, long long t,
                                           float* buf, float* sv, unsigned char* nf, float* h_out, uint32_t* peak, int* flags) {
    const int tid = threadIdx.x;
    const long long lo = t * LIM_TILE;
    const long long a = lo > s.pl.E0 ? lo : s.pl.E0;
    const long long b = lo + LIM_TILE < s.pl.E1 ? lo + LIM_TILE : s.pl.E1;
    const int own = (int)(b - a), span = own + p.L - 1;
    __syncthreads();                                    // whoever read buf and sv before has done so
    for (int k = tid; k < span + 12; k += LIM_TILE) buf[k] = s.X(a - 6 + k);
    __syncthreads();
    float ck[LIMS_C_PER_THREAD];
#pragma unroll
    for (int j = 0; j < LIMS_C_PER_THREAD; ++j) {
        const int k = tid + j * LIM_TILE;
        ck[j] = 1.f;
        if (k < span && a + k < s.pl.N1) {
            const uint32_t e = lims_env(p, buf + k);
            ck[j] = lims_need(e, s.h.T);
            if (OWN && k < own) {
                const bool bad = !lims_finite(e);
                nf[k] = bad;
                if (bad) *flags |= LIMS_NONFINITE;
                else *peak = lim_umax(*peak, e);
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < LIMS_C_PER_THREAD; ++j) {
        const int k = tid + j * LIM_TILE;
        if (k < span) buf[k] = ck[j];
    }
    __syncthreads();
    const long long i = lo + tid;
    float v = 1.f;
    if (i < s.pl.E0) v = hold_old[tid];
    else if (i < s.pl.E1)
        for (int k = 0; k < p.L; ++k) v = lim_min(v, buf[(int)(i - a) + k]);
    *h_out = v;
    for (int k = 0; k < LIM_LOG_TILE; ++k) {
        const int d = 1 << k;
        sv[tid] = v;
        __syncthreads();
        if (tid >= d) v = lim_min(v, sv[tid - d] + p.ds[k]);
        __syncthreads();
    }
    sv[tid] = v;
    __syncthreads();
    return v;
}

__device__ __forceinline__ bool lims_view(const unsigned char* __restrict__ state, const float* __restrict__ chunk, int n_cap,
                                          const int32_t* __restrict__ n_dev, int flush, LimsView* s) {
    s->h = *reinterpret_cast<const LimsHeader*>(state);
    if (s->h.magic != LIMS_MAGIC) return false;         // not a state gsv_limstream_init made: nothing is read through it
    s->pl = lims_plan(s->h, lims_len_dev(n_dev, n_cap), flush != 0);
    s->xhist = reinterpret_cast<const float*>(state + lims_xhist_off());
    s->chunk = chunk;
    s->HX = lims_hx(s->h.L);
    return true;
}

// Launch 1, one block per tile: v at the last sample of every tile the push completes -> ends; h of the tile it leaves open ->
// the other copy of hopen.
static __global__ __launch_bounds__(LIM_TILE) void lims_hold_kernel(unsigned char* __restrict__ state, const float* __restrict__ chunk,
                                                                    int n_cap, const int32_t* __restrict__ n_dev, int flush) {
    __shared__ float buf[LIMS_SPAN + 12];
    __shared__ float sv[LIM_TILE];
    LimsView s;
    if (!lims_view(state, chunk, n_cap, n_dev, flush, &s)) return;
    if ((long long)blockIdx.x >= s.pl.nt || blockIdx.x >= LIMS_MAX_TILES) return;     // block-uniform
    const LimParams p = *reinterpret_cast<const LimParams*>(state + lims_params_off());
    float* hopen = reinterpret_cast<float*>(state + lims_hopen_off(s.h.L));
    float* ends = reinterpret_cast<float*>(state + lims_ends_off(s.h.L));
    const long long t = s.pl.t0 + blockIdx.x, lo = t * LIM_TILE;
    float hh;
    const float v = lims_tile<false>(s, p, hopen + (size_t)s.h.parity * LIM_TILE, t, buf, sv, nullptr, &hh, nullptr, nullptr);
    const int tid = threadIdx.x;
    if (lo + LIM_TILE <= s.pl.E1) {
        if (tid == LIM_TILE - 1) ends[blockIdx.x] = v;
    } else if (!flush && lo + tid < s.pl.E1) {
        hopen[(size_t)(1 - s.h.parity) * LIM_TILE + tid] = hh;
    }
}

// Launch 2, one block per tile: the chain up to the tile (one thread, lim_chain's steps over `ends`), r of the L - 1 samples in
// front of the tile -- from rhist where they were emitted by an earlier push, else by redoing their tiles --, then stages 5 and 6
// and the statistics: one atomic per block on the bits of the peak and of the smallest gain.
static __global__ __launch_bounds__(LIM_TILE) void lims_attack_kernel(unsigned char* __restrict__ state, const float* __restrict__ chunk,
                                                                      int n_cap, const int32_t* __restrict__ n_dev, int flush,
                                                                      float* __restrict__ out) {
    __shared__ float buf[LIMS_SPAN + 12];
    __shared__ float sv[LIM_TILE];
    __shared__ float rs[LIMS_SPAN];                     // r of sample a - (L - 1) + k
    __shared__ unsigned char nf[LIM_TILE];
    __shared__ float st_s[LIM_MAX_L / LIM_TILE + 2];    // starts of the tiles q0 .. t
    __shared__ uint32_t peak_s, min_s;
    __shared__ int flags_s;
    LimsView s;
    if (!lims_view(state, chunk, n_cap, n_dev, flush, &s)) return;
    if ((long long)blockIdx.x >= s.pl.nt || blockIdx.x >= LIMS_MAX_TILES) return;     // block-uniform
    const LimParams p = *reinterpret_cast<const LimParams*>(state + lims_params_off());
    const int L = p.L, tid = threadIdx.x;
    const float* hold_old = reinterpret_cast<const float*>(state + lims_hopen_off(L)) + (size_t)s.h.parity * LIM_TILE;
    float* rhist = reinterpret_cast<float*>(state + lims_rhist_off(L));
    const float* r_old = rhist + (size_t)s.h.parity * lims_rstride(L);
    float* r_new = rhist + (size_t)(1 - s.h.parity) * lims_rstride(L);
    const float* ends = reinterpret_cast<const float*>(state + lims_ends_off(L));
    const long long E0 = s.pl.E0, E1 = s.pl.E1;
    const long long t = s.pl.t0 + blockIdx.x, lo = t * LIM_TILE;
    const long long a = lo > E0 ? lo : E0;
    const long long b = lo + LIM_TILE < E1 ? lo + LIM_TILE : E1;
    // the first tile whose r this block needs and has to make itself
    long long first = a - (L - 1);
    if (first < 0) first = 0;
    if (first < E0) first = E0;
    const long long q0 = first / LIM_TILE;              // t0 <= q0 <= t, t - q0 <= LIM_MAX_L / LIM_TILE
    if (tid == 0) {
        peak_s = 0; min_s = 0x3F800000u; flags_s = 0;
        float st = s.h.start;
        for (long long q = s.pl.t0; q <= t; ++q) {
            if (q >= q0) st_s[q - q0] = st;
            if (q < t) st = lims_chain_step(p, ends[q - s.pl.t0], st);
        }
    }
    // the samples in front of E0
    for (int k = tid; k < L - 1; k += LIM_TILE) {
        long long m = a - (L - 1) + k;
        if (m < 0) m = 0;
        if (m < E0) rs[k] = r_old[m - (E0 - (L - 1))];
    }
    uint32_t peak = 0;
    int flags = 0;
    float c = 1.f;
    for (long long q = q0; q <= t; ++q) {               // block-uniform
        float hh;
        if (q < t) lims_tile<false>(s, p, hold_old, q, buf, sv, nf, &hh, &peak, &flags);
        else lims_tile<true>(s, p, hold_old, q, buf, sv, nf, &hh, &peak, &flags);
        const long long i = q * LIM_TILE + tid;
        if (i >= E0 && i < b && i >= a - (L - 1)) rs[(int)(i - a) + L - 1] = lim_release(p, sv, &st_s[q - q0], tid);
        if (q == t && i >= a && i < b) c = buf[(int)(i - a)];
    }
    __syncthreads();
    if (E0 == 0 && a < L - 1) {                         // r[m < 0] = r[0], which this block has just made (block-uniform)
        const int k0 = (int)((L - 1) - a);              // the slot of sample 0
        const float r0 = rs[k0];
        __syncthreads();
        for (int k = tid; k < k0; k += LIM_TILE) rs[k] = r0;
        __syncthreads();
    }
    const long long i = lo + tid;
    float g = 1.f;
    if (i >= a && i < b) {
        const int k = (int)(i - a);
        if (!nf[k]) g = lims_attack(p, c, rs + k + L - 1);
        const float x = s.X(i);
        if (i - E0 < (long long)n_cap + lims_delay(L)) out[i - E0] = g == 1.f ? x : g * x;
        if (!flush && i >= E1 - (L - 1)) r_new[i - (E1 - (L - 1))] = rs[k + L - 1];
    }
    uint32_t gb = lim_abs_bits(g);
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)gb, d);
        gb = o < gb ? o : gb;
        peak = lim_umax(peak, (uint32_t)__shfl_xor((int)peak, d));
        flags |= __shfl_xor(flags, d);
    }
    if ((tid & 63) == 0) {
        atomicMin(&min_s, gb);
        atomicMax(&peak_s, peak);
        if (flags) atomicOr(&flags_s, flags);
    }
    __syncthreads();
    if (tid == 0) {
        LimsHeader* hd = reinterpret_cast<LimsHeader*>(state);
        if (min_s < 0x3F800000u) atomicMin(&hd->acc_min, min_s);
        if (peak_s) atomicMax(&hd->acc_peak, peak_s);
        if (flags_s) atomicOr(&hd->acc_flags, flags_s);
    }
}

// Launch 3, one block: r of the samples an earlier push emitted that the next still needs -> the new copy of rhist, the chunk
// into the history ring, the chain's start for the tile left open, the record, the header.  Every thread has read the header
// before the barrier; one thread rewrites it behind it.
static __global__ __launch_bounds__(LIM_TILE) void lims_commit_kernel(unsigned char* __restrict__ state, const float* __restrict__ chunk,
                                                                      int n_cap, const int32_t* __restrict__ n_dev, int flush,
                                                                      LimsRecord* __restrict__ rec) {
    LimsView s;
    if (!lims_view(state, chunk, n_cap, n_dev, flush, &s)) {
        if (threadIdx.x == 0) {
            LimsRecord r;
            memset(&r, 0, sizeof r);
            r.flags = -1;
            *rec = r;
        }
        return;
    }
    const LimParams p = *reinterpret_cast<const LimParams*>(state + lims_params_off());
    const int L = p.L, tid = threadIdx.x, HX = s.HX;
    float* xhist = reinterpret_cast<float*>(state + lims_xhist_off());
    float* rhist = reinterpret_cast<float*>(state + lims_rhist_off(L));
    const float* r_old = rhist + (size_t)s.h.parity * lims_rstride(L);
    float* r_new = rhist + (size_t)(1 - s.h.parity) * lims_rstride(L);
    const float* ends = reinterpret_cast<const float*>(state + lims_ends_off(L));
    const long long E0 = s.pl.E0, E1 = s.pl.E1, N0 = s.pl.N0;
    const long long n = s.pl.N1 - N0;
    const bool moved = E1 > E0;
    if (moved && !flush)
        for (int j = tid; j < L - 1; j += LIM_TILE) {
            const long long m = E1 - (L - 1) + j;
            if (m >= 0 && m < E0) r_new[j] = r_old[m - (E0 - (L - 1))];
        }
    for (long long i = (n > HX ? n - HX : 0) + tid; i < n; i += LIM_TILE) xhist[(N0 + i) % HX] = chunk[i];
    __syncthreads();
    if (tid == 0) {
        float st = s.h.start;
        for (long long q = 0; q < s.pl.nt && q < LIMS_MAX_TILES && (s.pl.t0 + q + 1) * LIM_TILE <= E1; ++q)
            st = lims_chain_step(p, ends[q], st);
        const uint32_t peak_run = lim_umax(s.h.peak_run, s.h.acc_peak);
        const bool ever = s.h.ever || s.h.acc_min < 0x3F800000u;
        *rec = lims_record(s.h, s.pl, peak_run, ever);
        LimsHeader h = s.h;
        h.n_in = flush ? 0 : s.pl.N1;
        h.n_out = flush ? 0 : E1;
        h.start = flush ? 1.f : st;
        h.peak_run = flush ? 0u : peak_run;
        h.ever = flush ? 0 : (int32_t)ever;
        h.acc_peak = 0; h.acc_min = 0x3F800000u; h.acc_flags = 0;
        if (moved) h.parity = 1 - h.parity;
        *reinterpret_cast<LimsHeader*>(state) = h;
    }
}
#endif

}  // namespace gsv
