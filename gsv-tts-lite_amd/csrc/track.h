// track: a stream of fp32 samples -> fixed s16 packets at another rate, for a real-time track.  A stateful
// form of torchaudio's sinc resampler (sv.h states the table) whose output does not depend on how the stream was cut into
// chunks, followed by flacenc.h's quantiser and a packetiser.  The scalar pieces below -- the rule that says how many
// outputs exist after N samples, the plan of one push, the tap sum with fmaf in tap order, the table entry -- are one text
// for the device kernels, for the host twin track_push_host (gsv_track_push_host: the CPU path and the device's oracle) and
// for the stand-alone checker tools/track_host_check.cpp.  Device bytes equal host bytes: both read the SAME table, built
// on the host in fp64 and cast to fp32 (track_init_host), never by a device kernel.
//
// The caller-owned state: [TrackHeader | table fp32 [w][L] | history fp32 [H] | carry int16 [packet * channels]], each part
// 16-byte aligned.  The history is a ring: input sample s of the stream lives at hist[s % H], H = L + o; an output never
// reads further back than L - 1 samples behind the newest, so no sample is overwritten while an output still needs it.
#pragma once
#include <math.h>
#include <stdint.h>

#include "flacenc.h"

namespace gsv {

constexpr int32_t TRACK_MAGIC = 0x4B525447;        // "GTRK"
constexpr int TRACK_MAX_PACKET = 4096;
constexpr int TRACK_TILE = 256;                    // outputs per block pass: one per thread
constexpr int TRACK_LDS_FLOATS = 8192;             // the staged input span of a tile; longer spans are read from memory

struct TrackHeader {
    long long n_in, n_out;      // samples pushed / outputs produced since the last flush
    int32_t carry;              // samples per channel waiting in the carry (< packet)
    int32_t o, w, width, L, H;  // gcd-reduced input / output rate, the kernel's half width, taps, ring length
    int32_t packet, channels;
    int32_t magic, pad[3];
};
static_assert(sizeof(TrackHeader) == 64, "state header");

FLAC_HD size_t track_align16(size_t v) { return (v + 15) & ~(size_t)15; }
FLAC_HD size_t track_table_off() { return sizeof(TrackHeader); }
FLAC_HD size_t track_hist_off(int o, int w, int L) { return track_table_off() + track_align16(o == w ? 0 : (size_t)w * L * sizeof(float)); }
FLAC_HD size_t track_carry_off(int o, int w, int L) { return track_hist_off(o, w, L) + track_align16((size_t)(L + o) * sizeof(float)); }
FLAC_HD size_t track_state_bytes(int o, int w, int L, int packet, int channels) {
    return track_carry_off(o, w, L) + track_align16((size_t)packet * channels * sizeof(int16_t));
}

// all the outputs of a stream of N samples: M = ceil(w N / o)
FLAC_HD long long track_total(long long N, int o, int w) { return o == w ? N : (w * N + o - 1) / o; }

// the outputs that exist once N samples have arrived: every whole frame j (w outputs reading x[j o - width, j o + width + o))
// whose last tap has arrived, never more than the stream has in all
FLAC_HD long long track_avail(long long N, int o, int w, int width) {
    if (o == w) return N;
    const long long J = N < width + o ? 0 : (N - width - o) / o + 1;
    const long long M = track_total(N, o, w);
    return w * J < M ? w * J : M;
}

// the most int16 elements one push of at most n_cap samples writes: the old carry, what n_cap samples can complete (a flush
// also takes the frames that were waiting for their last taps), rounded up to whole packets
FLAC_HD long long track_out_capacity(long long n_cap, int o, int w, int L, int packet, int channels) {
    const long long produced = o == w ? n_cap : (w * (n_cap + L) + o - 1) / o + 1;
    const long long samples = (packet - 1) + produced;
    return (samples + packet - 1) / packet * packet * channels;
}

struct TrackPlan {
    long long N0, P0, N1, P1;       // samples in / outputs out before and after this push
    long long produced, total;      // outputs of this push; with the old carry in front
    long long packets;              // whole packets written (a flush pads the last)
    int c0, carry_new, padded;
};

FLAC_HD TrackPlan track_plan(const TrackHeader& h, long long n, bool flush) {
    TrackPlan p;
    p.N0 = h.n_in; p.P0 = h.n_out; p.c0 = h.carry;
    p.N1 = p.N0 + n;
    p.P1 = flush ? track_total(p.N1, h.o, h.w) : track_avail(p.N1, h.o, h.w, h.width);
    p.produced = p.P1 - p.P0;
    p.total = p.c0 + p.produced;
    p.packets = flush ? (p.total + h.packet - 1) / h.packet : p.total / h.packet;
    p.padded = flush ? (int)(p.packets * h.packet - p.total) : 0;
    p.carry_new = flush ? 0 : (int)(p.total - p.packets * h.packet);
    return p;
}

// sum over the taps [i_lo, i_hi) of x(s0 + i) k[i]: fp32, tap order, fused multiply-add.  X maps a stream index to its sample.
template <typename X>
FLAC_HD float track_tap_sum(const X& x, long long s0, int i_lo, int i_hi, const float* k) {
    float acc = 0.f;
    for (int i = i_lo; i < i_hi; ++i) acc = fmaf(x(s0 + i), k[i], acc);
    return acc;
}

// output m of a stream that has N samples so far (samples outside [0, N) are skipped)
template <typename X>
FLAC_HD float track_output(const X& x, long long m, long long N, int o, int w, int width, int L, const float* table) {
    const long long j = m / w;
    const int p = (int)(m % w);
    const long long s0 = j * o - width;
    const int i_lo = s0 < 0 ? (int)-s0 : 0;
    const int i_hi = N - s0 < L ? (int)(N - s0) : L;
    return track_tap_sum(x, s0, i_lo, i_hi, table + (size_t)p * L);
}

// gcd-reduced rates and the half width, as rs_params (gsv_ref.hip) gives them; false on rates it refuses
inline bool track_params(int in_rate, int out_rate, int* o, int* w, int* width) {
    if (in_rate < 1 || out_rate < 1) return false;
    int a = in_rate, b = out_rate;
    while (b) { const int r = a % b; a = b; b = r; }
    *o = in_rate / a;
    *w = out_rate / a;
    const int lo = *o < *w ? *o : *w;
    *width = (int)ceil(6.0 * *o / ((double)lo * 0.99));
    return (long long)*w * (2 * *width + *o) <= (1LL << 24);
}

// torchaudio's _get_sinc_resample_kernel entry K[p][q] (sv.h): fp64 with the fp32 phase division, cast to fp32
inline float track_table_entry(int p, int q, int o, int w, int width) {
    const double kPi = 3.14159265358979323846;
    const double base = (double)(o < w ? o : w) * 0.99;
    double t = (double)((float)(-p) / (float)w) + (double)(q - width) / (double)o;
    t *= base;
    t = fmin(fmax(t, -6.0), 6.0);
    const double c = cos(t * kPi / 6.0 / 2.0);
    const double window = c * c;
    t *= kPi;
    const double k = t == 0.0 ? 1.0 : sin(t) / t;
    return (float)(k * (window * (base / (double)o)));
}

// a fresh state in host memory (`state` holds track_state_bytes): header, table, silent history, empty carry
inline void track_init_host(unsigned char* state, int o, int w, int width, int packet, int channels) {
    const int L = 2 * width + o;
    const size_t bytes = track_state_bytes(o, w, L, packet, channels);
    for (size_t i = 0; i < bytes; ++i) state[i] = 0;
    TrackHeader h;
    h.n_in = 0; h.n_out = 0; h.carry = 0;
    h.o = o; h.w = w; h.width = width; h.L = L; h.H = L + o;
    h.packet = packet; h.channels = channels;
    h.magic = TRACK_MAGIC; h.pad[0] = h.pad[1] = h.pad[2] = 0;
    __builtin_memcpy(state, &h, sizeof h);
    if (o != w) {
        float* K = reinterpret_cast<float*>(state + track_table_off());
        for (int p = 0; p < w; ++p)
            for (int q = 0; q < L; ++q) K[(size_t)p * L + q] = track_table_entry(p, q, o, w, width);
    }
}

// one push over host memory: the serial twin of the two launches.  out holds track_out_capacity elements.
inline void track_push_host(unsigned char* state, const float* chunk, long long n, bool flush, int16_t* out, int32_t* rec) {
    TrackHeader h;
    __builtin_memcpy(&h, state, sizeof h);
    const float* table = reinterpret_cast<const float*>(state + track_table_off());
    float* hist = reinterpret_cast<float*>(state + track_hist_off(h.o, h.w, h.L));
    int16_t* carry = reinterpret_cast<int16_t*>(state + track_carry_off(h.o, h.w, h.L));
    const TrackPlan p = track_plan(h, n, flush);
    const int ch = h.channels;
    for (long long e = 0; e < (long long)p.c0 * ch; ++e) out[e] = carry[e];
    const long long N0 = p.N0;
    const int H = h.H;
    auto x = [=](long long s) { return s >= N0 ? chunk[s - N0] : hist[s % H]; };
    for (long long t = p.c0; t < p.total; ++t) {
        const long long m = p.P0 + (t - p.c0);
        const float y = h.o == h.w ? chunk[m - N0] : track_output(x, m, p.N1, h.o, h.w, h.width, h.L, table);
        const int16_t q = (int16_t)flac_enc_quantise(y, 16);
        for (int c = 0; c < ch; ++c) out[t * ch + c] = q;
    }
    for (long long e = p.total * ch; e < p.packets * h.packet * ch; ++e) out[e] = 0;
    for (long long e = 0; e < (long long)p.carry_new * ch; ++e) carry[e] = out[p.packets * h.packet * ch + e];
    for (long long i = n > H ? n - H : 0; i < n; ++i) hist[(N0 + i) % H] = chunk[i];
    h.n_in = flush ? 0 : p.N1;
    h.n_out = flush ? 0 : p.P1;
    h.carry = p.carry_new;
    __builtin_memcpy(state, &h, sizeof h);
    rec[0] = (int32_t)p.packets; rec[1] = (int32_t)p.produced; rec[2] = p.carry_new; rec[3] = p.padded;
}

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------------------------------
// the device kernels
// ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ long long track_len_dev(const int32_t* __restrict__ n_dev, int n_cap) {
    if (!n_dev) return n_cap;
    const int v = *n_dev;
    return v < 0 ? 0 : v > n_cap ? n_cap : v;
}

// Launch 1: one element of `out` per thread and pass -- the old carry in front, then this push's outputs, then a flush's
// zeros --; a block walks the tiles blockIdx.x, blockIdx.x + gridDim.x, ... until the device-side count is covered (the grid
// is sized from n_cap alone: the host knows neither the rates nor the real length).  Each tile stages the input span of its
// outputs, history ring plus chunk, in LDS; a span longer than TRACK_LDS_FLOATS (a block-uniform condition) is read from
// memory instead.  out_cap: elements of `out`, from the same n_cap by track_out_capacity; nothing is written at or behind it.
static __global__ __launch_bounds__(TRACK_TILE) void track_outputs_kernel(const unsigned char* __restrict__ state,
                                                                          const float* __restrict__ chunk, int n_cap,
                                                                          const int32_t* __restrict__ n_dev, int flush,
                                                                          int16_t* __restrict__ out) {
    __shared__ float xs[TRACK_LDS_FLOATS];
    const TrackHeader h = *reinterpret_cast<const TrackHeader*>(state);
    if (h.magic != TRACK_MAGIC) return;         // not a state gsv_track_init made: nothing is read through it
    const float* __restrict__ table = reinterpret_cast<const float*>(state + track_table_off());
    const float* __restrict__ hist = reinterpret_cast<const float*>(state + track_hist_off(h.o, h.w, h.L));
    const int16_t* __restrict__ carry = reinterpret_cast<const int16_t*>(state + track_carry_off(h.o, h.w, h.L));
    const long long n = track_len_dev(n_dev, n_cap);
    const TrackPlan p = track_plan(h, n, flush != 0);
    const long long out_cap = track_out_capacity(n_cap, h.o, h.w, h.L, h.packet, h.channels);
    const long long end = p.packets * h.packet > p.total ? p.packets * h.packet : p.total;     // samples per channel to write
    const int ch = h.channels, tid = threadIdx.x;
    const long long N0 = p.N0;
    const int H = h.H;
    auto fetch = [=](long long s) { return s >= N0 ? chunk[s - N0] : hist[s % H]; };
    for (long long t0 = (long long)blockIdx.x * TRACK_TILE; t0 < end; t0 += (long long)gridDim.x * TRACK_TILE) {
        // the tile's computed outputs [m_lo, m_hi) and the input span behind them
        const long long a = t0 > p.c0 ? t0 : p.c0;
        const long long b = t0 + TRACK_TILE < p.total ? t0 + TRACK_TILE : p.total;
        const bool taps = h.o != h.w && a < b;
        long long s_lo = 0, span = 0;
        if (taps) {
            const long long m_lo = p.P0 + (a - p.c0), m_hi = p.P0 + (b - p.c0);
            const long long j_lo = m_lo / h.w, j_hi = (m_hi - 1) / h.w;
            s_lo = j_lo * h.o - h.width;
            span = (j_hi - j_lo) * h.o + h.L;
        }
        const bool staged = taps && span <= TRACK_LDS_FLOATS;
        if (staged) {
            for (long long k = tid; k < span; k += TRACK_TILE) {
                const long long s = s_lo + k;
                xs[k] = s >= 0 && s < p.N1 ? fetch(s) : 0.f;
            }
        }
        __syncthreads();
        const long long t = t0 + tid;
        if (t < end && (t + 1) * ch <= out_cap) {
            int16_t q = 0;
            if (t < p.c0) {
                for (int c = 0; c < ch; ++c) out[t * ch + c] = carry[t * ch + c];
            } else {
                if (t < p.total) {
                    const long long m = p.P0 + (t - p.c0);
                    float y;
                    if (h.o == h.w) {
                        y = chunk[m - N0];
                    } else if (staged) {
                        const float* xl = xs;
                        const long long base = s_lo;
                        y = track_output([=](long long s) { return xl[s - base]; }, m, p.N1, h.o, h.w, h.width, h.L, table);
                    } else {
                        y = track_output(fetch, m, p.N1, h.o, h.w, h.width, h.L, table);
                    }
                    q = (int16_t)flac_enc_quantise(y, 16);
                }
                for (int c = 0; c < ch; ++c) out[t * ch + c] = q;
            }
        }
        __syncthreads();        // the next pass stages over xs
    }
}

// Launch 2, one block: the new carry from the tail of `out`, the chunk into the history ring, the header, rec.  Every thread
// has read the header before the barrier; one thread rewrites it behind it.
static __global__ __launch_bounds__(TRACK_TILE) void track_commit_kernel(unsigned char* __restrict__ state,
                                                                         const float* __restrict__ chunk, int n_cap,
                                                                         const int32_t* __restrict__ n_dev, int flush,
                                                                         const int16_t* __restrict__ out, int32_t* __restrict__ rec) {
    const TrackHeader h = *reinterpret_cast<const TrackHeader*>(state);
    if (h.magic != TRACK_MAGIC) {
        if (threadIdx.x < 4) rec[threadIdx.x] = -1;
        return;
    }
    float* __restrict__ hist = reinterpret_cast<float*>(state + track_hist_off(h.o, h.w, h.L));
    int16_t* __restrict__ carry = reinterpret_cast<int16_t*>(state + track_carry_off(h.o, h.w, h.L));
    const long long n = track_len_dev(n_dev, n_cap);
    const TrackPlan p = track_plan(h, n, flush != 0);
    const long long out_cap = track_out_capacity(n_cap, h.o, h.w, h.L, h.packet, h.channels);
    const int tid = threadIdx.x;
    const long long whole = p.packets * h.packet * h.channels;
    for (long long e = tid; e < (long long)p.carry_new * h.channels; e += TRACK_TILE)
        if (whole + e < out_cap) carry[e] = out[whole + e];
    for (long long i = (n > h.H ? n - h.H : 0) + tid; i < n; i += TRACK_TILE) hist[(p.N0 + i) % h.H] = chunk[i];
    __syncthreads();
    if (tid == 0) {
        TrackHeader* hd = reinterpret_cast<TrackHeader*>(state);
        hd->n_in = flush ? 0 : p.N1;
        hd->n_out = flush ? 0 : p.P1;
        hd->carry = p.carry_new;
        rec[0] = (int32_t)p.packets; rec[1] = (int32_t)p.produced; rec[2] = p.carry_new; rec[3] = p.padded;
    }
}
#endif

}  // namespace gsv
