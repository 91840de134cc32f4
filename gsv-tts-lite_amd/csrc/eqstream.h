// eqstream: the equaliser of eq.h for a stream that arrives in pushes.  An equaliser is causal, so the stream form
// has no delay and no ring-out: a push of n samples emits n samples, and the emitted samples, concatenated, are the bytes gsv_eq
// returns for the same samples as one clip with the same design -- however the stream was cut into pushes.
//
// Why the bytes can be the clip's.  In eq_filter_kernel a sample's output depends on the chunk's start state and on the samples
// at or before it within the chunk alone: thread t of the Hillis-Steele prefix reads threads <= t, and what the zero padding
// behind a short span turns into never reaches an earlier output.  The start state of chunk k + 1 is J S_k + E_k, E_k the chunk's
// end state from zero state (eq_chain_row).  So the stream runs the same operations on EQ_CHUNK-aligned chunks of the STREAM index:
// the state keeps the joint start state S_k of the open chunk and the open chunk's input so far, a push reruns the open chunk's
// full pass from S_k over the kept samples and the new ones and writes the outputs that were not emitted before, and for every
// chunk the push completes it runs the pass from zero state, chains with J, and runs the chunks behind it: the clip's three
// launches.  Nothing is continued by a recurrence of its own, and the operations are the same because they are the same text:
// the sections of a span are eq.h's eq_sections (eq_sections_host in the twin) and the chain is its eq_chain_walk
// (eq_chain_host), called from here as from the clip's kernels.  What is the stream's own is where a sample comes from and
// which outputs are written.
//
// A sample that is not finite.  A clip holding one comes back unchanged, which a stream cannot know ahead of time; here such a
// sample enters the filter as 0.0 and is copied to the output bit for bit, so the state is never poisoned and every other output
// equals the stream with that sample replaced by 0.0 (cut-independent too).  The push's record says EQS_NONFINITE, the stream's
// EQS_NONFINITE_EVER, and such samples are kept out of both peaks.
//
// eq_design and loud_store are used as eq.h uses them; what is new here -- the plan of a push, the sample as it enters the filter, the
// record -- is one __host__ __device__ text for the kernels, for the host twin eqs_push_host
// (gsv_eqstream_push_host: the CPU path and the device's oracle) and for tools/eqstream_host_check.cpp.
//
// The caller-owned state, every part 16-byte aligned:
//   [EqsHeader | EqState S | EqDesign | stash fp32 [2][EQ_CHUNK] | ends EqState [EQS_MAX_BLOCKS] | starts EqState [EQS_MAX_BLOCKS + 1]]
//   S       the joint start state of the open chunk (the chunk that holds sample `n` of the stream)
//   stash   the open chunk's input so far, as it came (a NaN stays a NaN), [parity] the valid copy.  Two copies used in turn: the
//           block that runs the chunk a push leaves open writes the whole of its input so far to the other copy while the block of
//           the push's first chunk may still read the old one; and since a block stashes a span before it writes the span's
//           outputs, out == chunk (in place) is safe.  The commit launch turns `parity` over.
//   ends    E_k of every chunk this push completes, starts: S of every chunk it touches: scratch between the launches of a push
#pragma once
#include "eq.h"

namespace gsv {

constexpr int32_t EQS_MAGIC = 0x53514547;           // "GEQS"
constexpr int EQS_MAX_PUSH = 1 << 20;               // samples of one push
constexpr int EQS_MAX_BLOCKS = EQS_MAX_PUSH / EQ_CHUNK + 1;     // chunks one push can touch, wherever in a chunk it starts
constexpr int EQS_LANES = 64;                       // lanes of the chain and the commit wave
constexpr int EQS_EQUALISED = 1, EQS_NONFINITE_EVER = 2, EQS_NONFINITE = 4;     // record flags
static_assert(EQS_MAX_PUSH % EQ_CHUNK == 0, "blocks of a push");
static_assert(EQS_LANES == EQ_LANES, "eq_chain_walk's wave");

struct EqsHeader {
    long long n;                            // samples of the stream so far (since the last flush)
    uint32_t peak_in_run, peak_out_run;     // bits of max |x|, max |y| over the stream's finite samples so far
    uint32_t acc_in, acc_out;               // ... over this push's: integer maxima by the full pass, reset by the commit
    int32_t acc_flags, ever;                // EQS_NONFINITE of this push; of the stream so far
    int32_t parity, magic;
    int32_t pad[6];
};
static_assert(sizeof(EqsHeader) == 64, "state header");

struct EqsRecord {              // gsv_eqstream_record
    int32_t emitted;            // samples this push wrote to `out`: the next stage's n_dev
    int32_t flags;
    float peak_in, peak_out;            // max |x|, max |y| over the finite samples of this push (0 for none)
    float peak_in_run, peak_out_run;    // ... of the stream so far
    long long total;            // samples of the stream so far (this push included; a flush reports the stream's length)
};
static_assert(sizeof(EqsRecord) == 32, "record");

LOUD_HD size_t eqs_s_off() { return sizeof(EqsHeader); }
LOUD_HD size_t eqs_design_off() { return eqs_s_off() + loud_align16(sizeof(EqState)); }
LOUD_HD size_t eqs_stash_off() { return eqs_design_off() + loud_align16(sizeof(EqDesign)); }
LOUD_HD size_t eqs_ends_off() { return eqs_stash_off() + 2 * (size_t)EQ_CHUNK * sizeof(float); }
LOUD_HD size_t eqs_starts_off() { return eqs_ends_off() + loud_align16((size_t)EQS_MAX_BLOCKS * sizeof(EqState)); }
LOUD_HD size_t eqs_state_bytes() { return eqs_starts_off() + loud_align16((size_t)(EQS_MAX_BLOCKS + 1) * sizeof(EqState)); }

struct EqsPlan {
    long long N0, N1;           // samples of the stream before and after this push
    long long k0;               // the open chunk: the first one this push touches
    int nb, done;               // chunks the push touches (k0 .. k0 + nb - 1); chunks it completes (k0 .. k0 + done - 1)
};

LOUD_HD EqsPlan eqs_plan(long long seen, long long n) {
    EqsPlan p;
    p.N0 = seen;
    p.N1 = seen + n;
    p.k0 = seen / EQ_CHUNK;
    p.nb = n > 0 ? (int)((p.N1 - 1) / EQ_CHUNK - p.k0) + 1 : 0;
    p.done = (int)(p.N1 / EQ_CHUNK - p.k0);
    return p;
}

LOUD_HD int eqs_clamp(int v, int n_cap) { return v < 0 ? 0 : v > n_cap ? n_cap : v; }
LOUD_HD bool eqs_finite(float x) { return loud_abs_bits(x) < 0x7F800000u; }

// sample s of the stream as it came, for a block on chunk `lo / EQ_CHUNK`: from the stash in front of this push, else from the chunk
LOUD_HD float eqs_raw(const float* stash_old, const float* chunk, long long N0, long long lo, long long s) {
    return s < N0 ? stash_old[s - lo] : chunk[s - N0];
}

// the record of a push and the header behind it (S is the caller's: starts[done], or zero behind a flush)
LOUD_HD EqsRecord eqs_finish(EqsHeader& h, const EqsPlan& pl, bool flush) {
    EqsRecord r;
    const uint32_t pin = h.acc_in > h.peak_in_run ? h.acc_in : h.peak_in_run;
    const uint32_t pout = h.acc_out > h.peak_out_run ? h.acc_out : h.peak_out_run;
    const int32_t ever = h.ever | (h.acc_flags & EQS_NONFINITE);
    r.emitted = (int32_t)(pl.N1 - pl.N0);
    r.flags = EQS_EQUALISED | (h.acc_flags & EQS_NONFINITE) | (ever ? EQS_NONFINITE_EVER : 0);
    r.peak_in = loud_from_bits(h.acc_in);
    r.peak_out = loud_from_bits(h.acc_out);
    r.peak_in_run = loud_from_bits(pin);
    r.peak_out_run = loud_from_bits(pout);
    r.total = pl.N1;
    h.n = flush ? 0 : pl.N1;
    h.peak_in_run = flush ? 0u : pin;
    h.peak_out_run = flush ? 0u : pout;
    h.ever = flush ? 0 : ever;
    h.acc_in = 0; h.acc_out = 0; h.acc_flags = 0;
    if (pl.N1 > pl.N0) h.parity = 1 - h.parity;
    return r;
}

LOUD_HD EqsRecord eqs_bad_record() {
    EqsRecord r;
    r.emitted = 0; r.flags = -1;
    r.peak_in = r.peak_out = r.peak_in_run = r.peak_out_run = 0.f;
    r.total = 0;
    return r;
}

// ------------------------------------------------------------------------------------------------------------------
// host only
// ------------------------------------------------------------------------------------------------------------------
inline void eqs_init_host(unsigned char* state, const EqCoefs& d) {
    memset(state, 0, eqs_state_bytes());
    EqsHeader h;
    memset(&h, 0, sizeof h);
    h.magic = EQS_MAGIC;
    memcpy(state, &h, sizeof h);
    eq_design(d, reinterpret_cast<EqDesign*>(state + eqs_design_off()));
}

// the samples [lo, hi) of the stream (inside one chunk, lo its first sample) span by span from the joint state `carry`, as one
// block walks them -> the state behind them.  ends: the pass from zero state over a whole chunk, nothing written; else the outputs
// of the samples at or behind N0, both peaks' bits, the flags, and with stash_new the chunk's input as it came
inline EqState eqs_chunk_host(const float* stash_old, const float* chunk, long long N0, long long lo, long long hi, const EqDesign& D, EqState carry,
                              bool ends, float* out, float* stash_new, uint32_t* peak_in, uint32_t* peak_out, int32_t* flags) {
    static thread_local double v[EQ_T][EQ_R];
    for (long long s0 = lo; s0 < hi; s0 += EQ_SPAN) {
        const int cnt = hi - s0 < EQ_SPAN ? (int)(hi - s0) : EQ_SPAN;
        // a prefix of the scan reads the runs to its left alone, and the state behind a span the push leaves short is not used:
        // the runs behind the last sample are not walked (the device has the threads anyway)
        const int nt = !ends && cnt < EQ_SPAN ? (cnt + EQ_R - 1) / EQ_R : EQ_T;
        for (int k = 0; k < nt * EQ_R; ++k) {
            float xv = 0.f;
            if (k < cnt) {
                const float raw = eqs_raw(stash_old, chunk, N0, lo, s0 + k);
                if (stash_new) stash_new[s0 + k - lo] = raw;
                if (eqs_finite(raw)) {
                    xv = raw;
                    const uint32_t a = loud_abs_bits(raw);
                    if (!ends && s0 + k >= N0 && a > *peak_in) *peak_in = a;
                } else if (!ends && s0 + k >= N0) {
                    *flags |= EQS_NONFINITE;
                }
            }
            v[k / EQ_R][k % EQ_R] = (double)xv;
        }
        eq_sections_host(D, nt, ends, v, carry);
        for (int k = 0; !ends && k < cnt; ++k) {
            if (s0 + k < N0) continue;          // emitted by an earlier push
            const float raw = chunk[s0 + k - N0];       // out may be the chunk: read before the write
            float o = raw;
            if (eqs_finite(raw)) {
                o = loud_store(v[k / EQ_R][k % EQ_R]);
                const uint32_t a = loud_abs_bits(o);
                if (a > *peak_out) *peak_out = a;
            }
            out[s0 + k - N0] = o;
        }
    }
    return carry;
}

// one push over host memory: the serial twin of the four launches.  out holds n floats and may be the chunk.
inline void eqs_push_host(unsigned char* state, const float* chunk, int n, bool flush, float* out, EqsRecord* rec) {
    EqsHeader h;
    memcpy(&h, state, sizeof h);
    if (h.magic != EQS_MAGIC) {         // not a state eqs_init_host made: nothing is read through it
        *rec = eqs_bad_record();
        return;
    }
    const EqDesign& D = *reinterpret_cast<const EqDesign*>(state + eqs_design_off());
    EqState* S = reinterpret_cast<EqState*>(state + eqs_s_off());
    float* stash = reinterpret_cast<float*>(state + eqs_stash_off());
    const float* stash_old = stash + (size_t)h.parity * EQ_CHUNK;
    float* stash_new = stash + (size_t)(1 - h.parity) * EQ_CHUNK;
    EqState* ends = reinterpret_cast<EqState*>(state + eqs_ends_off());
    EqState* starts = reinterpret_cast<EqState*>(state + eqs_starts_off());
    const EqsPlan pl = eqs_plan(h.n, n);
    EqState zero;
    memset(&zero, 0, sizeof zero);
    for (int b = 0; b < pl.done; ++b) {
        const long long lo = (pl.k0 + b) * EQ_CHUNK;
        ends[b] = eqs_chunk_host(stash_old, chunk, pl.N0, lo, lo + EQ_CHUNK, D, zero, true, nullptr, nullptr, nullptr, nullptr, nullptr);
    }
    eq_chain_host(D, *S, pl.done, ends, starts);
    for (int b = 0; b < pl.nb; ++b) {
        const long long lo = (pl.k0 + b) * EQ_CHUNK;
        const bool open = lo + EQ_CHUNK > pl.N1;
        eqs_chunk_host(stash_old, chunk, pl.N0, lo, open ? pl.N1 : lo + EQ_CHUNK, D, starts[b], false, out, open ? stash_new : nullptr, &h.acc_in,
                       &h.acc_out, &h.acc_flags);
    }
    *S = flush ? zero : starts[pl.done];
    *rec = eqs_finish(h, pl, flush);
    memcpy(state, &h, sizeof h);
}

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------------------------------
// the device kernels
// ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int eqs_len_dev(const int32_t* n_dev, int n_cap) { return n_dev ? eqs_clamp(*n_dev, n_cap) : n_cap; }

// eq_filter_kernel for a push: one block per chunk of the stream that the push touches, block b on chunk k0 + b.  ENDS: over the
// chunks the push completes, from zero state to the chunk's end state -> ends[b], nothing else written.  Else the full pass from
// starts[b]: the outputs of the push's own samples, both peaks, the flags, and -- the block of the chunk left open -- the chunk's
// input so far into the other stash.  The padded runs in LDS are laid out as eq_filter_kernel's, and eq_sections runs over them.
// chunk and out may be one buffer: a block reads a span (and stashes it) before it writes the span's outputs, and no block reads
// another block's samples.
template <bool ENDS>
static __global__ __launch_bounds__(EQ_T) void eqs_filter_kernel(unsigned char* state, const float* chunk, int n_cap, const int32_t* n_dev, float* out) {
    __shared__ float xs[EQ_T * (EQ_R + 1)];
    __shared__ double sc[2][2][EQ_T];
    __shared__ double carry_s[EQ_NS];
    __shared__ uint32_t peak_s[2];
    __shared__ int flags_s;
    const EqsHeader h = *reinterpret_cast<const EqsHeader*>(state);
    if (h.magic != EQS_MAGIC) return;           // not a state gsv_eqstream_init made: nothing is read through it
    const EqsPlan pl = eqs_plan(h.n, eqs_len_dev(n_dev, n_cap));
    const int tid = threadIdx.x, blk = blockIdx.x;
    if (blk >= (ENDS ? pl.done : pl.nb) || blk >= EQS_MAX_BLOCKS) return;      // block-uniform
    const EqDesign* __restrict__ D = reinterpret_cast<const EqDesign*>(state + eqs_design_off());
    float* stash = reinterpret_cast<float*>(state + eqs_stash_off());
    const float* stash_old = stash + (size_t)h.parity * EQ_CHUNK;
    float* stash_new = stash + (size_t)(1 - h.parity) * EQ_CHUNK;
    const int ns = D->ns;
    const long long N0 = pl.N0;
    const long long lo = (pl.k0 + blk) * EQ_CHUNK, chunk_hi = lo + EQ_CHUNK;
    const long long hi = chunk_hi < pl.N1 ? chunk_hi : pl.N1;
    const bool open = !ENDS && chunk_hi > pl.N1;
    if (tid < 2) peak_s[tid] = 0;
    if (tid == 0) flags_s = 0;
    if (tid < EQ_NS) carry_s[tid] = ENDS ? 0.0 : reinterpret_cast<const EqState*>(state + eqs_starts_off())[blk].s[tid];
    uint32_t peak_in = 0, peak_out = 0;
    int flags = 0;
    float* mine = xs + tid * (EQ_R + 1);
    for (long long s0 = lo; s0 < hi; s0 += EQ_SPAN) {
        const int cnt = hi - s0 < EQ_SPAN ? (int)(hi - s0) : EQ_SPAN;
        uint32_t nf = 0;                // bit j: sample tid + j EQ_T of the span is this push's and not finite
#pragma unroll
        for (int j = 0; j < EQ_R; ++j) {
            const int k = tid + j * EQ_T;
            float xv = 0.f;
            if (k < cnt) {
                const long long s = s0 + k;
                const float raw = eqs_raw(stash_old, chunk, N0, lo, s);
                if (open) stash_new[s - lo] = raw;
                if (eqs_finite(raw)) {
                    xv = raw;
                    const uint32_t a = loud_abs_bits(raw);
                    if (s >= N0) peak_in = a > peak_in ? a : peak_in;
                } else if (s >= N0) {
                    nf |= 1u << j;
                }
            }
            xs[(k / EQ_R) * (EQ_R + 1) + k % EQ_R] = xv;
        }
        __syncthreads();                // xs, and carry_s of the last span (or of the prologue)
        double v[EQ_R];
        eq_sections<ENDS>(D, ns, mine, sc, carry_s, v);
        if (!ENDS) {
            if (tid * EQ_R < cnt) {
#pragma unroll
                for (int i = 0; i < EQ_R; ++i) mine[i] = loud_store(v[i]);
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < EQ_R; ++j) {
                const int k = tid + j * EQ_T;
                const long long s = s0 + k;
                if (k < cnt && s >= N0) {       // what an earlier push emitted is not written again
                    float o;
                    if (nf >> j & 1u) {
                        o = chunk[s - N0];      // copied bit for bit (in place: still the sample as it came)
                    } else {
                        o = xs[(k / EQ_R) * (EQ_R + 1) + k % EQ_R];
                        const uint32_t a = loud_abs_bits(o);
                        peak_out = a > peak_out ? a : peak_out;
                    }
                    out[s - N0] = o;
                }
            }
            if (nf) flags |= EQS_NONFINITE;
        }
        __syncthreads();        // the next span stages over xs and sc
    }
    if (ENDS) {
        if (tid < EQ_NS) reinterpret_cast<EqState*>(state + eqs_ends_off())[blk].s[tid] = carry_s[tid];
        return;
    }
    atomicMax(&peak_s[0], peak_in);
    atomicMax(&peak_s[1], peak_out);
    if (flags) atomicOr(&flags_s, flags);
    __syncthreads();
    EqsHeader* hd = reinterpret_cast<EqsHeader*>(state);
    if (tid == 0) {             // integer maxima: the order of the chunks does not show
        if (peak_s[0]) atomicMax(&hd->acc_in, peak_s[0]);
        if (peak_s[1]) atomicMax(&hd->acc_out, peak_s[1]);
        if (flags_s) atomicOr(&hd->acc_flags, flags_s);
    }
}

// between the two: one wave chains the chunks the push completes from the state's S (eq_chain_walk) -> the start state of every
// chunk the push touches
static __global__ __launch_bounds__(EQS_LANES) void eqs_chain_kernel(unsigned char* state, int n_cap, const int32_t* n_dev) {
    const EqsHeader h = *reinterpret_cast<const EqsHeader*>(state);
    if (h.magic != EQS_MAGIC) return;
    const EqsPlan pl = eqs_plan(h.n, eqs_len_dev(n_dev, n_cap));
    const int lane = threadIdx.x;
    const double mine = lane < EQ_NS ? reinterpret_cast<const EqState*>(state + eqs_s_off())->s[lane] : 0.0;
    eq_chain_walk(reinterpret_cast<const EqDesign*>(state + eqs_design_off())->J, mine, pl.done < EQS_MAX_BLOCKS ? pl.done : EQS_MAX_BLOCKS,
                  reinterpret_cast<const EqState*>(state + eqs_ends_off()), reinterpret_cast<EqState*>(state + eqs_starts_off()));
}

// last, one wave: the record, S of the chunk now open, the header.  Every lane has read the header before the barrier; one
// rewrites it behind it.
static __global__ __launch_bounds__(EQS_LANES) void eqs_commit_kernel(unsigned char* state, int n_cap, const int32_t* n_dev, int flush,
                                                                      EqsRecord* __restrict__ rec) {
    EqsHeader h = *reinterpret_cast<const EqsHeader*>(state);
    const int lane = threadIdx.x;
    if (h.magic != EQS_MAGIC) {
        if (lane == 0) *rec = eqs_bad_record();
        return;
    }
    const EqsPlan pl = eqs_plan(h.n, eqs_len_dev(n_dev, n_cap));
    const int done = pl.done < EQS_MAX_BLOCKS ? pl.done : EQS_MAX_BLOCKS;
    if (lane < EQ_NS)
        reinterpret_cast<EqState*>(state + eqs_s_off())->s[lane] = flush ? 0.0 : reinterpret_cast<const EqState*>(state + eqs_starts_off())[done].s[lane];
    __syncthreads();
    if (lane == 0) {
        *rec = eqs_finish(h, pl, flush != 0);
        *reinterpret_cast<EqsHeader*>(state) = h;
    }
}
#endif

}  // namespace gsv
