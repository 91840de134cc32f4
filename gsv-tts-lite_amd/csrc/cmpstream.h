// cmpstream: the compressor of compressor.h for a stream that arrives in pushes.  The compressor is causal, so the
// stream form has no delay and no ring-out: a push of n samples emits n samples, and the emitted samples, concatenated, are the
// bytes gsv_compressor returns for the same samples as one clip with the same parameters -- however the stream was cut into pushes.
//
// Why the bytes can be the clip's.  The clip runs CMP_CHUNK-aligned chunks in three passes (cmp_run_host): pass 0 gives the release
// map (B, C) of a chunk from zero state, a chain with JR turns these into every chunk's pstart, pass 1 gives eend from the true
// pstart and a zero e, a chain with JA turns these into every chunk's estart, and pass 2 is the full pass from (pstart, estart).
// Within a chunk an output depends on the chunk's start state and on the samples at or before it alone: a prefix of either scan of
// cmp_span reads the runs to its left, and what the zero padding behind a short span turns into never reaches an earlier output.
// So the stream runs the same operations on CMP_CHUNK-aligned chunks of the STREAM index: the state keeps (pstart, estart) of the
// open chunk and the open chunk's input so far; for every chunk a push completes it runs pass 0 from zero state, the JR chain from
// the kept pstart, pass 1, and the JA chain from the kept estart, and then the full pass over every chunk the push touches,
// writing the outputs that were not emitted before.  The open chunk is redone from its kept start state on every push.  Nothing
// is continued by a recurrence of its own: the p behind a chunk as the full pass leaves it is not, in general, the bits
// cmp_combine(JR, 0, st, B, C) gives, and only the chain's value may start the next chunk.  The operations are the same because
// they are the same text, compressor.h's: a block of the kernel is cmp_open, cmp_body per span (cmp_span, the products, the
// run's statistics) and cmp_close, a chain is cmp_chain_walk from the kept state, and the twin is cmp_drive_host and
// cmp_walk_host over the stream's samples.  What is the stream's own -- the plan of a push, where a sample comes from, how it
// enters the detector, which samples count and which outputs are written, the record -- is one __host__ __device__ text for the
// kernels, for the host twin cms_push_host (gsv_cmpstream_push_host: the CPU path and the device's oracle) and for
// tools/cmpstream_host_check.cpp.
//
// A sample that is not finite.  A clip holding one comes back unchanged, which a stream cannot know ahead of time; here (as in
// eqstream.h) such a sample enters the detector as 0.0 and is copied to the output bit for bit, so the state is never poisoned and
// every other output equals the stream with that sample replaced by 0.0 (cut-independent too).  The push's record says
// CMS_NONFINITE, the stream's CMS_NONFINITE_EVER, and such samples are kept out of both peaks and of the smallest gain.
//
// The caller-owned state, every part 16-byte aligned:
//   [CmsHeader | CmpDesign | CmsOpen | stash fp32 [2][CMP_CHUNK] | scratch CmpChunk [CMS_MAX_BLOCKS + 1]]
//   CmsOpen  (pstart, estart) of the open chunk (the chunk that holds sample `n` of the stream)
//   stash    the open chunk's input so far, as it came (a NaN stays a NaN), [parity] the valid copy.  Two copies used in turn: the
//            block that runs the chunk a push leaves open writes the whole of its input so far to the other copy while the block of
//            the push's first chunk may still read the old one; and since a block stashes a span before it writes the span's
//            outputs, out == chunk (in place) is safe.  The commit launch turns `parity` over.
//   scratch  what the passes and the chains leave per chunk the push touches, [b] for chunk k0 + b, between the launches of a push
#pragma once
#include "compressor.h"

namespace gsv {

constexpr int32_t CMS_MAGIC = 0x534D4347;           // "GCMS"
constexpr int CMS_MAX_PUSH = 1 << 20;               // samples of one push
constexpr int CMS_MAX_BLOCKS = CMS_MAX_PUSH / CMP_CHUNK + 1;    // chunks one push can touch, wherever in a chunk it starts
constexpr int CMS_LANES = 64;                       // lanes of the chain and the commit wave
constexpr int CMS_STREAM = 1, CMS_NONFINITE_EVER = 2, CMS_NONFINITE = 4, CMS_COMPRESSED = 8;    // record flags
static_assert(CMS_MAX_PUSH % CMP_CHUNK == 0, "blocks of a push");
static_assert(CMS_MAX_BLOCKS <= 2 * CMS_LANES, "the chain wave stages two chunks per lane");

struct CmsHeader {
    long long n;                                    // samples of the stream so far (since the last flush)
    uint32_t peak_in_run, peak_out_run, gmin_run;   // bits of max |x|, max |y|, min g over the stream's finite samples so far
    uint32_t acc_in, acc_out, acc_gmin;             // ... over this push's: integer extrema by the full pass, reset by the commit
    int32_t acc_flags, ever;                        // CMS_NONFINITE of this push; of the stream so far
    int32_t parity, magic;
    int32_t pad[4];
};
static_assert(sizeof(CmsHeader) == 64, "state header");

struct CmsOpen {
    double pstart, estart;
};
static_assert(sizeof(CmsOpen) == 16, "open chunk");

struct CmsRecord {              // gsv_cmpstream_record
    int32_t emitted;            // samples this push wrote to `out`: the next stage's n_dev
    int32_t flags;
    float peak_in, peak_out;    // max |x|, max |y| over the finite samples of this push (0 for none)
    float min_gain;             // the smallest g (makeup excluded) among them as fp32 (1 for none)
    float peak_in_run, peak_out_run, min_gain_run;      // ... of the stream so far
    long long total;            // samples of the stream so far (this push included; a flush reports the stream's length)
};
static_assert(sizeof(CmsRecord) == 40, "record");

LOUD_HD size_t cms_design_off() { return sizeof(CmsHeader); }
LOUD_HD size_t cms_open_off() { return cms_design_off() + loud_align16(sizeof(CmpDesign)); }
LOUD_HD size_t cms_stash_off() { return cms_open_off() + sizeof(CmsOpen); }
LOUD_HD size_t cms_scratch_off() { return cms_stash_off() + 2 * (size_t)CMP_CHUNK * sizeof(float); }
LOUD_HD size_t cms_state_bytes() { return cms_scratch_off() + loud_align16((size_t)(CMS_MAX_BLOCKS + 1) * sizeof(CmpChunk)); }

struct CmsPlan {
    long long N0, N1;           // samples of the stream before and after this push
    long long k0;               // the open chunk: the first one this push touches
    int nb, done;               // chunks the push touches (k0 .. k0 + nb - 1); chunks it completes (k0 .. k0 + done - 1)
};

LOUD_HD CmsPlan cms_plan(long long seen, long long n) {
    CmsPlan p;
    p.N0 = seen;
    p.N1 = seen + n;
    p.k0 = seen / CMP_CHUNK;
    p.nb = n > 0 ? (int)((p.N1 - 1) / CMP_CHUNK - p.k0) + 1 : 0;
    p.done = (int)(p.N1 / CMP_CHUNK - p.k0);
    return p;
}

LOUD_HD int cms_clamp(int v, int n_cap) { return v < 0 ? 0 : v > n_cap ? n_cap : v; }
LOUD_HD bool cms_finite(float x) { return loud_abs_bits(x) < 0x7F800000u; }

// sample s of the stream as it came, for a block on chunk `lo / CMP_CHUNK`: from the stash in front of this push, else from the chunk
LOUD_HD float cms_raw(const float* stash_old, const float* chunk, long long N0, long long lo, long long s) {
    return s < N0 ? stash_old[s - lo] : chunk[s - N0];
}

// ... and as it enters the detector
LOUD_HD float cms_enter(float raw) { return cms_finite(raw) ? raw : 0.f; }

// the record of a push and the header behind it (the open chunk's states are the caller's: scratch[done], or zero behind a flush)
LOUD_HD CmsRecord cms_finish(CmsHeader& h, const CmsPlan& pl, bool flush) {
    CmsRecord r;
    const uint32_t pin = h.acc_in > h.peak_in_run ? h.acc_in : h.peak_in_run;
    const uint32_t pout = h.acc_out > h.peak_out_run ? h.acc_out : h.peak_out_run;
    const uint32_t gmin = h.acc_gmin < h.gmin_run ? h.acc_gmin : h.gmin_run;
    const int32_t ever = h.ever | (h.acc_flags & CMS_NONFINITE);
    r.emitted = (int32_t)(pl.N1 - pl.N0);
    r.peak_in = loud_from_bits(h.acc_in);
    r.peak_out = loud_from_bits(h.acc_out);
    r.min_gain = loud_from_bits(h.acc_gmin);
    r.peak_in_run = loud_from_bits(pin);
    r.peak_out_run = loud_from_bits(pout);
    r.min_gain_run = loud_from_bits(gmin);
    r.flags = CMS_STREAM | (h.acc_flags & CMS_NONFINITE) | (ever ? CMS_NONFINITE_EVER : 0) | (r.min_gain < 1.f ? CMS_COMPRESSED : 0);
    r.total = pl.N1;
    h.n = flush ? 0 : pl.N1;
    h.peak_in_run = flush ? 0u : pin;
    h.peak_out_run = flush ? 0u : pout;
    h.gmin_run = flush ? CMP_ONE_BITS : gmin;
    h.ever = flush ? 0 : ever;
    h.acc_in = 0; h.acc_out = 0; h.acc_gmin = CMP_ONE_BITS; h.acc_flags = 0;
    if (pl.N1 > pl.N0) h.parity = 1 - h.parity;
    return r;
}

LOUD_HD CmsRecord cms_bad_record() {
    CmsRecord r;
    r.emitted = 0; r.flags = -1;
    r.peak_in = r.peak_out = r.peak_in_run = r.peak_out_run = 0.f;
    r.min_gain = r.min_gain_run = 1.f;
    r.total = 0;
    return r;
}

// ------------------------------------------------------------------------------------------------------------------
// host only
// ------------------------------------------------------------------------------------------------------------------
inline void cms_init_host(unsigned char* state, const CmpParams& d) {
    memset(state, 0, cms_state_bytes());
    CmsHeader h;
    memset(&h, 0, sizeof h);
    h.magic = CMS_MAGIC;
    h.gmin_run = h.acc_gmin = CMP_ONE_BITS;
    memcpy(state, &h, sizeof h);
    cmp_design(d, reinterpret_cast<CmpDesign*>(state + cms_design_off()));
}

// one push over host memory: the serial twin of the six launches.  out holds n floats and may be the chunk.
inline void cms_push_host(unsigned char* state, const float* chunk, int n, bool flush, float* out, CmsRecord* rec) {
    CmsHeader h;
    memcpy(&h, state, sizeof h);
    if (h.magic != CMS_MAGIC) {         // not a state cms_init_host made: nothing is read through it
        *rec = cms_bad_record();
        return;
    }
    const CmpDesign& D = *reinterpret_cast<const CmpDesign*>(state + cms_design_off());
    CmsOpen* open = reinterpret_cast<CmsOpen*>(state + cms_open_off());
    float* stash = reinterpret_cast<float*>(state + cms_stash_off());
    const float* stash_old = stash + (size_t)h.parity * CMP_CHUNK;
    float* stash_new = stash + (size_t)(1 - h.parity) * CMP_CHUNK;
    CmpChunk* ch = reinterpret_cast<CmpChunk*>(state + cms_scratch_off());
    const CmsPlan pl = cms_plan(h.n, n);
    const long long N0 = pl.N0, lo0 = pl.k0 * CMP_CHUNK;        // a sample in front of N0 lies in chunk k0: the stash's
    const auto raw = [&](long long s) { return cms_raw(stash_old, chunk, N0, lo0, s); };
    cmp_drive_host(D, lo0, pl.done, open->pstart, open->estart, ch, [&](long long s) { return cms_enter(raw(s)); });
    // the full pass: the outputs of the samples at or behind N0, the three statistics' bits, the flags, and over the chunk left
    // open its input as it came
    for (int b = 0; b < pl.nb; ++b) {
        const long long lo = lo0 + (long long)b * CMP_CHUNK;
        const bool left_open = lo + CMP_CHUNK > pl.N1;
        double carry[3] = {0.0, ch[b].pstart, ch[b].estart};
        cmp_walk_host(
            D, 2, lo, left_open ? pl.N1 : lo + CMP_CHUNK, carry,
            [&](long long s) {
                const float r = raw(s);
                if (left_open) stash_new[s - lo] = r;
                if (s >= N0) {
                    const uint32_t a = loud_abs_bits(r);
                    if (!cms_finite(r)) h.acc_flags |= CMS_NONFINITE;
                    else if (a > h.acc_in) h.acc_in = a;
                }
                return cms_enter(r);
            },
            [&](long long s, double g) {
                if (s < N0) return;                     // emitted by an earlier push
                float o = chunk[s - N0];                // out may be the chunk: read before the write
                if (cms_finite(o)) {
                    o = cmp_out(D.M, g, o);
                    const uint32_t a = loud_abs_bits(o), gb = loud_abs_bits((float)g);
                    if (a > h.acc_out) h.acc_out = a;
                    if (gb < h.acc_gmin) h.acc_gmin = gb;
                }
                out[s - N0] = o;
            });
    }
    open->pstart = flush ? 0.0 : ch[pl.done].pstart;
    open->estart = flush ? 0.0 : ch[pl.done].estart;
    *rec = cms_finish(h, pl, flush);
    memcpy(state, &h, sizeof h);
}

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------------------------------
// the device kernels
// ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int cms_len_dev(const int32_t* n_dev, int n_cap) { return n_dev ? cms_clamp(*n_dev, n_cap) : n_cap; }

// cmp_kernel for a push: one block per chunk of the stream that the push touches, block b on chunk k0 + b.  PASS 0 and 1 run over
// the chunks the push completes and write their scratch fields alone; PASS 2 runs over all it touches from the true start states:
// the outputs of the push's own samples, the three statistics, the flags, and -- the block of the chunk left open -- the chunk's
// input so far into the other stash.  The block's frame is compressor.h's: cmp_open, per span cmp_body between the barriers
// cmp_span states, cmp_close.  The kernel's own: the runs are staged as they came (cms_raw, into cmp_slot); the thread that owns a
// run then zeroes what is not finite in it (its own slots, which no other thread reads before the barrier behind cmp_body) and
// tells cmp_body which of its samples count: inside the span, at or behind N0, finite.
// chunk and out may be one buffer: a block reads a span (and stashes it) before it writes the span's outputs, and no block reads
// another block's samples.
template <int PASS>
static __global__ __launch_bounds__(CMP_T) void cms_kernel(unsigned char* state, const float* chunk, int n_cap, const int32_t* n_dev, float* out) {
    __shared__ float xs[CMP_T * (CMP_R + 1)];
    __shared__ double sc[2][2][CMP_T];
    __shared__ double carry_s[3];
    __shared__ uint32_t stat_s[3];
    __shared__ int flags_s;
    const CmsHeader h = *reinterpret_cast<const CmsHeader*>(state);
    if (h.magic != CMS_MAGIC) return;           // not a state gsv_cmpstream_init made: nothing is read through it
    const CmsPlan pl = cms_plan(h.n, cms_len_dev(n_dev, n_cap));
    const int tid = threadIdx.x, blk = blockIdx.x;
    if (blk >= (PASS < 2 ? pl.done : pl.nb) || blk >= CMS_MAX_BLOCKS) return;      // block-uniform
    const CmpDesign* __restrict__ D = reinterpret_cast<const CmpDesign*>(state + cms_design_off());
    float* stash = reinterpret_cast<float*>(state + cms_stash_off());
    const float* stash_old = stash + (size_t)h.parity * CMP_CHUNK;
    float* stash_new = stash + (size_t)(1 - h.parity) * CMP_CHUNK;
    CmpChunk* ch = reinterpret_cast<CmpChunk*>(state + cms_scratch_off()) + blk;
    const long long N0 = pl.N0;
    const long long lo = (pl.k0 + blk) * CMP_CHUNK, chunk_hi = lo + CMP_CHUNK;
    const long long hi = chunk_hi < pl.N1 ? chunk_hi : pl.N1;
    const bool left_open = PASS == 2 && chunk_hi > pl.N1;
    cmp_open<PASS>(stat_s, carry_s, ch);
    if (tid == 0) flags_s = 0;
    uint32_t peak_in = 0, peak_out = 0, gmin = CMP_ONE_BITS;
    int flags = 0;
    float* mine = xs + tid * (CMP_R + 1);
    for (long long s0 = lo; s0 < hi; s0 += CMP_SPAN) {
        const int cnt = hi - s0 < CMP_SPAN ? (int)(hi - s0) : CMP_SPAN;
        uint32_t nf = 0;                // bit j: sample tid + j CMP_T of the span is this push's and not finite
#pragma unroll
        for (int j = 0; j < CMP_R; ++j) {
            const int k = tid + j * CMP_T;
            float xv = 0.f;
            if (k < cnt) {
                const long long s = s0 + k;
                xv = cms_raw(stash_old, chunk, N0, lo, s);
                if (left_open) stash_new[s - lo] = xv;
                if (PASS == 2 && s >= N0) {
                    const uint32_t a = loud_abs_bits(xv);
                    if (!cms_finite(xv)) nf |= 1u << j;
                    else peak_in = a > peak_in ? a : peak_in;
                }
            }
            xs[cmp_slot(k)] = xv;
        }
        __syncthreads();                // xs, and carry_s of the last span (or of cmp_open)
        uint32_t own_nf = 0;            // bit i: sample i of this thread's run is not finite
#pragma unroll
        for (int i = 0; i < CMP_R; ++i) {
            const float raw = mine[i];
            if (!cms_finite(raw)) {
                own_nf |= 1u << i;
                mine[i] = cms_enter(raw);
            }
        }
        const int r0 = tid * CMP_R;
        cmp_body<PASS>(D, mine, sc, carry_s, cmp_run_bits(cnt - r0) & ~cmp_run_bits(N0 - s0 - r0) & ~own_nf, peak_out, gmin);
        if (PASS == 2) {
            __syncthreads();
#pragma unroll
            for (int j = 0; j < CMP_R; ++j) {
                const int k = tid + j * CMP_T;
                const long long s = s0 + k;
                if (k < cnt && s >= N0) {       // what an earlier push emitted is not written again
                    // not finite: copied bit for bit (in place: still the sample as it came)
                    out[s - N0] = nf >> j & 1u ? chunk[s - N0] : xs[cmp_slot(k)];
                }
            }
            if (nf) flags |= CMS_NONFINITE;
        }
        __syncthreads();        // the next span stages over xs and sc; carry_s is whole
    }
    if (PASS == 2 && flags) atomicOr(&flags_s, flags);
    if (!cmp_close<PASS>(carry_s, ch, stat_s, peak_in, peak_out, gmin)) return;
    CmsHeader* hd = reinterpret_cast<CmsHeader*>(state);
    if (tid == 0) {             // integer extrema: the order of the chunks does not show
        if (stat_s[0]) atomicMax(&hd->acc_in, stat_s[0]);
        if (stat_s[1]) atomicMax(&hd->acc_out, stat_s[1]);
        if (stat_s[2] < CMP_ONE_BITS) atomicMin(&hd->acc_gmin, stat_s[2]);
        if (flags_s) atomicOr(&hd->acc_flags, flags_s);
    }
}

// between the passes: one wave chains the chunks the push completes from the open chunk's kept state (cmp_chain_walk, one round)
// -> the start state of every chunk the push touches, scratch[0 .. done].  STAGE 0: pstart from (B, C); STAGE 1: estart from eend.
template <int STAGE>
static __global__ __launch_bounds__(CMS_LANES) void cms_chain_kernel(unsigned char* state, int n_cap, const int32_t* n_dev) {
    __shared__ CmpChunk in_s[2 * CMS_LANES];
    __shared__ double out_s[2 * CMS_LANES];
    const CmsHeader h = *reinterpret_cast<const CmsHeader*>(state);
    if (h.magic != CMS_MAGIC) return;
    const CmsPlan pl = cms_plan(h.n, cms_len_dev(n_dev, n_cap));
    const int done = pl.done < CMS_MAX_BLOCKS ? pl.done : CMS_MAX_BLOCKS;
    const CmpDesign* __restrict__ D = reinterpret_cast<const CmpDesign*>(state + cms_design_off());
    const CmsOpen* open = reinterpret_cast<const CmsOpen*>(state + cms_open_off());
    CmpChunk* ch = reinterpret_cast<CmpChunk*>(state + cms_scratch_off());
    const int lane = threadIdx.x;
    for (int b = lane; b < done; b += CMS_LANES) {
        if (STAGE == 0) { in_s[b].B = ch[b].B; in_s[b].C = ch[b].C; }
        else in_s[b].eend = ch[b].eend;
    }
    __syncthreads();
    if (lane == 0) {
        cmp_chain_walk(STAGE == 0 ? D->JR : D->JA, STAGE, STAGE == 0 ? open->pstart : open->estart, done + 1, done,
                       [&](int b) -> const CmpChunk& { return in_s[b]; }, [&](int b, double st) { out_s[b] = st; });
    }
    __syncthreads();
    for (int b = lane; b <= done; b += CMS_LANES) {
        if (STAGE == 0) ch[b].pstart = out_s[b];
        else ch[b].estart = out_s[b];
    }
}

// last, one wave: the record, the states of the chunk now open, the header.  Every lane has read the header before the barrier;
// one rewrites it behind it.
static __global__ __launch_bounds__(CMS_LANES) void cms_commit_kernel(unsigned char* state, int n_cap, const int32_t* n_dev, int flush,
                                                                      CmsRecord* __restrict__ rec) {
    CmsHeader h = *reinterpret_cast<const CmsHeader*>(state);
    const int lane = threadIdx.x;
    if (h.magic != CMS_MAGIC) {
        if (lane == 0) *rec = cms_bad_record();
        return;
    }
    const CmsPlan pl = cms_plan(h.n, cms_len_dev(n_dev, n_cap));
    const int done = pl.done < CMS_MAX_BLOCKS ? pl.done : CMS_MAX_BLOCKS;
    __syncthreads();
    if (lane == 0) {
        const CmpChunk* ch = reinterpret_cast<const CmpChunk*>(state + cms_scratch_off()) + done;
        CmsOpen* open = reinterpret_cast<CmsOpen*>(state + cms_open_off());
        open->pstart = flush ? 0.0 : ch->pstart;
        open->estart = flush ? 0.0 : ch->estart;
        *rec = cms_finish(h, pl, flush != 0);
        *reinterpret_cast<CmsHeader*>(state) = h;
    }
}
#endif

}  // namespace gsv
