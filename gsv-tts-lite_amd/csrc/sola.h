// sola: the streaming splice of TTS._sola_algorithm (reference gsv_tts/TTS.py:1612-1627) on the device.
//
// A streamed utterance is vocoded chunk by chunk; consecutive chunks overlap by `overlap` samples.  The new chunk is slid over the
// previous chunk's tail by the offset (0 .. search_len) that maximises the normalised cross-correlation
//     corr[k] / sqrt(energy[k]),  corr[k] = sum_j chunk[k + j] * tail[j],  energy[k] = sum_j chunk[k + j]^2 + 1e-8
// (first maximum, torch.argmax's rule), then cross-faded over the overlap with alpha = linspace(0, 1, overlap).
//
// Two launches: (1) one block per candidate offset -- 321 blocks for the default search, every lane streams the tail and its window
// of the chunk with coalesced 4-byte loads, wave shuffles + one LDS meeting reduce the two sums; (2) a grid-stride pass in which
// every block re-derives the arg-max from the 321 scores (an L2-resident 1.3 KB read; cheaper than a third launch), block 0
// publishes it, and everyone writes out[i] = fade(i) for i < overlap, chunk[offset + i] behind it.
#pragma once
#include <hip/hip_runtime.h>

namespace gsv {

__device__ __forceinline__ float sola_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// score[k] for k = blockIdx.x.  Sums in a fixed order (lane-strided partials, xor-tree, waves in index order): reproducible.
static __global__ __launch_bounds__(256) void sola_score_kernel(const float* __restrict__ tail, const float* __restrict__ chunk, int overlap,
                                                                 float* __restrict__ score) {
    __shared__ float red[2][4];
    const int k = blockIdx.x, tid = threadIdx.x;
    float c = 0.f, e = 0.f;
    for (int j = tid; j < overlap; j += 256) {
        const float x = chunk[k + j];
        c = fmaf(x, tail[j], c);
        e = fmaf(x, x, e);
    }
    c = sola_wave_sum(c);
    e = sola_wave_sum(e);
    if ((tid & 63) == 0) { red[0][tid >> 6] = c; red[1][tid >> 6] = e; }
    __syncthreads();
    if (tid == 0) {
        const float cs = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
        const float es = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]) + 1e-8f;
        score[k] = cs / sqrtf(es);
    }
}

// torch.linspace(0, 1, n)[j] as torch computes it (symmetric halves: start + step * j below the middle, end - step * (n - 1 - j) above)
__device__ __forceinline__ float sola_alpha(int j, int n) {
    if (n == 1) return 0.f;
    const float step = 1.0f / (float)(n - 1);
    return j < n / 2 ? step * (float)j : 1.0f - step * (float)(n - 1 - j);
}

// arg-max over the scores by a block of NW waves, FIRST maximum (a NaN score -- silence against silence gives 0 / sqrt(1e-8) = 0,
// never NaN -- would lose every comparison and leave offset 0).  Every thread returns it.
template <int NW>
__device__ __forceinline__ int sola_first_max(const float* __restrict__ score, int n_off, float* bv, int* bi) {
    const int tid = threadIdx.x;
    float best = -INFINITY;
    int at = 0x7fffffff;
    for (int k = tid; k < n_off; k += NW * 64) {
        const float s = score[k];
        if (s > best) { best = s; at = k; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o, 64);
        const int oa = __shfl_xor(at, o, 64);
        if (ob > best || (ob == best && oa < at)) { best = ob; at = oa; }
    }
    if ((tid & 63) == 0) { bv[tid >> 6] = best; bi[tid >> 6] = at; }
    __syncthreads();
    best = bv[0]; at = bi[0];
#pragma unroll
    for (int w = 1; w < NW; ++w)
        if (bv[w] > best || (bv[w] == best && bi[w] < at)) { best = bv[w]; at = bi[w]; }
    return at == 0x7fffffff ? 0 : at;
}

// the cross-fade of one sample: two products and their sum, each rounded (never contracted into a fused multiply-add), so that every
// kernel that splices gives the same bits.  gsv_sola's bits are pinned by tests/test_hip_sola.py (the reference's golden samples within
// one fp32 rounding), gsv_stream_emit's to gsv_sola's by tests/test_hip_stream_emit.py.
__device__ __forceinline__ float sola_fade(float t, float v, float a) {
#pragma clang fp contract(off)
    const float p = t * (1.0f - a), q = v * a;
    return p + q;
}

static __global__ __launch_bounds__(256) void sola_splice_kernel(const float* __restrict__ tail, const float* __restrict__ chunk, int n, int overlap,
                                                                  const float* __restrict__ score, int n_off, float* __restrict__ out,
                                                                  int* __restrict__ offset_out) {
    __shared__ float bv[4];
    __shared__ int bi[4];
    const int tid = threadIdx.x;
    const int off = sola_first_max<4>(score, n_off, bv, bi);
    if (blockIdx.x == 0 && tid == 0) *offset_out = off;
    const int m = n - off;                                   // samples of the spliced chunk
    for (int i = blockIdx.x * 256 + tid; i < m; i += gridDim.x * 256) {
        float v = chunk[off + i];
        if (i < overlap) {
            const float a = sola_alpha(i, overlap);
            v = sola_fade(tail[i], v, a);
        }
        out[i] = v;
    }
}

// ---- the chunk epilogue of a stream (gsv_stream_emit): splice, keep the tail back, trim the head, append the mute -- what
// TTS.infer_stream does on the host between a chunk's decode and its hand-out, with no value read by the host in between.
//
// Three launches: sola_score_kernel (only with a tail), one DECIDE block, one COPY grid.  The decide block reads the scores and --
// on the first chunk of a segment only -- the spliced signal up to its first loud frame (at most 64 000 samples, by one block that
// stops at the hit: not a pass over the chunk); it leaves rec = {n_out, k, h, 0}.  The copy grid reads rec and writes `out` and
// `tail_out`; the spliced signal s is never stored, both kernels evaluate s[i] from the chunk and the tail (stream_emit_sample).
//
// Head rule (TTS._find_head_threshold_offsets, TTS.py:1629-1644): frames of 512 samples, hop 256, over the first
// L = min(len(body), 64000) samples; the first frame f with sqrtf(sum_sq / 512) > 0.02f gives h = max(0, 256 f - 3200); no such
// frame, or L < 512: h = L.  ORDER OF THE SUM: sum_sq(f) = H[f] + H[f + 1], H[j] the sum over the 256 samples from 256 j: lane l
// of one wave accumulates s[256 j + l + 64 t]^2 for t = 0, 1, 2, 3 in that order with fmaf, then the 64 lanes meet in the xor-tree
// of sola_wave_sum (strides 32, 16, ..., 1).
constexpr int kEmitWaves = 16;
constexpr int kHeadSearch = 64000, kHeadFrame = 512, kHeadHop = 256, kHeadMargin = 3200;

// s[i]: sample i of the spliced signal, the bits sola_splice_kernel writes (tail == nullptr: the chunk itself, k = 0)
__device__ __forceinline__ float stream_emit_sample(const float* __restrict__ tail, const float* __restrict__ chunk, int k, int overlap,
                                                    int i) {
    float v = chunk[k + i];
    if (tail != nullptr && i < overlap) v = sola_fade(tail[i], v, sola_alpha(i, overlap));
    return v;
}

static __global__ __launch_bounds__(kEmitWaves * 64) void stream_emit_decide_kernel(const float* __restrict__ tail,
                                                                                    const float* __restrict__ chunk, int n, int overlap,
                                                                                    const float* __restrict__ score, int n_off, int is_final,
                                                                                    int trim_head, int mute_samples, int* __restrict__ rec) {
    __shared__ float bv[kEmitWaves];
    __shared__ int bi[kEmitWaves];
    __shared__ float hsum[kEmitWaves + 1];      // hsum[0]: H of the half-frame before this round's, hsum[1 + w]: wave w's
    __shared__ int found;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int k = tail != nullptr ? sola_first_max<kEmitWaves>(score, n_off, bv, bi) : 0;
    const int m = n - k;
    const int body = is_final ? m : m - overlap;
    int h = 0;
    if (trim_head) {
        const int L = body < kHeadSearch ? body : kHeadSearch;
        const int F = L < kHeadFrame ? 0 : (L - kHeadFrame) / kHeadHop + 1;     // frames; they span half-frames 0 .. F
        if (tid == 0) { found = -1; hsum[kEmitWaves] = 0.f; }
        __syncthreads();
        for (int j0 = 0; F > 0 && j0 <= F; j0 += kEmitWaves) {
            if (tid == 0) hsum[0] = hsum[kEmitWaves];
            const int j = j0 + wave;
            float e = 0.f;
            if (j <= F) {
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const float x = stream_emit_sample(tail, chunk, k, overlap, kHeadHop * j + lane + 64 * t);
                    e = fmaf(x, x, e);
                }
            }
            e = sola_wave_sum(e);
            __syncthreads();                    // hsum[0] taken before hsum[kEmitWaves] is overwritten
            if (lane == 0) hsum[1 + wave] = e;
            __syncthreads();
            if (tid == 0) {
                for (int w = 0; w < kEmitWaves; ++w) {      // frame f = half-frames f and f + 1
                    const int f = j0 - 1 + w;
                    if (f >= 0 && f < F && sqrtf((hsum[w] + hsum[w + 1]) / (float)kHeadFrame) > 0.02f) { found = f; break; }
                }
            }
            __syncthreads();
            if (found >= 0) break;
        }
        const int f = found;
        h = f < 0 ? L : (kHeadHop * f > kHeadMargin ? kHeadHop * f - kHeadMargin : 0);
    }
    if (tid == 0) {
        rec[0] = body - h + (is_final ? mute_samples : 0);
        rec[1] = k;
        rec[2] = h;
        rec[3] = 0;
    }
}

// out = body[h:] (+ mute_samples zeros behind a final chunk), tail_out = s[m - overlap : m]
static __global__ __launch_bounds__(256) void stream_emit_copy_kernel(const float* __restrict__ tail, const float* __restrict__ chunk, int n,
                                                                       int overlap, int is_final, const int* __restrict__ rec,
                                                                       float* __restrict__ out, float* __restrict__ tail_out) {
    const int n_out = rec[0], k = rec[1], h = rec[2];
    const int m = n - k;
    const int keep = (is_final ? m : m - overlap) - h;      // samples of the body handed out; behind them the mute
    const int total = n_out + overlap;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
        if (i < keep) out[i] = stream_emit_sample(tail, chunk, k, overlap, h + i);
        else if (i < n_out) out[i] = 0.f;
        else tail_out[i - n_out] = stream_emit_sample(tail, chunk, k, overlap, m - overlap + (i - n_out));
    }
}

}  // namespace gsv
