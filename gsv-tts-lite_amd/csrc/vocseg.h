// vocseg: what SynthesizerTrn.decode does between enc_p and the flow (SoVITS/models.py:217-219, 402-404) -- the speed
// resampling of the projected statistics, the noise draw and the per-frame conditioning map -- as per-frame arithmetic
// (`__device__` functions, shared by the kernels of gsv_voc_decode in gsv_voc.hip) and as ONE launch over a time-concatenated
// batch whose utterances each have their own speed, noise scale and seed (gsv_voc_decode_segments).
//
// The segmented kernel runs one lane per (output frame, row): rows [0, C) write z_p (row 0 also writes the mask), the
// rows after them write the per-frame conditioning (gin rows; ONE row that copies the gin values when ge is broadcast).
// A lane finds its segment by a binary search over the running output offsets of the by-value table (at most 6 dependent
// loads from the kernel-argument segment, the same addresses for every row of a column of blocks), then reads only that segment's
// frames: both taps of the interpolation are clamped to the segment.  Consecutive lanes write consecutive frames of one
// row (coalesced stores); the loads of a lane pair are at most two neighbouring input frames.  No LDS, no atomics, no
// scratch, plain vector loads and stores.
#pragma once
#include <stdint.h>

#include "gsv_common.h"

namespace gsv {

constexpr int VOC_MAX_SEGMENTS = 64;    // GSV_VOC_MAX_SEGMENTS

__device__ __forceinline__ uint32_t dec_lowbias32(uint32_t h) {
    h ^= h >> 16; h *= 0x7feb352du; h ^= h >> 15; h *= 0x846ca68bu; h ^= h >> 16;
    return h;
}
// standard normal for element `i` of the stream `seed`: Box-Muller over two counter-based uniforms (lowbias32 of the element
// index mixed with the seed halves) -- replayable, no generator state; oracle.device_normal restates it
__device__ __forceinline__ float dec_normal(uint32_t seed_lo, uint32_t seed_hi, uint32_t i) {
    const uint32_t a = dec_lowbias32(dec_lowbias32(i * 0x9E3779B1u ^ seed_lo) + seed_hi);
    const uint32_t b = dec_lowbias32(dec_lowbias32(i * 0x85EBCA77u ^ seed_hi ^ 0x68E31DA4u) + seed_lo);
    const float u1 = ((float)(a >> 8) + 0.5f) * (1.0f / 16777216.0f);
    const float u2 = ((float)(b >> 8) + 0.5f) * (1.0f / 16777216.0f);
    return sqrtf(-2.0f * logf(u1)) * cosf(6.283185307179586f * u2);
}

// point j of the linear resampling of x[0 .. T_in) to T_out points, torch's F.interpolate(mode="linear", align_corners=False):
// src = (j + 0.5) * T_in / T_out - 0.5 clamped at 0, weights (1 - frac, frac), right neighbour clamped to T_in - 1
__device__ __forceinline__ float resample_linear_at(const float* __restrict__ x, int T_in, int T_out, int j) {
    const float scale = (float)T_in / (float)T_out;
    float src = ((float)j + 0.5f) * scale - 0.5f;
    if (src < 0.f) src = 0.f;
    const int i0 = min((int)src, T_in - 1), i1 = min(i0 + 1, T_in - 1);
    const float f = src - (float)i0;
    return (1.0f - f) * x[i0] + f * x[i1];
}

// z_p = m_p + N(0,1) * exp(logs_p) * noise_scale (models.py:404); `i` is the element's index in the noise stream
__device__ __forceinline__ float dec_zp_at(float m, float logs, float noise_scale, uint32_t seed_lo, uint32_t seed_hi, uint32_t i) {
    float v = m;
    v += dec_normal(seed_lo, seed_hi, i) * expf(logs) * noise_scale;
    return v;
}

// the input FRAME whose conditioning output frame j takes: x2 nearest (models.py:389), then F.interpolate(mode="nearest") of
// the T_in = 2 * tokens frames to T_out (models.py:402); the token column is this >> 1
__device__ __forceinline__ int dec_ge_frame_at(int j, int T_in, int T_out, int resized) {
    const float scale = (float)T_in / (float)T_out;
    return resized ? min((int)floorf((float)j * scale), T_in - 1) : j;
}

// the utterances of one gsv_voc_decode_segments call, by value in the kernel arguments: segment i reads input frames
// [in0[i], in0[i + 1]) and writes output frames [out0[i], out0[i + 1]); in0 is even (2 * the running token count)
struct VocSegs {
    int n;
    int in0[VOC_MAX_SEGMENTS + 1], out0[VOC_MAX_SEGMENTS + 1];
    float noise_scale[VOC_MAX_SEGMENTS];
    uint32_t seed_lo[VOC_MAX_SEGMENTS], seed_hi[VOC_MAX_SEGMENTS];
};

// grid (ceil(T_out / 256), C + (Tg == 1 ? 1 : gin)).  stats = [m_p | logs_p] [2C][T] of the whole concatenation;
// ge [gin][Tg], Tg == 1 or T / 2 -> z [C][T_out], mask [T_out] = 1, ge_fr [gin][T_out] (Tg == 1: [gin])
static __global__ __launch_bounds__(256) void dec_segments_kernel(const float* __restrict__ stats, int C, int T, VocSegs sg,
                                                                  const float* __restrict__ ge, int gin, int Tg,
                                                                  float* __restrict__ z, float* __restrict__ mask,
                                                                  float* __restrict__ ge_fr, int T_out) {
    const int j = blockIdx.x * 256 + threadIdx.x, row = blockIdx.y;
    if (row >= C && Tg == 1) {           // broadcast conditioning: copied once, by the blocks of this one row
        for (int g = j; g < gin; g += gridDim.x * 256) ge_fr[g] = ge[g];
        return;
    }
    if (j >= T_out) return;
    int lo = 0, hi = sg.n - 1;           // the last segment whose first output frame is <= j
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (sg.out0[mid] <= j) lo = mid; else hi = mid - 1;
    }
    const int s = sg.in0[lo], t_in = sg.in0[lo + 1] - s, o = sg.out0[lo], t_out = sg.out0[lo + 1] - o, jl = j - o;
    const int resized = t_out != t_in;
    if (row < C) {
        const float* m = stats + (size_t)row * T + s;
        const float* logs = stats + (size_t)(C + row) * T + s;
        float v = resized ? resample_linear_at(m, t_in, t_out, jl) : m[jl];
        const float ns = sg.noise_scale[lo];
        if (ns != 0.f)
            v = dec_zp_at(v, resized ? resample_linear_at(logs, t_in, t_out, jl) : logs[jl], ns, sg.seed_lo[lo], sg.seed_hi[lo],
                          (uint32_t)row * (uint32_t)t_out + (uint32_t)jl);
        z[(size_t)row * T_out + j] = v;
        if (row == 0) mask[j] = 1.0f;
    } else {
        const int g = row - C;
        ge_fr[(size_t)g * T_out + j] = ge[(size_t)g * Tg + ((s + dec_ge_frame_at(jl, t_in, t_out, resized)) >> 1)];
    }
}

}  // namespace gsv
