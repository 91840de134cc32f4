// wavpcm: the samples of a WAV file's data chunk -> fp32 mono, what TTS._load_audio (gsv_tts/TTS.py:1811-1823) gets from
// PyAV's av.AudioResampler(format='flt', layout='mono', rate=stream.rate), i.e. libswresample's sample conversions to
// flt and its default stereo -> mono rematrix.
//
//   u8    (x - 128) / 2^7          s16   x / 2^15          s24 (3 bytes, packed)   x / 2^23
//   s32   x / 2^31 (x rounded to fp32 first)               f32   as is             f64   cast to float
//
// Every scale is a power of two, so a mono sample is exact whatever the order of operations.  Stereo is mixed as
// L * g + R * g with g = WAV_STEREO_GAIN (sqrt(1/2)), both products rounded before the sum (no FMA): in fp32 for every
// format but f64, in fp64 for f64 and then cast, as libswresample mixes in its internal format (float planar, double
// planar for 8-byte input).  The byte buffer carries no alignment guarantee (an s24 frame is 3 or 6 bytes, a clip of a
// packed upload starts anywhere), so each lane assembles its frame from byte loads; one lane per output sample, plain
// vector stores.  (A byte load run may be merged into wider loads by the compiler: global memory takes unaligned
// loads on gfx950.)
#pragma once
#include "refaudio.h"

namespace gsv {

enum WavFormat { WAV_U8 = 0, WAV_S16 = 1, WAV_S24 = 2, WAV_S32 = 3, WAV_F32 = 4, WAV_F64 = 5, WAV_N_FORMATS = 6 };

__host__ __device__ constexpr int wav_sample_bytes(int fmt) {
    return fmt == WAV_U8 ? 1 : fmt == WAV_S16 ? 2 : fmt == WAV_S24 ? 3 : fmt == WAV_F64 ? 8 : 4;
}

// libswresample's default stereo -> mono coefficient for float output (no renormalisation of the matrix); see DESIGN
// 4.15 for how far it is verified
constexpr double WAV_STEREO_GAIN = 0.70710678118654752440;

// the clips of one call, by value in the kernel arguments: clip z reads n[z] frames of ch[z] channels of format fmt[z]
// from byte off[z] and writes out0[z] .. out0[z] + n[z]
struct WavClips {
    long long off[AUX_MAX_CLIPS], out0[AUX_MAX_CLIPS];
    int n[AUX_MAX_CLIPS];
    short fmt[AUX_MAX_CLIPS], ch[AUX_MAX_CLIPS];
};

__device__ __forceinline__ unsigned long long wav_le(const unsigned char* __restrict__ p, int nbytes) {
    unsigned long long v = 0;
    for (int b = 0; b < nbytes; ++b) v |= (unsigned long long)p[b] << (8 * b);
    return v;
}

template <typename T>
__device__ __forceinline__ T wav_bits_as(unsigned long long v) {
    T x;
    __builtin_memcpy(&x, &v, sizeof(T));
    return x;
}

// one sample -> fp32 (f64: see wav_sample_d)
__device__ __forceinline__ float wav_sample_f(const unsigned char* __restrict__ p, int fmt) {
    switch (fmt) {
    case WAV_U8: return (float)((int)p[0] - 128) * (1.f / 128.f);
    case WAV_S16: return (float)wav_bits_as<short>(wav_le(p, 2)) * (1.f / 32768.f);
    case WAV_S24: return (float)((int)((unsigned)wav_le(p, 3) << 8) >> 8) * (1.f / 8388608.f);
    case WAV_S32: return (float)wav_bits_as<int>(wav_le(p, 4)) * (1.f / 2147483648.f);
    default: return wav_bits_as<float>(wav_le(p, 4));   // WAV_F32
    }
}

__device__ __forceinline__ double wav_sample_d(const unsigned char* __restrict__ p) { return wav_bits_as<double>(wav_le(p, 8)); }

// grid (frames of the longest clip / 256, clips): block (x, z) converts frames [256 x, 256 x + 256) of clip z
static __global__ __launch_bounds__(256) void wav_to_mono_kernel(const unsigned char* __restrict__ pcm, WavClips cl,
                                                                 float* __restrict__ out) {
#pragma clang fp contract(off)   // libswresample rounds both products before the sum
    const int z = blockIdx.y;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= cl.n[z]) return;
    const int fmt = cl.fmt[z], ch = cl.ch[z], sb = wav_sample_bytes(fmt);
    const unsigned char* p = pcm + cl.off[z] + t * (long long)(sb * ch);
    float y;
    if (fmt == WAV_F64) {
        if (ch == 1) {
            y = (float)wav_sample_d(p);
        } else {
            const double g = WAV_STEREO_GAIN;
            y = (float)(wav_sample_d(p) * g + wav_sample_d(p + 8) * g);
        }
    } else {
        y = wav_sample_f(p, fmt);
        if (ch == 2) {
            const float g = (float)WAV_STEREO_GAIN;
            y = y * g + wav_sample_f(p + sb, fmt) * g;
        }
    }
    out[cl.out0[z] + t] = y;
}

}  // namespace gsv
