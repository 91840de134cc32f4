// sv: the speaker-verification side of the reference-audio path on the device, what TTS.cache_spk_audio runs for v2Pro /
// v2ProPlus (gsv_tts/TTS.py:1346-1389, 1591-1610; GPT_SoVITS/SV/{sv.py, ERes2NetV2.py, fusion.py}), fp32 throughout:
//   resample   torchaudio.transforms.Resample(orig, new) defaults: sinc_interp_hann, lowpass_filter_width 6, rolloff
//              0.99; the polyphase kernel table evaluated in fp64, stored fp32; one output sample per thread
//   fbank      torchaudio.compliance.kaldi.fbank(num_mel_bins=80, sample_frequency=16000, dither=0): 400-sample frames
//              every 160 (snip_edges), DC removal, pre-emphasis 0.97, Povey window, |rfft 512|^2, 80 mel filters
//              20..8000 Hz, log(max(e, FLT_EPSILON)).  The DFT and the mel filter bank are refaudio.h's fgemm.
//   forward3   ERes2NetV2(baseWidth 24, scale 4, expansion 4).forward3: stem conv + BN + ReLU, 4 stages of Res2Net
//              blocks (AFF fusion in stages 3-4), layer3_ds, fuse34 AFF, mean over time of fuse34.flatten(1, 2)
//
// Every conv is sv_conv_kernel: an implicit GEMM on fp32 MFMA (v_mfma_f32_32x32x2_f32) over channels-last activations
// zero-padded by one pixel on every side, [F + 2][T + 2][C], so a 3x3 conv reads, per output pixel, three rows of 3*C
// contiguous values (or nine of C when the input is a channel slice of a wider buffer) and no im2col copy exists.  BN is
// folded into the weights and a bias at finalize.  A second input source serves Res2Net's sp + spx[i] (summed in the
// prologue) and AFF's cat(x, y) (a second K range); the output goes through a channel slice, so torch.cat is no copy.
// Nothing uses atomics or scratch: every sum has a fixed order, so a call is bit-reproducible.
// Batches (gsv_sv_forward_batch / gsv_sv_embed_batch) run each conv once for all clips: every clip keeps its own padded
// images, sv_conv_batch_kernel takes the clip as grid z and shares sv_conv_kernel's tile, so a clip's embedding is
// bit-identical to its single-clip call.
#pragma once
#include "refaudio.h"

namespace gsv {

// ---- resample ----------------------------------------------------------------------------------------------------
// torchaudio.functional.functional._get_sinc_resample_kernel for gcd-reduced orig / new: K[p][i], p < new,
// i < 2 * width + orig.  The phase offset -p / new is an fp32 division (torch divides the int64 arange in the default
// dtype) before it joins the fp64 index.
static __global__ void sv_resample_table_kernel(float* __restrict__ K, int orig, int nw, int width) {
    const int L = 2 * width + orig;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nw * L) return;
    const int p = i / L, q = i % L;
    const double base = (double)min(orig, nw) * 0.99;
    double t = (double)((float)(-p) / (float)nw) + (double)(q - width) / (double)orig;
    t *= base;
    t = fmin(fmax(t, -6.0), 6.0);
    const double c = cos(t * M_PI / 6.0 / 2.0);
    const double window = c * c;
    t *= M_PI;
    const double k = t == 0.0 ? 1.0 : sin(t) / t;
    K[i] = (float)(k * (window * (base / (double)orig)));
}

// y[j * new + p] = sum_i xpad[j * orig + i] K[p][i], xpad = x zero-padded by width in front; n_out = ceil(new n / orig)
static __global__ void sv_resample_kernel(const float* __restrict__ x, int n, const float* __restrict__ K, int orig, int nw,
                                          int width, float* __restrict__ y, int n_out) {
    const int o = blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= n_out) return;
    const int L = 2 * width + orig;
    const int j = o / nw, p = o % nw;
    const long long s0 = (long long)j * orig - width;
    const float* kr = K + (long long)p * L;
    float acc = 0.f;
    for (int i = 0; i < L; ++i) {
        const long long s = s0 + i;
        if (s >= 0 && s < n) acc += x[s] * kr[i];
    }
    y[o] = acc;
}

// ---- fbank -------------------------------------------------------------------------------------------------------
constexpr int FB_WIN = 400, FB_HOP = 160, FB_NFFT = 512, FB_BINS = FB_NFFT / 2 + 1, FB_MELS = 80;

// one block (256 threads) per frame: mean over the 400 samples (fixed tree), x - mean, pre-emphasis with the first
// sample replicated, Povey window hann(400, periodic=False)^0.85, zeros to 512 -> fr [frames][512]
static __global__ __launch_bounds__(256) void sv_frames_kernel(const float* __restrict__ x, float* __restrict__ fr) {
    __shared__ float red[256];
    __shared__ float xs[FB_WIN];
    const int f = blockIdx.x, tid = threadIdx.x;
    const float* src = x + (long long)f * FB_HOP;
    float s = 0.f;
    for (int i = tid; i < FB_WIN; i += 256) {
        xs[i] = src[i];
        s += xs[i];
    }
    red[tid] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) red[tid] += red[tid + w];
        __syncthreads();
    }
    const float mean = red[0] / (float)FB_WIN;
    float* out = fr + (long long)f * FB_NFFT;
    for (int i = tid; i < FB_NFFT; i += 256) {
        float v = 0.f;
        if (i < FB_WIN) {
            const float cur = xs[i] - mean, prev = xs[i > 0 ? i - 1 : 0] - mean;
            const double h = 0.5 - 0.5 * cospi(2.0 * i / (FB_WIN - 1));
            v = (cur - 0.97f * prev) * (float)pow(h, 0.85);
        }
        out[i] = v;
    }
}

// D[2j][k] = cos(2 pi j k / 512), D[2j+1][k] = -sin(2 pi j k / 512), j < 257 (the window is applied in the framing)
static __global__ void sv_dft_kernel(float* __restrict__ D) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= FB_BINS * FB_NFFT) return;
    const int k = i % FB_NFFT, j = i / FB_NFFT;
    const double ang = 2.0 * ((j * k) % FB_NFFT) / FB_NFFT;
    D[(2 * j) * FB_NFFT + k] = (float)cospi(ang);
    D[(2 * j + 1) * FB_NFFT + k] = (float)(-sinpi(ang));
}

// kaldi get_mel_banks (vtln off) in fp64: triangles on the mel scale 1127 ln(1 + f / 700) between 20 Hz and 8000 Hz over
// the FFT bins k * 31.25 Hz, k < 256; the Nyquist column (k = 256) is zero.  M [80][257]
static __global__ void sv_mel_kernel(float* __restrict__ M) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= FB_MELS * FB_BINS) return;
    const int b = i / FB_BINS, k = i % FB_BINS;
    float v = 0.f;
    if (k < FB_NFFT / 2) {
        const double lo = 1127.0 * log(1.0 + 20.0 / 700.0), hi = 1127.0 * log(1.0 + 8000.0 / 700.0);
        const double d = (hi - lo) / (FB_MELS + 1);
        const double l = lo + b * d, c = lo + (b + 1.0) * d, r = lo + (b + 2.0) * d;
        const double mel = 1127.0 * log(1.0 + (16000.0 / FB_NFFT) * k / 700.0);
        const double up = (mel - l) / (c - l), down = (r - mel) / (r - c);
        v = (float)fmax(0.0, fmin(up, down));
    }
    M[i] = v;
}

// P[t][j] = re^2 + im^2 of Z [t][2j, 2j+1]
static __global__ void sv_power_kernel(const float* __restrict__ Z, int T, float* __restrict__ P) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)T * FB_BINS) return;
    const long long t = i / FB_BINS;
    const int j = (int)(i % FB_BINS);
    const float re = Z[t * 2 * FB_BINS + 2 * j], im = Z[t * 2 * FB_BINS + 2 * j + 1];
    P[i] = re * re + im * im;
}

static __global__ void sv_log_kernel(const float* __restrict__ E, long long n, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = logf(fmaxf(E[i], 1.1920928955078125e-07f));
}

// ---- ERes2NetV2 ----------------------------------------------------------------------------------------------------
// fbank feats [T][F] -> the stem's input, zero-padded single-channel [F + 2][T + 2]
static __global__ void sv_feat_pad_kernel(const float* __restrict__ feat, int T, int F, float* __restrict__ P) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)T * F) return;
    const long long t = i / F;
    const int f = (int)(i % F);
    P[(long long)(f + 1) * (T + 2) + t + 1] = feat[i];
}

enum { SV_ACT_NONE = 0, SV_ACT_RELU = 1, SV_ACT_HTANH = 2, SV_ACT_SILU = 3, SV_ACT_AFF = 4 };
enum { SV_SRC_ONE = 0, SV_SRC_ADD = 1, SV_SRC_CAT = 2 };

struct SvConvArgs {
    const float* X1;       // input at channel offset 0 of its slice; padded [Fi + 2][Ti + 2][ldx]
    const float* X2;       // SV_SRC_ADD: X1 + X2 elementwise; SV_SRC_CAT: channels [Cin, 2 Cin) of the K range (1x1 only)
    int src, ldx, Tpi, Cin, k, s;
    const float* W;        // [N][nsrc][k][k][Cin], BN folded
    const float* bias;     // [N]
    float* Y; int ldy;     // output slice, padded [Fo + 2][To + 2][ldy]
    int Fo, To, N;
    const float* R; int ldr;                    // residual added before the activation (same geometry as Y), or null
    const float* A; int lda; const float* B; int ldb;   // SV_ACT_AFF: Y = A a + B (2 - a), a = 1 + tanh(conv + bias)
    int act;
};

__device__ __forceinline__ float sv_act(float v, int act) {
    if (act == SV_ACT_RELU) return fmaxf(v, 0.f);
    if (act == SV_ACT_HTANH) return fminf(fmaxf(v, 0.f), 20.f);
    if (act == SV_ACT_SILU) return v / (1.f + expf(-v));
    return v;
}

// one (32 WM) x (32 WN) output tile per block, 4 waves of 32 x 32, K staged through LDS in chunks of 32.  The K range
// is walked as segments: each (source, kernel row) when the input is contiguous (ldx == Cin: k * Cin values in a row),
// else each (source, tap) of Cin values.  Staging: 8 rows x 32 k per pass.
constexpr int SV_KC = 32, SV_LD = SV_KC + 1;
template <int WM, int WN>
__device__ __forceinline__ void sv_conv_tile(const SvConvArgs& a) {
    constexpr int BM = 32 * WM, BN = 32 * WN, PM = BM / 8, PN = BN / 8;
    __shared__ float xs[BM * SV_LD];
    __shared__ float ws[BN * SV_LD];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm = wid / WN, wn = wid % WN;
    const int j = lane & 31, hf = lane >> 5;
    const int lr = tid >> 5, lc = tid & 31;
    const int M = a.Fo * a.To;
    const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
    const int off = 1 - a.k / 2;   // padded input: 3x3 pad 1 starts at the border, 1x1 at the interior
    long long rb[PM];
#pragma unroll
    for (int p = 0; p < PM; ++p) {
        const int m = m0 + lr + p * 8;
        if (m < M) {
            const int fo = m / a.To, to = m % a.To;
            rb[p] = ((long long)(fo * a.s + off) * a.Tpi + (to * a.s + off)) * a.ldx;
        } else {
            rb[p] = -1;
        }
    }
    const int nsrc = a.src == SV_SRC_CAT ? 2 : 1;
    const bool contig = a.ldx == a.Cin && a.src != SV_SRC_ADD;
    const int nseg = contig ? a.k : a.k * a.k, seglen = contig ? a.k * a.Cin : a.Cin;
    const int Kw = nsrc * a.k * a.k * a.Cin;
    fa16 acc;
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = 0.f;
    int wk0 = 0;
    for (int sidx = 0; sidx < nsrc; ++sidx) {
        const float* X = sidx ? a.X2 : a.X1;
        for (int seg = 0; seg < nseg; ++seg, wk0 += seglen) {
            const int df = contig ? seg : seg / a.k, dt = contig ? 0 : seg % a.k;
            const long long so = ((long long)df * a.Tpi + dt) * a.ldx;
            for (int c0 = 0; c0 < seglen; c0 += SV_KC) {
                const int c = c0 + lc;
                float xv[PM], wv[PN];
#pragma unroll
                for (int p = 0; p < PM; ++p) {
                    float v = 0.f;
                    if (rb[p] >= 0 && c < seglen) {
                        v = X[rb[p] + so + c];
                        if (a.src == SV_SRC_ADD) v += a.X2[rb[p] + so + c];
                    }
                    xv[p] = v;
                }
#pragma unroll
                for (int p = 0; p < PN; ++p) {
                    const int n = n0 + lr + p * 8;
                    wv[p] = (n < a.N && c < seglen) ? a.W[(long long)n * Kw + wk0 + c] : 0.f;
                }
                __syncthreads();
#pragma unroll
                for (int p = 0; p < PM; ++p) xs[(lr + p * 8) * SV_LD + lc] = xv[p];
#pragma unroll
                for (int p = 0; p < PN; ++p) ws[(lr + p * 8) * SV_LD + lc] = wv[p];
                __syncthreads();
#pragma unroll
                for (int kk = 0; kk < SV_KC; kk += 2) {
                    const float av = xs[(wm * 32 + j) * SV_LD + kk + hf];
                    const float bv = ws[(wn * 32 + j) * SV_LD + kk + hf];
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
                }
            }
        }
    }
    const int n = n0 + wn * 32 + j;
    if (n >= a.N) return;
    const float bn = a.bias[n];
    const int Tpo = a.To + 2;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int m = m0 + wm * 32 + (q & 3) + 8 * (q >> 2) + 4 * hf;
        if (m < M) {
            const int fo = m / a.To, to = m % a.To;
            const long long o = (long long)(fo + 1) * Tpo + to + 1;
            float v = acc[q] + bn;
            if (a.R) v += a.R[o * a.ldr + n];
            if (a.act == SV_ACT_AFF) {
                const float at = 1.f + tanhf(v);
                v = a.A[o * a.lda + n] * at + a.B[o * a.ldb + n] * (2.f - at);
            } else {
                v = sv_act(v, a.act);
            }
            a.Y[o * a.ldy + n] = v;
        }
    }
}

template <int WM, int WN>
__global__ __launch_bounds__(256) void sv_conv_kernel(SvConvArgs a) {
    sv_conv_tile<WM, WN>(a);
}

// a batch of clips, each with its own padded images in every buffer (never concatenated along T: a stride-2 conv would
// read across the separators): clip z's input image starts in_off[z] pixels into X1 / X2, its output image out_off[z]
// pixels into Y / R / A / B; Ti / To its frames.  F is the same for every clip.
struct SvClips {
    long long in_off[AUX_MAX_CLIPS], out_off[AUX_MAX_CLIPS];
    int Ti[AUX_MAX_CLIPS], To[AUX_MAX_CLIPS];
};

// blockIdx.z = clip; row tiles past the clip's Fo * To pixels exit.  The tile is sv_conv_kernel's, so every clip's
// output is bit-identical to its single-clip call.
template <int WM, int WN>
__global__ __launch_bounds__(256) void sv_conv_batch_kernel(SvConvArgs a, SvClips cl) {
    const int z = blockIdx.z;
    a.To = cl.To[z];
    a.Tpi = cl.Ti[z] + 2;
    if ((int)blockIdx.y * 32 * WM >= a.Fo * a.To) return;
    const long long io = cl.in_off[z], oo = cl.out_off[z];
    a.X1 += io * a.ldx;
    if (a.X2) a.X2 += io * a.ldx;
    a.Y += oo * a.ldy;
    if (a.R) a.R += oo * a.ldr;
    if (a.A) a.A += oo * a.lda;
    if (a.B) a.B += oo * a.ldb;
    sv_conv_tile<WM, WN>(a);
}

// emb[c * F + f] = (sum_t X[f][t][c]) / T over the padded [F + 2][T + 2][C] interior, t in order (forward3's
// fuse34.flatten(1, 2).mean(-1))
static __global__ void sv_mean_kernel(const float* __restrict__ X, int F, int T, int C, float* __restrict__ emb) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= F * C) return;
    const int c = i % C, f = i / C;
    const float* p = X + ((long long)(f + 1) * (T + 2) + 1) * C + c;
    float s = 0.f;
    for (int t = 0; t < T; ++t) s += p[(long long)t * C];
    emb[(long long)c * F + f] = s / (float)T;
}

// BN folding: Wf[o][tap][c] = W[o][c][tap] * sc[o], bf[o] = beta[o] + (cb[o] - mean[o]) * sc[o],
// sc = gamma / sqrt(var + eps); without BN (gamma null) sc = 1, beta = mean = 0; cb (the conv bias) may be null
static __global__ void sv_fold_kernel(const float* __restrict__ W, int cout, int cin, int taps, const float* __restrict__ gamma,
                                      const float* __restrict__ beta, const float* __restrict__ mean, const float* __restrict__ var,
                                      const float* __restrict__ cb, float eps, float* __restrict__ Wf, float* __restrict__ bf) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)cout * cin * taps) return;
    const int t = (int)(i % taps), c = (int)((i / taps) % cin), o = (int)(i / ((long long)taps * cin));
    const float sc = gamma ? gamma[o] / sqrtf(var[o] + eps) : 1.f;
    Wf[((long long)o * taps + t) * cin + c] = W[i] * sc;
    if (i % ((long long)cin * taps) == 0) {
        const float b = cb ? cb[o] : 0.f;
        bf[o] = gamma ? beta[o] + (b - mean[o]) * sc : b;
    }
}

}  // namespace gsv
