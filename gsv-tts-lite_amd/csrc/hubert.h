// hubert: CN-HuBERT (transformers HubertModel, the chinese-hubert-base shapes) on the device, the model behind
// TTS._get_prompt (gsv_tts/TTS.py:1556-1570) -- prompt waveform (16 kHz) -> last_hidden_state, fp32 throughout.
//   feature encoder   conv 0 (k 10, stride 5, 1 -> C) + GroupNorm(C, C) over ALL frames + GELU, then convs 1..6
//                     (stride 2, GELU) as fgemm overlapping-row GEMMs on channels-last activations (refaudio.h)
//   projection        LayerNorm(C) + Linear C -> H
//   positional conv   Conv1d(H, H, k, padding k/2, groups G), weight norm over dims 0, 1 (folded at finalize), last
//                     output frame dropped, GELU, x + pos, encoder.layer_norm
//   12 post-LN layers x = LN(x + out_proj(attn(x))), x = LN(x + fc2(gelu(fc1(x))))
// The GEMMs are refaudio.h's fgemm_kernel; the kernels below are the pieces it does not cover.  None uses atomics:
// every reduction has a fixed order, so a call is bit-reproducible.
// Batches (gsv_hubert_forward_batch) pack the clips' frames as rows: fgemm has no K split and LayerNorm is per row, so
// packing keeps every sum as it is.  The positional conv and the attention take HubClips and never mix clips; the
// *_batch kernels share their tile bodies with the single-clip kernels, so a clip's output is bit-identical either way.
#pragma once
#include "refaudio.h"

namespace gsv {

// packed clips of one batch, by value in the kernel arguments: clip z holds rows [row0, row0 + T) of the packed
// activations and rows [prow0, prow0 + T + k - 1) of the group-major padded copy of the positional conv
struct HubClips {
    int n;
    int row0[AUX_MAX_CLIPS], prow0[AUX_MAX_CLIPS], T[AUX_MAX_CLIPS];
};

// ---- GroupNorm(C, C) of conv 0: per-channel statistics over every frame, in two deterministic passes.
// Pass 1: block (channel tile of 64, chunk of GN_ROWS frames) -> the chunk's mean and sum of squared deviations
// about that mean (two sweeps over the chunk, which stays in cache).
constexpr int GN_ROWS = 256;
static __global__ __launch_bounds__(256) void gn_partial_kernel(const float* __restrict__ x, int T, int C,
                                                                float* __restrict__ pmean, float* __restrict__ pm2) {
    __shared__ float red[4][64];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + tx;
    const int r0 = blockIdx.y * GN_ROWS, r1 = min(T, r0 + GN_ROWS);
    float s = 0.f;
    for (int r = r0 + ty; r < r1; r += 4) s += x[(long long)r * C + c];
    red[ty][tx] = s;
    __syncthreads();
    const float mean = (((red[0][tx] + red[1][tx]) + red[2][tx]) + red[3][tx]) / (float)(r1 - r0);
    __syncthreads();
    float m2 = 0.f;
    for (int r = r0 + ty; r < r1; r += 4) {
        const float d = x[(long long)r * C + c] - mean;
        m2 += d * d;
    }
    red[ty][tx] = m2;
    __syncthreads();
    if (ty == 0) {
        pmean[(long long)blockIdx.y * C + c] = mean;
        pm2[(long long)blockIdx.y * C + c] = ((red[0][tx] + red[1][tx]) + red[2][tx]) + red[3][tx];
    }
}

// Pass 2: one thread per channel merges the chunks in index order (Chan et al.'s pairwise update) ->
// mean[c], a[c] = gamma[c] / sqrt(var + eps) (biased variance, as nn.GroupNorm)
static __global__ void gn_finalize_kernel(const float* __restrict__ pmean, const float* __restrict__ pm2, int nchunk, int T,
                                          int C, const float* __restrict__ gamma, float eps, float* __restrict__ mean,
                                          float* __restrict__ scale) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    float n = 0.f, mu = 0.f, m2 = 0.f;
    for (int b = 0; b < nchunk; ++b) {
        const float nb = (float)min(GN_ROWS, T - b * GN_ROWS);
        const float mb = pmean[(long long)b * C + c], m2b = pm2[(long long)b * C + c];
        const float nn = n + nb, d = mb - mu;
        mu += d * (nb / nn);
        m2 += m2b + d * d * (n * nb / nn);
        n = nn;
    }
    mean[c] = mu;
    scale[c] = gamma[c] / sqrtf(m2 / (float)T + eps);
}

// in place: x[r][c] = gelu((x - mean[c]) * scale[c] + beta[c]); C % 4 == 0
static __global__ void gn_apply_gelu_kernel(float* __restrict__ x, long long n4, int C, const float* __restrict__ mean,
                                            const float* __restrict__ scale, const float* __restrict__ beta) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    float4 v = reinterpret_cast<float4*>(x)[i];
    const int c = (int)((i * 4) % C);
    v.x = gelu_f((v.x - mean[c + 0]) * scale[c + 0] + beta[c + 0]);
    v.y = gelu_f((v.y - mean[c + 1]) * scale[c + 1] + beta[c + 1]);
    v.z = gelu_f((v.z - mean[c + 2]) * scale[c + 2] + beta[c + 2]);
    v.w = gelu_f((v.w - mean[c + 3]) * scale[c + 3] + beta[c + 3]);
    reinterpret_cast<float4*>(x)[i] = v;
}

// ---- LayerNorm over rows of C = 64 * npl values (npl <= 16): one wave per row, the row held in registers, mean then
// variance about the mean (two passes, as torch).  In place allowed (y == x).
constexpr int LN_MAX_NPL = 16;
static __global__ __launch_bounds__(256) void ln_rows_kernel(const float* x, float* y, int rows, int C,
                                                             const float* __restrict__ g, const float* __restrict__ b, float eps) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const int npl = C >> 6;
    const float* xr = x + (long long)r * C;
    float v[LN_MAX_NPL];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < LN_MAX_NPL; ++i) {
        v[i] = i < npl ? xr[lane + 64 * i] : 0.f;
        s += v[i];
    }
    const float mean = wave_sum(s) / (float)C;
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < LN_MAX_NPL; ++i) {
        const float d = i < npl ? v[i] - mean : 0.f;
        ss += d * d;
    }
    const float rstd = 1.f / sqrtf(wave_sum(ss) / (float)C + eps);
    float* yr = y + (long long)r * C;
#pragma unroll
    for (int i = 0; i < LN_MAX_NPL; ++i)
        if (i < npl) {
            const int c = lane + 64 * i;
            yr[c] = (v[i] - mean) * rstd * g[c] + b[c];
        }
}

// ---- positional conv input: x [T][H] channels-last -> group-major, zero-padded P [G][T + k - 1][H / G] with k/2 zero
// frames in front, so that output frame t of group g is ONE row of k * (H/G) contiguous values at stride H/G.
static __global__ void pos_pad_group_kernel(const float* __restrict__ x, int T, int H, int G, int k, float* __restrict__ P) {
    const int cg = H / G, Tp = T + k - 1;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)G * Tp * cg) return;
    const int c = (int)(i % cg), p = (int)((i / cg) % Tp), g = (int)(i / ((long long)cg * Tp));
    const int t = p - k / 2;
    P[i] = (t >= 0 && t < T) ? x[(long long)t * H + g * cg + c] : 0.f;
}

// batched: blockIdx.y = clip; clip z's rows of x [rows][H] -> its own zero-haloed segment of P [G][Rp][H / G]
static __global__ void pos_pad_group_batch_kernel(const float* __restrict__ x, int H, int G, int k, long long Rp, HubClips cl,
                                                  float* __restrict__ P) {
    const int z = blockIdx.y, T = cl.T[z];
    const int cg = H / G, Tp = T + k - 1;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)G * Tp * cg) return;
    const int c = (int)(i % cg), p = (int)((i / cg) % Tp), g = (int)(i / ((long long)cg * Tp));
    const int t = p - k / 2;
    P[((long long)g * Rp + cl.prow0[z] + p) * cg + c] = (t >= 0 && t < T) ? x[(long long)(cl.row0[z] + t) * H + g * cg + c] : 0.f;
}

// ---- the positional conv as ONE launch over (row tile, group x K slice): block z = g * POS_SPLIT + s contracts the s-th
// slice of group g's k * (H/G) values (an fgemm tile over the padded group-major rows) into part[s][T][H]; pos_reduce
// then sums the slices in index order (deterministic) and applies bias, GELU and the residual.  Per-group launches left
// 3-9 blocks per launch walking K = 6144 alone.
constexpr int POS_SPLIT = 8;
// the tile (m0, n0) of block z over one clip: P its first padded row (group stride gstride floats), part its first
// output row (slice stride pstride floats), T its frames
__device__ __forceinline__ void pos_conv_tile(const float* __restrict__ P, long long gstride, const float* __restrict__ w,
                                              float* __restrict__ part, long long pstride, int T, int H, int G, int k, int z,
                                              int m0, int n0) {
    __shared__ float xs[64 * FG_LD];
    __shared__ float ws[64 * FG_LD];
    const int cg = H / G, Kt = k * cg;
    const int g = z / POS_SPLIT, sp = z % POS_SPLIT;
    const int k0 = (int)((long long)Kt * sp / POS_SPLIT), k1 = (int)((long long)Kt * (sp + 1) / POS_SPLIT);
    FGemmArgs a;
    a.X = P + g * gstride + k0; a.ldx = cg;
    a.W = w + (long long)g * cg * Kt + k0; a.ldw = Kt;
    a.Y = part + sp * pstride + g * cg; a.ldy = H;
    a.bias_n = nullptr; a.bias_m = nullptr; a.R = nullptr; a.ldr = 0;
    a.M = T; a.N = cg; a.K = k1 - k0; a.alpha = 1.f; a.act = 0;
    fgemm_tile(a, m0, n0, xs, ws);
}

static __global__ __launch_bounds__(256) void pos_conv_split_kernel(const float* __restrict__ P, const float* __restrict__ w,
                                                                    float* __restrict__ part, int T, int H, int G, int k) {
    const int cg = H / G, Tp = T + k - 1;
    pos_conv_tile(P, (long long)Tp * cg, w, part, (long long)T * H, T, H, G, k, blockIdx.z, blockIdx.y * 64, blockIdx.x * 64);
}

// batched: blockIdx.x = clip * column tiles + column tile (the clip is not in z, which G * POS_SPLIT already fills);
// row tiles past the clip's frames exit; P [G][Rp][H / G], part [POS_SPLIT][rows][H]
static __global__ __launch_bounds__(256) void pos_conv_split_batch_kernel(const float* __restrict__ P, long long Rp,
                                                                          const float* __restrict__ w, float* __restrict__ part,
                                                                          int rows, int H, int G, int k, HubClips cl) {
    const int cg = H / G, ntn = (cg + 63) / 64, z = blockIdx.x / ntn;
    const int T = cl.T[z];
    if ((int)blockIdx.y * 64 >= T) return;
    pos_conv_tile(P + (long long)cl.prow0[z] * cg, Rp * cg, w, part + (long long)cl.row0[z] * H, (long long)rows * H, T, H, G,
                  k, blockIdx.z, blockIdx.y * 64, (blockIdx.x % ntn) * 64);
}

// out[t][c] = hid[t][c] + gelu(bias[c] + sum_s part[s][t][c]), s in index order
static __global__ void pos_reduce_kernel(const float* __restrict__ part, long long n, int H, const float* __restrict__ bias,
                                         const float* __restrict__ hid, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float s = part[i];
#pragma unroll
    for (int sp = 1; sp < POS_SPLIT; ++sp) s += part[sp * n + i];
    out[i] = hid[i] + gelu_f(s + bias[(int)(i % H)]);
}

// ---- weight norm with dim=2 (norm over dims 0 and 1 for every tap): norm[j] = sqrt(sum_{o,c} v[o][c][j]^2), one block
// per tap, fixed-order block reduction
static __global__ __launch_bounds__(256) void wn_tap_norm_kernel(const float* __restrict__ v, long long rows, int k,
                                                                 float* __restrict__ norm) {
    __shared__ float red[8];
    const int j = blockIdx.x;
    float s = 0.f;
    for (long long r = threadIdx.x; r < rows; r += 256) {
        const float e = v[r * k + j];
        s += e * e;
    }
    s = block_sum<4>(s, red);
    if (threadIdx.x == 0) norm[j] = sqrtf(s);
}

// w = v * (g / norm) (torch._weight_norm), written as [cout][k][cin] -- the row order of the overlapping-row GEMM
static __global__ void wn_fold_kc_kernel(const float* __restrict__ v, const float* __restrict__ g, const float* __restrict__ norm,
                                         float* __restrict__ out, int cout, int cin, int k) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)cout * cin * k) return;
    const int t = (int)(i % k), c = (int)((i / k) % cin), o = (int)(i / ((long long)k * cin));
    out[((long long)o * k + t) * cin + c] = v[i] * (g[t] / norm[t]);
}

// ---- fused self-attention, head dim 64, no mask: out[t][h*64 + d] = softmax_s(scale * q_t . k_s) v_s[d].
// Block = 32 queries of one head (128 threads); a query is 4 adjacent lanes with 16 dims each.  K / V tiles of 64 keys
// are staged in LDS; the 64 scores of a tile stay in registers and fold into a running max / sum (online softmax), so
// no [heads][T][T] tensor exists and T has no limit.  All 32 queries read the same key row: every ds_read_b128 is 4
// distinct 16-B slots (banks 0-3, 16-19, 32-35, 48-51) broadcast to 16 lanes each, conflict-free.
// qkv [T][ld]: q at column h*64, k at H + h*64, v at 2H + h*64.
constexpr int ATT_QB = 32, ATT_KT = 64;
// query block qb of head h over the T rows at qkv (the keys are those T rows)
__device__ __forceinline__ void hubert_attn_block(const float* __restrict__ qkv, long long ld, int T, int H, float scale,
                                                  float* __restrict__ out, long long ldo, int qb, int h) {
    __shared__ float4 ks[ATT_KT * 16], vs[ATT_KT * 16];
    const int tid = threadIdx.x, part = tid & 3;
    const int row = qb * ATT_QB + (tid >> 2);
    float q[16], o[16];
    {
        const float* qp = qkv + (long long)row * ld + h * 64 + part * 16;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float4 v = row < T ? reinterpret_cast<const float4*>(qp)[i] : make_float4(0.f, 0.f, 0.f, 0.f);
            q[4 * i + 0] = v.x * scale; q[4 * i + 1] = v.y * scale; q[4 * i + 2] = v.z * scale; q[4 * i + 3] = v.w * scale;
        }
    }
#pragma unroll
    for (int d = 0; d < 16; ++d) o[d] = 0.f;
    float m = -INFINITY, l = 0.f;
    for (int k0 = 0; k0 < T; k0 += ATT_KT) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < ATT_KT * 16 / 128; ++i) {
            const int idx = tid + 128 * i, r = idx >> 4, c4 = idx & 15;
            const int key = k0 + r;
            float4 kv = make_float4(0.f, 0.f, 0.f, 0.f), vv = kv;
            if (key < T) {
                const float* base = qkv + (long long)key * ld + h * 64 + c4 * 4;
                kv = *reinterpret_cast<const float4*>(base + H);
                vv = *reinterpret_cast<const float4*>(base + 2 * H);
            }
            ks[idx] = kv;
            vs[idx] = vv;
        }
        __syncthreads();
        float s[ATT_KT];
        float mx = m;
#pragma unroll
        for (int j = 0; j < ATT_KT; ++j) {
            float d = 0.f;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float4 kv = ks[j * 16 + part * 4 + i];
                d += q[4 * i + 0] * kv.x + q[4 * i + 1] * kv.y + q[4 * i + 2] * kv.z + q[4 * i + 3] * kv.w;
            }
            d = quad_sum(d);
            s[j] = k0 + j < T ? d : -INFINITY;
            mx = fmaxf(mx, s[j]);
        }
        const float corr = expf(m - mx);   // 0 on the first tile (m = -inf, mx finite: every tile holds a valid key)
        l *= corr;
#pragma unroll
        for (int d = 0; d < 16; ++d) o[d] *= corr;
#pragma unroll
        for (int j = 0; j < ATT_KT; ++j) {
            const float p = expf(s[j] - mx);
            l += p;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float4 vv = vs[j * 16 + part * 4 + i];
                o[4 * i + 0] += p * vv.x; o[4 * i + 1] += p * vv.y; o[4 * i + 2] += p * vv.z; o[4 * i + 3] += p * vv.w;
            }
        }
        m = mx;
    }
    if (row >= T) return;
    const float inv = 1.f / l;
    float* op = out + (long long)row * ldo + h * 64 + part * 16;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        reinterpret_cast<float4*>(op)[i] = make_float4(o[4 * i] * inv, o[4 * i + 1] * inv, o[4 * i + 2] * inv, o[4 * i + 3] * inv);
}

static __global__ __launch_bounds__(128) void hubert_attn_kernel(const float* __restrict__ qkv, long long ld, int T, int H,
                                                                 float scale, float* __restrict__ out, long long ldo) {
    hubert_attn_block(qkv, ld, T, H, scale, out, ldo, blockIdx.x, blockIdx.y);
}

// batched: blockIdx.z = clip, whose queries attend to its own rows only; query blocks past the clip's frames exit
static __global__ __launch_bounds__(128) void hubert_attn_batch_kernel(const float* __restrict__ qkv, long long ld, int H,
                                                                       float scale, float* __restrict__ out, long long ldo,
                                                                       HubClips cl) {
    const int z = blockIdx.z, T = cl.T[z];
    if ((int)blockIdx.x * ATT_QB >= T) return;
    const long long r0 = cl.row0[z];
    hubert_attn_block(qkv + r0 * ld, ld, T, H, scale, out + r0 * ldo, ldo, blockIdx.x, blockIdx.y);
}

}  // namespace gsv
