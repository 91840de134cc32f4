// roberta: chinese-roberta-wwm-ext-large (transformers BertForMaskedLM) on the device, the model behind
// get_phones_and_bert -> CNRoberta._forward_pytorch (gsv_tts/GPT_SoVITS/Featurizer/cnroberta.py) -- word2ph texts ->
// hidden_states[-3] -> phone features, fp32 throughout.
//   embeddings   LN(word[id] + token_type[0] + position[t]) with positions restarting at every packed text
//   L - 2 post-LN layers x = LN(x + dense(attn(x))), x = LN(x + dense(gelu(dense(x))))   (hidden_states[-3])
//   phones       rows 1 .. len-2 of every text, repeated by word2ph["ph"] through a host-built index map
// Texts run PACKED: rows of all texts back to back, seq_starts[n + 1] delimiting them, no padding rows.  Every kernel
// below treats a row the same way wherever it lands, and every reduction has an order fixed by (N, K) alone, so one
// text's rows are bit-identical alone or inside any batch.  No atomics, no scratch.
#pragma once
#include "hubert.h"

namespace gsv {

// ---- embeddings + LayerNorm: one wave per packed row, the row in registers (H = 64 * npl, npl <= LN_MAX_NPL).
// v = (word[id] + type0) + pos[t] in BertEmbeddings' order, then ln_rows_kernel's two-pass statistics.
// Out-of-range ids / positions are clamped (the host refuses them first); they never read outside the tables.
static __global__ __launch_bounds__(256) void rb_embed_ln_kernel(const int* __restrict__ ids, const int* __restrict__ starts,
                                                                 int n_seq, int rows, const float* __restrict__ word, int vocab,
                                                                 const float* __restrict__ posw, int max_pos,
                                                                 const float* __restrict__ type0, int H,
                                                                 const float* __restrict__ g, const float* __restrict__ b,
                                                                 float eps, float* __restrict__ y) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    // the text holding row r: the last i with starts[i] <= r (binary search over n_seq + 1 starts)
    int lo = 0, hi = n_seq;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (starts[mid] <= r) lo = mid; else hi = mid;
    }
    const int t = min(max(r - starts[lo], 0), max_pos - 1);
    const int id = min(max(ids[r], 0), vocab - 1);
    const float* wr = word + (long long)id * H;
    const float* pr = posw + (long long)t * H;
    const int npl = H >> 6;
    float v[LN_MAX_NPL];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < LN_MAX_NPL; ++i) {
        const int c = lane + 64 * i;
        v[i] = i < npl ? (wr[c] + type0[c]) + pr[c] : 0.f;
        s += v[i];
    }
    const float mean = wave_sum(s) / (float)H;
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < LN_MAX_NPL; ++i) {
        const float d = i < npl ? v[i] - mean : 0.f;
        ss += d * d;
    }
    const float rstd = 1.f / sqrtf(wave_sum(ss) / (float)H + eps);
    float* yr = y + (long long)r * H;
#pragma unroll
    for (int i = 0; i < LN_MAX_NPL; ++i)
        if (i < npl) {
            const int c = lane + 64 * i;
            yr[c] = (v[i] - mean) * rstd * g[c] + b[c];
        }
}

// ---- GEMM for few rows: Y[M][N] = epi(X[M][K] . W[N][K]^T).  One launch of 64 x 64 fgemm tiles over (column tile,
// row tile, K slice s) writes part[s][M][N]; rb_splitk_reduce sums the slices in index order and applies the epilogue.
// The split count and the slice bounds are functions of (N, K) only (rb_splits), and inside a slice fgemm_tile walks K
// in the same 32-wide MFMA chunks for every row: an output element's summation order never depends on M, on the tile
// its row lands in or on the other texts.  At M <= 64 the single row tile still gives ~RB_TARGET_BLOCKS blocks, each
// streaming a disjoint N x K-slice block of weights.
constexpr int RB_TARGET_BLOCKS = 256;
__host__ __device__ inline int rb_splits(int N, int K) {
    const int tiles_n = (N + 63) / 64;
    int s = (RB_TARGET_BLOCKS + tiles_n - 1) / tiles_n;
    const int chunks = (K + 2 * FG_KC - 1) / (2 * FG_KC);   // at least 64 values of K per slice
    s = s < chunks ? s : chunks;
    return s < 1 ? 1 : s;
}
// slice s covers [rb_kbound(s), rb_kbound(s + 1)), 32-aligned except at K
__host__ __device__ inline int rb_kbound(int K, int S, int s) {
    const int chunks = (K + FG_KC - 1) / FG_KC;
    const int k = (int)((long long)chunks * s / S) * FG_KC;
    return k < K ? k : K;
}

static __global__ __launch_bounds__(256) void rb_splitk_kernel(const float* __restrict__ X, const float* __restrict__ W,
                                                               float* __restrict__ part, int M, int N, int K, int S) {
    __shared__ float xs[64 * FG_LD];
    __shared__ float ws[64 * FG_LD];
    const int sp = blockIdx.z;
    const int k0 = rb_kbound(K, S, sp), k1 = rb_kbound(K, S, sp + 1);
    FGemmArgs a;
    a.X = X + k0; a.ldx = K;
    a.W = W + k0; a.ldw = K;
    a.Y = part + (long long)sp * M * N; a.ldy = N;
    a.bias_n = nullptr; a.bias_m = nullptr; a.R = nullptr; a.ldr = 0;
    a.M = M; a.N = N; a.K = k1 - k0; a.alpha = 1.f; a.act = 0;
    fgemm_tile(a, blockIdx.y * 64, blockIdx.x * 64, xs, ws);
}

// Y[i] = act(sum_s part[s][i] (s in index order) + bias[i % N]) (+ R[i]); N % 4 == 0, four outputs per thread
static __global__ void rb_splitk_reduce_kernel(const float* __restrict__ part, int S, long long n4, int N,
                                               const float* __restrict__ bias, int act, const float* __restrict__ R,
                                               float* __restrict__ Y) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    const float4* p = reinterpret_cast<const float4*>(part);
    float4 v = p[i];
    for (int s = 1; s < S; ++s) {
        const float4 w = p[s * n4 + i];
        v.x += w.x; v.y += w.y; v.z += w.z; v.w += w.w;
    }
    const int c = (int)((i * 4) % N);
    v.x += bias[c]; v.y += bias[c + 1]; v.z += bias[c + 2]; v.w += bias[c + 3];
    if (act == 2) { v.x = gelu_f(v.x); v.y = gelu_f(v.y); v.z = gelu_f(v.z); v.w = gelu_f(v.w); }
    if (R) {
        const float4 r = reinterpret_cast<const float4*>(R)[i];
        v.x += r.x; v.y += r.y; v.z += r.z; v.w += r.w;
    }
    reinterpret_cast<float4*>(Y)[i] = v;
}

// ---- variable-length self-attention, head dim 64: hubert_attn_kernel's online softmax with blockIdx.z = text.  Text z
// owns the packed rows [starts[z], starts[z + 1]); its queries attend to those keys only (what the padded batch's
// finfo.min key mask computes: exp underflows to exactly 0).  Blocks whose query tile lies past the text's end exit
// before the first barrier.  Row bounds are clamped to [0, rows].
static __global__ __launch_bounds__(128) void rb_attn_kernel(const float* __restrict__ qkv, const int* __restrict__ starts,
                                                             int rows, int H, float scale, float* __restrict__ out) {
    __shared__ float4 ks[ATT_KT * 16], vs[ATT_KT * 16];
    const long long ld = 3LL * H;
    const int s0 = min(max(starts[blockIdx.z], 0), rows);
    const int T = min(max(starts[blockIdx.z + 1], s0), rows) - s0;
    if ((int)blockIdx.x * ATT_QB >= T) return;
    const int tid = threadIdx.x, part = tid & 3;
    const int h = blockIdx.y, row = blockIdx.x * ATT_QB + (tid >> 2);
    const float* base0 = qkv + (long long)s0 * ld;
    float q[16], o[16];
    {
        const float* qp = base0 + (long long)row * ld + h * 64 + part * 16;
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
                const float* base = base0 + (long long)key * ld + h * 64 + c4 * 4;
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
        const float corr = expf(m - mx);
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
    float* op = out + (long long)(s0 + row) * H + h * 64 + part * 16;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        reinterpret_cast<float4*>(op)[i] = make_float4(o[4 * i] * inv, o[4 * i + 1] * inv, o[4 * i + 2] * inv, o[4 * i + 3] * inv);
}

// ---- phone expansion: out[p][:] = hid[index[p]][:], one block per phone, H / 4 float4 lanes (H <= 1024).  An index
// outside [0, rows) writes zeros instead of reading out of bounds (the host builds the map and never produces one).
static __global__ __launch_bounds__(256) void rb_phone_gather_kernel(const float* __restrict__ hid, int rows, int H,
                                                                     const int* __restrict__ index, float* __restrict__ out) {
    const int p = blockIdx.x, c4 = threadIdx.x;
    if (c4 * 4 >= H) return;
    const int r = index[p];
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r >= 0 && r < rows) v = reinterpret_cast<const float4*>(hid + (long long)r * H)[c4];
    reinterpret_cast<float4*>(out + (long long)p * H)[c4] = v;
}

}  // namespace gsv
