// C-ABI of the reference-audio path (include/gsv_tts_hip.h, "reference audio" section; kernels in refaudio.h) and of
// CN-HuBERT (gsv_hubert_*; kernels in hubert.h, which shares refaudio.h's fgemm).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/gsv_tts_hip.h"
#include "gsv_error.h"
#include "hubert.h"
#include "refaudio.h"

using namespace gsv;

#define RCHK(expr)                                                                                        \
    do {                                                                                                  \
        hipError_t e_ = (expr);                                                                           \
        if (e_ != hipSuccess) return abi_fail(GSV_ERR_HIP, "%s: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

struct gsv_ref {
    gsv_ref_config cfg;
    std::map<std::string, std::pair<float*, int64_t>> t;   // loaded tensors (device, fp32)
    bool finalized = false;
    // derived at finalize
    float *w_qk = nullptr, *b_qk = nullptr;                 // [2H][H], [2H]
    float *w_c0 = nullptr, *w_c1 = nullptr;                 // temporal convs as [2H][5*H]
    float *w_ssl = nullptr;                                 // [ssl][2*ssl]
    float *e2 = nullptr;                                    // [bins]
    float *dft = nullptr;                                   // [2*(n_fft/2+1)][n_fft]
    std::vector<void*> owned;
};

namespace {

inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }
inline size_t up(size_t v) { return (v + 63) / 64 * 64; }   // in floats: 256-byte slots

int fgemm(hipStream_t st, const float* X, long long ldx, const float* W, long long ldw, float* Y, long long ldy, int M, int N, int K,
          const float* bias_n = nullptr, int act = 0, const float* R = nullptr, long long ldr = 0, float alpha = 1.f,
          const float* bias_m = nullptr) {
    FGemmArgs a;
    a.X = X; a.ldx = ldx; a.W = W; a.ldw = ldw; a.Y = Y; a.ldy = ldy;
    a.bias_n = bias_n; a.bias_m = bias_m; a.R = R; a.ldr = ldr;
    a.M = M; a.N = N; a.K = K; a.alpha = alpha; a.act = act;
    fgemm_kernel<<<dim3((N + 63) / 64, (M + 63) / 64), 256, 0, st>>>(a);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

const float* T_(gsv_ref* h, const char* name) { return h->t.at(name).first; }

struct Need { const char* name; int64_t numel; };

int dev_alloc(gsv_ref* h, float** p, size_t floats) {
    RCHK(hipMalloc(reinterpret_cast<void**>(p), floats * sizeof(float)));
    h->owned.push_back(*p);
    return GSV_OK;
}

}  // namespace

extern "C" {

int gsv_ref_create(const gsv_ref_config* cfg, gsv_ref** out) {
    if (!cfg || !out) return abi_fail(GSV_ERR_ARG, "null argument");
    if (cfg->hidden != 128 || cfg->n_head != 2 || cfg->spec_bins < 1 || cfg->spec_bins > cfg->n_fft / 2 + 1 || cfg->gin < 1 ||
        cfg->n_fft < 64 || cfg->n_fft % 2 || cfg->hop < 1 || cfg->ssl_dim < 1 || cfg->bins < 2 || cfg->kernel != 5)
        return abi_fail(GSV_ERR_ARG, "ref: unsupported config (MelStyleEncoder hidden 128 / 2 heads / kernel 5 expected)");
    gsv_ref* h = new gsv_ref();
    h->cfg = *cfg;
    *out = h;
    return GSV_OK;
}

int gsv_ref_destroy(gsv_ref* h) {
    if (!h) return GSV_OK;
    for (auto& kv : h->t) (void)hipFree(kv.second.first);
    for (void* p : h->owned) (void)hipFree(p);
    delete h;
    return GSV_OK;
}

int gsv_ref_load_tensor(gsv_ref* h, const char* name, const float* data, int64_t numel, void* stream) {
    if (!h || !name || !data || numel < 1) return abi_fail(GSV_ERR_ARG, "null argument");
    if (h->finalized) return abi_fail(GSV_ERR_STATE, "ref: load after finalize");
    const std::string n(name);
    if (n.rfind("ref_enc.", 0) != 0 && n.rfind("sv_emb.", 0) != 0 && n != "prelu.weight" && n.rfind("ssl_proj.", 0) != 0 &&
        n != "quantizer.vq.layers.0._codebook.embed")
        return abi_fail(GSV_ERR_ARG, "ref: unknown tensor %s", name);
    float* d = nullptr;
    RCHK(hipMalloc(reinterpret_cast<void**>(&d), numel * sizeof(float)));
    RCHK(hipMemcpyAsync(d, data, numel * sizeof(float), hipMemcpyDeviceToDevice, S(stream)));
    auto it = h->t.find(n);
    if (it != h->t.end()) (void)hipFree(it->second.first);
    h->t[n] = {d, numel};
    return GSV_OK;
}

int gsv_ref_finalize(gsv_ref* h, void* stream) {
    if (!h) return abi_fail(GSV_ERR_ARG, "null argument");
    if (h->finalized) return GSV_OK;
    const gsv_ref_config& c = h->cfg;
    const int64_t H = c.hidden;
    std::vector<Need> need = {
        {"ref_enc.spectral.0.fc.weight", H * c.spec_bins}, {"ref_enc.spectral.0.fc.bias", H},
        {"ref_enc.spectral.3.fc.weight", H * H}, {"ref_enc.spectral.3.fc.bias", H},
        {"ref_enc.temporal.0.conv1.conv.weight", 2 * H * H * 5}, {"ref_enc.temporal.0.conv1.conv.bias", 2 * H},
        {"ref_enc.temporal.1.conv1.conv.weight", 2 * H * H * 5}, {"ref_enc.temporal.1.conv1.conv.bias", 2 * H},
        {"ref_enc.slf_attn.w_qs.weight", H * H}, {"ref_enc.slf_attn.w_qs.bias", H},
        {"ref_enc.slf_attn.w_ks.weight", H * H}, {"ref_enc.slf_attn.w_ks.bias", H},
        {"ref_enc.slf_attn.w_vs.weight", H * H}, {"ref_enc.slf_attn.w_vs.bias", H},
        {"ref_enc.slf_attn.fc.weight", H * H}, {"ref_enc.slf_attn.fc.bias", H},
        {"ref_enc.fc.fc.weight", (int64_t)c.gin * H}, {"ref_enc.fc.fc.bias", c.gin},
        {"ssl_proj.weight", (int64_t)c.ssl_dim * c.ssl_dim * 2}, {"ssl_proj.bias", c.ssl_dim},
        {"quantizer.vq.layers.0._codebook.embed", (int64_t)c.bins * c.ssl_dim},
    };
    if (c.sv_dim > 0) {
        need.push_back({"sv_emb.weight", (int64_t)c.gin * c.sv_dim});
        need.push_back({"sv_emb.bias", c.gin});
        need.push_back({"prelu.weight", c.gin});
    }
    for (const Need& n : need) {
        auto it = h->t.find(n.name);
        if (it == h->t.end()) return abi_fail(GSV_ERR_STATE, "ref: tensor %s was not loaded", n.name);
        if (it->second.second != n.numel)
            return abi_fail(GSV_ERR_ARG, "ref: tensor %s has %lld elements, expected %lld", n.name, (long long)it->second.second, (long long)n.numel);
    }
    hipStream_t st = S(stream);
    int rc;
    if ((rc = dev_alloc(h, &h->w_qk, 2 * H * H)) || (rc = dev_alloc(h, &h->b_qk, 2 * H)) || (rc = dev_alloc(h, &h->w_c0, 2 * H * H * 5)) ||
        (rc = dev_alloc(h, &h->w_c1, 2 * H * H * 5)) || (rc = dev_alloc(h, &h->w_ssl, (size_t)c.ssl_dim * c.ssl_dim * 2)) ||
        (rc = dev_alloc(h, &h->e2, c.bins)) || (rc = dev_alloc(h, &h->dft, (size_t)(c.n_fft + 2) * c.n_fft)))
        return rc;
    RCHK(hipMemcpyAsync(h->w_qk, T_(h, "ref_enc.slf_attn.w_qs.weight"), H * H * 4, hipMemcpyDeviceToDevice, st));
    RCHK(hipMemcpyAsync(h->w_qk + H * H, T_(h, "ref_enc.slf_attn.w_ks.weight"), H * H * 4, hipMemcpyDeviceToDevice, st));
    RCHK(hipMemcpyAsync(h->b_qk, T_(h, "ref_enc.slf_attn.w_qs.bias"), H * 4, hipMemcpyDeviceToDevice, st));
    RCHK(hipMemcpyAsync(h->b_qk + H, T_(h, "ref_enc.slf_attn.w_ks.bias"), H * 4, hipMemcpyDeviceToDevice, st));
    const int nconv = (int)(2 * H * H * 5);
    conv_weight_kc_kernel<<<(nconv + 255) / 256, 256, 0, st>>>(T_(h, "ref_enc.temporal.0.conv1.conv.weight"), h->w_c0, (int)(2 * H), (int)H, 5);
    conv_weight_kc_kernel<<<(nconv + 255) / 256, 256, 0, st>>>(T_(h, "ref_enc.temporal.1.conv1.conv.weight"), h->w_c1, (int)(2 * H), (int)H, 5);
    const int nssl = c.ssl_dim * c.ssl_dim * 2;
    conv_weight_kc_kernel<<<(nssl + 255) / 256, 256, 0, st>>>(T_(h, "ssl_proj.weight"), h->w_ssl, c.ssl_dim, c.ssl_dim, 2);
    rowsq_kernel<<<(c.bins + 3) / 4, 256, 0, st>>>(T_(h, "quantizer.vq.layers.0._codebook.embed"), c.ssl_dim, c.bins, c.ssl_dim, h->e2);
    const long long ndft = (long long)(c.n_fft / 2 + 1) * c.n_fft;
    dft_rows_kernel<<<(unsigned)((ndft + 255) / 256), 256, 0, st>>>(h->dft, c.n_fft, c.n_fft / 2 + 1);
    RCHK(hipGetLastError());
    h->finalized = true;
    return GSV_OK;
}

size_t gsv_ref_workspace(gsv_ref* h, int n_samples, int n_frames, int n_ssl) {
    if (!h) return 0;
    const gsv_ref_config& c = h->cfg;
    size_t spec = 0, ge = 0, lat = 0;
    if (n_samples > 0) {
        const size_t T = 1 + n_samples / c.hop;
        spec = up((size_t)n_samples + c.n_fft) + up(T * (c.n_fft + 2));
    }
    if (n_frames > 0) {
        const size_t T = n_frames, H = c.hidden;
        ge = up(T * c.spec_bins) + 2 * up(T * H) + 2 * up((T + 4) * H) + 2 * up(T * 2 * H) + up(H * T) + up(T * T) + 2 * up(T * H) +
             up(T * c.gin) + up(c.gin);
    }
    if (n_ssl > 0) {
        const size_t Th = n_ssl, To = n_ssl / 2;
        lat = up(Th * c.ssl_dim) + up(To * c.ssl_dim) + up(To * c.bins) + up(To);
    }
    return sizeof(float) * std::max(spec, std::max(ge, lat));
}

int gsv_ref_spectrogram(gsv_ref* h, const float* audio, int n_samples, float* spec, void* workspace, size_t workspace_bytes,
                        void* stream) {
    if (!h || !audio || !spec || !workspace) return abi_fail(GSV_ERR_ARG, "null argument");
    if (!h->finalized) return abi_fail(GSV_ERR_STATE, "ref: not finalized");
    const gsv_ref_config& c = h->cfg;
    if (n_samples <= c.n_fft / 2) return abi_fail(GSV_ERR_ARG, "ref: reflect padding needs more than n_fft/2 samples (got %d)", n_samples);
    if (workspace_bytes < gsv_ref_workspace(h, n_samples, 0, 0)) return abi_fail(GSV_ERR_ARG, "ref: workspace too small");
    hipStream_t st = S(stream);
    const int T = 1 + n_samples / c.hop, bins = c.n_fft / 2 + 1;
    float* padded = static_cast<float*>(workspace);
    float* Z = padded + up((size_t)n_samples + c.n_fft);
    reflect_pad_kernel<<<(n_samples + c.n_fft + 255) / 256, 256, 0, st>>>(audio, n_samples, c.n_fft / 2, padded);
    if (fgemm(st, padded, c.hop, h->dft, c.n_fft, Z, 2 * bins, T, 2 * bins, c.n_fft)) return abi_fail(GSV_ERR_HIP, "ref: DFT launch failed");
    const long long n = (long long)T * bins;
    magnitude_t_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(Z, T, bins, spec);
    RCHK(hipGetLastError());
    return GSV_OK;
}

int gsv_ref_get_ge(gsv_ref* h, const float* spec, int n_frames, const float* sv_emb, float* ge, void* workspace,
                   size_t workspace_bytes, void* stream) {
    if (!h || !spec || !ge || !workspace) return abi_fail(GSV_ERR_ARG, "null argument");
    if (!h->finalized) return abi_fail(GSV_ERR_STATE, "ref: not finalized");
    const gsv_ref_config& c = h->cfg;
    if (n_frames < 1) return abi_fail(GSV_ERR_ARG, "ref: no frames");
    if (sv_emb && c.sv_dim <= 0) return abi_fail(GSV_ERR_ARG, "ref: this handle has no sv_emb (v2)");
    if (workspace_bytes < gsv_ref_workspace(h, 0, n_frames, 0)) return abi_fail(GSV_ERR_ARG, "ref: workspace too small");
    hipStream_t st = S(stream);
    const int T = n_frames, H = c.hidden, D = H / c.n_head;
    float* p = static_cast<float*>(workspace);
    auto take = [&](size_t n) { float* r = p; p += up(n); return r; };
    float* X0 = take((size_t)T * c.spec_bins);
    float* H1 = take((size_t)T * H);
    float* G2 = take((size_t)T * H);
    float* P0 = take((size_t)(T + 4) * H);
    float* P1 = take((size_t)(T + 4) * H);
    float* C = take((size_t)T * 2 * H);
    float* QK = take((size_t)T * 2 * H);
    float* VT = take((size_t)H * T);
    float* Sm = take((size_t)T * T);
    float* O = take((size_t)T * H);
    float* A = take((size_t)T * H);
    float* F = take((size_t)T * c.gin);
    float* sv = take(c.gin);
    int bad = 0;
    // refer[:, :704] channels-first -> frames-major
    transpose_kernel<<<dim3((T + 31) / 32, (c.spec_bins + 31) / 32), 256, 0, st>>>(spec, T, X0, c.spec_bins, c.spec_bins, T);
    // spectral: Linear + Mish, twice (modules.py:385-392); the second lands in the zero-padded buffer of the first conv
    bad |= fgemm(st, X0, c.spec_bins, T_(h, "ref_enc.spectral.0.fc.weight"), c.spec_bins, H1, H, T, H, c.spec_bins, T_(h, "ref_enc.spectral.0.fc.bias"), 1);
    RCHK(hipMemsetAsync(P0, 0, (size_t)(T + 4) * H * sizeof(float), st));
    RCHK(hipMemsetAsync(P1, 0, (size_t)(T + 4) * H * sizeof(float), st));
    bad |= fgemm(st, H1, H, T_(h, "ref_enc.spectral.3.fc.weight"), H, P0 + 2 * H, H, T, H, H, T_(h, "ref_enc.spectral.3.fc.bias"), 1);
    // temporal: two Conv1dGLU (k 5, same padding) as overlapping-row GEMMs
    const int nel = T * H;
    bad |= fgemm(st, P0, H, h->w_c0, 5 * H, C, 2 * H, T, 2 * H, 5 * H, T_(h, "ref_enc.temporal.0.conv1.conv.bias"));
    glu_residual_kernel<<<(nel + 255) / 256, 256, 0, st>>>(P0 + 2 * H, C, P1 + 2 * H, T, H);
    bad |= fgemm(st, P1, H, h->w_c1, 5 * H, C, 2 * H, T, 2 * H, 5 * H, T_(h, "ref_enc.temporal.1.conv1.conv.bias"));
    glu_residual_kernel<<<(nel + 255) / 256, 256, 0, st>>>(P1 + 2 * H, C, G2, T, H);
    // self-attention (modules.py:291-343): temperature sqrt(d_model), no mask (the reference mask is all ones)
    bad |= fgemm(st, G2, H, h->w_qk, H, QK, 2 * H, T, 2 * H, H, h->b_qk);
    bad |= fgemm(st, T_(h, "ref_enc.slf_attn.w_vs.weight"), H, G2, H, VT, T, H, T, H, nullptr, 0, nullptr, 0, 1.f, T_(h, "ref_enc.slf_attn.w_vs.bias"));
    const float inv_temp = 1.f / sqrtf((float)H);
    for (int hd = 0; hd < c.n_head; ++hd) {
        bad |= fgemm(st, QK + hd * D, 2 * H, QK + H + hd * D, 2 * H, Sm, T, T, T, D, nullptr, 0, nullptr, 0, inv_temp);
        softmax_rows_kernel<<<(T + 3) / 4, 256, 0, st>>>(Sm, T, T);
        bad |= fgemm(st, Sm, T, VT + (size_t)hd * D * T, T, O + hd * D, H, T, D, T);
    }
    bad |= fgemm(st, O, H, T_(h, "ref_enc.slf_attn.fc.weight"), H, A, H, T, H, H, T_(h, "ref_enc.slf_attn.fc.bias"), 0, G2, H);
    bad |= fgemm(st, A, H, T_(h, "ref_enc.fc.fc.weight"), H, F, c.gin, T, c.gin, H, T_(h, "ref_enc.fc.fc.bias"));
    if (sv_emb) gemv_rows_kernel<<<(c.gin + 3) / 4, 256, 0, st>>>(sv_emb, T_(h, "sv_emb.weight"), T_(h, "sv_emb.bias"), sv, c.gin, c.sv_dim);
    pool_prelu_kernel<<<(c.gin + 255) / 256, 256, 0, st>>>(F, T, c.gin, sv_emb ? sv : nullptr, sv_emb ? T_(h, "prelu.weight") : nullptr, ge);
    if (bad) return abi_fail(GSV_ERR_HIP, "ref: a get_ge launch failed");
    RCHK(hipGetLastError());
    return GSV_OK;
}

int gsv_ref_extract_latent(gsv_ref* h, const float* ssl, int n_ssl, int64_t* codes, float* margin, void* workspace,
                           size_t workspace_bytes, void* stream) {
    if (!h || !ssl || !codes || !workspace) return abi_fail(GSV_ERR_ARG, "null argument");
    if (!h->finalized) return abi_fail(GSV_ERR_STATE, "ref: not finalized");
    const gsv_ref_config& c = h->cfg;
    if (n_ssl < 2) return abi_fail(GSV_ERR_ARG, "ref: extract_latent needs at least 2 ssl frames");
    if (workspace_bytes < gsv_ref_workspace(h, 0, 0, n_ssl)) return abi_fail(GSV_ERR_ARG, "ref: workspace too small");
    hipStream_t st = S(stream);
    const int Th = n_ssl, To = n_ssl / 2, Dm = c.ssl_dim;
    float* p = static_cast<float*>(workspace);
    auto take = [&](size_t n) { float* r = p; p += up(n); return r; };
    float* Xt = take((size_t)Th * Dm);
    float* Y = take((size_t)To * Dm);
    float* dot = take((size_t)To * c.bins);
    float* x2 = take(To);
    int bad = 0;
    transpose_kernel<<<dim3((Th + 31) / 32, (Dm + 31) / 32), 256, 0, st>>>(ssl, Th, Xt, Dm, Dm, Th);
    // Conv1d(ssl, ssl, 2, stride 2): frames 2i, 2i+1 are one contiguous row of the frames-major buffer
    bad |= fgemm(st, Xt, 2 * Dm, h->w_ssl, 2 * Dm, Y, Dm, To, Dm, 2 * Dm, T_(h, "ssl_proj.bias"));
    bad |= fgemm(st, Y, Dm, T_(h, "quantizer.vq.layers.0._codebook.embed"), Dm, dot, c.bins, To, c.bins, Dm);
    rowsq_kernel<<<(To + 3) / 4, 256, 0, st>>>(Y, Dm, To, Dm, x2);
    nearest_code_kernel<<<(To + 3) / 4, 256, 0, st>>>(dot, x2, h->e2, To, c.bins, reinterpret_cast<long long*>(codes), margin);
    if (bad) return abi_fail(GSV_ERR_HIP, "ref: an extract_latent launch failed");
    RCHK(hipGetLastError());
    return GSV_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------------------------
// CN-HuBERT
// ------------------------------------------------------------------------------------------------------------------
struct gsv_hubert {
    gsv_hubert_config cfg;
    std::map<std::string, std::pair<float*, int64_t>> t;   // loaded tensors (device, fp32)
    bool finalized = false;
    // derived at finalize
    float* w_conv[GSV_HUBERT_MAX_CONV] = {};                 // conv i >= 1 as [cout][k][cin]
    float* w_pos = nullptr;                                 // folded weight norm, [H][k][H/G]
    std::vector<float*> w_qkv, b_qkv;                       // per layer [3H][H], [3H] (q, k, v)
    std::vector<void*> owned;
};

namespace {

const float* HT(gsv_hubert* h, const std::string& name) { return h->t.at(name).first; }

int hub_alloc(gsv_hubert* h, float** p, size_t floats) {
    RCHK(hipMalloc(reinterpret_cast<void**>(p), floats * sizeof(float)));
    h->owned.push_back(*p);
    return GSV_OK;
}

// frame counts after every conv of the feature encoder; false when the input is too short for one
bool hub_frames(const gsv_hubert_config& c, int n, int* T) {
    int len = n;
    for (int i = 0; i < c.n_conv; ++i) {
        if (len < c.conv_kernel[i]) return false;
        len = (len - c.conv_kernel[i]) / c.conv_stride[i] + 1;
        T[i] = len;
    }
    return true;
}

std::string hub_layer(int l, const char* rest) { return "encoder.layers." + std::to_string(l) + "." + rest; }

// workspace carve-up of one forward, in floats (256-byte slots); the same walk sizes and assigns it
struct HubWs {
    float *act[2], *pmean, *pm2, *gmean, *gscale, *hid, *pg, *part, *x, *tmp, *qkv, *att, *ffn;
    size_t total;
};
HubWs hub_carve(const gsv_hubert_config& c, const int* T, float* base) {
    HubWs w;
    size_t off = 0;
    auto take = [&](size_t n) { float* r = base ? base + off : nullptr; off += up(n); return r; };
    size_t a0 = 0, a1 = 0;   // ping-pong: conv i writes act[i & 1]
    for (int i = 0; i < c.n_conv; ++i) {
        size_t& a = (i & 1) ? a1 : a0;
        a = std::max(a, (size_t)T[i] * c.conv_dim[i]);
    }
    const int C0 = c.conv_dim[0], nch = (T[0] + GN_ROWS - 1) / GN_ROWS;
    const size_t Th = T[c.n_conv - 1], H = c.hidden;
    w.act[0] = take(a0);
    w.act[1] = take(a1);
    w.pmean = take((size_t)nch * C0);
    w.pm2 = take((size_t)nch * C0);
    w.gmean = take(C0);
    w.gscale = take(C0);
    w.hid = take(Th * H);
    w.pg = take((Th + c.pos_k - 1) * H);
    w.part = take(POS_SPLIT * Th * H);
    w.x = take(Th * H);
    w.tmp = take(Th * H);
    w.qkv = take(Th * 3 * H);
    w.att = take(Th * H);
    w.ffn = take(Th * c.ffn);
    w.total = off;
    return w;
}

int ln(hipStream_t st, const float* x, float* y, int rows, int C, const float* g, const float* b, float eps) {
    ln_rows_kernel<<<(rows + 3) / 4, 256, 0, st>>>(x, y, rows, C, g, b, eps);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

}  // namespace

extern "C" {

int gsv_hubert_create(const gsv_hubert_config* cfg, gsv_hubert** out) {
    if (!cfg || !out) return abi_fail(GSV_ERR_ARG, "null argument");
    const gsv_hubert_config& c = *cfg;
    if (c.hidden < 64 || c.hidden % 64 || c.hidden > 64 * LN_MAX_NPL)
        return abi_fail(GSV_ERR_ARG, "hubert: hidden %d unsupported (a multiple of 64 up to %d)", c.hidden, 64 * LN_MAX_NPL);
    if (c.n_head < 1 || c.hidden != 64 * c.n_head)
        return abi_fail(GSV_ERR_ARG, "hubert: %d heads over hidden %d unsupported (the attention kernel needs head dim 64)", c.n_head, c.hidden);
    if (c.n_layer < 0 || c.ffn < 1) return abi_fail(GSV_ERR_ARG, "hubert: n_layer %d / ffn %d unsupported", c.n_layer, c.ffn);
    if (c.n_conv < 1 || c.n_conv > GSV_HUBERT_MAX_CONV) return abi_fail(GSV_ERR_ARG, "hubert: %d feature-encoder convs (1..%d)", c.n_conv, GSV_HUBERT_MAX_CONV);
    for (int i = 0; i < c.n_conv; ++i) {
        if (c.conv_dim[i] < 64 || c.conv_dim[i] % 64 || c.conv_dim[i] > 64 * LN_MAX_NPL)
            return abi_fail(GSV_ERR_ARG, "hubert: conv_dim[%d] = %d unsupported (a multiple of 64 up to %d)", i, c.conv_dim[i], 64 * LN_MAX_NPL);
        if (c.conv_kernel[i] < 1 || c.conv_stride[i] < 1)
            return abi_fail(GSV_ERR_ARG, "hubert: conv %d kernel %d / stride %d unsupported", i, c.conv_kernel[i], c.conv_stride[i]);
    }
    if (c.pos_k < 2 || c.pos_k % 2 || c.pos_groups < 1 || c.hidden % c.pos_groups)
        return abi_fail(GSV_ERR_ARG, "hubert: positional conv k %d / groups %d unsupported (even k, groups dividing hidden)", c.pos_k, c.pos_groups);
    if (!(c.eps > 0.f)) return abi_fail(GSV_ERR_ARG, "hubert: layer_norm_eps must be > 0");
    gsv_hubert* h = new gsv_hubert();
    h->cfg = c;
    *out = h;
    return GSV_OK;
}

int gsv_hubert_destroy(gsv_hubert* h) {
    if (!h) return GSV_OK;
    for (auto& kv : h->t) (void)hipFree(kv.second.first);
    for (void* p : h->owned) (void)hipFree(p);
    delete h;
    return GSV_OK;
}

int gsv_hubert_load_tensor(gsv_hubert* h, const char* name, const float* data, int64_t numel, void* stream) {
    if (!h || !name || !data || numel < 1) return abi_fail(GSV_ERR_ARG, "null argument");
    if (h->finalized) return abi_fail(GSV_ERR_STATE, "hubert: load after finalize");
    std::string n(name);
    if (n == "encoder.pos_conv_embed.conv.parametrizations.weight.original0") n = "encoder.pos_conv_embed.conv.weight_g";
    if (n == "encoder.pos_conv_embed.conv.parametrizations.weight.original1") n = "encoder.pos_conv_embed.conv.weight_v";
    if (n.rfind("feature_extractor.", 0) != 0 && n.rfind("feature_projection.", 0) != 0 && n.rfind("encoder.", 0) != 0)
        return abi_fail(GSV_ERR_ARG, "hubert: unknown tensor %s", name);
    float* d = nullptr;
    RCHK(hipMalloc(reinterpret_cast<void**>(&d), numel * sizeof(float)));
    RCHK(hipMemcpyAsync(d, data, numel * sizeof(float), hipMemcpyDeviceToDevice, S(stream)));
    auto it = h->t.find(n);
    if (it != h->t.end()) (void)hipFree(it->second.first);
    h->t[n] = {d, numel};
    return GSV_OK;
}

int gsv_hubert_finalize(gsv_hubert* h, void* stream) {
    if (!h) return abi_fail(GSV_ERR_ARG, "null argument");
    if (h->finalized) return GSV_OK;
    const gsv_hubert_config& c = h->cfg;
    const int64_t H = c.hidden, F = c.ffn, C0 = c.conv_dim[0], CL = c.conv_dim[c.n_conv - 1], cg = H / c.pos_groups;
    std::vector<std::pair<std::string, int64_t>> need = {
        {"feature_extractor.conv_layers.0.conv.weight", C0 * c.conv_kernel[0]},
        {"feature_extractor.conv_layers.0.layer_norm.weight", C0}, {"feature_extractor.conv_layers.0.layer_norm.bias", C0},
        {"feature_projection.layer_norm.weight", CL}, {"feature_projection.layer_norm.bias", CL},
        {"feature_projection.projection.weight", H * CL}, {"feature_projection.projection.bias", H},
        {"encoder.pos_conv_embed.conv.weight_g", c.pos_k}, {"encoder.pos_conv_embed.conv.weight_v", H * cg * c.pos_k},
        {"encoder.pos_conv_embed.conv.bias", H},
        {"encoder.layer_norm.weight", H}, {"encoder.layer_norm.bias", H},
    };
    for (int i = 1; i < c.n_conv; ++i)
        need.push_back({"feature_extractor.conv_layers." + std::to_string(i) + ".conv.weight",
                        (int64_t)c.conv_dim[i] * c.conv_dim[i - 1] * c.conv_kernel[i]});
    for (int l = 0; l < c.n_layer; ++l) {
        for (const char* p : {"attention.q_proj", "attention.k_proj", "attention.v_proj", "attention.out_proj"}) {
            need.push_back({hub_layer(l, p) + ".weight", H * H});
            need.push_back({hub_layer(l, p) + ".bias", H});
        }
        need.push_back({hub_layer(l, "feed_forward.intermediate_dense.weight"), F * H});
        need.push_back({hub_layer(l, "feed_forward.intermediate_dense.bias"), F});
        need.push_back({hub_layer(l, "feed_forward.output_dense.weight"), H * F});
        need.push_back({hub_layer(l, "feed_forward.output_dense.bias"), H});
        for (const char* p : {"layer_norm.weight", "layer_norm.bias", "final_layer_norm.weight", "final_layer_norm.bias"})
            need.push_back({hub_layer(l, p), H});
    }
    for (const auto& n : need) {
        auto it = h->t.find(n.first);
        if (it == h->t.end()) return abi_fail(GSV_ERR_STATE, "hubert: tensor %s was not loaded", n.first.c_str());
        if (it->second.second != n.second)
            return abi_fail(GSV_ERR_ARG, "hubert: tensor %s has %lld elements, expected %lld", n.first.c_str(),
                            (long long)it->second.second, (long long)n.second);
    }
    hipStream_t st = S(stream);
    int rc;
    for (int i = 1; i < c.n_conv; ++i) {
        const int co = c.conv_dim[i], ci = c.conv_dim[i - 1], k = c.conv_kernel[i];
        const long long nw = (long long)co * ci * k;
        if ((rc = hub_alloc(h, &h->w_conv[i], nw))) return rc;
        conv_weight_kc_kernel<<<(unsigned)((nw + 255) / 256), 256, 0, st>>>(
            HT(h, "feature_extractor.conv_layers." + std::to_string(i) + ".conv.weight"), h->w_conv[i], co, ci, k);
    }
    float* norm = nullptr;
    const long long npos = H * cg * c.pos_k;
    if ((rc = hub_alloc(h, &h->w_pos, npos)) || (rc = hub_alloc(h, &norm, c.pos_k))) return rc;
    wn_tap_norm_kernel<<<c.pos_k, 256, 0, st>>>(HT(h, "encoder.pos_conv_embed.conv.weight_v"), H * cg, c.pos_k, norm);
    wn_fold_kc_kernel<<<(unsigned)((npos + 255) / 256), 256, 0, st>>>(HT(h, "encoder.pos_conv_embed.conv.weight_v"),
                                                                     HT(h, "encoder.pos_conv_embed.conv.weight_g"), norm, h->w_pos, (int)H, (int)cg, c.pos_k);
    h->w_qkv.assign(c.n_layer, nullptr);
    h->b_qkv.assign(c.n_layer, nullptr);
    for (int l = 0; l < c.n_layer; ++l) {
        if ((rc = hub_alloc(h, &h->w_qkv[l], 3 * H * H)) || (rc = hub_alloc(h, &h->b_qkv[l], 3 * H))) return rc;
        const char* p[3] = {"attention.q_proj", "attention.k_proj", "attention.v_proj"};
        for (int j = 0; j < 3; ++j) {
            RCHK(hipMemcpyAsync(h->w_qkv[l] + j * H * H, HT(h, hub_layer(l, p[j]) + ".weight"), H * H * 4, hipMemcpyDeviceToDevice, st));
            RCHK(hipMemcpyAsync(h->b_qkv[l] + j * H, HT(h, hub_layer(l, p[j]) + ".bias"), H * 4, hipMemcpyDeviceToDevice, st));
        }
    }
    RCHK(hipGetLastError());
    h->finalized = true;
    return GSV_OK;
}

int gsv_hubert_frames(gsv_hubert* h, int n_samples) {
    if (!h) return 0;
    int T[GSV_HUBERT_MAX_CONV];
    return hub_frames(h->cfg, n_samples, T) ? T[h->cfg.n_conv - 1] : 0;
}

size_t gsv_hubert_workspace(gsv_hubert* h, int n_samples) {
    if (!h) return 0;
    int T[GSV_HUBERT_MAX_CONV];
    if (!hub_frames(h->cfg, n_samples, T)) return 0;
    return sizeof(float) * hub_carve(h->cfg, T, nullptr).total;
}

int gsv_hubert_forward(gsv_hubert* h, const float* audio, int n_samples, float* ssl, void* workspace, size_t workspace_bytes,
                       void* stream) {
    if (!h || !audio || !ssl || !workspace) return abi_fail(GSV_ERR_ARG, "null argument");
    if (!h->finalized) return abi_fail(GSV_ERR_STATE, "hubert: not finalized");
    const gsv_hubert_config& c = h->cfg;
    int T[GSV_HUBERT_MAX_CONV];
    if (!hub_frames(c, n_samples, T)) return abi_fail(GSV_ERR_ARG, "hubert: %d samples are too short for the feature encoder", n_samples);
    if (workspace_bytes < gsv_hubert_workspace(h, n_samples)) return abi_fail(GSV_ERR_ARG, "hubert: workspace too small");
    if ((reinterpret_cast<size_t>(workspace) & 15) != 0) return abi_fail(GSV_ERR_ARG, "hubert: workspace must be 16-byte aligned");
    hipStream_t st = S(stream);
    const HubWs w = hub_carve(c, T, static_cast<float*>(workspace));
    const int H = c.hidden, Th = T[c.n_conv - 1], C0 = c.conv_dim[0], CL = c.conv_dim[c.n_conv - 1];
    const int G = c.pos_groups, cg = H / G, K = c.pos_k, Tp = Th + K - 1;
    int bad = 0;
    // conv 0: rows of k0 samples at stride s0 over the waveform, then GroupNorm(C0, C0) over all T0 frames + GELU
    bad |= fgemm(st, audio, c.conv_stride[0], HT(h, "feature_extractor.conv_layers.0.conv.weight"), c.conv_kernel[0], w.act[0], C0,
                 T[0], C0, c.conv_kernel[0]);
    const int nch = (T[0] + GN_ROWS - 1) / GN_ROWS;
    gn_partial_kernel<<<dim3(C0 / 64, nch), 256, 0, st>>>(w.act[0], T[0], C0, w.pmean, w.pm2);
    gn_finalize_kernel<<<(C0 + 255) / 256, 256, 0, st>>>(w.pmean, w.pm2, nch, T[0], C0, HT(h, "feature_extractor.conv_layers.0.layer_norm.weight"),
                                                        1e-5f, w.gmean, w.gscale);
    const long long n4 = (long long)T[0] * C0 / 4;
    gn_apply_gelu_kernel<<<(unsigned)((n4 + 255) / 256), 256, 0, st>>>(w.act[0], n4, C0, w.gmean, w.gscale,
                                                                       HT(h, "feature_extractor.conv_layers.0.layer_norm.bias"));
    // convs 1..: rows of k * cin values at stride s * cin over the channels-last activations, GELU epilogue
    for (int i = 1; i < c.n_conv; ++i) {
        const int ci = c.conv_dim[i - 1], co = c.conv_dim[i];
        bad |= fgemm(st, w.act[(i - 1) & 1], (long long)c.conv_stride[i] * ci, h->w_conv[i], (long long)c.conv_kernel[i] * ci,
                     w.act[i & 1], co, T[i], co, c.conv_kernel[i] * ci, nullptr, 2);
    }
    float* feat = w.act[(c.n_conv - 1) & 1];
    // feature projection: LayerNorm(CL) in place, Linear CL -> H
    bad |= ln(st, feat, feat, Th, CL, HT(h, "feature_projection.layer_norm.weight"), HT(h, "feature_projection.layer_norm.bias"), c.eps);
    bad |= fgemm(st, feat, CL, HT(h, "feature_projection.projection.weight"), CL, w.hid, H, Th, H, CL, HT(h, "feature_projection.projection.bias"));
    // positional conv over the group-major padded copy: tmp = hid + gelu(conv(hid) + bias), the last frame never made
    {
        const long long np = (long long)G * Tp * cg, n = (long long)Th * H;
        pos_pad_group_kernel<<<(unsigned)((np + 255) / 256), 256, 0, st>>>(w.hid, Th, H, G, K, w.pg);
        pos_conv_split_kernel<<<dim3((cg + 63) / 64, (Th + 63) / 64, G * POS_SPLIT), 256, 0, st>>>(w.pg, h->w_pos, w.part, Th, H, G, K);
        pos_reduce_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(w.part, n, H, HT(h, "encoder.pos_conv_embed.conv.bias"), w.hid, w.tmp);
    }
    bad |= ln(st, w.tmp, w.x, Th, H, HT(h, "encoder.layer_norm.weight"), HT(h, "encoder.layer_norm.bias"), c.eps);
    const float scale = 1.f / sqrtf(64.f);
    for (int l = 0; l < c.n_layer; ++l) {
        bad |= fgemm(st, w.x, H, h->w_qkv[l], H, w.qkv, 3 * H, Th, 3 * H, H, h->b_qkv[l]);
        hubert_attn_kernel<<<dim3((Th + ATT_QB - 1) / ATT_QB, c.n_head), 128, 0, st>>>(w.qkv, 3 * H, Th, H, scale, w.att, H);
        bad |= fgemm(st, w.att, H, HT(h, hub_layer(l, "attention.out_proj.weight")), H, w.tmp, H, Th, H, H,
                     HT(h, hub_layer(l, "attention.out_proj.bias")), 0, w.x, H);
        bad |= ln(st, w.tmp, w.x, Th, H, HT(h, hub_layer(l, "layer_norm.weight")), HT(h, hub_layer(l, "layer_norm.bias")), c.eps);
        bad |= fgemm(st, w.x, H, HT(h, hub_layer(l, "feed_forward.intermediate_dense.weight")), H, w.ffn, c.ffn, Th, c.ffn, H,
                     HT(h, hub_layer(l, "feed_forward.intermediate_dense.bias")), 2);
        bad |= fgemm(st, w.ffn, c.ffn, HT(h, hub_layer(l, "feed_forward.output_dense.weight")), c.ffn, w.tmp, H, Th, H, c.ffn,
                     HT(h, hub_layer(l, "feed_forward.output_dense.bias")), 0, w.x, H);
        bad |= ln(st, w.tmp, w.x, Th, H, HT(h, hub_layer(l, "final_layer_norm.weight")), HT(h, hub_layer(l, "final_layer_norm.bias")), c.eps);
    }
    // [Th][H] -> ssl [H][Th]
    transpose_kernel<<<dim3((H + 31) / 32, (Th + 31) / 32), 256, 0, st>>>(w.x, H, ssl, Th, Th, H);
    if (bad) return abi_fail(GSV_ERR_HIP, "hubert: a forward launch failed");
    RCHK(hipGetLastError());
    return GSV_OK;
}

}  // extern "C"
