// C-ABI of the reference-audio path (include/gsv_tts_hip.h, "reference audio" section; kernels in refaudio.h), of
// CN-HuBERT (gsv_hubert_*; kernels in hubert.h, which shares refaudio.h's fgemm) and of ERes2NetV2 with its resampler and
// fbank (gsv_sv_*; kernels in sv.h, which uses the same fgemm for the DFT and the mel filter bank) and of Chinese RoBERTa
// (gsv_roberta_*; kernels in roberta.h, which reuses hubert.h's LayerNorm and fgemm's tile body), and the WAV sample
// conversion in front of them all (gsv_wav_*; kernel in wavpcm.h) with the FLAC frame decode that feeds it (gsv_flac_*;
// flacdec.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/gsv_tts_hip.h"
#include "gsv_error.h"
#include "hubert.h"
#include "refaudio.h"
#include "roberta.h"
#include "sv.h"
#include "wavpcm.h"
#include "flacdec.h"

using namespace gsv;

static_assert(WAV_U8 == GSV_PCM_U8 && WAV_S16 == GSV_PCM_S16 && WAV_S24 == GSV_PCM_S24 && WAV_S32 == GSV_PCM_S32 &&
              WAV_F32 == GSV_PCM_F32 && WAV_F64 == GSV_PCM_F64, "wavpcm.h's formats are the ABI's GSV_PCM_* codes");
static_assert(AUX_MAX_CLIPS == GSV_AUX_MAX_CLIPS, "the kernels' per-clip argument arrays hold GSV_AUX_MAX_CLIPS clips");

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

// workspace carve-up of one forward, in floats (256-byte slots); the same walk sizes and assigns it.  T: the encoder
// frames of the (longest) clip; rows / prows: the transformer rows and the padded positional-conv rows; feat_rows: rows of
// a batch's packed encoder output (0 for one clip, whose encoder output stays in act)
struct HubWs {
    float *act[2], *pmean, *pm2, *gmean, *gscale, *hid, *pg, *part, *x, *tmp, *qkv, *att, *ffn, *feat;
    size_t total;
};
HubWs hub_carve(const gsv_hubert_config& c, const int* T, size_t rows, size_t prows, size_t feat_rows, float* base) {
    HubWs w;
    size_t off = 0;
    auto take = [&](size_t n) { float* r = base ? base + off : nullptr; off += up(n); return r; };
    size_t a0 = 0, a1 = 0;   // ping-pong: conv i writes act[i & 1]
    for (int i = 0; i < c.n_conv; ++i) {
        size_t& a = (i & 1) ? a1 : a0;
        a = std::max(a, (size_t)T[i] * c.conv_dim[i]);
    }
    const int C0 = c.conv_dim[0], nch = (T[0] + GN_ROWS - 1) / GN_ROWS;
    const size_t H = c.hidden;
    w.act[0] = take(a0);
    w.act[1] = take(a1);
    w.pmean = take((size_t)nch * C0);
    w.pm2 = take((size_t)nch * C0);
    w.gmean = take(C0);
    w.gscale = take(C0);
    w.hid = take(rows * H);
    w.pg = take(prows * H);
    w.part = take(POS_SPLIT * rows * H);
    w.x = take(rows * H);
    w.tmp = take(rows * H);
    w.qkv = take(rows * 3 * H);
    w.att = take(rows * H);
    w.ffn = take(rows * c.ffn);
    w.feat = take(feat_rows * c.conv_dim[c.n_conv - 1]);
    w.total = off;
    return w;
}

// one clip's carve-up
HubWs hub_carve1(const gsv_hubert_config& c, const int* T, float* base) {
    const size_t Th = T[c.n_conv - 1];
    return hub_carve(c, T, Th, Th + c.pos_k - 1, 0, base);
}

// a batch: every clip's encoder frames, its first sample, and the packing of its rows
struct HubBatch {
    int n, longest;                                  // clips; the longest (the largest encoder buffers)
    int T[GSV_AUX_MAX_CLIPS][GSV_HUBERT_MAX_CONV];
    long long a0[GSV_AUX_MAX_CLIPS];
    HubClips cl;
    int rows, prows;                                 // packed transformer rows, padded positional-conv rows
};
// -1, or the index of the first clip too short for the feature encoder (n when the packed rows overflow)
int hub_batch(const gsv_hubert_config& c, const int* ns, int n, HubBatch& b) {
    b.n = n;
    b.longest = 0;
    b.cl.n = n;
    long long a = 0, rows = 0, prows = 0;
    for (int i = 0; i < n; ++i) {
        if (!hub_frames(c, ns[i], b.T[i])) return i;
        const int Th = b.T[i][c.n_conv - 1];
        b.a0[i] = a;
        b.cl.row0[i] = (int)rows;
        b.cl.prow0[i] = (int)prows;
        b.cl.T[i] = Th;
        a += ns[i];
        rows += Th;
        prows += Th + c.pos_k - 1;
        if (prows > 0x7fffffff) return n;
        if (ns[i] > ns[b.longest]) b.longest = i;
    }
    b.rows = (int)rows;
    b.prows = (int)prows;
    return -1;
}

HubWs hub_carve_batch(const gsv_hubert_config& c, const HubBatch& b, float* base) {
    return hub_carve(c, b.T[b.longest], b.rows, b.prows, b.rows, base);
}

int ln(hipStream_t st, const float* x, float* y, int rows, int C, const float* g, const float* b, float eps) {
    ln_rows_kernel<<<(rows + 3) / 4, 256, 0, st>>>(x, y, rows, C, g, b, eps);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

// feature encoder of one clip: conv 0 as rows of k0 samples at stride s0 over the waveform, GroupNorm(C0, C0) over the
// clip's T0 frames + GELU, then convs 1.. (rows of k * cin values at stride s * cin over the channels-last activations,
// GELU epilogue).  The last conv writes out [T_last][C_last], the others ping-pong through w.act.
int hub_encoder(gsv_hubert* h, hipStream_t st, const float* audio, const int* T, const HubWs& w, float* out) {
    const gsv_hubert_config& c = h->cfg;
    const int C0 = c.conv_dim[0];
    auto dst = [&](int i) { return i == c.n_conv - 1 ? out : w.act[i & 1]; };
    int bad = fgemm(st, audio, c.conv_stride[0], HT(h, "feature_extractor.conv_layers.0.conv.weight"), c.conv_kernel[0], dst(0),
                    C0, T[0], C0, c.conv_kernel[0]);
    const int nch = (T[0] + GN_ROWS - 1) / GN_ROWS;
    gn_partial_kernel<<<dim3(C0 / 64, nch), 256, 0, st>>>(dst(0), T[0], C0, w.pmean, w.pm2);
    gn_finalize_kernel<<<(C0 + 255) / 256, 256, 0, st>>>(w.pmean, w.pm2, nch, T[0], C0, HT(h, "feature_extractor.conv_layers.0.layer_norm.weight"),
                                                        1e-5f, w.gmean, w.gscale);
    const long long n4 = (long long)T[0] * C0 / 4;
    gn_apply_gelu_kernel<<<(unsigned)((n4 + 255) / 256), 256, 0, st>>>(dst(0), n4, C0, w.gmean, w.gscale,
                                                                       HT(h, "feature_extractor.conv_layers.0.layer_norm.bias"));
    for (int i = 1; i < c.n_conv; ++i) {
        const int ci = c.conv_dim[i - 1], co = c.conv_dim[i];
        bad |= fgemm(st, dst(i - 1), (long long)c.conv_stride[i] * ci, h->w_conv[i], (long long)c.conv_kernel[i] * ci, dst(i), co,
                     T[i], co, c.conv_kernel[i] * ci, nullptr, 2);
    }
    return bad;
}

// everything after the encoder, over `rows` packed rows of feat [rows][C_last] -> w.x [rows][H]: cl null for one clip
// (the single-clip kernels), else the clips it describes (prows padded rows in w.pg)
int hub_body(gsv_hubert* h, hipStream_t st, const HubWs& w, float* feat, int rows, const HubClips* cl, int prows) {
    const gsv_hubert_config& c = h->cfg;
    const int H = c.hidden, CL = c.conv_dim[c.n_conv - 1];
    const int G = c.pos_groups, cg = H / G, K = c.pos_k;
    int tmax = rows;   // the longest clip's frames
    if (cl) {
        tmax = 0;
        for (int z = 0; z < cl->n; ++z) tmax = std::max(tmax, cl->T[z]);
    }
    int bad = 0;
    // feature projection: LayerNorm(CL) in place, Linear CL -> H
    bad |= ln(st, feat, feat, rows, CL, HT(h, "feature_projection.layer_norm.weight"), HT(h, "feature_projection.layer_norm.bias"), c.eps);
    bad |= fgemm(st, feat, CL, HT(h, "feature_projection.projection.weight"), CL, w.hid, H, rows, H, CL, HT(h, "feature_projection.projection.bias"));
    // positional conv over the group-major padded copy: tmp = hid + gelu(conv(hid) + bias), the last frame never made
    {
        const long long np = (long long)G * (tmax + K - 1) * cg, n = (long long)rows * H;
        if (!cl) {
            pos_pad_group_kernel<<<(unsigned)((np + 255) / 256), 256, 0, st>>>(w.hid, rows, H, G, K, w.pg);
            pos_conv_split_kernel<<<dim3((cg + 63) / 64, (rows + 63) / 64, G * POS_SPLIT), 256, 0, st>>>(w.pg, h->w_pos, w.part, rows, H, G, K);
        } else {
            pos_pad_group_batch_kernel<<<dim3((unsigned)((np + 255) / 256), cl->n), 256, 0, st>>>(w.hid, H, G, K, prows, *cl, w.pg);
            pos_conv_split_batch_kernel<<<dim3((cg + 63) / 64 * cl->n, (tmax + 63) / 64, G * POS_SPLIT), 256, 0, st>>>(
                w.pg, prows, h->w_pos, w.part, rows, H, G, K, *cl);
        }
        pos_reduce_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(w.part, n, H, HT(h, "encoder.pos_conv_embed.conv.bias"), w.hid, w.tmp);
    }
    bad |= ln(st, w.tmp, w.x, rows, H, HT(h, "encoder.layer_norm.weight"), HT(h, "encoder.layer_norm.bias"), c.eps);
    const float scale = 1.f / sqrtf(64.f);
    for (int l = 0; l < c.n_layer; ++l) {
        bad |= fgemm(st, w.x, H, h->w_qkv[l], H, w.qkv, 3 * H, rows, 3 * H, H, h->b_qkv[l]);
        if (!cl)
            hubert_attn_kernel<<<dim3((rows + ATT_QB - 1) / ATT_QB, c.n_head), 128, 0, st>>>(w.qkv, 3 * H, rows, H, scale, w.att, H);
        else
            hubert_attn_batch_kernel<<<dim3((tmax + ATT_QB - 1) / ATT_QB, c.n_head, cl->n), 128, 0, st>>>(w.qkv, 3 * H, H, scale, w.att, H, *cl);
        bad |= fgemm(st, w.att, H, HT(h, hub_layer(l, "attention.out_proj.weight")), H, w.tmp, H, rows, H, H,
                     HT(h, hub_layer(l, "attention.out_proj.bias")), 0, w.x, H);
        bad |= ln(st, w.tmp, w.x, rows, H, HT(h, hub_layer(l, "layer_norm.weight")), HT(h, hub_layer(l, "layer_norm.bias")), c.eps);
        bad |= fgemm(st, w.x, H, HT(h, hub_layer(l, "feed_forward.intermediate_dense.weight")), H, w.ffn, c.ffn, rows, c.ffn, H,
                     HT(h, hub_layer(l, "feed_forward.intermediate_dense.bias")), 2);
        bad |= fgemm(st, w.ffn, c.ffn, HT(h, hub_layer(l, "feed_forward.output_dense.weight")), c.ffn, w.tmp, H, rows, H, c.ffn,
                     HT(h, hub_layer(l, "feed_forward.output_dense.bias")), 0, w.x, H);
        bad |= ln(st, w.tmp, w.x, rows, H, HT(h, hub_layer(l, "final_layer_norm.weight")), HT(h, hub_layer(l, "final_layer_norm.bias")), c.eps);
    }
    return bad;
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
    return sizeof(float) * hub_carve1(h->cfg, T, nullptr).total;
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
    const HubWs w = hub_carve1(c, T, static_cast<float*>(workspace));
    const int H = c.hidden, Th = T[c.n_conv - 1];
    float* feat = w.act[(c.n_conv - 1) & 1];
    int bad = hub_encoder(h, st, audio, T, w, feat);
    bad |= hub_body(h, st, w, feat, Th, nullptr, 0);
    // [Th][H] -> ssl [H][Th]
    transpose_kernel<<<dim3((H + 31) / 32, (Th + 31) / 32), 256, 0, st>>>(w.x, H, ssl, Th, Th, H);
    if (bad) return abi_fail(GSV_ERR_HIP, "hubert: a forward launch failed");
    RCHK(hipGetLastError());
    return GSV_OK;
}

size_t gsv_hubert_batch_workspace(gsv_hubert* h, const int* n_samples, int n_clips) {
    if (!h || !n_samples || n_clips < 1 || n_clips > GSV_AUX_MAX_CLIPS) return 0;
    HubBatch b;
    if (hub_batch(h->cfg, n_samples, n_clips, b) >= 0) return 0;
    return sizeof(float) * hub_carve_batch(h->cfg, b, nullptr).total;
}

int gsv_hubert_forward_batch(gsv_hubert* h, const float* audio, const int* n_samples, int n_clips, float* ssl, void* workspace,
                             size_t workspace_bytes, void* stream) {
    if (!h || !audio || !n_samples || !ssl || !workspace) return abi_fail(GSV_ERR_ARG, "null argument");
    if (!h->finalized) return abi_fail(GSV_ERR_STATE, "hubert: not finalized");
    if (n_clips < 1 || n_clips > GSV_AUX_MAX_CLIPS) return abi_fail(GSV_ERR_ARG, "hubert: %d clips (1..%d per call)", n_clips, GSV_AUX_MAX_CLIPS);
    const gsv_hubert_config& c = h->cfg;
    HubBatch b;
    const int badc = hub_batch(c, n_samples, n_clips, b);
    if (badc == n_clips) return abi_fail(GSV_ERR_ARG, "hubert: the batch's packed frames overflow");
    if (badc >= 0)
        return abi_fail(GSV_ERR_ARG, "hubert: clip %d: %d samples are too short for the feature encoder", badc, n_samples[badc]);
    if (workspace_bytes < sizeof(float) * hub_carve_batch(c, b, nullptr).total) return abi_fail(GSV_ERR_ARG, "hubert: workspace too small");
    if ((reinterpret_cast<size_t>(workspace) & 15) != 0) return abi_fail(GSV_ERR_ARG, "hubert: workspace must be 16-byte aligned");
    hipStream_t st = S(stream);
    const HubWs w = hub_carve_batch(c, b, static_cast<float*>(workspace));
    const int H = c.hidden, CL = c.conv_dim[c.n_conv - 1];
    int bad = 0;
    // the encoder per clip (its GroupNorm statistics are the clip's own), each into its rows of the packed feat
    for (int i = 0; i < n_clips; ++i) bad |= hub_encoder(h, st, audio + b.a0[i], b.T[i], w, w.feat + (long long)b.cl.row0[i] * CL);
    bad |= hub_body(h, st, w, w.feat, b.rows, &b.cl, b.prows);
    // clip i's rows [Th_i][H] -> its ssl block [H][Th_i] at H * row0
    for (int i = 0; i < n_clips; ++i) {
        const int Th = b.cl.T[i];
        const long long r0 = b.cl.row0[i];
        transpose_kernel<<<dim3((H + 31) / 32, (Th + 31) / 32), 256, 0, st>>>(w.x + r0 * H, H, ssl + r0 * H, Th, Th, H);
    }
    if (bad) return abi_fail(GSV_ERR_HIP, "hubert: a batched forward launch failed");
    RCHK(hipGetLastError());
    return GSV_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------------------------
// ERes2NetV2 (speaker verification): resample, fbank, forward3
// ------------------------------------------------------------------------------------------------------------------
struct gsv_sv {
    gsv_sv_config cfg;
    std::map<std::string, std::pair<float*, int64_t>> t;   // loaded tensors (device, fp32)
    bool finalized = false;
    struct Conv { float* w; float* b; int cout, cin, k; };
    std::map<std::string, Conv> conv;                       // BN-folded, [cout][k][k][cin], keyed by the conv's name
    float* dft = nullptr;                                   // [2 * 257][512]
    float* mel = nullptr;                                   // [80][257]
    std::vector<void*> owned;
};

namespace {

int sv_alloc(gsv_sv* h, float** p, size_t floats) {
    RCHK(hipMalloc(reinterpret_cast<void**>(p), floats * sizeof(float)));
    h->owned.push_back(*p);
    return GSV_OK;
}

int gcd_i(int a, int b) { while (b) { const int r = a % b; a = b; b = r; } return a; }

// gcd-reduced rates and the kernel half-width of torchaudio's sinc resampler; false on bad rates
bool rs_params(int orig, int nw, int* o, int* n, int* width) {
    if (orig < 1 || nw < 1) return false;
    const int g = gcd_i(orig, nw);
    *o = orig / g;
    *n = nw / g;
    *width = (int)std::ceil(6.0 * *o / ((double)std::min(*o, *n) * 0.99));
    return (long long)*n * (2 * *width + *o) <= (1LL << 24);
}

long long rs_length(long long n, int orig, int nw) {
    int o, w, width;
    if (n < 0 || !rs_params(orig, nw, &o, &w, &width)) return -1;
    if (o == w) return n;
    return (w * n + o - 1) / o;
}

int fb_frames(long long n16) { return n16 < FB_WIN ? 0 : (int)(1 + (n16 - FB_WIN) / FB_HOP); }

// stage geometry: frequency rows F[s], frames T[s] (stage 0 stride 1, stages 1-3 stride 2 in both axes)
struct SvGeo { int F[4], T[4]; };
SvGeo sv_geo(const gsv_sv_config& c, int T) {
    SvGeo g;
    int f = c.feat_dim, t = T;
    for (int s = 0; s < 4; ++s) {
        if (s > 0) { f = (f + 1) / 2; t = (t + 1) / 2; }
        g.F[s] = f;
        g.T[s] = t;
    }
    return g;
}

// the clips of one forward3 (one for the single-clip calls): every clip's frames and the pixel offset of its padded
// [F + 2][T + 2] image at each stage geometry ("level" s: stage s; level 0 is also the stem's), and its first fbank row
struct SvBatch {
    int n;
    int F[4];
    int T[4][GSV_AUX_MAX_CLIPS];
    long long off[4][GSV_AUX_MAX_CLIPS];
    size_t px[4];                          // pixels of all clips' images at each level
    int feat0[GSV_AUX_MAX_CLIPS];
    size_t rows;                           // fbank rows of all clips
};
SvBatch sv_batch(const gsv_sv_config& c, const int* T, int n) {
    SvBatch b;
    b.n = n;
    b.rows = 0;
    for (int s = 0; s < 4; ++s) b.px[s] = 0;
    for (int i = 0; i < n; ++i) {
        const SvGeo g = sv_geo(c, T[i]);
        for (int s = 0; s < 4; ++s) {
            b.F[s] = g.F[s];
            b.T[s][i] = g.T[s];
            b.off[s][i] = (long long)b.px[s];
            b.px[s] += (size_t)(g.F[s] + 2) * (g.T[s] + 2);
        }
        b.feat0[i] = (int)b.rows;
        b.rows += T[i];
    }
    return b;
}

// workspace of one embed: resample table and output, fbank buffers, then the model's zero-padded activations.  A batch
// (n_max: its longest clip, whose buffers the per-clip resample / fbank reuse) keeps every clip's fbank rows and every
// clip's images of each model buffer back to back.
struct SvWs {
    float *tab, *y16, *fr, *Z, *P, *E, *feat;
    float *model;                          // start of the zero-filled model region
    float *in0, *stem;
    float *x[4][2], *c1[4], *cat[4], *hh[4], *fu[4];
    float *ds, *h34, *fuse;
    size_t model_floats, total;
};
SvWs sv_carve_batch(const gsv_sv_config& c, long long n_max, int sr, const SvBatch& b, float* base) {
    SvWs w;
    size_t off = 0;
    auto take = [&](size_t k) { float* r = base ? base + off : nullptr; off += up(k); return r; };
    int o = 1, nw = 1, width = 0;
    rs_params(sr, 16000, &o, &nw, &width);
    const long long n16 = rs_length(n_max, sr, 16000);
    const int T = fb_frames(n16);
    w.tab = take(o == nw ? 0 : (size_t)nw * (2 * width + o));
    w.y16 = take(sr == 16000 ? 0 : (size_t)n16);
    w.fr = take((size_t)T * FB_NFFT);
    w.Z = take((size_t)T * 2 * FB_BINS);
    w.P = take((size_t)T * FB_BINS);
    w.E = take((size_t)T * FB_MELS);
    w.feat = take(b.rows * FB_MELS);
    const size_t m0 = off;
    w.model = base ? base + off : nullptr;
    const int m = c.m_channels;
    w.in0 = take(b.px[0]);
    w.stem = take(b.px[0] * m);
    for (int s = 0; s < 4; ++s) {
        const size_t p = b.px[s];
        const int C = 4 * (m << s), wd = c.width[s];
        w.x[s][0] = take(p * C);
        w.x[s][1] = take(p * C);
        w.c1[s] = take(p * 4 * wd);
        w.cat[s] = take(p * 4 * wd);
        w.hh[s] = s >= 2 ? take(p * (wd / 4)) : nullptr;
        w.fu[s] = s >= 2 ? take(p * wd) : nullptr;
    }
    const size_t p4 = b.px[3];
    w.ds = take(p4 * 32 * m);
    w.h34 = take(p4 * 8 * m);
    w.fuse = take(p4 * 32 * m);
    w.model_floats = off - m0;
    w.total = off;
    return w;
}

// one clip of n samples at sr
SvWs sv_carve(const gsv_sv_config& c, long long n, int sr, float* base) {
    const int T = fb_frames(rs_length(n, sr, 16000));
    return sv_carve_batch(c, n, sr, sv_batch(c, &T, 1), base);
}

std::string sv_blk(int s, int b, const char* rest) {
    return "layer" + std::to_string(s + 1) + "." + std::to_string(b) + "." + rest;
}

// every conv forward3 runs: (conv name, weight, BN prefix or "", conv bias or "", cout, cin, k)
struct SvConvSpec { std::string key, weight, bn, bias; int cout, cin, k; };
std::vector<SvConvSpec> sv_specs(const gsv_sv_config& c) {
    std::vector<SvConvSpec> v;
    const int m = c.m_channels;
    v.push_back({"conv1", "conv1.weight", "bn1.", "", m, 1, 3});
    int in = m;
    for (int s = 0; s < 4; ++s) {
        const int P = m << s, C = 4 * P, wd = c.width[s];
        for (int b = 0; b < c.blocks[s]; ++b) {
            const int stride = (b == 0 && s > 0) ? 2 : 1;
            v.push_back({sv_blk(s, b, "conv1"), sv_blk(s, b, "conv1.weight"), sv_blk(s, b, "bn1."), "", 4 * wd, in, 1});
            for (int i = 0; i < 4; ++i) {
                const std::string ci = "convs." + std::to_string(i), bi = "bns." + std::to_string(i) + ".";
                v.push_back({sv_blk(s, b, ci.c_str()), sv_blk(s, b, (ci + ".weight").c_str()), sv_blk(s, b, bi.c_str()), "", wd, wd, 3});
            }
            if (s >= 2)
                for (int j = 0; j < 3; ++j) {
                    const std::string f = "fuse_models." + std::to_string(j) + ".local_att.";
                    v.push_back({sv_blk(s, b, (f + "0").c_str()), sv_blk(s, b, (f + "0.weight").c_str()), sv_blk(s, b, (f + "1.").c_str()),
                                 sv_blk(s, b, (f + "0.bias").c_str()), wd / 4, 2 * wd, 1});
                    v.push_back({sv_blk(s, b, (f + "3").c_str()), sv_blk(s, b, (f + "3.weight").c_str()), sv_blk(s, b, (f + "4.").c_str()),
                                 sv_blk(s, b, (f + "3.bias").c_str()), wd, wd / 4, 1});
                }
            v.push_back({sv_blk(s, b, "conv3"), sv_blk(s, b, "conv3.weight"), sv_blk(s, b, "bn3."), "", C, 4 * wd, 1});
            if (stride != 1 || in != C)
                v.push_back({sv_blk(s, b, "shortcut"), sv_blk(s, b, "shortcut.0.weight"), sv_blk(s, b, "shortcut.1."), "", C, in, 1});
            in = C;
        }
    }
    v.push_back({"layer3_ds", "layer3_ds.weight", "", "", 32 * m, 16 * m, 3});
    v.push_back({"fuse34.0", "fuse34.local_att.0.weight", "fuse34.local_att.1.", "fuse34.local_att.0.bias", 8 * m, 64 * m, 1});
    v.push_back({"fuse34.3", "fuse34.local_att.3.weight", "fuse34.local_att.4.", "fuse34.local_att.3.bias", 32 * m, 8 * m, 1});
    return v;
}

// one conv over padded channels-last buffers: input at level lin (geometry F[lin] x T[lin][clip]), output at level lin
// (stride 1) or lin + 1 (stride 2: (Fi - 1) / 2 + 1 x (Ti - 1) / 2 + 1); one clip runs sv_conv_kernel, a batch
// sv_conv_batch_kernel with a clip grid dimension
struct SvIO {
    const float* x1; const float* x2; int src, ldx;
    float* y; int ldy;
    const float* r = nullptr; int ldr = 0;
    const float* a = nullptr; int lda = 0; const float* b = nullptr; int ldb = 0;
};
int sv_conv(hipStream_t st, const gsv_sv::Conv& cw, int stride, const SvBatch& B, int lin, const SvIO& io, int act) {
    const int Fi = B.F[lin], lout = stride == 1 ? lin : lin + 1;
    SvConvArgs a;
    a.X1 = io.x1; a.X2 = io.x2; a.src = io.src; a.ldx = io.ldx; a.Tpi = B.T[lin][0] + 2;
    a.Cin = io.src == SV_SRC_CAT ? cw.cin / 2 : cw.cin;
    a.k = cw.k; a.s = stride; a.W = cw.w; a.bias = cw.b;
    a.Y = io.y; a.ldy = io.ldy;
    a.Fo = (Fi - 1) / stride + 1; a.To = (B.T[lin][0] - 1) / stride + 1; a.N = cw.cout;
    a.R = io.r; a.ldr = io.ldr; a.A = io.a; a.lda = io.lda; a.B = io.b; a.ldb = io.ldb; a.act = act;
    if (B.n == 1) {
        const long long M = (long long)a.Fo * a.To;
        if (a.N <= 32)
            sv_conv_kernel<4, 1><<<dim3((a.N + 31) / 32, (unsigned)((M + 127) / 128)), 256, 0, st>>>(a);
        else
            sv_conv_kernel<2, 2><<<dim3((a.N + 63) / 64, (unsigned)((M + 63) / 64)), 256, 0, st>>>(a);
        return hipGetLastError() == hipSuccess ? 0 : 1;
    }
    SvClips cl;
    int tmax = 0;
    for (int z = 0; z < B.n; ++z) {
        cl.in_off[z] = B.off[lin][z];
        cl.out_off[z] = B.off[lout][z];
        cl.Ti[z] = B.T[lin][z];
        cl.To[z] = B.T[lout][z];
        tmax = std::max(tmax, cl.To[z]);
    }
    const long long M = (long long)a.Fo * tmax;
    if (a.N <= 32)
        sv_conv_batch_kernel<4, 1><<<dim3((a.N + 31) / 32, (unsigned)((M + 127) / 128), B.n), 256, 0, st>>>(a, cl);
    else
        sv_conv_batch_kernel<2, 2><<<dim3((a.N + 63) / 64, (unsigned)((M + 63) / 64), B.n), 256, 0, st>>>(a, cl);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

int sv_resample_run(hipStream_t st, const float* x, int n, int orig, int nw_sr, float* y, float* tab) {
    int o, nw, width;
    rs_params(orig, nw_sr, &o, &nw, &width);
    if (o == nw) {
        if (n > 0) RCHK(hipMemcpyAsync(y, x, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, st));
        return GSV_OK;
    }
    const int L = 2 * width + o;
    const long long n_out = rs_length(n, orig, nw_sr);
    sv_resample_table_kernel<<<(nw * L + 255) / 256, 256, 0, st>>>(tab, o, nw, width);
    if (n_out > 0) sv_resample_kernel<<<(unsigned)((n_out + 255) / 256), 256, 0, st>>>(x, n, tab, o, nw, width, y, (int)n_out);
    RCHK(hipGetLastError());
    return GSV_OK;
}

int sv_fbank_run(gsv_sv* h, hipStream_t st, const float* x16, int T, float* feat, const SvWs& w) {
    sv_frames_kernel<<<T, 256, 0, st>>>(x16, w.fr);
    int bad = fgemm(st, w.fr, FB_NFFT, h->dft, FB_NFFT, w.Z, 2 * FB_BINS, T, 2 * FB_BINS, FB_NFFT);
    const long long np = (long long)T * FB_BINS, ne = (long long)T * FB_MELS;
    sv_power_kernel<<<(unsigned)((np + 255) / 256), 256, 0, st>>>(w.Z, T, w.P);
    bad |= fgemm(st, w.P, FB_BINS, h->mel, FB_BINS, w.E, FB_MELS, T, FB_MELS, FB_BINS);
    sv_log_kernel<<<(unsigned)((ne + 255) / 256), 256, 0, st>>>(w.E, ne, feat);
    if (bad) return abi_fail(GSV_ERR_HIP, "sv: an fbank launch failed");
    RCHK(hipGetLastError());
    return GSV_OK;
}

int sv_forward_run(gsv_sv* h, hipStream_t st, const float* feat, const SvBatch& B, float* emb, const SvWs& w) {
    const gsv_sv_config& c = h->cfg;
    const int m = c.m_channels, F = c.feat_dim;
    auto CW = [&](const std::string& k) -> const gsv_sv::Conv& { return h->conv.at(k); };
    RCHK(hipMemsetAsync(w.model, 0, w.model_floats * sizeof(float), st));
    for (int i = 0; i < B.n; ++i) {
        const int T = B.T[0][i];
        const long long nf = (long long)T * F;
        sv_feat_pad_kernel<<<(unsigned)((nf + 255) / 256), 256, 0, st>>>(feat + (long long)B.feat0[i] * F, T, F, w.in0 + B.off[0][i]);
    }
    int bad = 0;
    {
        SvIO io{w.in0, nullptr, SV_SRC_ONE, 1, w.stem, m};
        bad |= sv_conv(st, CW("conv1"), 1, B, 0, io, SV_ACT_RELU);   // F.relu(bn1(conv1(x)))
    }
    const float* prev = w.stem;
    int in = m;
    for (int s = 0; s < 4; ++s) {
        const int C = 4 * (m << s), wd = c.width[s], W4 = 4 * wd;
        for (int b = 0; b < c.blocks[s]; ++b) {
            const int stride = (b == 0 && s > 0) ? 2 : 1;
            const float* X = b == 0 ? prev : w.x[s][(b - 1) & 1];
            const int lin = stride == 2 ? s - 1 : s;   // the block's input level
            float* Y = w.x[s][b & 1];
            SvIO i1{X, nullptr, SV_SRC_ONE, in, w.c1[s], W4};
            bad |= sv_conv(st, CW(sv_blk(s, b, "conv1")), stride, B, lin, i1, SV_ACT_HTANH);
            const float* R = X;
            if (stride != 1 || in != C) {
                SvIO isc{X, nullptr, SV_SRC_ONE, in, w.x[s][1], C};   // block 0 only: its output is x[s][0]
                bad |= sv_conv(st, CW(sv_blk(s, b, "shortcut")), stride, B, lin, isc, SV_ACT_NONE);
                R = w.x[s][1];
            }
            for (int i = 0; i < 4; ++i) {
                SvIO ic{w.c1[s], nullptr, SV_SRC_ONE, W4, w.cat[s] + i * wd, W4};
                if (i > 0 && s < 2) {            // sp = sp + spx[i]
                    ic.x1 = w.cat[s] + (i - 1) * wd;
                    ic.x2 = w.c1[s] + i * wd;
                    ic.src = SV_SRC_ADD;
                } else if (i > 0) {              // sp = AFF(sp, spx[i])
                    const std::string f = "fuse_models." + std::to_string(i - 1) + ".local_att.";
                    SvIO ih{w.cat[s] + (i - 1) * wd, w.c1[s] + i * wd, SV_SRC_CAT, W4, w.hh[s], wd / 4};
                    bad |= sv_conv(st, CW(sv_blk(s, b, (f + "0").c_str())), 1, B, s, ih, SV_ACT_SILU);
                    SvIO ia{w.hh[s], nullptr, SV_SRC_ONE, wd / 4, w.fu[s], wd};
                    ia.a = w.cat[s] + (i - 1) * wd; ia.lda = W4;
                    ia.b = w.c1[s] + i * wd; ia.ldb = W4;
                    bad |= sv_conv(st, CW(sv_blk(s, b, (f + "3").c_str())), 1, B, s, ia, SV_ACT_AFF);
                    ic.x1 = w.fu[s];
                    ic.ldx = wd;
                } else {
                    ic.x1 = w.c1[s];
                }
                bad |= sv_conv(st, CW(sv_blk(s, b, ("convs." + std::to_string(i)).c_str())), 1, B, s, ic, SV_ACT_HTANH);
            }
            SvIO i3{w.cat[s], nullptr, SV_SRC_ONE, W4, Y, C};
            i3.r = R;
            i3.ldr = C;
            bad |= sv_conv(st, CW(sv_blk(s, b, "conv3")), 1, B, s, i3, SV_ACT_HTANH);
            in = C;
        }
        prev = w.x[s][(c.blocks[s] - 1) & 1];
    }
    const float* out3 = w.x[2][(c.blocks[2] - 1) & 1];
    const float* out4 = prev;
    const int C4 = 32 * m, F3 = B.F[3];
    {
        SvIO ids{out3, nullptr, SV_SRC_ONE, 16 * m, w.ds, C4};
        bad |= sv_conv(st, CW("layer3_ds"), 2, B, 2, ids, SV_ACT_NONE);
        SvIO ih{out4, w.ds, SV_SRC_CAT, C4, w.h34, 8 * m};
        bad |= sv_conv(st, CW("fuse34.0"), 1, B, 3, ih, SV_ACT_SILU);
        SvIO ia{w.h34, nullptr, SV_SRC_ONE, 8 * m, w.fuse, C4};
        ia.a = out4; ia.lda = C4; ia.b = w.ds; ia.ldb = C4;
        bad |= sv_conv(st, CW("fuse34.3"), 1, B, 3, ia, SV_ACT_AFF);
    }
    // clip i's time mean -> emb[i] (emb_dim = C4 * F3)
    for (int i = 0; i < B.n; ++i)
        sv_mean_kernel<<<(F3 * C4 + 255) / 256, 256, 0, st>>>(w.fuse + B.off[3][i] * C4, F3, B.T[3][i], C4,
                                                              emb + (long long)i * C4 * F3);
    if (bad) return abi_fail(GSV_ERR_HIP, "sv: a forward launch failed");
    RCHK(hipGetLastError());
    return GSV_OK;
}

int sv_check_ws(gsv_sv* h, long long n, int sr, void* ws, size_t bytes) {
    if (!h->finalized) return abi_fail(GSV_ERR_STATE, "sv: not finalized");
    if (!ws) return abi_fail(GSV_ERR_ARG, "null argument");
    if (bytes < sizeof(float) * sv_carve(h->cfg, n, sr, nullptr).total) return abi_fail(GSV_ERR_ARG, "sv: workspace too small");
    if ((reinterpret_cast<size_t>(ws) & 15) != 0) return abi_fail(GSV_ERR_ARG, "sv: workspace must be 16-byte aligned");
    return GSV_OK;
}

// a batch's fbank frames per clip and its longest clip (in samples), from host sample counts at sr
struct SvBatchIn {
    int T[GSV_AUX_MAX_CLIPS];
    long long n_max;
};
int sv_batch_in(const int* ns, int n, int sr, SvBatchIn& in) {
    if (!ns) return abi_fail(GSV_ERR_ARG, "null argument");
    if (n < 1 || n > GSV_AUX_MAX_CLIPS) return abi_fail(GSV_ERR_ARG, "sv: %d clips (1..%d per call)", n, GSV_AUX_MAX_CLIPS);
    int o, nw, width;
    if (!rs_params(sr, 16000, &o, &nw, &width)) return abi_fail(GSV_ERR_ARG, "sv: sample rate %d unsupported", sr);
    in.n_max = 0;
    for (int i = 0; i < n; ++i) {
        const long long n16 = rs_length(ns[i], sr, 16000);
        in.T[i] = n16 < 0 ? 0 : fb_frames(n16);
        if (in.T[i] < 1)
            return abi_fail(GSV_ERR_ARG, "sv: clip %d: %d samples at %d Hz are too short for one fbank frame", i, ns[i], sr);
        in.n_max = std::max(in.n_max, (long long)ns[i]);
    }
    return GSV_OK;
}

int sv_check_batch(gsv_sv* h, const int* ns, int n, int sr, void* ws, size_t bytes, SvBatchIn& in) {
    if (!h->finalized) return abi_fail(GSV_ERR_STATE, "sv: not finalized");
    int rc;
    if ((rc = sv_batch_in(ns, n, sr, in))) return rc;
    if (!ws) return abi_fail(GSV_ERR_ARG, "null argument");
    if (bytes < sizeof(float) * sv_carve_batch(h->cfg, in.n_max, sr, sv_batch(h->cfg, in.T, n), nullptr).total)
        return abi_fail(GSV_ERR_ARG, "sv: workspace too small");
    if ((reinterpret_cast<size_t>(ws) & 15) != 0) return abi_fail(GSV_ERR_ARG, "sv: workspace must be 16-byte aligned");
    return GSV_OK;
}

}  // namespace

extern "C" {

int gsv_sv_create(const gsv_sv_config* cfg, gsv_sv** out) {
    if (!cfg || !out) return abi_fail(GSV_ERR_ARG, "null argument");
    const gsv_sv_config& c = *cfg;
    if (c.scale != 4) return abi_fail(GSV_ERR_ARG, "sv: scale %d unsupported (ERes2NetV2 with scale 4 only)", c.scale);
    if (c.expansion != 4) return abi_fail(GSV_ERR_ARG, "sv: expansion %d unsupported (4 only)", c.expansion);
    if (c.feat_dim != 80) return abi_fail(GSV_ERR_ARG, "sv: feat_dim %d unsupported (80-bin fbank only)", c.feat_dim);
    if (c.m_channels < 1 || c.m_channels > 1024) return abi_fail(GSV_ERR_ARG, "sv: m_channels %d unsupported", c.m_channels);
    for (int s = 0; s < 4; ++s) {
        if (c.blocks[s] < 1 || c.blocks[s] > 64) return abi_fail(GSV_ERR_ARG, "sv: %d blocks in stage %d unsupported", c.blocks[s], s + 1);
        if (c.width[s] < 4 || c.width[s] > (c.m_channels << s) * 4)
            return abi_fail(GSV_ERR_ARG, "sv: split width %d in stage %d unsupported (4 .. 4 * planes)", c.width[s], s + 1);
    }
    gsv_sv* h = new gsv_sv();
    h->cfg = c;
    *out = h;
    return GSV_OK;
}

int gsv_sv_destroy(gsv_sv* h) {
    if (!h) return GSV_OK;
    for (auto& kv : h->t) (void)hipFree(kv.second.first);
    for (void* p : h->owned) (void)hipFree(p);
    delete h;
    return GSV_OK;
}

int gsv_sv_load_tensor(gsv_sv* h, const char* name, const float* data, int64_t numel, void* stream) {
    if (!h || !name || !data || numel < 1) return abi_fail(GSV_ERR_ARG, "null argument");
    if (h->finalized) return abi_fail(GSV_ERR_STATE, "sv: load after finalize");
    const std::string n(name);
    bool known = false;
    for (const char* p : {"conv1.", "bn1.", "layer1.", "layer2.", "layer3.", "layer4.", "layer3_ds.", "fuse34."})
        known |= n.rfind(p, 0) == 0;
    if (!known || n.find("num_batches_tracked") != std::string::npos) return abi_fail(GSV_ERR_ARG, "sv: unknown tensor %s", name);
    float* d = nullptr;
    RCHK(hipMalloc(reinterpret_cast<void**>(&d), numel * sizeof(float)));
    RCHK(hipMemcpyAsync(d, data, numel * sizeof(float), hipMemcpyDeviceToDevice, S(stream)));
    auto it = h->t.find(n);
    if (it != h->t.end()) (void)hipFree(it->second.first);
    h->t[n] = {d, numel};
    return GSV_OK;
}

int gsv_sv_finalize(gsv_sv* h, void* stream) {
    if (!h) return abi_fail(GSV_ERR_ARG, "null argument");
    if (h->finalized) return GSV_OK;
    hipStream_t st = S(stream);
    const std::vector<SvConvSpec> specs = sv_specs(h->cfg);
    auto need = [&](const std::string& n, int64_t numel) -> int {
        auto it = h->t.find(n);
        if (it == h->t.end()) return abi_fail(GSV_ERR_STATE, "sv: tensor %s was not loaded", n.c_str());
        if (it->second.second != numel)
            return abi_fail(GSV_ERR_ARG, "sv: tensor %s has %lld elements, expected %lld", n.c_str(), (long long)it->second.second,
                            (long long)numel);
        return GSV_OK;
    };
    int rc;
    for (const auto& sp : specs) {
        if ((rc = need(sp.weight, (int64_t)sp.cout * sp.cin * sp.k * sp.k))) return rc;
        if (!sp.bn.empty())
            for (const char* f : {"weight", "bias", "running_mean", "running_var"})
                if ((rc = need(sp.bn + f, sp.cout))) return rc;
        if (!sp.bias.empty() && (rc = need(sp.bias, sp.cout))) return rc;
    }
    for (const auto& sp : specs) {
        gsv_sv::Conv cv{nullptr, nullptr, sp.cout, sp.cin, sp.k};
        const long long nw = (long long)sp.cout * sp.cin * sp.k * sp.k;
        if ((rc = sv_alloc(h, &cv.w, nw)) || (rc = sv_alloc(h, &cv.b, sp.cout))) return rc;
        auto T = [&](const std::string& n) -> const float* { return h->t.at(n).first; };
        const bool bn = !sp.bn.empty();
        sv_fold_kernel<<<(unsigned)((nw + 255) / 256), 256, 0, st>>>(
            T(sp.weight), sp.cout, sp.cin, sp.k * sp.k, bn ? T(sp.bn + "weight") : nullptr, bn ? T(sp.bn + "bias") : nullptr,
            bn ? T(sp.bn + "running_mean") : nullptr, bn ? T(sp.bn + "running_var") : nullptr,
            sp.bias.empty() ? nullptr : T(sp.bias), 1e-5f, cv.w, cv.b);
        h->conv[sp.key] = cv;
    }
    if ((rc = sv_alloc(h, &h->dft, (size_t)2 * FB_BINS * FB_NFFT)) || (rc = sv_alloc(h, &h->mel, (size_t)FB_MELS * FB_BINS))) return rc;
    sv_dft_kernel<<<(FB_BINS * FB_NFFT + 255) / 256, 256, 0, st>>>(h->dft);
    sv_mel_kernel<<<(FB_MELS * FB_BINS + 255) / 256, 256, 0, st>>>(h->mel);
    RCHK(hipGetLastError());
    // the folded copies are all forward3 reads: the loaded originals go once the folds have run
    RCHK(hipStreamSynchronize(st));
    for (auto& kv : h->t) (void)hipFree(kv.second.first);
    h->t.clear();
    h->finalized = true;
    return GSV_OK;
}

int gsv_sv_resample_length(int n_samples, int orig_sr, int new_sr) {
    const long long r = rs_length(n_samples, orig_sr, new_sr);
    return (r < 0 || r > 0x7fffffff) ? 0 : (int)r;
}

size_t gsv_sv_resample_workspace(int orig_sr, int new_sr) {
    int o, nw, width;
    if (!rs_params(orig_sr, new_sr, &o, &nw, &width)) return 0;
    return sizeof(float) * up((size_t)nw * (2 * width + o));
}

int gsv_sv_resample(const float* x, int n_samples, int orig_sr, int new_sr, float* y, void* workspace, size_t workspace_bytes,
                    void* stream) {
    int o, nw, width;
    if (!x || !y || n_samples < 1) return abi_fail(GSV_ERR_ARG, "null argument");
    if (!rs_params(orig_sr, new_sr, &o, &nw, &width)) return abi_fail(GSV_ERR_ARG, "sv: resampling %d -> %d Hz unsupported", orig_sr, new_sr);
    if (o != nw && (!workspace || workspace_bytes < gsv_sv_resample_workspace(orig_sr, new_sr)))
        return abi_fail(GSV_ERR_ARG, "sv: resample workspace too small");
    return sv_resample_run(S(stream), x, n_samples, orig_sr, new_sr, y, static_cast<float*>(workspace));
}

int gsv_sv_frames(gsv_sv* h, int n_samples, int sample_rate) {
    if (!h) return 0;
    const long long n16 = rs_length(n_samples, sample_rate, 16000);
    return n16 < 0 ? 0 : fb_frames(n16);
}

size_t gsv_sv_workspace(gsv_sv* h, int n_samples, int sample_rate) {
    if (!h || gsv_sv_frames(h, n_samples, sample_rate) < 1) return 0;
    return sizeof(float) * sv_carve(h->cfg, n_samples, sample_rate, nullptr).total;
}

int gsv_sv_fbank(gsv_sv* h, const float* wav16k, int n_samples, float* feat, void* workspace, size_t workspace_bytes, void* stream) {
    if (!h || !wav16k || !feat) return abi_fail(GSV_ERR_ARG, "null argument");
    const int T = fb_frames(n_samples);
    if (T < 1) return abi_fail(GSV_ERR_ARG, "sv: %d samples are too short for one fbank frame (400)", n_samples);
    int rc;
    if ((rc = sv_check_ws(h, n_samples, 16000, workspace, workspace_bytes))) return rc;
    const SvWs w = sv_carve(h->cfg, n_samples, 16000, static_cast<float*>(workspace));
    return sv_fbank_run(h, S(stream), wav16k, T, feat, w);
}

int gsv_sv_forward(gsv_sv* h, const float* feat, int n_frames, float* sv_emb, void* workspace, size_t workspace_bytes, void* stream) {
    if (!h || !feat || !sv_emb) return abi_fail(GSV_ERR_ARG, "null argument");
    if (n_frames < 1 || n_frames > (0x7fffffff - FB_WIN) / FB_HOP) return abi_fail(GSV_ERR_ARG, "sv: %d frames", n_frames);
    const long long n16 = FB_WIN + (long long)FB_HOP * (n_frames - 1);
    int rc;
    if ((rc = sv_check_ws(h, n16, 16000, workspace, workspace_bytes))) return rc;
    const SvWs w = sv_carve(h->cfg, n16, 16000, static_cast<float*>(workspace));
    return sv_forward_run(h, S(stream), feat, sv_batch(h->cfg, &n_frames, 1), sv_emb, w);
}

int gsv_sv_embed(gsv_sv* h, const float* wav, int n_samples, int sample_rate, float* sv_emb, void* workspace, size_t workspace_bytes,
                 void* stream) {
    if (!h || !wav || !sv_emb) return abi_fail(GSV_ERR_ARG, "null argument");
    int o, nw, width;
    if (!rs_params(sample_rate, 16000, &o, &nw, &width)) return abi_fail(GSV_ERR_ARG, "sv: sample rate %d unsupported", sample_rate);
    const int T = gsv_sv_frames(h, n_samples, sample_rate);
    if (T < 1) return abi_fail(GSV_ERR_ARG, "sv: %d samples at %d Hz are too short for one fbank frame", n_samples, sample_rate);
    int rc;
    if ((rc = sv_check_ws(h, n_samples, sample_rate, workspace, workspace_bytes))) return rc;
    hipStream_t st = S(stream);
    const SvWs w = sv_carve(h->cfg, n_samples, sample_rate, static_cast<float*>(workspace));
    const float* x16 = wav;
    if (sample_rate != 16000) {
        if ((rc = sv_resample_run(st, wav, n_samples, sample_rate, 16000, w.y16, w.tab))) return rc;
        x16 = w.y16;
    }
    if ((rc = sv_fbank_run(h, st, x16, T, w.feat, w))) return rc;
    return sv_forward_run(h, st, w.feat, sv_batch(h->cfg, &T, 1), sv_emb, w);
}

size_t gsv_sv_batch_workspace(gsv_sv* h, const int* n_samples, int n_clips, int sample_rate) {
    SvBatchIn in;
    if (!h || sv_batch_in(n_samples, n_clips, sample_rate, in) != GSV_OK) return 0;
    return sizeof(float) * sv_carve_batch(h->cfg, in.n_max, sample_rate, sv_batch(h->cfg, in.T, n_clips), nullptr).total;
}

int gsv_sv_forward_batch(gsv_sv* h, const float* feat, const int* n_frames, int n_clips, float* sv_emb, void* workspace,
                         size_t workspace_bytes, void* stream) {
    if (!h || !feat || !n_frames || !sv_emb) return abi_fail(GSV_ERR_ARG, "null argument");
    if (n_clips < 1 || n_clips > GSV_AUX_MAX_CLIPS) return abi_fail(GSV_ERR_ARG, "sv: %d clips (1..%d per call)", n_clips, GSV_AUX_MAX_CLIPS);
    // the workspace of the clips' equivalent 16 kHz lengths, as gsv_sv_forward sizes it
    int n16[GSV_AUX_MAX_CLIPS];
    for (int i = 0; i < n_clips; ++i) {
        if (n_frames[i] < 1 || n_frames[i] > (0x7fffffff - FB_WIN) / FB_HOP)
            return abi_fail(GSV_ERR_ARG, "sv: clip %d: %d frames", i, n_frames[i]);
        n16[i] = FB_WIN + FB_HOP * (n_frames[i] - 1);
    }
    SvBatchIn in;
    int rc;
    if ((rc = sv_check_batch(h, n16, n_clips, 16000, workspace, workspace_bytes, in))) return rc;
    const SvBatch B = sv_batch(h->cfg, n_frames, n_clips);
    const SvWs w = sv_carve_batch(h->cfg, in.n_max, 16000, B, static_cast<float*>(workspace));
    return sv_forward_run(h, S(stream), feat, B, sv_emb, w);
}

int gsv_sv_embed_batch(gsv_sv* h, const float* wav, const int* n_samples, int n_clips, int sample_rate, float* sv_emb,
                       void* workspace, size_t workspace_bytes, void* stream) {
    if (!h || !wav || !n_samples || !sv_emb) return abi_fail(GSV_ERR_ARG, "null argument");
    SvBatchIn in;
    int rc;
    if ((rc = sv_check_batch(h, n_samples, n_clips, sample_rate, workspace, workspace_bytes, in))) return rc;
    hipStream_t st = S(stream);
    const SvBatch B = sv_batch(h->cfg, in.T, n_clips);
    const SvWs w = sv_carve_batch(h->cfg, in.n_max, sample_rate, B, static_cast<float*>(workspace));
    // resample and fbank per clip (their buffers sized for the longest clip), each into its rows of the packed feat
    long long a0 = 0;
    for (int i = 0; i < n_clips; ++i) {
        const float* x16 = wav + a0;
        if (sample_rate != 16000) {
            if ((rc = sv_resample_run(st, wav + a0, n_samples[i], sample_rate, 16000, w.y16, w.tab))) return rc;
            x16 = w.y16;
        }
        if ((rc = sv_fbank_run(h, st, x16, in.T[i], w.feat + (long long)B.feat0[i] * FB_MELS, w))) return rc;
        a0 += n_samples[i];
    }
    return sv_forward_run(h, st, w.feat, B, sv_emb, w);
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------------------------
// Chinese RoBERTa (BertForMaskedLM hidden_states[-3]): packed texts -> hidden rows -> phone features
// ------------------------------------------------------------------------------------------------------------------
struct gsv_roberta {
    gsv_roberta_config cfg;
    std::map<std::string, std::pair<float*, int64_t>> t;   // loaded tensors (device, fp32)
    bool finalized = false;
    // derived at finalize
    std::vector<float*> w_qkv, b_qkv;                       // per run layer [3H][H], [3H] (query, key, value)
    std::vector<void*> owned;
};

namespace {

const float* RT(gsv_roberta* h, const std::string& name) { return h->t.at(name).first; }

std::string rb_layer(int l, const char* rest) { return "encoder.layer." + std::to_string(l) + "." + rest; }

// layers that feed hidden_states[-3]: 0 .. n_layer - 3
int rb_run_layers(const gsv_roberta_config& c) { return c.n_layer - 2; }

// floats of the split-K partial buffer of one M-row GEMM with N outputs over K
size_t rb_part(int M, int N, int K) { return (size_t)rb_splits(N, K) * M * N; }

struct RbWs {
    float *x, *tmp, *qkv, *att, *ffn, *part, *hid;
    size_t total;
};
RbWs rb_carve(const gsv_roberta_config& c, int rows, float* base) {
    RbWs w;
    size_t off = 0;
    auto take = [&](size_t n) { float* r = base ? base + off : nullptr; off += up(n); return r; };
    const size_t M = rows, H = c.hidden, F = c.ffn;
    const size_t part = std::max({rb_part(rows, 3 * c.hidden, c.hidden), rb_part(rows, c.hidden, c.hidden),
                                  rb_part(rows, c.ffn, c.hidden), rb_part(rows, c.hidden, c.ffn)});
    w.x = take(M * H);
    w.tmp = take(M * H);
    w.qkv = take(M * 3 * H);
    w.att = take(M * H);
    w.ffn = take(M * F);
    w.part = take(part);
    w.hid = take(M * H);
    w.total = off;
    return w;
}

// Y[M][N] = act(X . W^T + bias) (+ R): roberta.h's split-K GEMM (summation order fixed by N and K)
int rb_gemm(hipStream_t st, const float* X, const float* W, float* Y, int M, int N, int K, const float* bias, int act,
            const float* R, float* part) {
    const int S = rb_splits(N, K);
    rb_splitk_kernel<<<dim3((N + 63) / 64, (M + 63) / 64, S), 256, 0, st>>>(X, W, part, M, N, K, S);
    const long long n4 = (long long)M * N / 4;
    rb_splitk_reduce_kernel<<<(unsigned)((n4 + 255) / 256), 256, 0, st>>>(part, S, n4, N, bias, act, R, Y);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

int rb_check_call(gsv_roberta* h, const int* ids, const int* starts, int n_seq, int rows, int max_len, void* workspace,
                  size_t workspace_bytes) {
    if (!h || !ids || !starts || !workspace) return abi_fail(GSV_ERR_ARG, "null argument");
    if (!h->finalized) return abi_fail(GSV_ERR_STATE, "roberta: not finalized");
    if (n_seq < 1 || rows < n_seq * 2 || max_len < 2 || max_len > h->cfg.max_pos || max_len > rows ||
        (long long)max_len * n_seq < rows)
        return abi_fail(GSV_ERR_ARG, "roberta: %d texts over %d rows with max_len %d unsupported (2 <= len <= max_len <= %d)",
                        n_seq, rows, max_len, h->cfg.max_pos);
    if (workspace_bytes < gsv_roberta_workspace(h, rows, n_seq, max_len)) return abi_fail(GSV_ERR_ARG, "roberta: workspace too small");
    if ((reinterpret_cast<size_t>(workspace) & 15) != 0) return abi_fail(GSV_ERR_ARG, "roberta: workspace must be 16-byte aligned");
    return GSV_OK;
}

// hidden_states[-3] of the packed texts into out [rows][H]
int rb_run(gsv_roberta* h, hipStream_t st, const int* ids, const int* starts, int n_seq, int rows, int max_len, float* out,
           const RbWs& w) {
    const gsv_roberta_config& c = h->cfg;
    const int H = c.hidden, F = c.ffn, L = rb_run_layers(c);
    int bad = 0;
    rb_embed_ln_kernel<<<(rows + 3) / 4, 256, 0, st>>>(ids, starts, n_seq, rows, RT(h, "embeddings.word_embeddings.weight"), c.vocab,
                                                       RT(h, "embeddings.position_embeddings.weight"), c.max_pos,
                                                       RT(h, "embeddings.token_type_embeddings.weight"), H,
                                                       RT(h, "embeddings.LayerNorm.weight"), RT(h, "embeddings.LayerNorm.bias"), c.eps,
                                                       L > 0 ? w.x : out);
    const float scale = 1.f / sqrtf(64.f);
    for (int l = 0; l < L; ++l) {
        bad |= rb_gemm(st, w.x, h->w_qkv[l], w.qkv, rows, 3 * H, H, h->b_qkv[l], 0, nullptr, w.part);
        rb_attn_kernel<<<dim3((max_len + ATT_QB - 1) / ATT_QB, c.n_head, n_seq), 128, 0, st>>>(w.qkv, starts, rows, H, scale, w.att);
        bad |= rb_gemm(st, w.att, RT(h, rb_layer(l, "attention.output.dense.weight")), w.tmp, rows, H, H,
                       RT(h, rb_layer(l, "attention.output.dense.bias")), 0, w.x, w.part);
        bad |= ln(st, w.tmp, w.x, rows, H, RT(h, rb_layer(l, "attention.output.LayerNorm.weight")),
                  RT(h, rb_layer(l, "attention.output.LayerNorm.bias")), c.eps);
        bad |= rb_gemm(st, w.x, RT(h, rb_layer(l, "intermediate.dense.weight")), w.ffn, rows, F, H,
                       RT(h, rb_layer(l, "intermediate.dense.bias")), 2, nullptr, w.part);
        bad |= rb_gemm(st, w.ffn, RT(h, rb_layer(l, "output.dense.weight")), w.tmp, rows, H, F,
                       RT(h, rb_layer(l, "output.dense.bias")), 0, w.x, w.part);
        bad |= ln(st, w.tmp, l == L - 1 ? out : w.x, rows, H, RT(h, rb_layer(l, "output.LayerNorm.weight")),
                  RT(h, rb_layer(l, "output.LayerNorm.bias")), c.eps);
    }
    if (bad) return abi_fail(GSV_ERR_HIP, "roberta: a forward launch failed");
    RCHK(hipGetLastError());
    return GSV_OK;
}

}  // namespace

extern "C" {

int gsv_roberta_create(const gsv_roberta_config* cfg, gsv_roberta** out) {
    if (!cfg || !out) return abi_fail(GSV_ERR_ARG, "null argument");
    const gsv_roberta_config& c = *cfg;
    if (c.hidden < 64 || c.hidden % 64 || c.hidden > 64 * LN_MAX_NPL)
        return abi_fail(GSV_ERR_ARG, "roberta: hidden %d unsupported (a multiple of 64 up to %d)", c.hidden, 64 * LN_MAX_NPL);
    if (c.n_head < 1 || c.hidden != 64 * c.n_head)
        return abi_fail(GSV_ERR_ARG, "roberta: %d heads over hidden %d unsupported (the attention kernel needs head dim 64)", c.n_head, c.hidden);
    if (c.n_layer < 2) return abi_fail(GSV_ERR_ARG, "roberta: n_layer %d unsupported (hidden_states[-3] needs at least 2)", c.n_layer);
    if (c.ffn < 64 || c.ffn % 64) return abi_fail(GSV_ERR_ARG, "roberta: intermediate size %d unsupported (a multiple of 64)", c.ffn);
    if (c.vocab < 1 || c.type_vocab < 1 || c.max_pos < 2)
        return abi_fail(GSV_ERR_ARG, "roberta: vocab %d / type_vocab %d / max_pos %d unsupported", c.vocab, c.type_vocab, c.max_pos);
    if (!(c.eps > 0.f)) return abi_fail(GSV_ERR_ARG, "roberta: layer_norm_eps must be > 0");
    gsv_roberta* h = new gsv_roberta();
    h->cfg = c;
    *out = h;
    return GSV_OK;
}

int gsv_roberta_destroy(gsv_roberta* h) {
    if (!h) return GSV_OK;
    for (auto& kv : h->t) (void)hipFree(kv.second.first);
    for (void* p : h->owned) (void)hipFree(p);
    delete h;
    return GSV_OK;
}

int gsv_roberta_load_tensor(gsv_roberta* h, const char* name, const float* data, int64_t numel, void* stream) {
    if (!h || !name || !data || numel < 1) return abi_fail(GSV_ERR_ARG, "null argument");
    if (h->finalized) return abi_fail(GSV_ERR_STATE, "roberta: load after finalize");
    const std::string n(name);
    if (n.rfind("embeddings.", 0) == 0) {
        // every embeddings.* tensor is read
    } else if (n.rfind("encoder.layer.", 0) == 0) {
        const int l = std::atoi(n.c_str() + std::strlen("encoder.layer."));
        if (l >= rb_run_layers(h->cfg))
            return abi_fail(GSV_ERR_ARG, "roberta: %s is past hidden_states[-3] (only encoder.layer.0 .. %d run)", name,
                            rb_run_layers(h->cfg) - 1);
    } else {
        return abi_fail(GSV_ERR_ARG, "roberta: unknown tensor %s (pooler / cls.* are not read)", name);
    }
    float* d = nullptr;
    RCHK(hipMalloc(reinterpret_cast<void**>(&d), numel * sizeof(float)));
    RCHK(hipMemcpyAsync(d, data, numel * sizeof(float), hipMemcpyDeviceToDevice, S(stream)));
    auto it = h->t.find(n);
    if (it != h->t.end()) (void)hipFree(it->second.first);
    h->t[n] = {d, numel};
    return GSV_OK;
}

int gsv_roberta_finalize(gsv_roberta* h, void* stream) {
    if (!h) return abi_fail(GSV_ERR_ARG, "null argument");
    if (h->finalized) return GSV_OK;
    const gsv_roberta_config& c = h->cfg;
    const int64_t H = c.hidden, F = c.ffn;
    const int L = rb_run_layers(c);
    std::vector<std::pair<std::string, int64_t>> need = {
        {"embeddings.word_embeddings.weight", (int64_t)c.vocab * H},
        {"embeddings.position_embeddings.weight", (int64_t)c.max_pos * H},
        {"embeddings.token_type_embeddings.weight", (int64_t)c.type_vocab * H},
        {"embeddings.LayerNorm.weight", H}, {"embeddings.LayerNorm.bias", H},
    };
    for (int l = 0; l < L; ++l) {
        for (const char* p : {"attention.self.query", "attention.self.key", "attention.self.value", "attention.output.dense"}) {
            need.push_back({rb_layer(l, p) + ".weight", H * H});
            need.push_back({rb_layer(l, p) + ".bias", H});
        }
        need.push_back({rb_layer(l, "intermediate.dense.weight"), F * H});
        need.push_back({rb_layer(l, "intermediate.dense.bias"), F});
        need.push_back({rb_layer(l, "output.dense.weight"), H * F});
        need.push_back({rb_layer(l, "output.dense.bias"), H});
        for (const char* p : {"attention.output.LayerNorm.weight", "attention.output.LayerNorm.bias", "output.LayerNorm.weight",
                              "output.LayerNorm.bias"})
            need.push_back({rb_layer(l, p), H});
    }
    for (const auto& n : need) {
        auto it = h->t.find(n.first);
        if (it == h->t.end()) return abi_fail(GSV_ERR_STATE, "roberta: tensor %s was not loaded", n.first.c_str());
        if (it->second.second != n.second)
            return abi_fail(GSV_ERR_ARG, "roberta: tensor %s has %lld elements, expected %lld", n.first.c_str(),
                            (long long)it->second.second, (long long)n.second);
    }
    hipStream_t st = S(stream);
    h->w_qkv.assign(L, nullptr);
    h->b_qkv.assign(L, nullptr);
    const char* p[3] = {"attention.self.query", "attention.self.key", "attention.self.value"};
    for (int l = 0; l < L; ++l) {
        for (float** q : {&h->w_qkv[l], &h->b_qkv[l]}) {
            RCHK(hipMalloc(reinterpret_cast<void**>(q), (q == &h->w_qkv[l] ? 3 * H * H : 3 * H) * sizeof(float)));
            h->owned.push_back(*q);
        }
        for (int j = 0; j < 3; ++j) {
            RCHK(hipMemcpyAsync(h->w_qkv[l] + j * H * H, RT(h, rb_layer(l, p[j]) + ".weight"), H * H * 4, hipMemcpyDeviceToDevice, st));
            RCHK(hipMemcpyAsync(h->b_qkv[l] + j * H, RT(h, rb_layer(l, p[j]) + ".bias"), H * 4, hipMemcpyDeviceToDevice, st));
        }
    }
    // the separate q / k / v copies are not read again: free them once the fused copies are made
    RCHK(hipStreamSynchronize(st));
    for (int l = 0; l < L; ++l)
        for (int j = 0; j < 3; ++j)
            for (const char* suf : {".weight", ".bias"}) {
                auto it = h->t.find(rb_layer(l, p[j]) + suf);
                RCHK(hipFree(it->second.first));
                h->t.erase(it);
            }
    h->finalized = true;
    return GSV_OK;
}

size_t gsv_roberta_workspace(gsv_roberta* h, int total_rows, int n_seq, int max_len) {
    if (!h || total_rows < 1 || n_seq < 1 || max_len < 1) return 0;
    return sizeof(float) * rb_carve(h->cfg, total_rows, nullptr).total;
}

int gsv_roberta_forward(gsv_roberta* h, const int* ids, const int* seq_starts, int n_seq, int total_rows, int max_len,
                        float* hidden_out, void* workspace, size_t workspace_bytes, void* stream) {
    int rc;
    if ((rc = rb_check_call(h, ids, seq_starts, n_seq, total_rows, max_len, workspace, workspace_bytes))) return rc;
    if (!hidden_out) return abi_fail(GSV_ERR_ARG, "null argument");
    const RbWs w = rb_carve(h->cfg, total_rows, static_cast<float*>(workspace));
    return rb_run(h, S(stream), ids, seq_starts, n_seq, total_rows, max_len, hidden_out, w);
}

int gsv_roberta_features(gsv_roberta* h, const int* ids, const int* seq_starts, int n_seq, int total_rows, int max_len,
                         const int* phone_index, int n_phones, float* out, void* workspace, size_t workspace_bytes, void* stream) {
    int rc;
    if ((rc = rb_check_call(h, ids, seq_starts, n_seq, total_rows, max_len, workspace, workspace_bytes))) return rc;
    if (n_phones < 0 || (n_phones > 0 && (!phone_index || !out))) return abi_fail(GSV_ERR_ARG, "roberta: %d phones", n_phones);
    hipStream_t st = S(stream);
    const RbWs w = rb_carve(h->cfg, total_rows, static_cast<float*>(workspace));
    if ((rc = rb_run(h, st, ids, seq_starts, n_seq, total_rows, max_len, w.hid, w))) return rc;
    if (n_phones > 0) rb_phone_gather_kernel<<<n_phones, 256, 0, st>>>(w.hid, total_rows, h->cfg.hidden, phone_index, out);
    RCHK(hipGetLastError());
    return GSV_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------------------------
// WAV data chunk -> fp32 mono (wavpcm.h)
// ------------------------------------------------------------------------------------------------------------------
extern "C" {

int gsv_wav_to_mono_batch(const void* pcm, size_t pcm_bytes, const gsv_wav_clip* clips, int n_clips, float* out, void* stream) {
    if (!pcm || !clips || !out) return abi_fail(GSV_ERR_ARG, "null argument");
    if (n_clips < 1 || n_clips > GSV_AUX_MAX_CLIPS) return abi_fail(GSV_ERR_ARG, "wav: %d clips (1..%d per call)", n_clips, GSV_AUX_MAX_CLIPS);
    WavClips cl;
    long long out0 = 0;
    int n_max = 0;
    for (int i = 0; i < n_clips; ++i) {
        const gsv_wav_clip& c = clips[i];
        if (c.format < 0 || c.format >= WAV_N_FORMATS) return abi_fail(GSV_ERR_ARG, "wav: clip %d: unknown sample format %d", i, c.format);
        if (c.channels < 1 || c.channels > 2) return abi_fail(GSV_ERR_ARG, "wav: clip %d: %d channels (1 or 2)", i, c.channels);
        if (c.n_frames < 1) return abi_fail(GSV_ERR_ARG, "wav: clip %d: %d frames", i, c.n_frames);
        const long long frame = (long long)wav_sample_bytes(c.format) * c.channels;
        if (c.byte_offset < 0 || (unsigned long long)c.byte_offset > pcm_bytes ||
            (unsigned long long)c.n_frames * frame > pcm_bytes - (unsigned long long)c.byte_offset)
            return abi_fail(GSV_ERR_ARG, "wav: clip %d: %d frames at byte %lld run past the %zu bytes of pcm", i, c.n_frames,
                            (long long)c.byte_offset, pcm_bytes);
        cl.off[i] = c.byte_offset;
        cl.out0[i] = out0;
        cl.n[i] = c.n_frames;
        cl.fmt[i] = c.format;
        cl.ch[i] = c.channels;
        out0 += c.n_frames;
        n_max = std::max(n_max, (int)c.n_frames);
    }
    wav_to_mono_kernel<<<dim3((unsigned)((n_max + 255) / 256), n_clips), 256, 0, S(stream)>>>(
        static_cast<const unsigned char*>(pcm), cl, out);
    RCHK(hipGetLastError());
    return GSV_OK;
}

int gsv_wav_to_mono(const void* pcm, size_t pcm_bytes, int n_frames, int format, int channels, float* out, void* stream) {
    if (format < 0 || format >= WAV_N_FORMATS || channels < 1 || channels > 2)
        return abi_fail(GSV_ERR_ARG, "wav: format %d with %d channels (formats 0..%d, 1 or 2 channels)", format, channels,
                        WAV_N_FORMATS - 1);
    gsv_wav_clip c;
    c.byte_offset = 0;
    c.n_frames = n_frames;
    c.format = (int16_t)format;
    c.channels = (int16_t)channels;
    return gsv_wav_to_mono_batch(pcm, pcm_bytes, &c, 1, out, stream);
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------------------------
// FLAC frames -> s32 staging -> fp32 mono (flacdec.h, then wavpcm.h's WAV_S32)
// ------------------------------------------------------------------------------------------------------------------
static_assert(FLAC_E_OVERRUN == GSV_FLAC_OVERRUN && FLAC_E_SYNC == GSV_FLAC_SYNC && FLAC_E_RESERVED == GSV_FLAC_RESERVED &&
              FLAC_E_CRC8 == GSV_FLAC_CRC8 && FLAC_E_MISMATCH == GSV_FLAC_MISMATCH && FLAC_E_ORDER == GSV_FLAC_ORDER &&
              FLAC_E_PARTITION == GSV_FLAC_PARTITION && FLAC_E_RESIDUAL == GSV_FLAC_RESIDUAL && FLAC_E_RANGE == GSV_FLAC_RANGE &&
              FLAC_E_LENGTH == GSV_FLAC_LENGTH && FLAC_E_CRC16 == GSV_FLAC_CRC16 && FLAC_E_WASTED == GSV_FLAC_WASTED,
              "flacdec.h's status codes are the ABI's GSV_FLAC_* codes");
static_assert(sizeof(FlacFrameDev) == 32, "device frame table entry");

namespace {

constexpr size_t kFlacAlign = 256;
constexpr int kFlacWaveSlots = 1024;    // 256 CUs x 4 SIMDs: below this many frames each wave decodes one frame

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
inline int cdiv(int a, int b) { return (a + b - 1) / b; }

size_t flac_table_bytes(int n_frames) { return align_up((size_t)n_frames * sizeof(FlacFrameDev), kFlacAlign); }

// the argument checks of gsv_flac_decode / gsv_flac_decode_host; base[c]: clip c's first s32 in the interleaved
// staging (clips back to back), total: its length
int flac_check(const void* bytes, size_t n_bytes, const gsv_flac_clip* clips, int n_clips, const gsv_flac_frame* frames,
               int n_frames, long long* base, long long* total) {
    if (!bytes || !clips || !frames) return abi_fail(GSV_ERR_ARG, "null argument");
    if (n_clips < 1 || n_clips > GSV_AUX_MAX_CLIPS) return abi_fail(GSV_ERR_ARG, "flac: %d clips (1..%d per call)", n_clips, GSV_AUX_MAX_CLIPS);
    if (n_frames < 1) return abi_fail(GSV_ERR_ARG, "flac: %d frames", n_frames);
    long long next[GSV_AUX_MAX_CLIPS], at = 0;
    for (int c = 0; c < n_clips; ++c) {
        const gsv_flac_clip& k = clips[c];
        if (k.channels < 1 || k.channels > 2) return abi_fail(GSV_ERR_ARG, "flac: clip %d: %d channels (1 or 2)", c, k.channels);
        if (k.bits_per_sample < 8 || k.bits_per_sample > 24)
            return abi_fail(GSV_ERR_ARG, "flac: clip %d: %d bits per sample (8..24)", c, k.bits_per_sample);
        if (k.n_samples < 1) return abi_fail(GSV_ERR_ARG, "flac: clip %d: %d samples", c, k.n_samples);
        if (k.out_offset < 0) return abi_fail(GSV_ERR_ARG, "flac: clip %d: out_offset %lld", c, (long long)k.out_offset);
        base[c] = at;
        at += (long long)k.n_samples * k.channels;
        next[c] = 0;
    }
    *total = at;
    for (int f = 0; f < n_frames; ++f) {
        const gsv_flac_frame& r = frames[f];
        if (r.clip < 0 || r.clip >= n_clips) return abi_fail(GSV_ERR_ARG, "flac: frame %d: clip %d of %d", f, r.clip, n_clips);
        if (r.block_size < 1 || r.block_size > 65535) return abi_fail(GSV_ERR_ARG, "flac: frame %d: block size %d", f, r.block_size);
        if (r.byte_offset < 0 || r.byte_len < 1 || (unsigned long long)r.byte_offset > n_bytes ||
            (unsigned long long)r.byte_len > n_bytes - (unsigned long long)r.byte_offset)
            return abi_fail(GSV_ERR_ARG, "flac: frame %d: %d bytes at byte %lld run past the %zu bytes given", f, r.byte_len,
                            (long long)r.byte_offset, n_bytes);
        if (r.first_sample != next[r.clip])
            return abi_fail(GSV_ERR_ARG, "flac: frame %d: starts at sample %d of clip %d where sample %lld is next (frames of a clip "
                            "come in order and tile it)", f, r.first_sample, r.clip, next[r.clip]);
        next[r.clip] += r.block_size;
        if (next[r.clip] > clips[r.clip].n_samples)
            return abi_fail(GSV_ERR_ARG, "flac: frame %d: ends at sample %lld of clip %d, which has %d", f, next[r.clip], r.clip,
                            clips[r.clip].n_samples);
    }
    for (int c = 0; c < n_clips; ++c)
        if (next[c] != clips[c].n_samples)
            return abi_fail(GSV_ERR_ARG, "flac: clip %d: its frames hold %lld of %d samples", c, next[c], clips[c].n_samples);
    return GSV_OK;
}

}  // namespace

extern "C" {

size_t gsv_flac_decode_workspace(const gsv_flac_clip* clips, int n_clips, int n_frames) {
    if (!clips || n_clips < 1 || n_clips > GSV_AUX_MAX_CLIPS || n_frames < 1) return 0;
    size_t s32 = 0;
    for (int c = 0; c < n_clips; ++c) {
        if (clips[c].n_samples < 1 || clips[c].channels < 1 || clips[c].channels > 2) return 0;
        s32 += (size_t)clips[c].n_samples * clips[c].channels;
    }
    return flac_table_bytes(n_frames) + align_up(s32 * sizeof(int32_t), kFlacAlign);
}

int gsv_flac_decode(const void* bytes_dev, size_t n_bytes, const gsv_flac_clip* clips, int n_clips, const gsv_flac_frame* frames,
                    int n_frames, float* out, int32_t* status_dev, void* workspace, size_t workspace_bytes, void* stream) {
    if (!out || !status_dev || !workspace) return abi_fail(GSV_ERR_ARG, "null argument");
    long long base[GSV_AUX_MAX_CLIPS], total = 0;
    int rc;
    if ((rc = flac_check(bytes_dev, n_bytes, clips, n_clips, frames, n_frames, base, &total))) return rc;
    const size_t need = gsv_flac_decode_workspace(clips, n_clips, n_frames);
    if (workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 15))
        return abi_fail(GSV_ERR_ARG, "flac: workspace of %zu bytes (%zu needed, 16-byte aligned)", workspace_bytes, need);
    hipStream_t st = S(stream);
    FlacFrameDev* tab_dev = static_cast<FlacFrameDev*>(workspace);
    int32_t* staging = reinterpret_cast<int32_t*>(static_cast<char*>(workspace) + flac_table_bytes(n_frames));
    std::vector<FlacFrameDev> tab((size_t)n_frames);
    for (int f = 0; f < n_frames; ++f) {
        const gsv_flac_frame& r = frames[f];
        const gsv_flac_clip& k = clips[r.clip];
        FlacFrameDev& d = tab[f];
        d.byte_off = r.byte_offset;
        d.out_off = base[r.clip] + (long long)r.first_sample * k.channels;
        d.byte_len = (unsigned)r.byte_len;
        d.block_size = r.block_size;
        d.channels = (short)k.channels;
        d.bps = (short)k.bits_per_sample;
        d.open_end = r.flags & GSV_FLAC_OPEN_END;
    }
    // pageable host memory: the copy has left `tab` when the call returns
    RCHK(hipMemcpyAsync(tab_dev, tab.data(), tab.size() * sizeof(FlacFrameDev), hipMemcpyHostToDevice, st));
    const int fpb = std::min(64, std::max(1, cdiv(n_frames, kFlacWaveSlots)));
    flac_frames_kernel<<<dim3((unsigned)cdiv(n_frames, fpb)), 64, 0, st>>>(static_cast<const unsigned char*>(bytes_dev), tab_dev,
                                                                          n_frames, fpb, staging, status_dev);
    RCHK(hipGetLastError());
    WavClips cl;
    int n_max = 0;
    for (int c = 0; c < n_clips; ++c) {
        cl.off[c] = base[c] * (long long)sizeof(int32_t);
        cl.out0[c] = clips[c].out_offset;
        cl.n[c] = clips[c].n_samples;
        cl.fmt[c] = WAV_S32;
        cl.ch[c] = (short)clips[c].channels;
        n_max = std::max(n_max, (int)clips[c].n_samples);
    }
    wav_to_mono_kernel<<<dim3((unsigned)((n_max + 255) / 256), n_clips), 256, 0, st>>>(
        reinterpret_cast<const unsigned char*>(staging), cl, out);
    RCHK(hipGetLastError());
    return GSV_OK;
}

int gsv_flac_decode_host(const void* bytes, size_t n_bytes, const gsv_flac_clip* clips, int n_clips, const gsv_flac_frame* frames,
                         int n_frames, int32_t* pcm_interleaved, int32_t* status) {
    if (!pcm_interleaved || !status) return abi_fail(GSV_ERR_ARG, "null argument");
    long long base[GSV_AUX_MAX_CLIPS], total = 0;
    int rc;
    if ((rc = flac_check(bytes, n_bytes, clips, n_clips, frames, n_frames, base, &total))) return rc;
    for (int f = 0; f < n_frames; ++f) {
        const gsv_flac_frame& r = frames[f];
        const gsv_flac_clip& k = clips[r.clip];
        status[f] = flac_decode_frame(static_cast<const unsigned char*>(bytes) + r.byte_offset, (uint32_t)r.byte_len, k.channels,
                                      k.bits_per_sample, r.block_size,
                                      pcm_interleaved + base[r.clip] + (long long)r.first_sample * k.channels, 0,
                                      (r.flags & GSV_FLAC_OPEN_END) != 0);
    }
    return GSV_OK;
}

}  // extern "C"
