// C-ABI of the true-peak limiter (include/gsv_tts_hip.h, gsv_limiter*; kernels and the host twin in limiter.h): the argument
// checks, the rows and constants built on the host, and the launches of a call.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/gsv_tts_hip.h"
#include "gsv_error.h"
#include "limiter.h"

using namespace gsv;

#define RCHK(expr)                                                                                        \
    do {                                                                                                  \
        hipError_t e_ = (expr);                                                                           \
        if (e_ != hipSuccess) return abi_fail(GSV_ERR_HIP, "%s: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

static_assert(sizeof(gsv_limiter_clip) == sizeof(LimClip) && sizeof(gsv_limiter_record) == sizeof(LimRecord), "ABI structs");

namespace {

int lim_check(const float* x, size_t n_x, const gsv_limiter_clip* clips, int n_clips, int lookahead, int release, const void* records,
              const void* work, size_t work_bytes, LimLayout* L) {
    if (!clips || !records || !work || (!x && n_x > 0)) return abi_fail(GSV_ERR_ARG, "null argument");
    if (!lim_times_ok(lookahead, release))
        return abi_fail(GSV_ERR_ARG, "limiter: a look-ahead of %d samples (1..%d) or a release of %d (1..%d)", lookahead, LIM_MAX_L, release,
                        LIM_MAX_R);
    if (!lim_layout(reinterpret_cast<const LimClip*>(clips), n_clips, n_x, true, L, nullptr))
        return abi_fail(GSV_ERR_ARG, "limiter: %d clips (1..%d), a ceiling outside -200..0 dBTP, or a clip outside the %zu samples given",
                        n_clips, LIM_MAX_CLIPS, n_x);
    if (work_bytes < L->bytes || (reinterpret_cast<uintptr_t>(work) & 15))
        return abi_fail(GSV_ERR_ARG, "limiter: workspace of %zu bytes (%zu needed, 16-byte aligned)", work_bytes, L->bytes);
    return GSV_OK;
}

}  // namespace

extern "C" {

size_t gsv_limiter_work_bytes(const gsv_limiter_clip* clips, int n_clips) {
    LimLayout L;
    if (!lim_layout(reinterpret_cast<const LimClip*>(clips), n_clips, 0, false, &L, nullptr)) return 0;
    return L.bytes;
}

int gsv_limiter(const float* x, size_t n_x, const gsv_limiter_clip* clips, int n_clips, int lookahead, int release, float* out,
                gsv_limiter_record* records, void* work, size_t work_bytes, void* stream) {
    LimLayout L;
    int rc;
    if ((rc = lim_check(x, n_x, clips, n_clips, lookahead, release, records, work, work_bytes, &L))) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    unsigned char* w = static_cast<unsigned char*>(work);
    // the rows and the cleared statistics are one upload: they lie side by side at the head of the workspace
    std::vector<unsigned char> head(L.c_off, 0);
    lim_layout(reinterpret_cast<const LimClip*>(clips), n_clips, n_x, true, &L, reinterpret_cast<LimRow*>(head.data()));
    LimStat* hstats = reinterpret_cast<LimStat*>(head.data() + L.stats_off);
    for (int c = 0; c < n_clips; ++c) hstats[c].min_gain = 0x3F800000u;
    const LimParams p = lim_params(lookahead, release);
    // pageable host memory: the copy has left `head` when the call returns
    RCHK(hipMemcpyAsync(w, head.data(), head.size(), hipMemcpyHostToDevice, st));
    const LimRow* drows = reinterpret_cast<const LimRow*>(w + L.rows_off);
    LimStat* stats = reinterpret_cast<LimStat*>(w + L.stats_off);
    auto arr = [&](size_t off) { return reinterpret_cast<float*>(w + off); };
    LimRecord* rec = reinterpret_cast<LimRecord*>(records);
    const unsigned nc = (unsigned)n_clips;
    if (L.max_n > 0) {
        const unsigned env_blocks = (unsigned)(((long long)L.max_n + LIM_ENV_SPAN - 1) / LIM_ENV_SPAN);
        lim_envelope_kernel<true><<<dim3(env_blocks, nc), LIM_ENV_T, 0, st>>>(x, drows, p, arr(L.c_off), stats);
        RCHK(hipGetLastError());
        if (out) {
            lim_hold_kernel<<<dim3((unsigned)L.max_nt, nc), LIM_TILE, 0, st>>>(drows, p, arr(L.c_off), arr(L.h_off), arr(L.v_off),
                                                                              arr(L.ends_off));
            RCHK(hipGetLastError());
            lim_chain_kernel<<<(n_clips + 63) / 64, 64, 0, st>>>(drows, n_clips, p, arr(L.ends_off), arr(L.starts_off));
            RCHK(hipGetLastError());
            lim_attack_kernel<<<dim3((unsigned)L.max_nt, nc), LIM_TILE, 0, st>>>(x, drows, p, arr(L.c_off), arr(L.v_off), arr(L.starts_off),
                                                                                arr(L.r_off), arr(L.g_off), stats, out);
            RCHK(hipGetLastError());
            lim_envelope_kernel<false><<<dim3(env_blocks, nc), LIM_ENV_T, 0, st>>>(out, drows, p, nullptr, stats);
            RCHK(hipGetLastError());
        }
    }
    const unsigned gx = (unsigned)std::max(1, std::min(256, (L.max_n + 255) / 256));
    lim_trim_kernel<<<dim3(gx, nc), 256, 0, st>>>(drows, p, stats, out, rec);
    RCHK(hipGetLastError());
    return GSV_OK;
}

int gsv_limiter_host(const float* x, size_t n_x, const gsv_limiter_clip* clips, int n_clips, int lookahead, int release, float* out,
                     gsv_limiter_record* records, void* work, size_t work_bytes) {
    LimLayout L;
    int rc;
    if ((rc = lim_check(x, n_x, clips, n_clips, lookahead, release, records, work, work_bytes, &L))) return rc;
    lim_run_host(x, reinterpret_cast<const LimClip*>(clips), n_clips, lookahead, release, out, reinterpret_cast<LimRecord*>(records),
                 static_cast<unsigned char*>(work));
    return GSV_OK;
}

}  // extern "C"
