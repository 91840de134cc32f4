// C-ABI of the loudness meter (include/gsv_tts_hip.h, gsv_loudness*; kernels and the host twin in loudness.h): the argument
// checks, the rows and constants built on the host, and the launches of a call.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/gsv_tts_hip.h"
#include "gsv_error.h"
#include "loudness.h"

using namespace gsv;

#define RCHK(expr)                                                                                        \
    do {                                                                                                  \
        hipError_t e_ = (expr);                                                                           \
        if (e_ != hipSuccess) return abi_fail(GSV_ERR_HIP, "%s: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

static_assert(sizeof(gsv_loudness_clip) == sizeof(LoudClip) && sizeof(gsv_loudness_record) == sizeof(LoudRecord), "ABI structs");

namespace {

int loud_check(const float* x, size_t n_x, const gsv_loudness_clip* clips, int n_clips, int rate, float peak_limit, const void* records,
               const void* work, size_t work_bytes, LoudLayout* L) {
    if (!clips || !records || !work || (!x && n_x > 0)) return abi_fail(GSV_ERR_ARG, "null argument");
    if (rate < LOUD_MIN_RATE || rate > LOUD_MAX_RATE)
        return abi_fail(GSV_ERR_ARG, "loudness: a rate of %d Hz (%d..%d)", rate, LOUD_MIN_RATE, LOUD_MAX_RATE);
    if (!(peak_limit > 0.f)) return abi_fail(GSV_ERR_ARG, "loudness: a peak limit of %g", (double)peak_limit);
    if (!loud_layout(reinterpret_cast<const LoudClip*>(clips), n_clips, rate, n_x, true, L, nullptr))
        return abi_fail(GSV_ERR_ARG, "loudness: %d clips (1..%d), or a clip outside the %zu samples given", n_clips, LOUD_MAX_CLIPS, n_x);
    if (work_bytes < L->bytes || (reinterpret_cast<uintptr_t>(work) & 15))
        return abi_fail(GSV_ERR_ARG, "loudness: workspace of %zu bytes (%zu needed, 16-byte aligned)", work_bytes, L->bytes);
    return GSV_OK;
}

}  // namespace

extern "C" {

size_t gsv_loudness_work_bytes(const gsv_loudness_clip* clips, int n_clips, int rate) {
    LoudLayout L;
    if (!loud_layout(reinterpret_cast<const LoudClip*>(clips), n_clips, rate, 0, false, &L, nullptr)) return 0;
    return L.bytes;
}

int gsv_loudness(const float* x, size_t n_x, const gsv_loudness_clip* clips, int n_clips, int rate, float peak_limit, float* out,
                 gsv_loudness_record* records, void* work, size_t work_bytes, void* stream) {
    LoudLayout L;
    int rc;
    if ((rc = loud_check(x, n_x, clips, n_clips, rate, peak_limit, records, work, work_bytes, &L))) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    unsigned char* w = static_cast<unsigned char*>(work);
    std::vector<LoudRow> rows((size_t)n_clips);
    loud_layout(reinterpret_cast<const LoudClip*>(clips), n_clips, rate, n_x, true, &L, rows.data());
    const LoudParams p = loud_params(rate, peak_limit);
    // pageable host memory: the copy has left `rows` when the call returns
    RCHK(hipMemcpyAsync(w + L.rows_off, rows.data(), rows.size() * sizeof(LoudRow), hipMemcpyHostToDevice, st));
    const LoudRow* drows = reinterpret_cast<const LoudRow*>(w + L.rows_off);
    float* y = reinterpret_cast<float*>(w + L.y_off);
    double* z = reinterpret_cast<double*>(w + L.z_off);
    uint32_t* peaks = reinterpret_cast<uint32_t*>(w + L.peak_off);
    LoudState* ends = reinterpret_cast<LoudState*>(w + L.ends_off);
    LoudState* starts = reinterpret_cast<LoudState*>(w + L.starts_off);
    LoudRecord* rec = reinterpret_cast<LoudRecord*>(records);
    if (L.max_nch > 1) {
        loud_filter_kernel<true><<<dim3((unsigned)L.max_nch - 1, (unsigned)n_clips), LOUD_T, 0, st>>>(x, drows, p, y, ends, starts, peaks);
        RCHK(hipGetLastError());
    }
    loud_chain_kernel<<<(n_clips + LOUD_LANES - 1) / LOUD_LANES, LOUD_LANES, 0, st>>>(drows, n_clips, p, ends, starts, peaks);
    RCHK(hipGetLastError());
    if (L.max_nch > 0) {
        loud_filter_kernel<false><<<dim3((unsigned)L.max_nch, (unsigned)n_clips), LOUD_T, 0, st>>>(x, drows, p, y, ends, starts, peaks);
        RCHK(hipGetLastError());
    }
    if (L.max_nb > 0) {
        loud_blocks_kernel<<<dim3((unsigned)L.max_nb, (unsigned)n_clips), LOUD_LANES, 0, st>>>(drows, p, y, z);
        RCHK(hipGetLastError());
    }
    loud_decide_kernel<<<n_clips, LOUD_LANES, 0, st>>>(drows, p, z, peaks, rec);
    RCHK(hipGetLastError());
    if (out && L.max_n > 0) {
        const unsigned gx = (unsigned)std::min(256, (L.max_n + 255) / 256);
        loud_scale_kernel<<<dim3(gx, (unsigned)n_clips), 256, 0, st>>>(x, drows, rec, out);
        RCHK(hipGetLastError());
    }
    return GSV_OK;
}

int gsv_loudness_host(const float* x, size_t n_x, const gsv_loudness_clip* clips, int n_clips, int rate, float peak_limit, float* out,
                      gsv_loudness_record* records, void* work, size_t work_bytes) {
    LoudLayout L;
    int rc;
    if ((rc = loud_check(x, n_x, clips, n_clips, rate, peak_limit, records, work, work_bytes, &L))) return rc;
    loud_run_host(x, reinterpret_cast<const LoudClip*>(clips), n_clips, rate, peak_limit, out, reinterpret_cast<LoudRecord*>(records),
                  static_cast<unsigned char*>(work));
    return GSV_OK;
}

}  // extern "C"
