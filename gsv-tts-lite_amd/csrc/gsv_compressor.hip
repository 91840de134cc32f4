// C-ABI of the compressor (include/gsv_tts_hip.h, gsv_compressor*; kernels and the host twin in compressor.h): the argument
// checks, the rows and the powers built on the host, and the launches of a call.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/gsv_tts_hip.h"
#include "compressor.h"
#include "gsv_error.h"

using namespace gsv;

#define RCHK(expr)                                                                                        \
    do {                                                                                                  \
        hipError_t e_ = (expr);                                                                           \
        if (e_ != hipSuccess) return abi_fail(GSV_ERR_HIP, "%s: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

static_assert(sizeof(gsv_compressor_clip) == sizeof(CmpClip) && sizeof(gsv_compressor_record) == sizeof(CmpRecord) &&
              sizeof(gsv_compressor_params) == sizeof(CmpParams), "ABI structs");
static_assert(GSV_CMP_COMPRESSED == CMP_COMPRESSED && GSV_CMP_NONFINITE == CMP_NONFINITE, "ABI constants");

namespace {

int cmp_check(const float* x, size_t n_x, const gsv_compressor_clip* clips, int n_clips, const gsv_compressor_params* params, int n_params,
              const float* out, const void* records, const void* work, size_t work_bytes, CmpLayout* L) {
    if (!clips || !records || !work || (n_x > 0 && (!x || !out)) || (n_params > 0 && !params)) return abi_fail(GSV_ERR_ARG, "null argument");
    if (!cmp_layout(reinterpret_cast<const CmpClip*>(clips), n_clips, n_params, n_x, true, L, nullptr))
        return abi_fail(GSV_ERR_ARG, "compressor: %d clips (1..%d) over %d parameter sets (0..%d), an index outside them, or a clip outside the "
                        "%zu samples given", n_clips, CMP_MAX_CLIPS, n_params, CMP_MAX_DESIGNS, n_x);
    for (int d = 0; d < n_params; ++d)
        if (!cmp_params_ok(reinterpret_cast<const CmpParams*>(params)[d]))
            return abi_fail(GSV_ERR_ARG, "compressor: parameter set %d: attack and release coefficients in (0, 1), a positive finite threshold "
                            "and makeup, a slope in [-1, 0]", d);
    if (work_bytes < L->bytes || (reinterpret_cast<uintptr_t>(work) & 15))
        return abi_fail(GSV_ERR_ARG, "compressor: workspace of %zu bytes (%zu needed, 16-byte aligned)", work_bytes, L->bytes);
    return GSV_OK;
}

}  // namespace

extern "C" {

size_t gsv_compressor_work_bytes(const gsv_compressor_clip* clips, int n_clips, const gsv_compressor_params* params, int n_params) {
    CmpLayout L;
    if (n_params > 0 && !params) return 0;
    if (!cmp_layout(reinterpret_cast<const CmpClip*>(clips), n_clips, n_params, 0, false, &L, nullptr)) return 0;
    return L.bytes;
}

int gsv_compressor(const float* x, size_t n_x, const gsv_compressor_clip* clips, int n_clips, const gsv_compressor_params* params, int n_params,
                   float* out, gsv_compressor_record* records, void* work, size_t work_bytes, void* stream) {
    CmpLayout L;
    int rc;
    if ((rc = cmp_check(x, n_x, clips, n_clips, params, n_params, out, records, work, work_bytes, &L))) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    unsigned char* w = static_cast<unsigned char*>(work);
    // rows and designs are neighbours in the workspace: one upload
    std::vector<unsigned char> head(L.y_off, 0);
    cmp_layout(reinterpret_cast<const CmpClip*>(clips), n_clips, n_params, n_x, true, &L, reinterpret_cast<CmpRow*>(head.data()));
    for (int d = 0; d < n_params; ++d)
        cmp_design(reinterpret_cast<const CmpParams*>(params)[d], reinterpret_cast<CmpDesign*>(head.data() + L.designs_off) + d);
    // pageable host memory: the copy has left `head` when the call returns
    RCHK(hipMemcpyAsync(w, head.data(), head.size(), hipMemcpyHostToDevice, st));
    const CmpRow* drows = reinterpret_cast<const CmpRow*>(w + L.rows_off);
    const CmpDesign* ddes = reinterpret_cast<const CmpDesign*>(w + L.designs_off);
    float* y = reinterpret_cast<float*>(w + L.y_off);
    CmpChunk* chunks = reinterpret_cast<CmpChunk*>(w + L.chunks_off);
    uint32_t* stats = reinterpret_cast<uint32_t*>(w + L.stats_off);
    const dim3 inner((unsigned)std::max(1, L.max_nch - 1), (unsigned)n_clips);
    if (L.max_nch > 1) {
        cmp_kernel<0><<<inner, CMP_T, 0, st>>>(x, drows, ddes, y, chunks, stats);
        RCHK(hipGetLastError());
        cmp_chain_kernel<0><<<n_clips, CMP_LANES, 0, st>>>(drows, ddes, chunks, stats);
        RCHK(hipGetLastError());
        cmp_kernel<1><<<inner, CMP_T, 0, st>>>(x, drows, ddes, y, chunks, stats);
        RCHK(hipGetLastError());
    }
    // also for clips of one chunk: their start states are zero, and the statistics are cleared here
    cmp_chain_kernel<1><<<n_clips, CMP_LANES, 0, st>>>(drows, ddes, chunks, stats);
    RCHK(hipGetLastError());
    if (L.max_nch > 0) {
        cmp_kernel<2><<<dim3((unsigned)L.max_nch, (unsigned)n_clips), CMP_T, 0, st>>>(x, drows, ddes, y, chunks, stats);
        RCHK(hipGetLastError());
    }
    const unsigned gx = (unsigned)std::max(1, std::min(256, (L.max_n + 255) / 256));
    cmp_commit_kernel<<<dim3(gx, (unsigned)n_clips), 256, 0, st>>>(x, drows, y, stats, reinterpret_cast<CmpRecord*>(records), out);
    RCHK(hipGetLastError());
    return GSV_OK;
}

int gsv_compressor_host(const float* x, size_t n_x, const gsv_compressor_clip* clips, int n_clips, const gsv_compressor_params* params,
                        int n_params, float* out, gsv_compressor_record* records, void* work, size_t work_bytes) {
    CmpLayout L;
    int rc;
    if ((rc = cmp_check(x, n_x, clips, n_clips, params, n_params, out, records, work, work_bytes, &L))) return rc;
    cmp_run_host(x, reinterpret_cast<const CmpClip*>(clips), n_clips, reinterpret_cast<const CmpParams*>(params), n_params, out,
                 reinterpret_cast<CmpRecord*>(records), static_cast<unsigned char*>(work));
    return GSV_OK;
}

int gsv_compressor_math_host(int which, const double* in, double* out, size_t n) {
    if (which < 0 || which > 1 || (n > 0 && (!in || !out))) return abi_fail(GSV_ERR_ARG, "compressor: routine %d (0: log2, 1: exp2) or a null array", which);
    for (size_t i = 0; i < n; ++i) out[i] = which == 0 ? cmp_log2(in[i]) : cmp_exp2(in[i]);
    return GSV_OK;
}

}  // extern "C"
