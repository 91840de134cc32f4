// C-ABI of the reverb (include/gsv_tts_hip.h, gsv_reverb*; kernels and the host twin in reverb.h): the argument checks, the rows
// and the scan's powers built on the host, and the launches of a call.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/gsv_tts_hip.h"
#include "reverb.h"
#include "gsv_error.h"

using namespace gsv;

#define RCHK(expr)                                                                                        \
    do {                                                                                                  \
        hipError_t e_ = (expr);                                                                           \
        if (e_ != hipSuccess) return abi_fail(GSV_ERR_HIP, "%s: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

static_assert(sizeof(gsv_reverb_clip) == sizeof(RvbClip) && sizeof(gsv_reverb_record) == sizeof(RvbRecord) &&
              sizeof(gsv_reverb_params) == sizeof(RvbParams), "ABI structs");
static_assert(GSV_RVB_REVERBED == RVB_REVERBED && GSV_RVB_NONFINITE == RVB_NONFINITE && GSV_RVB_MAX_DELAY == RVB_MAX_DELAY, "ABI constants");

namespace {

int rvb_check(const float* x, size_t n_x, const gsv_reverb_clip* clips, int n_clips, const gsv_reverb_params* params, int n_params,
              const float* out, const void* records, const void* work, size_t work_bytes, RvbLayout* L) {
    if (!clips || !records || !work || (n_x > 0 && (!x || !out)) || (n_params > 0 && !params)) return abi_fail(GSV_ERR_ARG, "null argument");
    if (!rvb_layout(reinterpret_cast<const RvbClip*>(clips), n_clips, n_params, n_x, true, L, nullptr))
        return abi_fail(GSV_ERR_ARG, "reverb: %d clips (1..%d) over %d parameter sets (0..%d), an index outside them, or a clip outside the "
                        "%zu samples given", n_clips, RVB_MAX_CLIPS, n_params, RVB_MAX_DESIGNS, n_x);
    for (int d = 0; d < n_params; ++d) {
        const int bad = rvb_params_bad(reinterpret_cast<const RvbParams*>(params)[d]);
        if (bad == 1) return abi_fail(GSV_ERR_ARG, "reverb: parameter set %d: a delay outside 1..%d samples", d, RVB_MAX_DELAY);
        if (bad == 2) return abi_fail(GSV_ERR_ARG, "reverb: parameter set %d: damping d and feedback fb in [0, 1)", d);
        if (bad == 3) return abi_fail(GSV_ERR_ARG, "reverb: parameter set %d: a gain that is not finite", d);
    }
    if (work_bytes < L->bytes) return abi_fail(GSV_ERR_ARG, "reverb: workspace of %zu bytes (%zu needed)", work_bytes, L->bytes);
    if (reinterpret_cast<uintptr_t>(work) & 15) return abi_fail(GSV_ERR_ARG, "reverb: workspace not 16-byte aligned");
    return GSV_OK;
}

}  // namespace

extern "C" {

size_t gsv_reverb_work_bytes(const gsv_reverb_clip* clips, int n_clips, const gsv_reverb_params* params, int n_params) {
    RvbLayout L;
    if (n_params > 0 && !params) return 0;
    if (!rvb_layout(reinterpret_cast<const RvbClip*>(clips), n_clips, n_params, 0, false, &L, nullptr)) return 0;
    return L.bytes;
}

int gsv_reverb(const float* x, size_t n_x, const gsv_reverb_clip* clips, int n_clips, const gsv_reverb_params* params, int n_params,
               float* out, gsv_reverb_record* records, void* work, size_t work_bytes, void* stream) {
    RvbLayout L;
    int rc;
    if ((rc = rvb_check(x, n_x, clips, n_clips, params, n_params, out, records, work, work_bytes, &L))) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    unsigned char* w = static_cast<unsigned char*>(work);
    // rows, designs and the cleared statistics are neighbours in the workspace: one upload
    std::vector<unsigned char> head(L.head_bytes, 0);
    rvb_layout(reinterpret_cast<const RvbClip*>(clips), n_clips, n_params, n_x, true, &L, reinterpret_cast<RvbRow*>(head.data()));
    int max_e[RVB_APS] = {0, 0, 0, 0};
    for (int d = 0; d < n_params; ++d) {
        const RvbParams& p = reinterpret_cast<const RvbParams*>(params)[d];
        rvb_design(p, reinterpret_cast<RvbDesign*>(head.data() + L.designs_off) + d);
        for (int j = 0; j < RVB_APS; ++j) max_e[j] = std::max(max_e[j], p.allpass[j]);
    }
    // pageable host memory: the copy has left `head` when the call returns
    RCHK(hipMemcpyAsync(w, head.data(), head.size(), hipMemcpyHostToDevice, st));
    const RvbRow* drows = reinterpret_cast<const RvbRow*>(w + L.rows_off);
    const RvbDesign* ddes = reinterpret_cast<const RvbDesign*>(w + L.designs_off);
    uint32_t* stats = reinterpret_cast<uint32_t*>(w + L.stats_off);
    double* b = reinterpret_cast<double*>(w + L.b_off);
    double* s = reinterpret_cast<double*>(w + L.s_off);
    const unsigned nc = (unsigned)n_clips;
    auto blocks = [](int e) { return (unsigned)std::max(1, (e + RVB_AT - 1) / RVB_AT); };
    rvb_comb_kernel<<<dim3(RVB_COMBS, nc), RVB_T, 0, st>>>(x, drows, ddes, b, L.plane, stats);
    RCHK(hipGetLastError());
    if (n_params > 0) {
        rvb_sum_kernel<<<dim3((unsigned)std::max(1, std::min(1024, (L.max_n + RVB_AT - 1) / RVB_AT)), nc), RVB_AT, 0, st>>>(drows, ddes, b, L.plane, s);
        RCHK(hipGetLastError());
        rvb_ap_kernel<0><<<dim3(blocks(max_e[0]), nc), RVB_AT, 0, st>>>(x, drows, ddes, s, stats, out);
        RCHK(hipGetLastError());
        rvb_ap_kernel<1><<<dim3(blocks(max_e[1]), nc), RVB_AT, 0, st>>>(x, drows, ddes, s, stats, out);
        RCHK(hipGetLastError());
        rvb_ap_kernel<2><<<dim3(blocks(max_e[2]), nc), RVB_AT, 0, st>>>(x, drows, ddes, s, stats, out);
        RCHK(hipGetLastError());
    }
    // the last all-pass also copies: enough blocks for the longest clip when the call has a clip with params -1
    unsigned g3 = blocks(max_e[3]);
    if (L.any_copy) g3 = std::max(g3, (unsigned)std::min(64, (L.max_n + 4 * RVB_AT - 1) / (4 * RVB_AT)));
    rvb_ap_kernel<3><<<dim3(g3, nc), RVB_AT, 0, st>>>(x, drows, ddes, s, stats, out);
    RCHK(hipGetLastError());
    rvb_record_kernel<<<(n_clips + RVB_AT - 1) / RVB_AT, RVB_AT, 0, st>>>(drows, stats, reinterpret_cast<RvbRecord*>(records), n_clips);
    RCHK(hipGetLastError());
    return GSV_OK;
}

int gsv_reverb_host(const float* x, size_t n_x, const gsv_reverb_clip* clips, int n_clips, const gsv_reverb_params* params, int n_params,
                    float* out, gsv_reverb_record* records, void* work, size_t work_bytes) {
    RvbLayout L;
    int rc;
    if ((rc = rvb_check(x, n_x, clips, n_clips, params, n_params, out, records, work, work_bytes, &L))) return rc;
    rvb_run_host(x, reinterpret_cast<const RvbClip*>(clips), n_clips, reinterpret_cast<const RvbParams*>(params), n_params, out,
                 reinterpret_cast<RvbRecord*>(records), static_cast<unsigned char*>(work));
    return GSV_OK;
}

}  // extern "C"
