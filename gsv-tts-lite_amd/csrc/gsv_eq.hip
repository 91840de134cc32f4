// C-ABI of the equaliser (include/gsv_tts_hip.h, gsv_eq*; kernels and the host twin in eq.h): the argument checks, the rows and
// the matrices built on the host, and the launches of a call.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/gsv_tts_hip.h"
#include "eq.h"
#include "gsv_error.h"

using namespace gsv;

#define RCHK(expr)                                                                                        \
    do {                                                                                                  \
        hipError_t e_ = (expr);                                                                           \
        if (e_ != hipSuccess) return abi_fail(GSV_ERR_HIP, "%s: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

static_assert(sizeof(gsv_eq_clip) == sizeof(EqClip) && sizeof(gsv_eq_record) == sizeof(EqRecord) && sizeof(gsv_eq_design) == sizeof(EqCoefs),
              "ABI structs");
static_assert(GSV_EQ_MAX_SECTIONS == EQ_MAX_SECTIONS && GSV_EQ_EQUALISED == EQ_EQUALISED && GSV_EQ_NONFINITE == EQ_NONFINITE, "ABI constants");

namespace {

int eq_check(const float* x, size_t n_x, const gsv_eq_clip* clips, int n_clips, const gsv_eq_design* designs, int n_designs, const float* out,
             const void* records, const void* work, size_t work_bytes, EqLayout* L) {
    if (!clips || !records || !work || (n_x > 0 && (!x || !out)) || (n_designs > 0 && !designs)) return abi_fail(GSV_ERR_ARG, "null argument");
    if (!eq_layout(reinterpret_cast<const EqClip*>(clips), n_clips, n_designs, n_x, true, L, nullptr))
        return abi_fail(GSV_ERR_ARG, "eq: %d clips (1..%d) over %d designs (0..%d), a design index outside them, or a clip outside the %zu samples given",
                        n_clips, EQ_MAX_CLIPS, n_designs, EQ_MAX_DESIGNS, n_x);
    for (int d = 0; d < n_designs; ++d)
        if (!eq_coefs_ok(reinterpret_cast<const EqCoefs*>(designs)[d]))
            return abi_fail(GSV_ERR_ARG, "eq: design %d: 1..%d sections of finite coefficients with both poles inside the unit circle "
                            "(|a2| < 1, |a1| < 1 + a2)", d, EQ_MAX_SECTIONS);
    if (work_bytes < L->bytes || (reinterpret_cast<uintptr_t>(work) & 15))
        return abi_fail(GSV_ERR_ARG, "eq: workspace of %zu bytes (%zu needed, 16-byte aligned)", work_bytes, L->bytes);
    return GSV_OK;
}

}  // namespace

extern "C" {

size_t gsv_eq_work_bytes(const gsv_eq_clip* clips, int n_clips, const gsv_eq_design* designs, int n_designs) {
    EqLayout L;
    if (n_designs > 0 && !designs) return 0;
    if (!eq_layout(reinterpret_cast<const EqClip*>(clips), n_clips, n_designs, 0, false, &L, nullptr)) return 0;
    return L.bytes;
}

int gsv_eq(const float* x, size_t n_x, const gsv_eq_clip* clips, int n_clips, const gsv_eq_design* designs, int n_designs, float* out,
           gsv_eq_record* records, void* work, size_t work_bytes, void* stream) {
    EqLayout L;
    int rc;
    if ((rc = eq_check(x, n_x, clips, n_clips, designs, n_designs, out, records, work, work_bytes, &L))) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    unsigned char* w = static_cast<unsigned char*>(work);
    // rows and designs are neighbours in the workspace: one upload
    std::vector<unsigned char> head(L.y_off, 0);
    eq_layout(reinterpret_cast<const EqClip*>(clips), n_clips, n_designs, n_x, true, &L, reinterpret_cast<EqRow*>(head.data()));
    for (int d = 0; d < n_designs; ++d)
        eq_design(reinterpret_cast<const EqCoefs*>(designs)[d], reinterpret_cast<EqDesign*>(head.data() + L.designs_off) + d);
    // pageable host memory: the copy has left `head` when the call returns
    RCHK(hipMemcpyAsync(w, head.data(), head.size(), hipMemcpyHostToDevice, st));
    const EqRow* drows = reinterpret_cast<const EqRow*>(w + L.rows_off);
    const EqDesign* ddes = reinterpret_cast<const EqDesign*>(w + L.designs_off);
    float* y = reinterpret_cast<float*>(w + L.y_off);
    EqState* ends = reinterpret_cast<EqState*>(w + L.ends_off);
    EqState* starts = reinterpret_cast<EqState*>(w + L.starts_off);
    uint32_t* peaks = reinterpret_cast<uint32_t*>(w + L.peak_off);
    if (L.max_nch > 1) {
        eq_filter_kernel<true><<<dim3((unsigned)L.max_nch - 1, (unsigned)n_clips), EQ_T, 0, st>>>(x, drows, ddes, y, ends, starts, peaks);
        RCHK(hipGetLastError());
    }
    eq_chain_kernel<<<n_clips, EQ_LANES, 0, st>>>(drows, ddes, ends, starts, peaks);
    RCHK(hipGetLastError());
    if (L.max_nch > 0) {
        eq_filter_kernel<false><<<dim3((unsigned)L.max_nch, (unsigned)n_clips), EQ_T, 0, st>>>(x, drows, ddes, y, ends, starts, peaks);
        RCHK(hipGetLastError());
    }
    const unsigned gx = (unsigned)std::max(1, std::min(256, (L.max_n + 255) / 256));
    eq_commit_kernel<<<dim3(gx, (unsigned)n_clips), 256, 0, st>>>(x, drows, ddes, y, peaks, reinterpret_cast<EqRecord*>(records), out);
    RCHK(hipGetLastError());
    return GSV_OK;
}

int gsv_eq_host(const float* x, size_t n_x, const gsv_eq_clip* clips, int n_clips, const gsv_eq_design* designs, int n_designs, float* out,
                gsv_eq_record* records, void* work, size_t work_bytes) {
    EqLayout L;
    int rc;
    if ((rc = eq_check(x, n_x, clips, n_clips, designs, n_designs, out, records, work, work_bytes, &L))) return rc;
    eq_run_host(x, reinterpret_cast<const EqClip*>(clips), n_clips, reinterpret_cast<const EqCoefs*>(designs), n_designs, out,
                reinterpret_cast<EqRecord*>(records), static_cast<unsigned char*>(work));
    return GSV_OK;
}

}  // extern "C"
