// C-ABI of the stream compressor (include/gsv_tts_hip.h, gsv_cmpstream_*; kernels and the host twin in cmpstream.h): the argument
// checks, the state built on the host and uploaded, and the six launches of a push.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/gsv_tts_hip.h"
#include "cmpstream.h"
#include "gsv_error.h"

using namespace gsv;

#define RCHK(expr)                                                                                        \
    do {                                                                                                  \
        hipError_t e_ = (expr);                                                                           \
        if (e_ != hipSuccess) return abi_fail(GSV_ERR_HIP, "%s: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

static_assert(sizeof(gsv_cmpstream_record) == sizeof(CmsRecord) && sizeof(gsv_compressor_params) == sizeof(CmpParams), "ABI structs");
static_assert(GSV_CMS_STREAM == CMS_STREAM && GSV_CMS_NONFINITE == CMS_NONFINITE && GSV_CMS_NONFINITE_EVER == CMS_NONFINITE_EVER &&
              GSV_CMS_COMPRESSED == CMS_COMPRESSED, "ABI constants");

namespace {

int init_check(const void* state, size_t bytes, const gsv_compressor_params* params) {
    if (!state || !params) return abi_fail(GSV_ERR_ARG, "null argument");
    if (!cmp_params_ok(*reinterpret_cast<const CmpParams*>(params)))
        return abi_fail(GSV_ERR_ARG, "cmpstream: attack and release coefficients in (0, 1), a positive finite threshold and makeup, a slope "
                        "in [-1, 0]");
    const size_t need = cms_state_bytes();
    if (bytes < need || (reinterpret_cast<uintptr_t>(state) & 15))
        return abi_fail(GSV_ERR_ARG, "cmpstream: state of %zu bytes (%zu needed, 16-byte aligned)", bytes, need);
    return GSV_OK;
}

int push_check(const void* state, const float* chunk, int n_cap, const float* out, const void* rec) {
    if (n_cap < 0 || n_cap > CMS_MAX_PUSH) return abi_fail(GSV_ERR_ARG, "cmpstream: a chunk of %d samples (0..%d)", n_cap, CMS_MAX_PUSH);
    if (!state || !rec || ((!chunk || !out) && n_cap > 0)) return abi_fail(GSV_ERR_ARG, "null argument");
    if (reinterpret_cast<uintptr_t>(state) & 15) return abi_fail(GSV_ERR_ARG, "cmpstream: the state is not 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(rec) & 7) return abi_fail(GSV_ERR_ARG, "cmpstream: the record is not 8-byte aligned");
    return GSV_OK;
}

}  // namespace

extern "C" {

size_t gsv_cmpstream_state_bytes(void) { return cms_state_bytes(); }

int gsv_cmpstream_init(void* state, size_t bytes, const gsv_compressor_params* params, void* stream) {
    int rc;
    if ((rc = init_check(state, bytes, params))) return rc;
    std::vector<unsigned char> host(cms_state_bytes());
    cms_init_host(host.data(), *reinterpret_cast<const CmpParams*>(params));
    // pageable host memory: the copy has left `host` when the call returns
    RCHK(hipMemcpyAsync(state, host.data(), host.size(), hipMemcpyHostToDevice, reinterpret_cast<hipStream_t>(stream)));
    return GSV_OK;
}

int gsv_cmpstream_init_host(void* state, size_t bytes, const gsv_compressor_params* params) {
    int rc;
    if ((rc = init_check(state, bytes, params))) return rc;
    cms_init_host(static_cast<unsigned char*>(state), *reinterpret_cast<const CmpParams*>(params));
    return GSV_OK;
}

int gsv_cmpstream_push(void* state, const float* chunk, int n_cap, const int32_t* n_dev, int flush, float* out, gsv_cmpstream_record* rec,
                       void* stream) {
    int rc;
    if ((rc = push_check(state, chunk, n_cap, out, rec))) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    unsigned char* s = static_cast<unsigned char*>(state);
    // sized by n_cap alone: the host does not know where in its open chunk the stream stands, so one block more than n_cap's chunks
    const unsigned blocks = (unsigned)std::min(CMS_MAX_BLOCKS, (n_cap + CMP_CHUNK - 1) / CMP_CHUNK + 1);
    if (n_cap > 0) {
        cms_kernel<0><<<blocks, CMP_T, 0, st>>>(s, chunk, n_cap, n_dev, out);
        RCHK(hipGetLastError());
    }
    cms_chain_kernel<0><<<1, CMS_LANES, 0, st>>>(s, n_cap, n_dev);
    RCHK(hipGetLastError());
    if (n_cap > 0) {
        cms_kernel<1><<<blocks, CMP_T, 0, st>>>(s, chunk, n_cap, n_dev, out);
        RCHK(hipGetLastError());
    }
    cms_chain_kernel<1><<<1, CMS_LANES, 0, st>>>(s, n_cap, n_dev);
    RCHK(hipGetLastError());
    if (n_cap > 0) {
        cms_kernel<2><<<blocks, CMP_T, 0, st>>>(s, chunk, n_cap, n_dev, out);
        RCHK(hipGetLastError());
    }
    cms_commit_kernel<<<1, CMS_LANES, 0, st>>>(s, n_cap, n_dev, flush, reinterpret_cast<CmsRecord*>(rec));
    RCHK(hipGetLastError());
    return GSV_OK;
}

int gsv_cmpstream_push_host(void* state, const float* chunk, int n_cap, const int32_t* n_host, int flush, float* out, gsv_cmpstream_record* rec) {
    int rc;
    if ((rc = push_check(state, chunk, n_cap, out, rec))) return rc;
    const int n = n_host ? cms_clamp(*n_host, n_cap) : n_cap;
    cms_push_host(static_cast<unsigned char*>(state), chunk, n, flush != 0, out, reinterpret_cast<CmsRecord*>(rec));
    return GSV_OK;
}

}  // extern "C"
