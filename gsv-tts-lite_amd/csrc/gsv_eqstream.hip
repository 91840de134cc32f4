// C-ABI of the stream equaliser (include/gsv_tts_hip.h, gsv_eqstream_*; kernels and the host twin in eqstream.h): the argument
// checks, the state built on the host and uploaded, and the four launches of a push.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/gsv_tts_hip.h"
#include "eqstream.h"
#include "gsv_error.h"

using namespace gsv;

#define RCHK(expr)                                                                                        \
    do {                                                                                                  \
        hipError_t e_ = (expr);                                                                           \
        if (e_ != hipSuccess) return abi_fail(GSV_ERR_HIP, "%s: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

static_assert(sizeof(gsv_eqstream_record) == sizeof(EqsRecord) && sizeof(gsv_eq_design) == sizeof(EqCoefs), "ABI structs");
static_assert(GSV_EQS_EQUALISED == EQS_EQUALISED && GSV_EQS_NONFINITE == EQS_NONFINITE && GSV_EQS_NONFINITE_EVER == EQS_NONFINITE_EVER,
              "ABI constants");

namespace {

int init_check(const void* state, size_t bytes, const gsv_eq_design* design) {
    if (!state || !design) return abi_fail(GSV_ERR_ARG, "null argument");
    if (!eq_coefs_ok(*reinterpret_cast<const EqCoefs*>(design)))
        return abi_fail(GSV_ERR_ARG, "eqstream: 1..%d sections of finite coefficients with both poles inside the unit circle "
                        "(|a2| < 1, |a1| < 1 + a2)", EQ_MAX_SECTIONS);
    const size_t need = eqs_state_bytes();
    if (bytes < need || (reinterpret_cast<uintptr_t>(state) & 15))
        return abi_fail(GSV_ERR_ARG, "eqstream: state of %zu bytes (%zu needed, 16-byte aligned)", bytes, need);
    return GSV_OK;
}

int push_check(const void* state, const float* chunk, int n_cap, const float* out, const void* rec) {
    if (n_cap < 0 || n_cap > EQS_MAX_PUSH) return abi_fail(GSV_ERR_ARG, "eqstream: a chunk of %d samples (0..%d)", n_cap, EQS_MAX_PUSH);
    if (!state || !rec || ((!chunk || !out) && n_cap > 0)) return abi_fail(GSV_ERR_ARG, "null argument");
    if (reinterpret_cast<uintptr_t>(state) & 15) return abi_fail(GSV_ERR_ARG, "eqstream: the state is not 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(rec) & 7) return abi_fail(GSV_ERR_ARG, "eqstream: the record is not 8-byte aligned");
    return GSV_OK;
}

}  // namespace

extern "C" {

size_t gsv_eqstream_state_bytes(void) { return eqs_state_bytes(); }

int gsv_eqstream_init(void* state, size_t bytes, const gsv_eq_design* design, void* stream) {
    int rc;
    if ((rc = init_check(state, bytes, design))) return rc;
    std::vector<unsigned char> host(eqs_state_bytes());
    eqs_init_host(host.data(), *reinterpret_cast<const EqCoefs*>(design));
    // pageable host memory: the copy has left `host` when the call returns
    RCHK(hipMemcpyAsync(state, host.data(), host.size(), hipMemcpyHostToDevice, reinterpret_cast<hipStream_t>(stream)));
    return GSV_OK;
}

int gsv_eqstream_init_host(void* state, size_t bytes, const gsv_eq_design* design) {
    int rc;
    if ((rc = init_check(state, bytes, design))) return rc;
    eqs_init_host(static_cast<unsigned char*>(state), *reinterpret_cast<const EqCoefs*>(design));
    return GSV_OK;
}

int gsv_eqstream_push(void* state, const float* chunk, int n_cap, const int32_t* n_dev, int flush, float* out, gsv_eqstream_record* rec,
                      void* stream) {
    int rc;
    if ((rc = push_check(state, chunk, n_cap, out, rec))) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    unsigned char* s = static_cast<unsigned char*>(state);
    // sized by n_cap alone: the host does not know where in its open chunk the stream stands, so one block more than n_cap's chunks
    const unsigned blocks = (unsigned)std::min(EQS_MAX_BLOCKS, (n_cap + EQ_CHUNK - 1) / EQ_CHUNK + 1);
    if (n_cap > 0) {
        eqs_filter_kernel<true><<<blocks, EQ_T, 0, st>>>(s, chunk, n_cap, n_dev, out);
        RCHK(hipGetLastError());
    }
    eqs_chain_kernel<<<1, EQS_LANES, 0, st>>>(s, n_cap, n_dev);
    RCHK(hipGetLastError());
    if (n_cap > 0) {
        eqs_filter_kernel<false><<<blocks, EQ_T, 0, st>>>(s, chunk, n_cap, n_dev, out);
        RCHK(hipGetLastError());
    }
    eqs_commit_kernel<<<1, EQS_LANES, 0, st>>>(s, n_cap, n_dev, flush, reinterpret_cast<EqsRecord*>(rec));
    RCHK(hipGetLastError());
    return GSV_OK;
}

int gsv_eqstream_push_host(void* state, const float* chunk, int n_cap, const int32_t* n_host, int flush, float* out, gsv_eqstream_record* rec) {
    int rc;
    if ((rc = push_check(state, chunk, n_cap, out, rec))) return rc;
    const int n = n_host ? eqs_clamp(*n_host, n_cap) : n_cap;
    eqs_push_host(static_cast<unsigned char*>(state), chunk, n, flush != 0, out, reinterpret_cast<EqsRecord*>(rec));
    return GSV_OK;
}

}  // extern "C"
