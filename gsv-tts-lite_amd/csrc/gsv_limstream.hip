// C-ABI of the stream limiter (include/gsv_tts_hip.h, gsv_limstream_*; kernels and the host twin in limstream.h): the argument
// checks, the state built on the host and uploaded, and the three launches of a push.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/gsv_tts_hip.h"
#include "gsv_error.h"
#include "limstream.h"

using namespace gsv;

#define RCHK(expr)                                                                                        \
    do {                                                                                                  \
        hipError_t e_ = (expr);                                                                           \
        if (e_ != hipSuccess) return abi_fail(GSV_ERR_HIP, "%s: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

static_assert(sizeof(gsv_limstream_record) == sizeof(LimsRecord), "ABI structs");

namespace {

int init_check(const void* state, size_t bytes, float ceiling_db, int lookahead, int release) {
    if (!state) return abi_fail(GSV_ERR_ARG, "null argument");
    if (!lim_times_ok(lookahead, release))
        return abi_fail(GSV_ERR_ARG, "limstream: a look-ahead of %d samples (1..%d) or a release of %d (1..%d)", lookahead, LIM_MAX_L,
                        release, LIM_MAX_R);
    if (!(ceiling_db <= 0.f && ceiling_db >= -200.f))
        return abi_fail(GSV_ERR_ARG, "limstream: a ceiling of %g dBTP (-200..0)", (double)ceiling_db);
    const size_t need = lims_state_bytes(lookahead);
    if (bytes < need || (reinterpret_cast<uintptr_t>(state) & 15))
        return abi_fail(GSV_ERR_ARG, "limstream: state of %zu bytes (%zu needed, 16-byte aligned)", bytes, need);
    return GSV_OK;
}

int push_check(const void* state, const float* chunk, int n_cap, const float* out, const void* rec) {
    if (!state || !out || !rec || (!chunk && n_cap > 0)) return abi_fail(GSV_ERR_ARG, "null argument");
    if (n_cap < 0 || n_cap > LIMS_MAX_CHUNK) return abi_fail(GSV_ERR_ARG, "limstream: a chunk of %d samples (0..%d)", n_cap, LIMS_MAX_CHUNK);
    if (out == chunk) return abi_fail(GSV_ERR_ARG, "limstream: out is the chunk (a push emits samples of the push before it)");
    if (reinterpret_cast<uintptr_t>(state) & 15) return abi_fail(GSV_ERR_ARG, "limstream: the state is not 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(rec) & 7) return abi_fail(GSV_ERR_ARG, "limstream: the record is not 8-byte aligned");
    return GSV_OK;
}

}  // namespace

extern "C" {

size_t gsv_limstream_state_bytes(int lookahead, int release) {
    return lim_times_ok(lookahead, release) ? lims_state_bytes(lookahead) : 0;
}

size_t gsv_limstream_out_capacity(int n_cap, int lookahead) {
    if (n_cap < 0 || n_cap > LIMS_MAX_CHUNK || lookahead < 1 || lookahead > LIM_MAX_L) return 0;
    return (size_t)n_cap + (size_t)lims_delay(lookahead);
}

int gsv_limstream_init(void* state, size_t bytes, float ceiling_db, int lookahead, int release, void* stream) {
    int rc;
    if ((rc = init_check(state, bytes, ceiling_db, lookahead, release))) return rc;
    std::vector<unsigned char> host(lims_state_bytes(lookahead));
    lims_init_host(host.data(), ceiling_db, lookahead, release);
    // pageable host memory: the copy has left `host` when the call returns
    RCHK(hipMemcpyAsync(state, host.data(), host.size(), hipMemcpyHostToDevice, reinterpret_cast<hipStream_t>(stream)));
    return GSV_OK;
}

int gsv_limstream_init_host(void* state, size_t bytes, float ceiling_db, int lookahead, int release) {
    int rc;
    if ((rc = init_check(state, bytes, ceiling_db, lookahead, release))) return rc;
    lims_init_host(static_cast<unsigned char*>(state), ceiling_db, lookahead, release);
    return GSV_OK;
}

int gsv_limstream_push(void* state, const float* chunk, int n_cap, const int32_t* n_dev, int flush, float* out,
                       gsv_limstream_record* rec, void* stream) {
    int rc;
    if ((rc = push_check(state, chunk, n_cap, out, rec))) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    unsigned char* s = static_cast<unsigned char*>(state);
    // sized by n_cap alone: the host does not know the look-ahead, so it counts the tiles of n_cap + the longest delay
    const unsigned blocks = (unsigned)std::min(LIMS_MAX_TILES, (n_cap + lims_delay(LIM_MAX_L) + LIM_TILE - 1) / LIM_TILE + 1);
    lims_hold_kernel<<<blocks, LIM_TILE, 0, st>>>(s, chunk, n_cap, n_dev, flush);
    RCHK(hipGetLastError());
    lims_attack_kernel<<<blocks, LIM_TILE, 0, st>>>(s, chunk, n_cap, n_dev, flush, out);
    RCHK(hipGetLastError());
    lims_commit_kernel<<<1, LIM_TILE, 0, st>>>(s, chunk, n_cap, n_dev, flush, reinterpret_cast<LimsRecord*>(rec));
    RCHK(hipGetLastError());
    return GSV_OK;
}

int gsv_limstream_push_host(void* state, const float* chunk, int n_cap, const int32_t* n_host, int flush, float* out,
                            gsv_limstream_record* rec) {
    int rc;
    if ((rc = push_check(state, chunk, n_cap, out, rec))) return rc;
    LimsHeader h;
    memcpy(&h, state, sizeof h);
    if (h.magic != LIMS_MAGIC) return abi_fail(GSV_ERR_ARG, "limstream: not a state gsv_limstream_init_host made");
    const int n = n_host ? std::min(std::max(*n_host, 0), n_cap) : n_cap;
    lims_push_host(static_cast<unsigned char*>(state), chunk, n, flush != 0, out, reinterpret_cast<LimsRecord*>(rec));
    return GSV_OK;
}

}  // extern "C"
