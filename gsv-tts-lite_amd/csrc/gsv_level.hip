// C-ABI of the stream leveller (include/gsv_tts_hip.h, gsv_level_*; kernels and the host twin in level.h): the argument
// checks, the state built on the host and uploaded, and the two launches of a push.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/gsv_tts_hip.h"
#include "gsv_error.h"
#include "level.h"

using namespace gsv;

#define RCHK(expr)                                                                                        \
    do {                                                                                                  \
        hipError_t e_ = (expr);                                                                           \
        if (e_ != hipSuccess) return abi_fail(GSV_ERR_HIP, "%s: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

static_assert(sizeof(gsv_level_record) == sizeof(LevelRecord), "ABI struct");
static_assert(GSV_LEVEL_MEASURED == LEVEL_MEASURED && GSV_LEVEL_NONFINITE == LEVEL_NONFINITE && GSV_LEVEL_FULL == LEVEL_FULL, "flags");

namespace {

size_t state_bytes(int rate, int max_seconds) {
    if (!level_rate_ok(rate, max_seconds)) return 0;
    const int cap_blocks = level_cap_blocks(rate, max_seconds);
    return level_state_bytes(cap_blocks + 3, cap_blocks, level_ring_len(rate));
}

int init_check(void* state, size_t bytes, int rate, double target, double seed_lufs, double seed_blocks, double slew_db_s,
               double max_gain_db, float peak_limit, int max_seconds) {
    if (!state) return abi_fail(GSV_ERR_ARG, "null argument");
    if (!level_rate_ok(rate, max_seconds))
        return abi_fail(GSV_ERR_ARG, "level: %d Hz (%d..%d) with a history of %d s (1..%d)", rate, LEVEL_MIN_RATE, LEVEL_MAX_RATE,
                        max_seconds, LEVEL_MAX_SECONDS);
    if (!level_config_ok(target, seed_lufs, seed_blocks, slew_db_s, max_gain_db, peak_limit))
        return abi_fail(GSV_ERR_ARG, "level: target %g, seed %g with %g blocks, slew %g dB/s, at most %g dB, peak limit %g", target,
                        seed_lufs, seed_blocks, slew_db_s, max_gain_db, (double)peak_limit);
    const size_t need = state_bytes(rate, max_seconds);
    if (bytes < need || (reinterpret_cast<uintptr_t>(state) & 15))
        return abi_fail(GSV_ERR_ARG, "level: state of %zu bytes (%zu needed, 16-byte aligned)", bytes, need);
    return GSV_OK;
}

int push_check(const void* state, const float* chunk, int n_cap, const void* out, const void* rec) {
    if (!state || !rec || ((!chunk || !out) && n_cap > 0)) return abi_fail(GSV_ERR_ARG, "null argument");
    if (n_cap < 0) return abi_fail(GSV_ERR_ARG, "level: a chunk of %d samples", n_cap);
    if (reinterpret_cast<uintptr_t>(state) & 15) return abi_fail(GSV_ERR_ARG, "level: the state is not 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(rec) & 7) return abi_fail(GSV_ERR_ARG, "level: the record is not 8-byte aligned");
    return GSV_OK;
}

}  // namespace

extern "C" {

size_t gsv_level_state_bytes(int rate, int max_seconds) { return state_bytes(rate, max_seconds); }

int gsv_level_init(void* state, size_t bytes, int rate, double target, double seed_lufs, double seed_blocks, double slew_db_s,
                   double max_gain_db, float peak_limit, int max_seconds, void* stream) {
    int rc;
    if ((rc = init_check(state, bytes, rate, target, seed_lufs, seed_blocks, slew_db_s, max_gain_db, peak_limit, max_seconds))) return rc;
    // a fresh state is zeros behind the header and the first two knots: those are uploaded, the rest is set on the device
    const size_t need = state_bytes(rate, max_seconds), head = level_knots_off() + 2 * sizeof(double);
    std::vector<unsigned char> host(need);
    level_init_host(host.data(), rate, target, seed_lufs, seed_blocks, slew_db_s, max_gain_db, peak_limit, max_seconds);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    RCHK(hipMemsetAsync(static_cast<unsigned char*>(state) + head, 0, need - head, st));
    // pageable host memory: the copy has left `host` when the call returns
    RCHK(hipMemcpyAsync(state, host.data(), head, hipMemcpyHostToDevice, st));
    return GSV_OK;
}

int gsv_level_init_host(void* state, size_t bytes, int rate, double target, double seed_lufs, double seed_blocks, double slew_db_s,
                        double max_gain_db, float peak_limit, int max_seconds) {
    int rc;
    if ((rc = init_check(state, bytes, rate, target, seed_lufs, seed_blocks, slew_db_s, max_gain_db, peak_limit, max_seconds))) return rc;
    level_init_host(static_cast<unsigned char*>(state), rate, target, seed_lufs, seed_blocks, slew_db_s, max_gain_db, peak_limit,
                    max_seconds);
    return GSV_OK;
}

int gsv_level_push(void* state, const float* chunk, int n_cap, const int32_t* n_dev, int flush, float* out, gsv_level_record* rec,
                   void* stream) {
    int rc;
    if ((rc = push_check(state, chunk, n_cap, out, rec))) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    unsigned char* s = static_cast<unsigned char*>(state);
    LevelRecord* r = reinterpret_cast<LevelRecord*>(rec);
    level_measure_kernel<<<1, LEVEL_T, 0, st>>>(s, chunk, n_cap, n_dev, flush, r);
    RCHK(hipGetLastError());
    if (n_cap > 0) {
        const unsigned blocks = (unsigned)std::min(1024, (n_cap + LEVEL_APPLY_T - 1) / LEVEL_APPLY_T);
        level_apply_kernel<<<blocks, LEVEL_APPLY_T, 0, st>>>(s, chunk, n_cap, n_dev, out, r);
        RCHK(hipGetLastError());
    }
    return GSV_OK;
}

int gsv_level_push_host(void* state, const float* chunk, int n_cap, const int32_t* n_host, int flush, float* out,
                        gsv_level_record* rec) {
    int rc;
    if ((rc = push_check(state, chunk, n_cap, out, rec))) return rc;
    LevelHeader h;
    __builtin_memcpy(&h, state, sizeof(int32_t));
    if (h.magic != LEVEL_MAGIC) return abi_fail(GSV_ERR_ARG, "level: not a state gsv_level_init_host made");
    const int n = n_host ? std::min(std::max(*n_host, 0), n_cap) : n_cap;
    level_push_host(static_cast<unsigned char*>(state), chunk, n, flush != 0, out, reinterpret_cast<LevelRecord*>(rec));
    return GSV_OK;
}

}  // extern "C"
