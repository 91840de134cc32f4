// C-ABI of the real-time track output (include/gsv_tts_hip.h, gsv_track_*; kernels and the host twin in track.h): the
// argument checks, the state built on the host and uploaded, and the two launches of a push.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/gsv_tts_hip.h"
#include "gsv_error.h"
#define GSV_FLACDEC_NO_KERNEL
#define GSV_FLACENC_NO_KERNEL
#include "track.h"

using namespace gsv;

#define RCHK(expr)                                                                                        \
    do {                                                                                                  \
        hipError_t e_ = (expr);                                                                           \
        if (e_ != hipSuccess) return abi_fail(GSV_ERR_HIP, "%s: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

namespace {

struct TrackGeo { int o, w, width, L; };

// the checks every entry shares; quiet: the size queries answer 0 and leave gsv_last_error alone
int track_check(int in_rate, int out_rate, int packet, int channels, TrackGeo* g, bool quiet) {
    if (!track_params(in_rate, out_rate, &g->o, &g->w, &g->width))
        return quiet ? GSV_ERR_ARG : abi_fail(GSV_ERR_ARG, "track: resampling %d -> %d Hz unsupported", in_rate, out_rate);
    if (packet < 1 || packet > TRACK_MAX_PACKET)
        return quiet ? GSV_ERR_ARG : abi_fail(GSV_ERR_ARG, "track: packets of %d samples (1..%d)", packet, TRACK_MAX_PACKET);
    if (channels != 1 && channels != 2) return quiet ? GSV_ERR_ARG : abi_fail(GSV_ERR_ARG, "track: %d channels (1 or 2)", channels);
    g->L = 2 * g->width + g->o;
    return GSV_OK;
}

int init_check(void* state, size_t bytes, int in_rate, int out_rate, int packet, int channels, TrackGeo* g) {
    if (!state) return abi_fail(GSV_ERR_ARG, "null argument");
    int rc;
    if ((rc = track_check(in_rate, out_rate, packet, channels, g, false))) return rc;
    const size_t need = track_state_bytes(g->o, g->w, g->L, packet, channels);
    if (bytes < need || (reinterpret_cast<uintptr_t>(state) & 15))
        return abi_fail(GSV_ERR_ARG, "track: state of %zu bytes (%zu needed, 16-byte aligned)", bytes, need);
    return GSV_OK;
}

int push_check(const void* state, const float* chunk, int n_cap, const void* out, const void* rec) {
    if (!state || !out || !rec || (!chunk && n_cap > 0)) return abi_fail(GSV_ERR_ARG, "null argument");
    if (n_cap < 0) return abi_fail(GSV_ERR_ARG, "track: a chunk of %d samples", n_cap);
    if (reinterpret_cast<uintptr_t>(state) & 15) return abi_fail(GSV_ERR_ARG, "track: the state is not 16-byte aligned");
    return GSV_OK;
}

}  // namespace

extern "C" {

size_t gsv_track_state_bytes(int in_rate, int out_rate, int packet, int channels) {
    TrackGeo g;
    if (track_check(in_rate, out_rate, packet, channels, &g, true)) return 0;
    return track_state_bytes(g.o, g.w, g.L, packet, channels);
}

size_t gsv_track_out_capacity(int n_cap, int in_rate, int out_rate, int packet, int channels) {
    TrackGeo g;
    if (n_cap < 0 || track_check(in_rate, out_rate, packet, channels, &g, true)) return 0;
    return (size_t)track_out_capacity(n_cap, g.o, g.w, g.L, packet, channels);
}

int gsv_track_init(void* state, size_t bytes, int in_rate, int out_rate, int packet, int channels, void* stream) {
    TrackGeo g;
    int rc;
    if ((rc = init_check(state, bytes, in_rate, out_rate, packet, channels, &g))) return rc;
    std::vector<unsigned char> host(track_state_bytes(g.o, g.w, g.L, packet, channels));
    track_init_host(host.data(), g.o, g.w, g.width, packet, channels);
    // pageable host memory: the copy has left `host` when the call returns
    RCHK(hipMemcpyAsync(state, host.data(), host.size(), hipMemcpyHostToDevice, reinterpret_cast<hipStream_t>(stream)));
    return GSV_OK;
}

int gsv_track_init_host(void* state, size_t bytes, int in_rate, int out_rate, int packet, int channels) {
    TrackGeo g;
    int rc;
    if ((rc = init_check(state, bytes, in_rate, out_rate, packet, channels, &g))) return rc;
    track_init_host(static_cast<unsigned char*>(state), g.o, g.w, g.width, packet, channels);
    return GSV_OK;
}

int gsv_track_push(void* state, const float* chunk, int n_cap, const int32_t* n_dev, int flush, int16_t* out, int32_t* rec,
                   void* stream) {
    int rc;
    if ((rc = push_check(state, chunk, n_cap, out, rec))) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    unsigned char* s = static_cast<unsigned char*>(state);
    // sized by n_cap alone: a block walks further tiles when the rates make more outputs than inputs
    const unsigned blocks = (unsigned)std::min(4096, std::max(1, (n_cap + TRACK_TILE - 1) / TRACK_TILE));
    track_outputs_kernel<<<blocks, TRACK_TILE, 0, st>>>(s, chunk, n_cap, n_dev, flush, out);
    RCHK(hipGetLastError());
    track_commit_kernel<<<1, TRACK_TILE, 0, st>>>(s, chunk, n_cap, n_dev, flush, out, rec);
    RCHK(hipGetLastError());
    return GSV_OK;
}

int gsv_track_push_host(void* state, const float* chunk, int n_cap, const int32_t* n_host, int flush, int16_t* out, int32_t* rec) {
    int rc;
    if ((rc = push_check(state, chunk, n_cap, out, rec))) return rc;
    TrackHeader h;
    __builtin_memcpy(&h, state, sizeof h);
    if (h.magic != TRACK_MAGIC) return abi_fail(GSV_ERR_ARG, "track: not a state gsv_track_init_host made");
    const int n = n_host ? std::min(std::max(*n_host, 0), n_cap) : n_cap;
    track_push_host(static_cast<unsigned char*>(state), chunk, n, flush != 0, out, rec);
    return GSV_OK;
}

}  // extern "C"
