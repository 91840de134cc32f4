// C-ABI of the FLAC writer (include/gsv_tts_hip.h, gsv_flac_encode*; kernels and the serial encoder in flacenc.h): the
// argument checks, the device frame table, and the three launches (frames, scan, copy).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/gsv_tts_hip.h"
#include "gsv_error.h"
#define GSV_FLACDEC_NO_KERNEL
#include "flacenc.h"

using namespace gsv;

static_assert(sizeof(FlacEncChoice) == sizeof(gsv_flac_enc_choice) && sizeof(gsv_flac_enc_choice) == 68, "choice record");
static_assert(FLAC_ENC_CONSTANT == GSV_FLAC_ENC_CONSTANT && FLAC_ENC_VERBATIM == GSV_FLAC_ENC_VERBATIM &&
              FLAC_ENC_FIXED == GSV_FLAC_ENC_FIXED, "flacenc.h's kinds are the ABI's GSV_FLAC_ENC_* codes");
static_assert(sizeof(FlacEncFrameDev) == 40, "device frame table entry");
static_assert(sizeof(gsv_flac_enc_frame) == 32 && sizeof(gsv_flac_enc_clip) == 16, "host tables");

#define RCHK(expr)                                                                                        \
    do {                                                                                                  \
        hipError_t e_ = (expr);                                                                           \
        if (e_ != hipSuccess) return abi_fail(GSV_ERR_HIP, "%s: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

namespace {

constexpr size_t kAlign = 256;

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// what the checks leave behind: the worst case of all frames, and of the largest (rounded up to 16: the slot stride)
struct EncPlan {
    size_t bound;
    uint32_t stride;
};

// the argument checks of gsv_flac_encode / gsv_flac_encode_host; `samples` may be null for the size queries
int enc_check(size_t n_samples, const gsv_flac_enc_clip* clips, int n_clips, const gsv_flac_enc_frame* frames, int n_frames,
              EncPlan* plan) {
    if (!clips || !frames) return abi_fail(GSV_ERR_ARG, "null argument");
    if (n_clips < 1 || n_clips > GSV_AUX_MAX_CLIPS)
        return abi_fail(GSV_ERR_ARG, "flac encode: %d clips (1..%d per call)", n_clips, GSV_AUX_MAX_CLIPS);
    if (n_frames < 1) return abi_fail(GSV_ERR_ARG, "flac encode: %d frames", n_frames);
    long long next[GSV_AUX_MAX_CLIPS];
    for (int c = 0; c < n_clips; ++c) {
        const gsv_flac_enc_clip& k = clips[c];
        if (k.bits_per_sample != 16 && k.bits_per_sample != 24)
            return abi_fail(GSV_ERR_ARG, "flac encode: clip %d: %d bits per sample (16 or 24)", c, k.bits_per_sample);
        if (k.n_samples < 1) return abi_fail(GSV_ERR_ARG, "flac encode: clip %d: %d samples", c, k.n_samples);
        if (k.in_offset < 0 || (unsigned long long)k.in_offset > n_samples ||
            (unsigned long long)k.n_samples > n_samples - (unsigned long long)k.in_offset)
            return abi_fail(GSV_ERR_ARG, "flac encode: clip %d: %d samples at sample %lld run past the %zu samples given", c,
                            k.n_samples, (long long)k.in_offset, n_samples);
        next[c] = 0;
    }
    size_t bound = 0;
    uint32_t worst = 0;
    for (int f = 0; f < n_frames; ++f) {
        const gsv_flac_enc_frame& r = frames[f];
        if (r.clip < 0 || r.clip >= n_clips) return abi_fail(GSV_ERR_ARG, "flac encode: frame %d: clip %d of %d", f, r.clip, n_clips);
        if (r.block_size < 1 || r.block_size > FLAC_ENC_MAX_BLOCK)
            return abi_fail(GSV_ERR_ARG, "flac encode: frame %d: block size %d (1..%d)", f, r.block_size, FLAC_ENC_MAX_BLOCK);
        if (r.header_len < FLAC_ENC_MIN_HEADER || r.header_len > FLAC_ENC_MAX_HEADER)
            return abi_fail(GSV_ERR_ARG, "flac encode: frame %d: header of %d bytes (%d..%d)", f, r.header_len, FLAC_ENC_MIN_HEADER,
                            FLAC_ENC_MAX_HEADER);
        if (r.first_sample != next[r.clip])
            return abi_fail(GSV_ERR_ARG, "flac encode: frame %d: starts at sample %d of clip %d where sample %lld is next (frames "
                            "of a clip come in order and tile it)", f, r.first_sample, r.clip, next[r.clip]);
        next[r.clip] += r.block_size;
        if (next[r.clip] > clips[r.clip].n_samples)
            return abi_fail(GSV_ERR_ARG, "flac encode: frame %d: ends at sample %lld of clip %d, which has %d", f, next[r.clip],
                            r.clip, clips[r.clip].n_samples);
        const uint32_t wb = flac_enc_worst_bytes(r.header_len, r.block_size, clips[r.clip].bits_per_sample);
        bound += wb;
        worst = std::max(worst, wb);
    }
    for (int c = 0; c < n_clips; ++c)
        if (next[c] != clips[c].n_samples)
            return abi_fail(GSV_ERR_ARG, "flac encode: clip %d: its frames hold %lld of %d samples", c, next[c], clips[c].n_samples);
    plan->bound = bound;
    plan->stride = (worst + 15u) & ~15u;
    return GSV_OK;
}

size_t table_bytes(int n_frames) { return align_up((size_t)n_frames * sizeof(FlacEncFrameDev), kAlign); }
size_t lengths_bytes(int n_frames) { return align_up((size_t)n_frames * sizeof(int32_t), kAlign); }

// the clips only have to be well-formed for the size queries: any input length will do
size_t total_in(const gsv_flac_enc_clip* clips, int n_clips) {
    size_t t = 0;
    if (!clips || n_clips < 1 || n_clips > GSV_AUX_MAX_CLIPS) return 0;
    for (int c = 0; c < n_clips; ++c)
        if (clips[c].in_offset >= 0 && clips[c].n_samples > 0) t = std::max(t, (size_t)clips[c].in_offset + (size_t)clips[c].n_samples);
    return t;
}

}  // namespace

extern "C" {

size_t gsv_flac_encode_bound(const gsv_flac_enc_clip* clips, int n_clips, const gsv_flac_enc_frame* frames, int n_frames) {
    EncPlan plan;
    if (enc_check(total_in(clips, n_clips), clips, n_clips, frames, n_frames, &plan)) return 0;
    return plan.bound;
}

size_t gsv_flac_encode_workspace(const gsv_flac_enc_clip* clips, int n_clips, const gsv_flac_enc_frame* frames, int n_frames) {
    EncPlan plan;
    if (enc_check(total_in(clips, n_clips), clips, n_clips, frames, n_frames, &plan)) return 0;
    return table_bytes(n_frames) + lengths_bytes(n_frames) + align_up((size_t)n_frames * plan.stride, kAlign);
}

// the body of gsv_flac_encode; ev: null, or four events recorded around the table upload, the frames kernel and scan + copy;
// serial_crc: the frames kernel with the one-lane CRC-16 (the measuring entry only)
static int enc_launch(const float* samples_dev, size_t n_samples, const gsv_flac_enc_clip* clips, int n_clips,
                      const gsv_flac_enc_frame* frames, int n_frames, uint8_t* out_dev, size_t out_bytes,
                      int64_t* frame_offsets_dev, gsv_flac_enc_choice* choices_dev, void* workspace, size_t workspace_bytes,
                      void* stream, hipEvent_t* ev, bool serial_crc) {
    if (!samples_dev || !out_dev || !frame_offsets_dev || !workspace) return abi_fail(GSV_ERR_ARG, "null argument");
    EncPlan plan;
    int rc;
    if ((rc = enc_check(n_samples, clips, n_clips, frames, n_frames, &plan))) return rc;
    if (out_bytes < plan.bound)
        return abi_fail(GSV_ERR_ARG, "flac encode: out_bytes %zu (%zu needed: every frame VERBATIM)", out_bytes, plan.bound);
    const size_t need = table_bytes(n_frames) + lengths_bytes(n_frames) + align_up((size_t)n_frames * plan.stride, kAlign);
    if (workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 15))
        return abi_fail(GSV_ERR_ARG, "flac encode: workspace of %zu bytes (%zu needed, 16-byte aligned)", workspace_bytes, need);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    FlacEncFrameDev* tab_dev = reinterpret_cast<FlacEncFrameDev*>(ws);
    int32_t* lengths = reinterpret_cast<int32_t*>(ws + table_bytes(n_frames));
    unsigned char* slots = reinterpret_cast<unsigned char*>(ws + table_bytes(n_frames) + lengths_bytes(n_frames));
    std::vector<FlacEncFrameDev> tab((size_t)n_frames);
    for (int f = 0; f < n_frames; ++f) {
        const gsv_flac_enc_frame& r = frames[f];
        FlacEncFrameDev& d = tab[f];
        d.in_off = clips[r.clip].in_offset + r.first_sample;
        d.block_size = r.block_size;
        d.bits = clips[r.clip].bits_per_sample;
        d.header_len = r.header_len;
        d.reserved = 0;
        for (int i = 0; i < FLAC_ENC_MAX_HEADER; ++i) d.header[i] = r.header[i];
    }
    if (ev) RCHK(hipEventRecord(ev[0], st));
    // pageable host memory: the copy has left `tab` when the call returns
    RCHK(hipMemcpyAsync(tab_dev, tab.data(), tab.size() * sizeof(FlacEncFrameDev), hipMemcpyHostToDevice, st));
    if (ev) RCHK(hipEventRecord(ev[1], st));
    FlacEncChoice* ch = reinterpret_cast<FlacEncChoice*>(choices_dev);
    if (serial_crc)
        flac_enc_frames_kernel<false><<<dim3((unsigned)n_frames), 64, 0, st>>>(samples_dev, tab_dev, n_frames, slots, plan.stride, lengths, ch);
    else
        flac_enc_frames_kernel<true><<<dim3((unsigned)n_frames), 64, 0, st>>>(samples_dev, tab_dev, n_frames, slots, plan.stride, lengths, ch);
    RCHK(hipGetLastError());
    if (ev) RCHK(hipEventRecord(ev[2], st));
    flac_enc_scan_kernel<<<1, 256, 0, st>>>(lengths, n_frames, reinterpret_cast<long long*>(frame_offsets_dev));
    RCHK(hipGetLastError());
    flac_enc_copy_kernel<<<dim3((unsigned)n_frames), 256, 0, st>>>(slots, plan.stride, lengths,
                                                                  reinterpret_cast<const long long*>(frame_offsets_dev), n_frames,
                                                                  out_dev, (unsigned long long)out_bytes);
    RCHK(hipGetLastError());
    if (ev) RCHK(hipEventRecord(ev[3], st));
    return GSV_OK;
}

int gsv_flac_encode(const float* samples_dev, size_t n_samples, const gsv_flac_enc_clip* clips, int n_clips,
                    const gsv_flac_enc_frame* frames, int n_frames, uint8_t* out_dev, size_t out_bytes,
                    int64_t* frame_offsets_dev, gsv_flac_enc_choice* choices_dev, void* workspace, size_t workspace_bytes,
                    void* stream) {
    return enc_launch(samples_dev, n_samples, clips, n_clips, frames, n_frames, out_dev, out_bytes, frame_offsets_dev, choices_dev,
                      workspace, workspace_bytes, stream, nullptr, false);
}

// Not part of the ABI (include/gsv_tts_hip.h does not declare it): tools/flac_encode_time.py and the GPU test that pins its
// bytes to gsv_flac_encode's bind it by name.  gsv_flac_encode with hipEvents around its parts; it waits for the stream, then
// ms[0] is the table upload, ms[1] the frames kernel, ms[2] scan + copy, in milliseconds.  serial_crc != 0 launches the
// frames kernel whose CRC-16 is one lane's pass: the yardstick of the lane-split form, same bytes.
int gsv_flac_encode_timed(const float* samples_dev, size_t n_samples, const gsv_flac_enc_clip* clips, int n_clips,
                          const gsv_flac_enc_frame* frames, int n_frames, uint8_t* out_dev, size_t out_bytes,
                          int64_t* frame_offsets_dev, gsv_flac_enc_choice* choices_dev, void* workspace, size_t workspace_bytes,
                          void* stream, int serial_crc, float* ms) {
    if (!ms) return abi_fail(GSV_ERR_ARG, "null argument");
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    int rc = GSV_OK;
    for (int i = 0; i < 4 && rc == GSV_OK; ++i)
        if (hipEventCreate(&ev[i]) != hipSuccess) rc = abi_fail(GSV_ERR_HIP, "hipEventCreate");
    if (rc == GSV_OK)
        rc = enc_launch(samples_dev, n_samples, clips, n_clips, frames, n_frames, out_dev, out_bytes, frame_offsets_dev, choices_dev,
                        workspace, workspace_bytes, stream, ev, serial_crc != 0);
    if (rc == GSV_OK && hipEventSynchronize(ev[3]) != hipSuccess) rc = abi_fail(GSV_ERR_HIP, "hipEventSynchronize");
    for (int i = 0; i < 3 && rc == GSV_OK; ++i)
        if (hipEventElapsedTime(&ms[i], ev[i], ev[i + 1]) != hipSuccess) rc = abi_fail(GSV_ERR_HIP, "hipEventElapsedTime");
    for (int i = 0; i < 4; ++i)
        if (ev[i]) (void)hipEventDestroy(ev[i]);
    return rc;
}

int gsv_flac_encode_host(const float* samples, size_t n_samples, const gsv_flac_enc_clip* clips, int n_clips,
                         const gsv_flac_enc_frame* frames, int n_frames, uint8_t* out, size_t out_bytes, int64_t* frame_offsets,
                         gsv_flac_enc_choice* choices) {
    if (!samples || !out || !frame_offsets) return abi_fail(GSV_ERR_ARG, "null argument");
    EncPlan plan;
    int rc;
    if ((rc = enc_check(n_samples, clips, n_clips, frames, n_frames, &plan))) return rc;
    if (out_bytes < plan.bound)
        return abi_fail(GSV_ERR_ARG, "flac encode: out_bytes %zu (%zu needed: every frame VERBATIM)", out_bytes, plan.bound);
    // a frame is written where it ends up: what lies behind it is at least the worst case of the frames still to come
    int64_t at = 0;
    for (int f = 0; f < n_frames; ++f) {
        const gsv_flac_enc_frame& r = frames[f];
        frame_offsets[f] = at;
        at += flac_encode_frame_host(samples + clips[r.clip].in_offset + r.first_sample, r.block_size, clips[r.clip].bits_per_sample,
                                     r.header, r.header_len, out + at, reinterpret_cast<FlacEncChoice*>(choices ? choices + f : nullptr));
    }
    frame_offsets[n_frames] = at;
    return GSV_OK;
}

}  // extern "C"
