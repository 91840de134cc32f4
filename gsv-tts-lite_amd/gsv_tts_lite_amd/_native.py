"""ctypes binding of the C ABI in include/gsv_tts_hip.h (libgsv_hip.so, gfx950 only).

There is no fallback: if the shared library is missing, or a call fails, this raises.
PyTorch is used by callers only for device memory and streams; every pointer crossing
this boundary is a raw device address (`tensor.data_ptr()`).
"""
from __future__ import annotations

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GSV_HIP_LIB") or os.path.join(os.path.dirname(_HERE), "lib", "libgsv_hip.so")   # GSV_HIP_LIB: an experimental build of the same ABI (tools/)
CSRC = os.path.join(os.path.dirname(_HERE), "csrc")

GSV_F32, GSV_BF16, GSV_FP8 = 0, 1, 2

EXPORTS = [
    "gsv_version", "gsv_last_error",
    "gsv_t2s_create", "gsv_t2s_destroy", "gsv_t2s_load_tensor", "gsv_t2s_finalize", "gsv_t2s_bind_state", "gsv_t2s_unbind_state",
    "gsv_t2s_embed_prompt", "gsv_t2s_prefill_workspace", "gsv_t2s_prefill", "gsv_t2s_set_eos_mirror", "gsv_t2s_set_slot_sampling", "gsv_t2s_put_slot_sampling", "gsv_t2s_seed_seen", "gsv_t2s_prefill_slots", "gsv_t2s_prefill_slots_staged", "gsv_t2s_commit_slots", "gsv_t2s_adopt_slots", "gsv_t2s_move_slots", "gsv_t2s_decode_hidden",
    "gsv_t2s_decode", "gsv_t2s_flush", "gsv_t2s_time_kernels", "gsv_t2s_set_debug", "gsv_t2s_batched_min", "gsv_t2s_ffn_slices", "gsv_t2s_device_bytes",
    "gsv_voc_create", "gsv_voc_destroy", "gsv_voc_load_tensor", "gsv_voc_finalize", "gsv_voc_workspace",
    "gsv_voc_flow_dec", "gsv_voc_flow_dec_graph", "gsv_voc_resample_linear", "gsv_voc_flow", "gsv_voc_dec", "gsv_voc_has_enc_p", "gsv_voc_enc_workspace", "gsv_voc_enc_p", "gsv_voc_decode_workspace", "gsv_voc_decode",
    "gsv_voc_decode_segments_workspace", "gsv_voc_decode_segments",
    "gsv_align_workspace", "gsv_align_viterbi", "gsv_sola_workspace", "gsv_sola", "gsv_stream_emit_workspace", "gsv_stream_emit",
    "gsv_ref_create", "gsv_ref_destroy", "gsv_ref_load_tensor", "gsv_ref_finalize", "gsv_ref_workspace",
    "gsv_ref_spectrogram", "gsv_ref_get_ge", "gsv_ref_extract_latent",
    "gsv_hubert_create", "gsv_hubert_destroy", "gsv_hubert_load_tensor", "gsv_hubert_finalize", "gsv_hubert_frames",
    "gsv_hubert_workspace", "gsv_hubert_forward", "gsv_hubert_batch_workspace", "gsv_hubert_forward_batch",
    "gsv_sv_create", "gsv_sv_destroy", "gsv_sv_load_tensor", "gsv_sv_finalize", "gsv_sv_resample_length",
    "gsv_sv_resample_workspace", "gsv_sv_resample", "gsv_sv_frames", "gsv_sv_workspace", "gsv_sv_fbank", "gsv_sv_forward",
    "gsv_sv_embed", "gsv_sv_batch_workspace", "gsv_sv_forward_batch", "gsv_sv_embed_batch",
    "gsv_roberta_create", "gsv_roberta_destroy", "gsv_roberta_load_tensor", "gsv_roberta_finalize", "gsv_roberta_workspace",
    "gsv_roberta_forward", "gsv_roberta_features",
    "gsv_wav_to_mono", "gsv_wav_to_mono_batch",
    "gsv_flac_decode_workspace", "gsv_flac_decode", "gsv_flac_decode_host",
    "gsv_flac_encode_bound", "gsv_flac_encode_workspace", "gsv_flac_encode", "gsv_flac_encode_host",
    "gsv_track_state_bytes", "gsv_track_out_capacity", "gsv_track_init", "gsv_track_push", "gsv_track_init_host", "gsv_track_push_host",
    "gsv_loudness_work_bytes", "gsv_loudness", "gsv_loudness_host",
    "gsv_level_state_bytes", "gsv_level_init", "gsv_level_push", "gsv_level_init_host", "gsv_level_push_host",
    "gsv_limiter_work_bytes", "gsv_limiter", "gsv_limiter_host",
    "gsv_limstream_state_bytes", "gsv_limstream_out_capacity", "gsv_limstream_init", "gsv_limstream_push", "gsv_limstream_init_host",
    "gsv_limstream_push_host",
    "gsv_eq_work_bytes", "gsv_eq", "gsv_eq_host",
    "gsv_eqstream_state_bytes", "gsv_eqstream_init", "gsv_eqstream_push", "gsv_eqstream_init_host", "gsv_eqstream_push_host",
    "gsv_compressor_work_bytes", "gsv_compressor", "gsv_compressor_host", "gsv_compressor_math_host",
    "gsv_cmpstream_state_bytes", "gsv_cmpstream_init", "gsv_cmpstream_push", "gsv_cmpstream_init_host", "gsv_cmpstream_push_host",
    "gsv_reverb_work_bytes", "gsv_reverb", "gsv_reverb_host",
]


class T2SConfig(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in
                ("n_layer", "hidden", "n_head", "vocab", "eos", "n_pos", "n_phoneme", "dtype")]


class T2SState(ctypes.Structure):
    _fields_ = [("batch", ctypes.c_int), ("max_kv", ctypes.c_int)] + [(n, ctypes.c_void_p) for n in (
        "k_cache", "v_cache", "kv_len", "x_len", "pre_tokens", "seen", "step", "eos_at", "logits", "hidden",
        "tok_override", "ctl", "fctl")]


class SlotSampling(ctypes.Structure):
    """gsv_t2s_slot_sampling: one slot's entry of the per-slot sampling table (32 bytes)"""
    _fields_ = [("sample_mode", ctypes.c_int32), ("top_k", ctypes.c_int32), ("temperature", ctypes.c_float),
                ("top_p", ctypes.c_float), ("seed_lo", ctypes.c_int32), ("seed_hi", ctypes.c_int32),
                ("rep_penalty", ctypes.c_float), ("suppress_steps", ctypes.c_int32)]


class VocConfig(ctypes.Structure):
    _fields_ = [("inter_channels", ctypes.c_int), ("hidden_channels", ctypes.c_int), ("gin_channels", ctypes.c_int),
                ("upsample_initial_channel", ctypes.c_int), ("n_upsample", ctypes.c_int),
                ("upsample_rates", ctypes.c_int * 8), ("upsample_kernel_sizes", ctypes.c_int * 8),
                ("n_resblock_kernels", ctypes.c_int), ("resblock_kernel_sizes", ctypes.c_int * 4),
                ("resblock_dilations", ctypes.c_int * 4), ("n_flows", ctypes.c_int), ("dtype", ctypes.c_int)]


VOC_MAX_SEGMENTS = 64   # GSV_VOC_MAX_SEGMENTS: utterances per gsv_voc_decode_segments call


class VocSegment(ctypes.Structure):
    """gsv_voc_segment: one utterance of gsv_voc_decode_segments (24 bytes)"""
    _fields_ = [("n_codes", ctypes.c_int32), ("out_frames", ctypes.c_int32), ("noise_scale", ctypes.c_float),
                ("seed", ctypes.c_uint64)]


class RefConfig(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in
                ("n_fft", "hop", "spec_bins", "hidden", "n_head", "kernel", "gin", "sv_dim", "ssl_dim", "bins")]


HUBERT_MAX_CONV = 8
AUX_MAX_CLIPS = 64      # GSV_AUX_MAX_CLIPS: clips per gsv_hubert_forward_batch / gsv_sv_*_batch call


class HubertConfig(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in ("hidden", "n_layer", "n_head", "ffn", "n_conv")] + [
        (n, ctypes.c_int * HUBERT_MAX_CONV) for n in ("conv_dim", "conv_kernel", "conv_stride")] + [
        ("pos_k", ctypes.c_int), ("pos_groups", ctypes.c_int), ("eps", ctypes.c_float)]


class SvConfig(ctypes.Structure):
    _fields_ = [("m_channels", ctypes.c_int), ("blocks", ctypes.c_int * 4), ("width", ctypes.c_int * 4),
                ("scale", ctypes.c_int), ("expansion", ctypes.c_int), ("feat_dim", ctypes.c_int)]


class WavClip(ctypes.Structure):
    """gsv_wav_clip: one clip of gsv_wav_to_mono_batch"""
    _fields_ = [("byte_offset", ctypes.c_int64), ("n_frames", ctypes.c_int32), ("format", ctypes.c_int16),
                ("channels", ctypes.c_int16)]


class FlacClip(ctypes.Structure):
    """gsv_flac_clip: one clip of gsv_flac_decode"""
    _fields_ = [("channels", ctypes.c_int32), ("bits_per_sample", ctypes.c_int32), ("n_samples", ctypes.c_int32),
                ("reserved", ctypes.c_int32), ("out_offset", ctypes.c_int64)]


class FlacFrame(ctypes.Structure):
    """gsv_flac_frame: one frame of gsv_flac_decode"""
    _fields_ = [("clip", ctypes.c_int32), ("block_size", ctypes.c_int32), ("byte_offset", ctypes.c_int64),
                ("byte_len", ctypes.c_int32), ("first_sample", ctypes.c_int32), ("flags", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


FLAC_OPEN_END = 1       # GSV_FLAC_OPEN_END


class FlacEncClip(ctypes.Structure):
    """gsv_flac_enc_clip: one clip of gsv_flac_encode"""
    _fields_ = [("in_offset", ctypes.c_int64), ("n_samples", ctypes.c_int32), ("bits_per_sample", ctypes.c_int32)]


class FlacEncFrame(ctypes.Structure):
    """gsv_flac_enc_frame: one frame of gsv_flac_encode; header: the frame header through its CRC-8"""
    _fields_ = [("clip", ctypes.c_int32), ("block_size", ctypes.c_int32), ("first_sample", ctypes.c_int32),
                ("header_len", ctypes.c_int32), ("header", ctypes.c_uint8 * 16)]


class FlacEncChoice(ctypes.Structure):
    """gsv_flac_enc_choice: what a frame was coded with"""
    _fields_ = [("kind", ctypes.c_uint8), ("order", ctypes.c_uint8), ("porder", ctypes.c_uint8), ("method", ctypes.c_uint8),
                ("k", ctypes.c_uint8 * 64)]


class LoudnessClip(ctypes.Structure):
    """gsv_loudness_clip: one clip of gsv_loudness; target NaN: measure only"""
    _fields_ = [("offset", ctypes.c_int64), ("n_samples", ctypes.c_int32), ("target", ctypes.c_float)]


class LoudnessRecord(ctypes.Structure):
    """gsv_loudness_record: what gsv_loudness found and did per clip"""
    _fields_ = [("zbar", ctypes.c_double), ("gain", ctypes.c_float), ("peak", ctypes.c_float), ("blocks", ctypes.c_int32),
                ("above_abs", ctypes.c_int32), ("kept", ctypes.c_int32), ("flags", ctypes.c_int32)]


LOUD_LIMITED, LOUD_MEASURED, LOUD_NONFINITE = 1, 2, 4       # GSV_LOUD_*


class LevelRecord(ctypes.Structure):
    """gsv_level_record: the running measure and the gains of one gsv_level_push"""
    _fields_ = [("zbar", ctypes.c_double), ("gain_first", ctypes.c_float), ("gain_last", ctypes.c_float), ("clamped", ctypes.c_int64),
                ("blocks", ctypes.c_int32), ("above_abs", ctypes.c_int32), ("kept", ctypes.c_int32), ("flags", ctypes.c_int32)]


LEVEL_MEASURED, LEVEL_NONFINITE, LEVEL_FULL = 2, 4, 8       # GSV_LEVEL_*

class LimiterClip(ctypes.Structure):
    """gsv_limiter_clip: one clip of gsv_limiter; ceiling_db NaN: measure only"""
    _fields_ = [("offset", ctypes.c_int64), ("n_samples", ctypes.c_int32), ("ceiling_db", ctypes.c_float)]


class LimiterRecord(ctypes.Structure):
    """gsv_limiter_record: what gsv_limiter found and did per clip"""
    _fields_ = [("true_peak_in", ctypes.c_float), ("true_peak_out", ctypes.c_float), ("min_gain", ctypes.c_float),
                ("trim", ctypes.c_float), ("flags", ctypes.c_int32), ("lookahead", ctypes.c_int32), ("release", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


LIM_LIMITED, LIM_NONFINITE = 1, 4       # GSV_LIM_*


class LimstreamRecord(ctypes.Structure):
    """gsv_limstream_record: what one gsv_limstream_push emitted and did"""
    _fields_ = [("emitted", ctypes.c_int32), ("flags", ctypes.c_int16), ("lookahead", ctypes.c_int16), ("peak_in", ctypes.c_float),
                ("peak_run", ctypes.c_float), ("min_gain", ctypes.c_float), ("release", ctypes.c_int32), ("total", ctypes.c_int64)]


LIMS_LIMITED, LIMS_LIMITED_EVER, LIMS_NONFINITE = 1, 2, 4       # GSV_LIMS_*
LIMS_MAX_CHUNK = 1 << 20                # csrc/limstream.h: samples of one push
LIM_TILE, LIM_MAX_LOOKAHEAD, LIM_MAX_RELEASE = 1024, 4096, 1 << 24      # csrc/limiter.h: LIM_TILE, LIM_MAX_L, LIM_MAX_R

EQ_MAX_SECTIONS = 6             # GSV_EQ_MAX_SECTIONS


class EqClip(ctypes.Structure):
    """gsv_eq_clip: one clip of gsv_eq; design -1: measure the peaks, copy"""
    _fields_ = [("offset", ctypes.c_int64), ("n_samples", ctypes.c_int32), ("design", ctypes.c_int32)]


class EqDesign(ctypes.Structure):
    """gsv_eq_design: per section b0 b1 b2 a1 a2, normalised by a0"""
    _fields_ = [("n_sections", ctypes.c_int32), ("reserved", ctypes.c_int32), ("coef", (ctypes.c_double * 5) * EQ_MAX_SECTIONS)]


class EqRecord(ctypes.Structure):
    """gsv_eq_record: what gsv_eq found and did per clip"""
    _fields_ = [("peak_in", ctypes.c_float), ("peak_out", ctypes.c_float), ("sections", ctypes.c_int32), ("flags", ctypes.c_int32)]


EQ_EQUALISED, EQ_NONFINITE = 1, 4       # GSV_EQ_*
EQ_RUN, EQ_SPAN, EQ_CHUNK = 16, 512 * 16, 2 * 512 * 16      # csrc/eq.h: EQ_R, EQ_SPAN, EQ_CHUNK


class EqstreamRecord(ctypes.Structure):
    """gsv_eqstream_record: what one gsv_eqstream_push emitted and found"""
    _fields_ = [("emitted", ctypes.c_int32), ("flags", ctypes.c_int32), ("peak_in", ctypes.c_float), ("peak_out", ctypes.c_float),
                ("peak_in_run", ctypes.c_float), ("peak_out_run", ctypes.c_float), ("total", ctypes.c_int64)]


EQS_EQUALISED, EQS_NONFINITE_EVER, EQS_NONFINITE = 1, 2, 4      # GSV_EQS_*
EQS_MAX_CHUNK = 1 << 20                 # csrc/eqstream.h: samples of one push


class CompressorClip(ctypes.Structure):
    """gsv_compressor_clip: one clip of gsv_compressor; params -1: measure the peaks, copy"""
    _fields_ = [("offset", ctypes.c_int64), ("n_samples", ctypes.c_int32), ("params", ctypes.c_int32)]


class CompressorParams(ctypes.Structure):
    """gsv_compressor_params: the one-pole coefficients, the linear threshold, 1 / ratio - 1, the linear makeup"""
    _fields_ = [("attack", ctypes.c_double), ("release", ctypes.c_double), ("threshold", ctypes.c_double), ("slope", ctypes.c_double),
                ("makeup", ctypes.c_double)]


class CompressorRecord(ctypes.Structure):
    """gsv_compressor_record: what gsv_compressor found and did per clip"""
    _fields_ = [("peak_in", ctypes.c_float), ("peak_out", ctypes.c_float), ("min_gain", ctypes.c_float), ("flags", ctypes.c_int32)]


CMP_COMPRESSED, CMP_NONFINITE = 1, 4    # GSV_CMP_*
CMP_RUN, CMP_SPAN, CMP_CHUNK = 16, 512 * 16, 2 * 512 * 16       # csrc/compressor.h: CMP_R, CMP_SPAN, CMP_CHUNK


class ReverbClip(ctypes.Structure):
    """gsv_reverb_clip: one clip of gsv_reverb; params -1: measure the peaks, copy"""
    _fields_ = [("offset", ctypes.c_int64), ("n_samples", ctypes.c_int32), ("params", ctypes.c_int32)]


class ReverbParams(ctypes.Structure):
    """gsv_reverb_params: the eight comb and four all-pass delays in samples, damping, feedback, the input, wet and dry gains"""
    _fields_ = [("comb", ctypes.c_int32 * 8), ("allpass", ctypes.c_int32 * 4), ("d", ctypes.c_double), ("fb", ctypes.c_double),
                ("gin", ctypes.c_double), ("gw", ctypes.c_double), ("gd", ctypes.c_double)]


class ReverbRecord(ctypes.Structure):
    """gsv_reverb_record: what gsv_reverb found and did per clip"""
    _fields_ = [("peak_in", ctypes.c_float), ("peak_out", ctypes.c_float), ("flags", ctypes.c_int32), ("pad", ctypes.c_int32)]


RVB_REVERBED, RVB_NONFINITE = 1, 4      # GSV_RVB_*
RVB_MAX_DELAY = 32768                   # GSV_RVB_MAX_DELAY
RVB_SPAN = 64 * 32                      # csrc/reverb.h: RVB_SPAN, the longest line a comb's wave keeps in registers


class CmpstreamRecord(ctypes.Structure):
    """gsv_cmpstream_record: what one gsv_cmpstream_push emitted and found"""
    _fields_ = [("emitted", ctypes.c_int32), ("flags", ctypes.c_int32), ("peak_in", ctypes.c_float), ("peak_out", ctypes.c_float),
                ("min_gain", ctypes.c_float), ("peak_in_run", ctypes.c_float), ("peak_out_run", ctypes.c_float),
                ("min_gain_run", ctypes.c_float), ("total", ctypes.c_int64)]


CMS_STREAM, CMS_NONFINITE_EVER, CMS_NONFINITE, CMS_COMPRESSED = 1, 2, 4, 8      # GSV_CMS_*
CMS_MAX_CHUNK = 1 << 20                 # csrc/cmpstream.h: samples of one push

FLAC_ENC_CONSTANT, FLAC_ENC_VERBATIM, FLAC_ENC_FIXED = range(3)     # GSV_FLAC_ENC_*
FLAC_ENC_MAX_BLOCK = 4608


# GSV_FLAC_*: what a frame's status says
FLAC_STATUS = ("ok", "overrun: the frame's structure needs more bits than the frame holds", "no frame sync code",
               "a reserved code", "header CRC-8 mismatch", "header disagrees with STREAMINFO or the frame index",
               "predictor order larger than the block", "residual partitions do not divide the block",
               "residual outside 32 bits", "sample outside the stream's bits per sample",
               "the frame's structure ends before its last bytes", "CRC-16 mismatch", "wasted bits leave no bit of the sample")
FLAC_CRC16 = 11

PCM_U8, PCM_S16, PCM_S24, PCM_S32, PCM_F32, PCM_F64 = range(6)   # GSV_PCM_*


class RobertaConfig(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in ("hidden", "n_layer", "n_head", "ffn", "vocab", "max_pos", "type_vocab")] + [
        ("eps", ctypes.c_float)]


_LIB = None


def lib():
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "gsv_tts_lite_amd: HIP extension %s is missing. Build it with `python -c \"import __graft_entry__ as g; "
            "g.build()\"` (hipcc --offload-arch=gfx950). There is no CPU or PyTorch fallback for the hot path." % LIB_PATH)
    L = ctypes.CDLL(LIB_PATH)
    vp, i, i64, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_size_t
    ip = ctypes.POINTER(ctypes.c_int)   # host int arrays
    L.gsv_version.restype = i
    L.gsv_last_error.restype = ctypes.c_char_p
    sig = {
        "gsv_t2s_create": [ctypes.POINTER(T2SConfig), ctypes.POINTER(vp)],
        "gsv_t2s_destroy": [vp],
        "gsv_t2s_load_tensor": [vp, ctypes.c_char_p, vp, i64, vp],
        "gsv_t2s_finalize": [vp, vp],
        "gsv_t2s_bind_state": [vp, ctypes.POINTER(T2SState)],
        "gsv_t2s_unbind_state": [vp, i],
        "gsv_t2s_embed_prompt": [vp, i, i, i, i, vp, vp, vp, vp, vp, vp, vp, vp],
        "gsv_t2s_prefill": [vp, i, i, i, i, vp, vp, vp, vp, sz, vp],
        "gsv_t2s_set_eos_mirror": [vp, i, vp],
        "gsv_t2s_set_slot_sampling": [vp, i, vp],
        "gsv_t2s_put_slot_sampling": [vp, i, vp, ctypes.POINTER(SlotSampling), i, vp],
        "gsv_t2s_seed_seen": [vp, i, vp, vp, vp, i, vp],
        "gsv_t2s_prefill_slots": [vp, i, vp, i, i, vp, vp, vp, vp, sz, vp],
        "gsv_t2s_prefill_slots_staged": [vp, i, vp, i, i, vp, vp, vp, vp, sz, vp],
        "gsv_t2s_commit_slots": [vp, i, vp, i, vp],
        "gsv_t2s_adopt_slots": [vp, i, vp, i, vp, vp, i, vp],
        "gsv_t2s_move_slots": [vp, i, vp, i, vp, i, vp],
        "gsv_t2s_decode_hidden": [vp, i, vp, vp],
        "gsv_t2s_decode": [vp, i, i, i, vp],
        "gsv_t2s_flush": [vp, i, vp],
        "gsv_t2s_set_debug": [vp, vp],
        "gsv_t2s_batched_min": [vp],
        "gsv_t2s_ffn_slices": [vp, ctypes.c_int],
        "gsv_t2s_time_kernels": [vp, i, i, ctypes.POINTER(ctypes.c_float), vp],
        "gsv_voc_create": [ctypes.POINTER(VocConfig), ctypes.POINTER(vp)],
        "gsv_voc_destroy": [vp],
        "gsv_voc_load_tensor": [vp, ctypes.c_char_p, vp, i64, vp],
        "gsv_voc_finalize": [vp, vp],
        "gsv_voc_flow_dec": [vp, vp, vp, vp, i, i, vp, vp, sz, vp],
        "gsv_voc_flow_dec_graph": [vp, vp, vp, vp, i, i, vp, vp, sz, vp],
        "gsv_voc_resample_linear": [vp, i, i, vp, i, vp],
        "gsv_voc_flow": [vp, vp, vp, vp, i, i, vp, vp, sz, vp],
        "gsv_voc_dec": [vp, vp, vp, i, i, vp, vp, sz, vp],
        "gsv_voc_has_enc_p": [vp],
        "gsv_voc_enc_p": [vp, vp, i, vp, i, vp, i, vp, vp, vp, vp, vp, sz, vp],
        "gsv_voc_decode": [vp, vp, i, vp, i, vp, i, vp, ctypes.c_float, ctypes.c_uint64, i, i, i, vp, i, i, vp, vp, vp, sz, vp],
        "gsv_voc_decode_segments": [vp, vp, i, vp, i, vp, i, vp, ctypes.POINTER(VocSegment), i, vp, vp, vp, sz, vp],
        "gsv_align_viterbi": [vp, i, i, i, vp, vp, sz, vp],
        "gsv_sola": [vp, vp, i, i, i, vp, vp, vp, sz, vp],
        "gsv_stream_emit": [vp, vp, i, i, i, i, i, i, vp, vp, vp, vp, sz, vp],
        "gsv_ref_create": [ctypes.POINTER(RefConfig), ctypes.POINTER(vp)],
        "gsv_ref_destroy": [vp],
        "gsv_ref_load_tensor": [vp, ctypes.c_char_p, vp, i64, vp],
        "gsv_ref_finalize": [vp, vp],
        "gsv_ref_spectrogram": [vp, vp, i, vp, vp, sz, vp],
        "gsv_ref_get_ge": [vp, vp, i, vp, vp, vp, sz, vp],
        "gsv_ref_extract_latent": [vp, vp, i, vp, vp, vp, sz, vp],
        "gsv_hubert_create": [ctypes.POINTER(HubertConfig), ctypes.POINTER(vp)],
        "gsv_hubert_destroy": [vp],
        "gsv_hubert_load_tensor": [vp, ctypes.c_char_p, vp, i64, vp],
        "gsv_hubert_finalize": [vp, vp],
        "gsv_hubert_frames": [vp, i],
        "gsv_hubert_forward": [vp, vp, i, vp, vp, sz, vp],
        "gsv_hubert_forward_batch": [vp, vp, ip, i, vp, vp, sz, vp],
        "gsv_sv_create": [ctypes.POINTER(SvConfig), ctypes.POINTER(vp)],
        "gsv_sv_destroy": [vp],
        "gsv_sv_load_tensor": [vp, ctypes.c_char_p, vp, i64, vp],
        "gsv_sv_finalize": [vp, vp],
        "gsv_sv_resample_length": [i, i, i],
        "gsv_sv_resample": [vp, i, i, i, vp, vp, sz, vp],
        "gsv_sv_frames": [vp, i, i],
        "gsv_sv_fbank": [vp, vp, i, vp, vp, sz, vp],
        "gsv_sv_forward": [vp, vp, i, vp, vp, sz, vp],
        "gsv_sv_embed": [vp, vp, i, i, vp, vp, sz, vp],
        "gsv_sv_forward_batch": [vp, vp, ip, i, vp, vp, sz, vp],
        "gsv_sv_embed_batch": [vp, vp, ip, i, i, vp, vp, sz, vp],
        "gsv_roberta_create": [ctypes.POINTER(RobertaConfig), ctypes.POINTER(vp)],
        "gsv_roberta_destroy": [vp],
        "gsv_roberta_load_tensor": [vp, ctypes.c_char_p, vp, i64, vp],
        "gsv_roberta_finalize": [vp, vp],
        "gsv_roberta_forward": [vp, vp, vp, i, i, i, vp, vp, sz, vp],
        "gsv_roberta_features": [vp, vp, vp, i, i, i, vp, i, vp, vp, sz, vp],
        "gsv_wav_to_mono": [vp, sz, i, i, i, vp, vp],
        "gsv_wav_to_mono_batch": [vp, sz, ctypes.POINTER(WavClip), i, vp, vp],
        "gsv_flac_decode": [vp, sz, ctypes.POINTER(FlacClip), i, ctypes.POINTER(FlacFrame), i, vp, vp, vp, sz, vp],
        "gsv_flac_decode_host": [vp, sz, ctypes.POINTER(FlacClip), i, ctypes.POINTER(FlacFrame), i, vp, vp],
        "gsv_flac_encode": [vp, sz, ctypes.POINTER(FlacEncClip), i, ctypes.POINTER(FlacEncFrame), i, vp, sz, vp, vp, vp, sz, vp],
        "gsv_flac_encode_host": [vp, sz, ctypes.POINTER(FlacEncClip), i, ctypes.POINTER(FlacEncFrame), i, vp, sz, vp, vp],
        "gsv_track_init": [vp, sz, i, i, i, i, vp],
        "gsv_track_push": [vp, vp, i, vp, i, vp, vp, vp],
        "gsv_track_init_host": [vp, sz, i, i, i, i],
        "gsv_track_push_host": [vp, vp, i, vp, i, vp, vp],
        "gsv_loudness": [vp, sz, ctypes.POINTER(LoudnessClip), i, i, ctypes.c_float, vp, vp, vp, sz, vp],
        "gsv_loudness_host": [vp, sz, ctypes.POINTER(LoudnessClip), i, i, ctypes.c_float, vp, vp, vp, sz],
        "gsv_level_init": [vp, sz, i] + [ctypes.c_double] * 5 + [ctypes.c_float, i, vp],
        "gsv_level_push": [vp, vp, i, vp, i, vp, vp, vp],
        "gsv_level_init_host": [vp, sz, i] + [ctypes.c_double] * 5 + [ctypes.c_float, i],
        "gsv_level_push_host": [vp, vp, i, vp, i, vp, vp],
        "gsv_limiter": [vp, sz, ctypes.POINTER(LimiterClip), i, i, i, vp, vp, vp, sz, vp],
        "gsv_limiter_host": [vp, sz, ctypes.POINTER(LimiterClip), i, i, i, vp, vp, vp, sz],
        "gsv_eq": [vp, sz, ctypes.POINTER(EqClip), i, ctypes.POINTER(EqDesign), i, vp, vp, vp, sz, vp],
        "gsv_eq_host": [vp, sz, ctypes.POINTER(EqClip), i, ctypes.POINTER(EqDesign), i, vp, vp, vp, sz],
        "gsv_limstream_init": [vp, sz, ctypes.c_float, i, i, vp],
        "gsv_limstream_push": [vp, vp, i, vp, i, vp, vp, vp],
        "gsv_limstream_init_host": [vp, sz, ctypes.c_float, i, i],
        "gsv_limstream_push_host": [vp, vp, i, vp, i, vp, vp],
        "gsv_eqstream_init": [vp, sz, ctypes.POINTER(EqDesign), vp],
        "gsv_eqstream_push": [vp, vp, i, vp, i, vp, vp, vp],
        "gsv_eqstream_init_host": [vp, sz, ctypes.POINTER(EqDesign)],
        "gsv_eqstream_push_host": [vp, vp, i, vp, i, vp, vp],
        "gsv_compressor": [vp, sz, ctypes.POINTER(CompressorClip), i, ctypes.POINTER(CompressorParams), i, vp, vp, vp, sz, vp],
        "gsv_compressor_host": [vp, sz, ctypes.POINTER(CompressorClip), i, ctypes.POINTER(CompressorParams), i, vp, vp, vp, sz],
        "gsv_compressor_math_host": [i, vp, vp, sz],
        "gsv_reverb": [vp, sz, ctypes.POINTER(ReverbClip), i, ctypes.POINTER(ReverbParams), i, vp, vp, vp, sz, vp],
        "gsv_reverb_host": [vp, sz, ctypes.POINTER(ReverbClip), i, ctypes.POINTER(ReverbParams), i, vp, vp, vp, sz],
        "gsv_cmpstream_init": [vp, sz, ctypes.POINTER(CompressorParams), vp],
        "gsv_cmpstream_push": [vp, vp, i, vp, i, vp, vp, vp],
        "gsv_cmpstream_init_host": [vp, sz, ctypes.POINTER(CompressorParams)],
        "gsv_cmpstream_push_host": [vp, vp, i, vp, i, vp, vp],
    }
    for name, args in sig.items():
        fn = getattr(L, name)
        fn.argtypes = args
        fn.restype = i
    L.gsv_t2s_prefill_workspace.argtypes = [vp, i, i]
    L.gsv_t2s_prefill_workspace.restype = sz
    L.gsv_t2s_device_bytes.argtypes = [vp]
    L.gsv_t2s_device_bytes.restype = sz
    L.gsv_voc_workspace.argtypes = [vp, i]
    L.gsv_voc_workspace.restype = sz
    L.gsv_voc_enc_workspace.argtypes = [vp, i, i]
    L.gsv_voc_enc_workspace.restype = sz
    L.gsv_voc_decode_workspace.argtypes = [vp, i, i, i, i, i]
    L.gsv_voc_decode_workspace.restype = sz
    L.gsv_voc_decode_segments_workspace.argtypes = [vp, i, i, i, ctypes.POINTER(VocSegment), i]
    L.gsv_voc_decode_segments_workspace.restype = sz
    L.gsv_ref_workspace.argtypes = [vp, i, i, i]
    L.gsv_ref_workspace.restype = sz
    L.gsv_hubert_workspace.argtypes = [vp, i]
    L.gsv_hubert_workspace.restype = sz
    L.gsv_sv_resample_workspace.argtypes = [i, i]
    L.gsv_sv_resample_workspace.restype = sz
    L.gsv_sv_workspace.argtypes = [vp, i, i]
    L.gsv_sv_workspace.restype = sz
    L.gsv_hubert_batch_workspace.argtypes = [vp, ip, i]
    L.gsv_hubert_batch_workspace.restype = sz
    L.gsv_sv_batch_workspace.argtypes = [vp, ip, i, i]
    L.gsv_sv_batch_workspace.restype = sz
    L.gsv_roberta_workspace.argtypes = [vp, i, i, i]
    L.gsv_roberta_workspace.restype = sz
    L.gsv_flac_decode_workspace.argtypes = [ctypes.POINTER(FlacClip), i, i]
    L.gsv_flac_decode_workspace.restype = sz
    for fn in (L.gsv_flac_encode_bound, L.gsv_flac_encode_workspace):
        fn.argtypes = [ctypes.POINTER(FlacEncClip), i, ctypes.POINTER(FlacEncFrame), i]
        fn.restype = sz
    L.gsv_track_state_bytes.argtypes = [i, i, i, i]
    L.gsv_track_state_bytes.restype = sz
    L.gsv_track_out_capacity.argtypes = [i, i, i, i, i]
    L.gsv_track_out_capacity.restype = sz
    L.gsv_loudness_work_bytes.argtypes = [ctypes.POINTER(LoudnessClip), i, i]
    L.gsv_loudness_work_bytes.restype = sz
    L.gsv_limiter_work_bytes.argtypes = [ctypes.POINTER(LimiterClip), i]
    L.gsv_limiter_work_bytes.restype = sz
    L.gsv_eq_work_bytes.argtypes = [ctypes.POINTER(EqClip), i, ctypes.POINTER(EqDesign), i]
    L.gsv_eq_work_bytes.restype = sz
    L.gsv_compressor_work_bytes.argtypes = [ctypes.POINTER(CompressorClip), i, ctypes.POINTER(CompressorParams), i]
    L.gsv_compressor_work_bytes.restype = sz
    L.gsv_reverb_work_bytes.argtypes = [ctypes.POINTER(ReverbClip), i, ctypes.POINTER(ReverbParams), i]
    L.gsv_reverb_work_bytes.restype = sz
    L.gsv_eqstream_state_bytes.argtypes = []
    L.gsv_eqstream_state_bytes.restype = sz
    L.gsv_cmpstream_state_bytes.argtypes = []
    L.gsv_cmpstream_state_bytes.restype = sz
    L.gsv_limstream_state_bytes.argtypes = [i, i]
    L.gsv_limstream_state_bytes.restype = sz
    L.gsv_limstream_out_capacity.argtypes = [i, i]
    L.gsv_limstream_out_capacity.restype = sz
    L.gsv_level_state_bytes.argtypes = [i, i]
    L.gsv_level_state_bytes.restype = sz
    L.gsv_align_workspace.argtypes = [i, i]
    L.gsv_align_workspace.restype = sz
    L.gsv_sola_workspace.argtypes = [i]
    L.gsv_sola_workspace.restype = sz
    L.gsv_stream_emit_workspace.argtypes = [i, i]
    L.gsv_stream_emit_workspace.restype = sz
    _LIB = L
    return L


def check(rc: int):
    if rc != 0:
        msg = lib().gsv_last_error()
        raise RuntimeError("gsv_tts_hip error %d: %s" % (rc, msg.decode("utf-8", "replace") if msg else "?"))


def dtype_code(torch_dtype) -> int:
    import torch
    if torch_dtype == torch.float32:
        return GSV_F32
    if torch_dtype == torch.bfloat16:
        return GSV_BF16
    if torch_dtype == torch.float8_e4m3fn:   # gsv_t2s only: bf16 + e4m3 QKV / FFN in the batched decode step
        return GSV_FP8
    raise ValueError("the MI355X hot path supports float32 (parity), bfloat16 (production) and float8_e4m3fn (GPT batched step); "
                     "got %s" % torch_dtype)


def current_stream_ptr(device=None) -> int:
    import torch
    return torch.cuda.current_stream(device).cuda_stream
