"""GPU tests of the track output of the streams: TTS.infer_stream(track=...) and TTS.infer_stream_batched(track=...) hand out, next to
the fp32 clips they hand out anyway, the s16 packets of a real-time track; all the packets of a text are AudioClip.to_pcm16 of all
its samples (one resampler state spans the text's segments and the mutes between them, the final clip flushes it), bit for bit
against the host twin on the CPU.

Setup: the toy front end and the synthetic 6-layer models exactly as tests/test_hip_stream_batched.py sets them up (copied): fp32,
greedy, noise_scale=0, stream_chunk=8, overlap_len=2, eos_gain 4."""
import asyncio

import numpy as np
import pytest
import torch

from gsv_tts_lite_amd import synth
from gsv_tts_lite_amd.track import TrackFormat, pcm16

pytestmark = pytest.mark.gpu

TWO_SEGMENTS = "willow violet. xenon tango yonder?"          # cut_minlen 8 cuts it behind the full stop
THREE = [TWO_SEGMENTS, "pixel delta beta?", "yonder willow!"]
KW = dict(top_k=1, noise_scale=0.0, stream_chunk=8, overlap_len=2, cut_minlen=8, debug=False)
REF = ("spk.wav", "prompt.wav", "prompt text.")
FMT = TrackFormat(rate=48000, channels=1, packet_ms=20)
STEREO_44K = TrackFormat(rate=44100, channels=2, packet_ms=10)


def _toy_frontend(text):
    ids = [1 + (ord(c) * 7) % 690 for c in text if not c.isspace()]
    return ids, {"word": list(text), "ph": [1] * len(text)}, None, text


@pytest.fixture(scope="module")
def tts():
    assert torch.cuda.is_available()
    from gsv_tts import TTS
    tts = TTS(gpt_cache=[(1, 160), (4, 160)], sovits_cache=[50, 55], device="cuda:0", dtype="float32")
    tts.load_gpt_model("synthetic://gpt?seed=1234&n_layer=6&eos_gain=4.0")
    tts.load_sovits_model("synthetic://sovits?version=v2Pro&seed=1234")
    tts.set_text_frontend(_toy_frontend)
    tts.cache_spk_audio("spk.wav", ge=torch.from_numpy(synth.synth_ge(0, 1024)))
    x, y, _, _ = synth.synth_request(0, 12, 0, 30)
    tts.cache_prompt_audio("prompt.wav", "prompt text.", prompt=torch.from_numpy(y)[None], phones1=x.tolist())
    return tts


@pytest.fixture(scope="module")
def solo(tts):
    """the yardstick, computed once: each text's clips through TTS.infer_stream without a track, left unchanged"""
    out = {t: list(tts.infer_stream(*REF, t, **KW)) for t in THREE}
    assert len(out[TWO_SEGMENTS]) >= 6 and all(len(c) >= 3 for c in out.values())
    return out


def _by_text(pairs, n):
    got = [[] for _ in range(n)]
    for t, clip in pairs:
        got[t].append(clip)
    return got


def _check_text(got, want, fmt):
    """the clips of one text: everything but the packets as without a track; the packets whole, and together the offline answer"""
    assert len(got) == len(want), (len(got), len(want))
    for g, w in zip(got, want):
        assert g.audio_data.dtype == np.float32 and np.array_equal(g.audio_data, w.audio_data)
        assert g.audio_len_s == w.audio_len_s and g.samplerate == w.samplerate and g.orig_text == w.orig_text
        assert g.subtitles == w.subtitles
        assert g.pcm_rate == fmt.rate and g.pcm.dtype == np.int16
        assert g.pcm.ndim == 2 and g.pcm.shape[1] == fmt.packet * fmt.channels                 # whole packets; there may be none
    audio = np.concatenate([g.audio_data for g in got])
    offline = pcm16(audio, got[0].samplerate, fmt, device="cpu")
    streamed = np.concatenate([g.pcm for g in got])
    assert streamed.shape == offline.shape and np.array_equal(streamed, offline)
    assert sum(g.pcm.shape[0] for g in got[:-1]) > 0                                           # packets leave before the text ends


def test_infer_stream_with_a_track(tts, solo):
    for fmt in (FMT, STEREO_44K):
        got = list(tts.infer_stream(*REF, TWO_SEGMENTS, track=fmt, **KW))
        _check_text(got, solo[TWO_SEGMENTS], fmt)


def test_infer_stream_batched_with_a_track(tts, solo):
    got = _by_text(tts.infer_stream_batched(*REF, THREE, track=FMT, **KW), len(THREE))
    for t, text in enumerate(THREE):
        _check_text(got[t], solo[text], FMT)
    # AudioClip.to_pcm16 of the whole text, wherever it runs, is the same answer
    whole = solo[THREE[1]]
    from gsv_tts_lite_amd.tts import AudioClip
    clip = AudioClip(None, np.concatenate([c.audio_data for c in whole]), whole[0].samplerate, whole[-1].audio_len_s, [], THREE[1])
    assert np.array_equal(clip.to_pcm16(), np.concatenate([g.pcm for g in got[1]]))


def test_the_async_wrapper_with_a_track(tts, solo):
    async def go():
        return [item async for item in tts.infer_stream_batched_async(*REF, THREE, track=STEREO_44K, **KW)]
    got = _by_text(asyncio.run(go()), len(THREE))
    for t, text in enumerate(THREE):
        _check_text(got[t], solo[text], STEREO_44K)


def test_without_a_track_the_clips_carry_none(tts, solo):
    assert all(c.pcm is None and c.pcm_rate is None for clips in solo.values() for c in clips)
    for _, clip in tts.infer_stream_batched(*REF, THREE[1:], **KW):
        assert clip.pcm is None and clip.pcm_rate is None
