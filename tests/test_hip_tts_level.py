"""GPU tests of loudness= on the streams: TTS.infer_stream(loudness=...) and TTS.infer_stream_batched(loudness=...) hand out the
clips they hand out anyway with a running BS.1770 gain applied on the device (level.StreamLeveller): all the audio of
a text is level.level() of all its unlevelled audio (one leveller spans the text's segments and the mutes between them, the final
clip flushes it), bit for bit against the host twin on the CPU; a track carries the levelled audio; a text without a value gets
the clips it gets today.

Setup: the toy front end and the synthetic 6-layer models exactly as tests/test_hip_tts_track.py sets them up (copied): fp32,
greedy, noise_scale=0, stream_chunk=8, overlap_len=2, eos_gain 4."""
import asyncio

import numpy as np
import pytest
import torch

from gsv_tts_lite_amd import level as lv
from gsv_tts_lite_amd import synth
from gsv_tts_lite_amd.level import StreamLeveller
from gsv_tts_lite_amd.track import TrackFormat, pcm16

pytestmark = pytest.mark.gpu

TWO_SEGMENTS = "willow violet. xenon tango yonder?"          # cut_minlen 8 cuts it behind the full stop
THREE = [TWO_SEGMENTS, "pixel delta beta?", "yonder willow!"]
KW = dict(top_k=1, noise_scale=0.0, stream_chunk=8, overlap_len=2, cut_minlen=8, debug=False)
REF = ("spk.wav", "prompt.wav", "prompt text.")
FMT = TrackFormat(rate=48000, channels=1, packet_ms=20)
TARGETS = [-18.0, None, -23.0]
SEEDS = [float("-inf"), -40.0, -30.0]          # -inf: the lufs of a clip without a measurement, no seed


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
    """the yardstick, computed once: each text's clips through TTS.infer_stream without loudness=, left unchanged"""
    out = {t: list(tts.infer_stream(*REF, t, **KW)) for t in THREE}
    assert len(out[TWO_SEGMENTS]) >= 6 and all(len(c) >= 3 for c in out.values())
    return out


def _by_text(pairs, n):
    got = [[] for _ in range(n)]
    for t, clip in pairs:
        got[t].append(clip)
    return got


def _check_text(got, want, target, seed, fmt=None):
    """the clips of one text against the unlevelled clips `want` levelled on the CPU twin, clip by clip as one stream"""
    assert len(got) == len(want), (len(got), len(want))
    # first: the gain moves over this text, or every comparison below would be one of copies
    whole, rec = lv.level(np.concatenate([w.audio_data for w in want]), want[0].samplerate, target, device="cpu", seed=seed)
    probe = StreamLeveller(target, want[0].samplerate, "cpu", seed=seed)
    probe.push(np.concatenate([w.audio_data for w in want]))
    A = probe.knot_gains()
    print("knot gains %s; final lufs %.3f" % (np.array2string(A, precision=3), rec.lufs))
    assert int((A != A[0]).sum()) >= 3, "the gain never moved"
    twin = StreamLeveller(target, want[0].samplerate, "cpu", seed=seed)
    levelled = []
    for i, (g, w) in enumerate(zip(got, want)):
        out = twin.push(w.audio_data, flush=i == len(want) - 1)
        levelled.append(out)
        assert g.audio_data.dtype == np.float32 and g.audio_data.shape == w.audio_data.shape
        assert np.array_equal(g.audio_data.view(np.uint32), out.view(np.uint32)), i
        assert g.audio_len_s == w.audio_len_s and g.samplerate == w.samplerate and g.orig_text == w.orig_text
        assert g.subtitles == w.subtitles
        assert g.lufs == twin.rec.lufs and g.gain == twin.rec.gain_last and g.limited == twin.rec.limited, i
    # the whole text in one push is the same stream
    assert np.array_equal(whole.view(np.uint32), np.concatenate(levelled).view(np.uint32)) and rec.zbar == twin.rec.zbar
    if fmt is not None:
        offline = pcm16(whole, want[0].samplerate, fmt, device="cpu")
        streamed = np.concatenate([g.pcm for g in got])
        assert all(g.pcm_rate == fmt.rate for g in got)
        assert streamed.shape == offline.shape and np.array_equal(streamed, offline)


def _check_plain(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert np.array_equal(g.audio_data.view(np.uint32), w.audio_data.view(np.uint32)) and g.audio_len_s == w.audio_len_s
        assert g.subtitles == w.subtitles and g.lufs is None and g.gain is None and g.limited is None and g.pcm is None


@pytest.mark.parametrize("target,seed", [(-18.0, None), (-23.0, -30.0)])
def test_infer_stream_with_loudness(tts, solo, target, seed):
    got = list(tts.infer_stream(*REF, TWO_SEGMENTS, loudness=target, loudness_seed=seed, **KW))
    _check_text(got, solo[TWO_SEGMENTS], target, seed)
    assert all(g.pcm is None for g in got)


def test_infer_stream_with_loudness_and_a_track(tts, solo):
    got = list(tts.infer_stream(*REF, TWO_SEGMENTS, loudness=-18.0, track=FMT, **KW))
    _check_text(got, solo[TWO_SEGMENTS], -18.0, None, FMT)


def test_infer_stream_batched_with_loudness_per_text(tts, solo):
    got = _by_text(tts.infer_stream_batched(*REF, THREE, loudness=TARGETS, loudness_seed=SEEDS, **KW), len(THREE))
    _check_text(got[0], solo[THREE[0]], -18.0, None)
    _check_plain(got[1], solo[THREE[1]])                    # None: today's clips, whatever its seed says
    _check_text(got[2], solo[THREE[2]], -23.0, -30.0)
    # one value for every text, with a track
    got = _by_text(tts.infer_stream_batched(*REF, THREE, loudness=-18.0, loudness_seed=-30.0, track=FMT, **KW), len(THREE))
    for t, text in enumerate(THREE):
        _check_text(got[t], solo[text], -18.0, -30.0, FMT)


def test_the_async_wrapper_with_loudness(tts, solo):
    async def go():
        return [item async for item in tts.infer_stream_batched_async(*REF, THREE, loudness=TARGETS, loudness_seed=SEEDS, **KW)]
    got = _by_text(asyncio.run(go()), len(THREE))
    _check_text(got[0], solo[THREE[0]], -18.0, None)
    _check_plain(got[1], solo[THREE[1]])
    _check_text(got[2], solo[THREE[2]], -23.0, -30.0)


def test_without_loudness_the_existing_bits(tts, solo):
    _check_plain(list(tts.infer_stream(*REF, THREE[1], loudness=None, **KW)), solo[THREE[1]])
    got = _by_text(tts.infer_stream_batched(*REF, THREE, loudness=None, loudness_seed=-30.0, **KW), len(THREE))
    for t, text in enumerate(THREE):
        _check_plain(got[t], solo[text])
    got = _by_text(tts.infer_stream_batched(*REF, THREE, loudness=[None] * 3, **KW), len(THREE))
    for t, text in enumerate(THREE):
        _check_plain(got[t], solo[text])


def test_loudness_is_validated(tts):
    with pytest.raises(ValueError):
        list(tts.infer_stream(*REF, THREE[1], loudness=float("nan"), **KW))
    with pytest.raises(ValueError):
        list(tts.infer_stream(*REF, THREE[1], loudness=-18.0, loudness_seed=float("inf"), **KW))
    with pytest.raises(ValueError):
        list(tts.infer_stream_batched(*REF, THREE, loudness=-18.0, loudness_seed=[-30.0, float("nan"), None], **KW))
    with pytest.raises(ValueError):
        list(tts.infer_stream_batched(*REF, THREE, loudness=[-18.0, None], **KW))
