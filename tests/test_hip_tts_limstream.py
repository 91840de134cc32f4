"""GPU tests of the true-peak ceiling of the streams: TTS.infer_stream(true_peak=...) and TTS.infer_stream_batched(true_peak=...) hand
out the text's audio -- its segments and the mutes between them, one stream -- through the stream limiter: the
concatenated clips are limiter.limit_stream (the host twin on the CPU) of the concatenated unlimited clips, bit for bit, clip for
clip as many, the first D samples shorter and the last D longer.  The ceiling is set 6 dB under the measured true peak of the
unlimited stream, so the limiter has work; a run in which it never acts would prove nothing, and that is asserted.

Setup: the toy front end and the synthetic 6-layer models exactly as tests/test_hip_tts_track.py sets them up (copied): fp32,
greedy, noise_scale=0, stream_chunk=8, overlap_len=2, eos_gain 4."""
import numpy as np
import pytest
import torch

from gsv_tts_lite_amd import level, limiter, synth
from gsv_tts_lite_amd.track import TrackFormat, pcm16

pytestmark = pytest.mark.gpu

TWO_SEGMENTS = "willow violet. xenon tango yonder?"          # cut_minlen 8 cuts it behind the full stop
THREE = [TWO_SEGMENTS, "pixel delta beta?", "yonder willow!"]
KW = dict(top_k=1, noise_scale=0.0, stream_chunk=8, overlap_len=2, cut_minlen=8, debug=False)
REF = ("spk.wav", "prompt.wav", "prompt text.")
FMT = TrackFormat(rate=48000, channels=1, packet_ms=20)


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
    """the yardstick, computed once: each text's clips through TTS.infer_stream without a ceiling, left unchanged"""
    out = {t: list(tts.infer_stream(*REF, t, return_subtitles=True, **KW)) for t in THREE}
    assert len(out[TWO_SEGMENTS]) >= 6 and all(len(c) >= 3 for c in out.values())
    return out


def _whole(clips):
    return np.concatenate([c.audio_data for c in clips])


@pytest.fixture(scope="module")
def ceilings(solo):
    """per text: 6 dB under the true peak of its unlimited stream, never above 0"""
    res = {}
    for t, clips in solo.items():
        measured = limiter.true_peak(_whole(clips), clips[0].samplerate, device="cpu")
        assert np.isfinite(measured)
        res[t] = min(0.0, measured - 6.0)
    return res


def _by_text(pairs, n):
    got = [[] for _ in range(n)]
    for t, clip in pairs:
        got[t].append(clip)
    return got


def _check_text(got, want_clips, want_audio, ceiling):
    """the clips of one limited text against the unlimited ones and the offline answer"""
    rate = want_clips[0].samplerate
    D = limiter.times(rate)[0] + 5
    assert len(got) == len(want_clips)
    audio = _whole(got)
    assert audio.dtype == np.float32 and len(audio) == len(want_audio) == len(_whole(want_clips))
    assert audio.tobytes() == want_audio.tobytes()
    assert any(c.limited for c in got) and got[-1].limited
    emitted, seen = 0, 0
    for k, (g, w) in enumerate(zip(got, want_clips)):
        seen += len(w.audio_data)
        due = seen if k + 1 == len(got) else max(0, seen - D)
        assert len(g.audio_data) == due - emitted, (k, len(g.audio_data), due - emitted)
        emitted = due
        assert g.audio_len_s == pytest.approx(emitted / rate, abs=1e-9) and g.subtitles == w.subtitles and g.orig_text == w.orig_text
        assert g.dbtp is None and g.dbtp_in is not None and g.gain_min <= 1
    assert len(got[0].audio_data) == len(want_clips[0].audio_data) - D and len(got[-1].audio_data) == len(want_clips[-1].audio_data) + D
    peaks = [g.dbtp_in for g in got]
    assert peaks == sorted(peaks) and (ceiling == 0.0 or abs(peaks[-1] - (ceiling + 6.0)) < 1e-3)
    assert np.all(np.abs(audio) <= np.float32(10.0 ** (ceiling / 20.0)) * np.float32(1 + 2.0 ** -22))


def test_infer_stream_under_a_ceiling(tts, solo, ceilings):
    text = TWO_SEGMENTS
    ceiling = ceilings[text]
    want, rec = limiter.limit_stream(_whole(solo[text]), solo[text][0].samplerate, ceiling, device="cpu")
    assert rec.limited_ever
    got = list(tts.infer_stream(*REF, text, return_subtitles=True, true_peak=ceiling, **KW))
    _check_text(got, solo[text], want, ceiling)
    assert all(c.pcm is None and c.lufs is None for c in got)
    # with a track: the packets are made from the limited samples
    got = list(tts.infer_stream(*REF, text, return_subtitles=True, true_peak=ceiling, track=FMT, **KW))
    _check_text(got, solo[text], want, ceiling)
    streamed = np.concatenate([g.pcm for g in got])
    assert np.array_equal(streamed, pcm16(want, got[0].samplerate, FMT, device="cpu"))


def test_infer_stream_with_loudness_and_a_ceiling(tts, solo):
    text = THREE[1]
    rate = solo[text][0].samplerate
    plain = _whole(solo[text])
    target = -12.0
    levelled, _ = level.level(plain, rate, target, device="cpu", peak_limit=float("inf"))
    ceiling = min(0.0, limiter.true_peak(levelled, rate, device="cpu") - 6.0)
    want, rec = limiter.limit_stream(levelled, rate, ceiling, device="cpu")
    assert rec.limited_ever
    got = list(tts.infer_stream(*REF, text, loudness=target, true_peak=ceiling, **KW))
    assert len(got) == len(solo[text]) and _whole(got).tobytes() == want.tobytes()
    assert got[-1].limited and all(c.lufs is not None and c.gain is not None and c.dbtp_in is not None for c in got)


def test_infer_stream_batched_under_ceilings(tts, solo, ceilings):
    per_text = [ceilings[THREE[0]], None, ceilings[THREE[2]]]
    got = _by_text(tts.infer_stream_batched(*REF, THREE, return_subtitles=True, true_peak=per_text, track=FMT, **KW), len(THREE))
    for t, text in enumerate(THREE):
        rate = solo[text][0].samplerate
        if per_text[t] is None:         # the clips it gets today
            assert len(got[t]) == len(solo[text])
            for g, w in zip(got[t], solo[text]):
                assert np.array_equal(g.audio_data, w.audio_data) and g.audio_len_s == w.audio_len_s and g.subtitles == w.subtitles
                assert g.limited is None and g.dbtp_in is None and g.gain_min is None
            continue
        want, _ = limiter.limit_stream(_whole(solo[text]), rate, per_text[t], device="cpu")
        _check_text(got[t], solo[text], want, per_text[t])
        assert np.array_equal(np.concatenate([g.pcm for g in got[t]]), pcm16(want, rate, FMT, device="cpu"))
    # one value for every text, and what infer_stream gives for the same text
    one = _by_text(tts.infer_stream_batched(*REF, THREE[:1], return_subtitles=True, true_peak=per_text[0], **KW), 1)[0]
    alone = list(tts.infer_stream(*REF, THREE[0], return_subtitles=True, true_peak=per_text[0], **KW))
    assert [c.audio_data.tobytes() for c in one] == [c.audio_data.tobytes() for c in alone]
    assert [(c.limited, c.dbtp_in, c.gain_min) for c in one] == [(c.limited, c.dbtp_in, c.gain_min) for c in alone]


def test_the_keyword_validates(tts):
    for bad in (0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="ceiling"):
            next(tts.infer_stream(*REF, "willow.", true_peak=bad, **KW))
        with pytest.raises(ValueError, match="ceiling"):
            next(tts.infer_stream_batched(*REF, THREE, true_peak=[-1.0, bad, None], **KW))
    with pytest.raises(ValueError, match="true_peak has 2 entries for 3 requests"):
        next(tts.infer_stream_batched(*REF, THREE, true_peak=[-1.0, None], **KW))
