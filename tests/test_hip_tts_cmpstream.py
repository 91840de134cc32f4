"""GPU tests of the compressor of the streams: TTS.infer_stream(compress=...) and TTS.infer_stream_batched(compress=...) hand out the
text's audio -- its segments and the mutes between them, one stream -- through the stream compressor: the
concatenated clips are compressor.compress (the host twin on the CPU) of the concatenated uncompressed clips, bit for bit, clip for
clip as many and as long.  With eq=, loudness= and true_peak= as well the order is eq -> compress -> level -> limit, as on the clip
path.

Setup: the toy front end and the synthetic 6-layer models exactly as tests/test_hip_tts_eqstream.py sets them up (copied): fp32,
greedy, noise_scale=0, stream_chunk=8, overlap_len=2, eos_gain 4.

The own compressor's threshold is set 12 dB under the peak of the plain audio of the text it runs over (whatever level the
synthetic vocoder gives), with 0 dB of makeup: it acts, and a sample that differs from the plain one differs by its gain."""
import math

import numpy as np
import pytest
import torch

from gsv_tts_lite_amd import compressor as cm
from gsv_tts_lite_amd import eq as eqm
from gsv_tts_lite_amd import level, limiter, synth
from gsv_tts_lite_amd.compressor import Compressor
from gsv_tts_lite_amd.eq import EQ, Band
from gsv_tts_lite_amd.track import TrackFormat, pcm16

pytestmark = pytest.mark.gpu

TWO_SEGMENTS = "willow violet. xenon tango yonder?"          # cut_minlen 8 cuts it behind the full stop
THREE = [TWO_SEGMENTS, "pixel delta beta?", "yonder willow!"]
KW = dict(top_k=1, noise_scale=0.0, stream_chunk=8, overlap_len=2, cut_minlen=8, debug=False)
REF = ("spk.wav", "prompt.wav", "prompt text.")
FMT = TrackFormat(rate=48000, channels=1, packet_ms=20)
OWN_EQ = EQ([Band("lowshelf", 200.0, gain_db=4.0), Band("peak", 2500.0, q=3.0, gain_db=-5.0), Band("lowpass", 9000.0)])


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
    """the yardstick, computed once: each text's clips through TTS.infer_stream without the keyword, left unchanged"""
    out = {t: list(tts.infer_stream(*REF, t, return_subtitles=True, **KW)) for t in THREE}
    assert len(out[TWO_SEGMENTS]) >= 6 and all(len(c) >= 3 for c in out.values())
    return out


def _whole(clips):
    return np.concatenate([c.audio_data for c in clips])


def _own(audio, ratio=4.0):
    """a compressor that acts on `audio`: the threshold 12 dB under its peak, 0 dB of makeup"""
    peak = float(np.abs(audio).max())
    assert peak > 1e-3
    return Compressor(max(-80.0, min(0.0, 20.0 * math.log10(peak) - 12.0)), ratio, 1.0, 100.0, 0.0)


def _by_text(pairs, n):
    got = [[] for _ in range(n)]
    for t, clip in pairs:
        got[t].append(clip)
    return got


def _check_text(got, want_clips, c, must_act):
    """the clips of one compressed text against the uncompressed ones and the offline answer"""
    rate = want_clips[0].samplerate
    plain = _whole(want_clips)
    want, rec = cm.compress(plain, rate, c, device="cpu")
    assert (want.tobytes() != plain.tobytes()) == rec.compressed
    if must_act:
        assert rec.compressed and rec.min_gain < 1
    assert len(got) == len(want_clips)
    audio = _whole(got)
    assert audio.dtype == np.float32 and audio.tobytes() == want.tobytes()
    seen = 0
    for g, w in zip(got, want_clips):
        assert len(g.audio_data) == len(w.audio_data) and g.audio_len_s == w.audio_len_s
        assert g.subtitles == w.subtitles and g.orig_text == w.orig_text
        seen += len(g.audio_data)
        assert isinstance(g.comp, cm.CmpStreamRecord) and g.comp.total == seen and g.comp.emitted == len(g.audio_data)
        assert g.comp.live and not g.comp.nonfinite_ever
        assert g.comp.peak_in == (np.abs(w.audio_data).max() if len(w.audio_data) else 0)
        assert g.comp.peak_out == (np.abs(g.audio_data).max() if len(g.audio_data) else 0)
    last = got[-1].comp
    assert last.peak_in_run == rec.peak_in and last.peak_out_run == rec.peak_out and last.min_gain_run == rec.min_gain
    return want


def test_infer_stream_through_the_voice_preset_and_an_own_compressor(tts, solo):
    text = TWO_SEGMENTS
    got = list(tts.infer_stream(*REF, text, return_subtitles=True, compress="voice", **KW))
    _check_text(got, solo[text], "voice", must_act=False)
    assert all(c.pcm is None and c.lufs is None and c.dbtp_in is None and c.eq is None for c in got)
    own = _own(_whole(solo[text]))
    got = list(tts.infer_stream(*REF, text, return_subtitles=True, compress=own, **KW))
    want = _check_text(got, solo[text], own, must_act=True)
    assert want.tobytes() != _whole(solo[text]).tobytes()
    # with a track: the packets are made from the compressed samples
    got = list(tts.infer_stream(*REF, text, return_subtitles=True, compress=own, track=FMT, **KW))
    want = _check_text(got, solo[text], own, must_act=True)
    assert np.array_equal(np.concatenate([g.pcm for g in got]), pcm16(want, got[0].samplerate, FMT, device="cpu"))
    assert not np.array_equal(np.concatenate([g.pcm for g in got]), pcm16(_whole(solo[text]), got[0].samplerate, FMT, device="cpu"))


def test_infer_stream_with_all_four_keywords(tts, solo):
    text = THREE[1]
    rate = solo[text][0].samplerate
    shaped, _ = eqm.equalise(_whole(solo[text]), rate, OWN_EQ, device="cpu")
    own = _own(shaped)
    squeezed, crec = cm.compress(shaped, rate, own, device="cpu")
    assert crec.compressed and squeezed.tobytes() != shaped.tobytes()
    target = -12.0
    levelled, _ = level.level(squeezed, rate, target, device="cpu", peak_limit=float("inf"))
    ceiling = min(0.0, limiter.true_peak(levelled, rate, device="cpu") - 6.0)
    want, rec = limiter.limit_stream(levelled, rate, ceiling, device="cpu")
    assert rec.limited_ever
    got = list(tts.infer_stream(*REF, text, eq=OWN_EQ, compress=own, loudness=target, true_peak=ceiling, track=FMT, **KW))
    assert len(got) == len(solo[text]) and _whole(got).tobytes() == want.tobytes()
    assert got[-1].limited and all(c.lufs is not None and c.dbtp_in is not None and c.eq is not None and c.comp is not None for c in got)
    assert got[-1].comp.total == len(shaped) and got[-1].comp.peak_in_run == np.abs(shaped).max()
    assert got[-1].comp.peak_out_run == crec.peak_out and got[-1].comp.min_gain_run == crec.min_gain
    assert np.array_equal(np.concatenate([g.pcm for g in got]), pcm16(want, rate, FMT, device="cpu"))
    # the equaliser, the compressor and the leveller alone: the leveller measures compressed audio
    got = list(tts.infer_stream(*REF, text, eq=OWN_EQ, compress=own, loudness=target, **KW))
    assert _whole(got).tobytes() == level.level(squeezed, rate, target, device="cpu")[0].tobytes()


def test_infer_stream_batched_with_a_compressor_per_text(tts, solo):
    per_text = [_own(_whole(solo[THREE[0]])), None, _own(_whole(solo[THREE[2]]), ratio=math.inf)]
    got = _by_text(tts.infer_stream_batched(*REF, THREE, return_subtitles=True, compress=per_text, **KW), len(THREE))
    plain = _by_text(tts.infer_stream_batched(*REF, THREE, return_subtitles=True, **KW), len(THREE))
    for t, text in enumerate(THREE):
        if per_text[t] is None:         # byte for byte the call without the keyword
            assert len(got[t]) == len(plain[t])
            for g, w in zip(got[t], plain[t]):
                assert g.audio_data.tobytes() == w.audio_data.tobytes() and g.audio_len_s == w.audio_len_s and g.subtitles == w.subtitles
                assert g.comp is None
            continue
        _check_text(got[t], solo[text], per_text[t], must_act=True)
        alone = list(tts.infer_stream(*REF, text, return_subtitles=True, compress=per_text[t], **KW))
        assert [c.audio_data.tobytes() for c in got[t]] == [c.audio_data.tobytes() for c in alone]
        key = lambda c: (c.comp.total, c.comp.peak_in_run, c.comp.peak_out_run, c.comp.min_gain_run, c.comp.min_gain)
        assert [key(c) for c in got[t]] == [key(c) for c in alone]
    with pytest.raises(ValueError, match="compress has 2 entries for 3 requests"):
        next(tts.infer_stream_batched(*REF, THREE, compress=["voice", None], **KW))
    # one value for every text, with the other stages and a track behind it
    rate = solo[THREE[2]][0].samplerate
    own = per_text[0]
    full = _by_text(tts.infer_stream_batched(*REF, THREE, eq=OWN_EQ, compress=own, loudness=-14.0, true_peak=-3.0, track=FMT, **KW), len(THREE))
    for t, text in enumerate(THREE):
        shaped, _ = eqm.equalise(_whole(solo[text]), rate, OWN_EQ, device="cpu")
        squeezed, _ = cm.compress(shaped, rate, own, device="cpu")
        levelled, _ = level.level(squeezed, rate, -14.0, device="cpu", peak_limit=float("inf"))
        want, _ = limiter.limit_stream(levelled, rate, -3.0, device="cpu")
        assert _whole(full[t]).tobytes() == want.tobytes(), t
        assert np.array_equal(np.concatenate([g.pcm for g in full[t]]), pcm16(want, rate, FMT, device="cpu"))
        assert full[t][-1].comp.total == len(shaped) and full[t][-1].eq.total == len(shaped)


def test_the_keyword_validates(tts):
    for bad in ([Compressor()], "radio", 3.0):
        with pytest.raises(ValueError, match="compress"):
            next(tts.infer_stream(*REF, "willow.", compress=bad, **KW))
    for bad in (["voice", "radio", None], "radio", ["voice", None, 3.0]):
        with pytest.raises(ValueError, match="compress"):
            next(tts.infer_stream_batched(*REF, THREE, compress=bad, **KW))


def test_no_keyword_and_an_identity_compressor_leave_the_stream_as_it_is(tts, solo):
    text = THREE[2]
    for same in (None, Compressor(ratio=1.0), Compressor(-40.0, 1.0, 5.0, 50.0, 0.0)):
        got = list(tts.infer_stream(*REF, text, return_subtitles=True, compress=same, **KW))
        assert len(got) == len(solo[text])
        for g, w in zip(got, solo[text]):
            assert g.audio_data.tobytes() == w.audio_data.tobytes() and g.comp is None and g.subtitles == w.subtitles
    got = _by_text(tts.infer_stream_batched(*REF, [text], compress=[Compressor(ratio=1.0)], **KW), 1)[0]
    assert _whole(got).tobytes() == _whole(solo[text]).tobytes() and all(c.comp is None for c in got)
