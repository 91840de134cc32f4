"""GPU tests of ambience= on the facade: TTS.infer, infer_vc and infer_batched return, for a reverb, the clip they return without it
through reverb.reverberate (AudioClip.ambient), bit for bit, with the record; a text of infer_batched with None comes back exactly as
without the parameter; with eq=, compress=, loudness= and true_peak= as well the order is EQ, compressor, reverb, gain, limiter --
the reference's -- and the clip carries all five records; a call without the keyword returns what it returned before and
issues no reverb call (counted at reverb.run_packed, which every call of the module goes through).

Setup: the toy front end and the synthetic 6-layer models exactly as tests/test_hip_tts_compressor.py sets them up (copied): fp32,
greedy, noise_scale=0."""
import asyncio
import math

import numpy as np
import pytest
import torch

from gsv_tts_lite_amd import reverb as RV
from gsv_tts_lite_amd import synth
from gsv_tts_lite_amd.compressor import Compressor
from gsv_tts_lite_amd.eq import EQ, Band
from gsv_tts_lite_amd.reverb import Reverb

pytestmark = pytest.mark.gpu

TWO_SEGMENTS = "willow violet. xenon tango yonder?"
THREE = [TWO_SEGMENTS, "pixel delta beta?", "yonder willow!"]
REF = ("spk.wav", "prompt.wav", "prompt text.")
VOICE = Reverb.preset("voice")
OTHER = Reverb(room_size=0.8, damping=0.2, wet_level=0.5, dry_level=0.3, width=0.5)
LOW = Compressor(-40.0, 3.5, 1.0, 100.0, 0.0)
AN_EQ = EQ([Band("lowshelf", 150.0, gain_db=4.0), Band("peak", 2500.0, q=3.0, gain_db=-6.0)])


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


def _check(clip, base, r):
    assert base.ambience is None
    want, rec = RV.reverberate(base.audio_data, base.samplerate, r)
    assert clip.audio_data.dtype == np.float32 and clip.audio_data.tobytes() == want.tobytes()
    assert clip.audio_data.tobytes() == base.ambient(r).audio_data.tobytes()
    assert clip.audio_data.tobytes() != base.audio_data.tobytes()              # the synthetic vocoder is not silent
    assert clip.subtitles == base.subtitles and clip.audio_len_s == base.audio_len_s and clip.orig_text == base.orig_text
    assert clip.ambience.reverbed and not clip.ambience.nonfinite
    assert clip.ambience.peak_out == np.abs(clip.audio_data).max() == rec.peak_out and clip.ambience.peak_in == np.abs(base.audio_data).max()
    assert clip.lufs is None and clip.dbtp is None and clip.eq is None and clip.comp is None


def _count_reverb_calls(monkeypatch):
    """every gsv_reverb / gsv_reverb_host call of the module goes through reverb.run_packed -> the list it is counted in"""
    calls, inner = [], RV.run_packed
    monkeypatch.setattr(RV, "run_packed", lambda x, o, lengths, index, *a, **k: (calls.append((len(lengths), list(index))),
                                                                                 inner(x, o, lengths, index, *a, **k))[1])
    return calls


def test_calls_without_the_keyword_issue_no_reverb_call(tts, monkeypatch):
    calls = _count_reverb_calls(monkeypatch)
    kw = dict(top_k=1, noise_scale=0.0)
    tts.infer(*REF, TWO_SEGMENTS, **kw)
    tts.infer(*REF, TWO_SEGMENTS, eq=AN_EQ, compress=LOW, loudness=-16.0, true_peak=-3.0, **kw)     # the other four keywords alone
    tts.infer(*REF, TWO_SEGMENTS, ambience=None, **kw)
    tts.infer(*REF, TWO_SEGMENTS, ambience=Reverb(wet_level=0.0, dry_level=0.5), **kw)              # the identity is as None
    tts.infer_vc(*REF, noise_scale=0.0)
    tts.infer_batched(*REF, THREE, cut_minlen=8, **kw)
    tts.infer_batched(*REF, THREE, ambience=[None, None, None], compress=LOW, cut_minlen=8, **kw)
    assert calls == []
    tts.infer(*REF, TWO_SEGMENTS, ambience="voice", **kw)
    assert calls == [(1, [0])]                                                  # with it: one call over the one clip
    tts.infer_batched(*REF, THREE, ambience=["voice", None, OTHER], cut_minlen=8, **kw)
    assert calls[1:] == [(2, [0, 1])]                                           # one packed call over the two texts that asked


def test_infer_with_a_reverb(tts):
    kw = dict(top_k=1, noise_scale=0.0, return_subtitles=True)
    base = tts.infer(*REF, TWO_SEGMENTS, **kw)
    again = tts.infer(*REF, TWO_SEGMENTS, **kw)                                 # without the keyword: the same bytes within the run
    assert again.audio_data.tobytes() == base.audio_data.tobytes() and again.ambience is None and again.subtitles == base.subtitles
    _check(tts.infer(*REF, TWO_SEGMENTS, ambience="voice", **kw), base, VOICE)
    _check(tts.infer(*REF, TWO_SEGMENTS, ambience=OTHER, **kw), base, OTHER)
    _check(asyncio.run(tts.infer_async(*REF, TWO_SEGMENTS, ambience=VOICE, **kw)), base, VOICE)
    same = tts.infer(*REF, TWO_SEGMENTS, ambience=Reverb(wet_level=0.0, dry_level=0.5), **kw)
    assert same.audio_data.tobytes() == base.audio_data.tobytes() and same.ambience is None   # the identity: today's branch
    for bad in ([VOICE], "radio", 0.5):
        with pytest.raises(ValueError):
            tts.infer(*REF, TWO_SEGMENTS, top_k=1, ambience=bad)


def test_infer_vc_with_a_reverb(tts):
    base = tts.infer_vc(*REF, noise_scale=0.0)
    _check(tts.infer_vc(*REF, noise_scale=0.0, ambience="voice"), base, VOICE)
    with pytest.raises(ValueError):
        tts.infer_vc(*REF, noise_scale=0.0, ambience="radio")


def test_infer_batched_with_a_reverb_per_text(tts):
    kw = dict(top_k=1, noise_scale=0.0, cut_minlen=8)
    base = tts.infer_batched(*REF, THREE, **kw)
    rs = ["voice", None, OTHER]
    got = tts.infer_batched(*REF, THREE, ambience=rs, **kw)
    assert len(got) == 3
    for clip, b, r in zip(got, base, rs):
        if r is None:
            assert clip.audio_data.tobytes() == b.audio_data.tobytes() and clip.ambience is None and clip.subtitles == b.subtitles
        else:
            _check(clip, b, r)
    base2 = tts.infer_batched(*REF, THREE[1:], **kw)
    one = asyncio.run(tts.infer_batched_async(*REF, THREE[1:], ambience="voice", **kw))     # one value for the call
    for clip, b in zip(one, base2):
        _check(clip, b, VOICE)
    with pytest.raises(ValueError):
        tts.infer_batched(*REF, THREE, ambience=[VOICE, None], **kw)                        # a wrong length
    with pytest.raises(ValueError):
        tts.infer_batched(*REF, THREE, ambience="radio", **kw)
    with pytest.raises(ValueError):
        tts.infer_batched(*REF, THREE, ambience=[VOICE, 3.0, None], **kw)


def test_all_five_keywords_in_the_references_order(tts):
    target, ceiling = -16.0, -3.0
    base = tts.infer(*REF, TWO_SEGMENTS, top_k=1, noise_scale=0.0)
    want = base.equalised(AN_EQ).compressed(LOW).ambient(OTHER).normalised(target, peak_limit=math.inf).limited_to(ceiling)
    clip = tts.infer(*REF, TWO_SEGMENTS, top_k=1, noise_scale=0.0, eq=AN_EQ, compress=LOW, ambience=OTHER, loudness=target, true_peak=ceiling)
    assert clip.audio_data.tobytes() == want.audio_data.tobytes()
    assert clip.eq.peak_out == want.eq.peak_out == clip.comp.peak_in and clip.comp.peak_out == want.comp.peak_out == clip.ambience.peak_in
    assert clip.ambience.reverbed and clip.ambience.peak_out == want.ambience.peak_out
    assert (clip.lufs, clip.gain, clip.dbtp, clip.limited) == (want.lufs, want.gain, want.dbtp, want.limited)
    assert math.isfinite(clip.lufs) and clip.dbtp <= ceiling + 1e-3
    other_order = base.ambient(OTHER).compressed(LOW)                           # the order matters, so the test can tell
    assert other_order.audio_data.tobytes() != base.compressed(LOW).ambient(OTHER).audio_data.tobytes()
    behind = tts.infer(*REF, TWO_SEGMENTS, top_k=1, noise_scale=0.0, eq=AN_EQ, compress=LOW, ambience="voice")      # behind eq= and compress=
    assert behind.audio_data.tobytes() == base.equalised(AN_EQ).compressed(LOW).ambient("voice").audio_data.tobytes()
    ahead = tts.infer(*REF, TWO_SEGMENTS, top_k=1, noise_scale=0.0, ambience="voice", loudness=target, true_peak=ceiling)  # ahead of the other two
    w = base.ambient("voice").normalised(target, peak_limit=math.inf).limited_to(ceiling)
    assert ahead.audio_data.tobytes() == w.audio_data.tobytes() and (ahead.lufs, ahead.dbtp) == (w.lufs, w.dbtp) and ahead.ambience.reverbed
    kw = dict(top_k=1, noise_scale=0.0, cut_minlen=8)
    base3 = tts.infer_batched(*REF, THREE, **kw)
    got = tts.infer_batched(*REF, THREE, eq=[AN_EQ, "voice", None], compress=[LOW, None, LOW], ambience=[OTHER, "voice", None],
                            loudness=[target, None, target], true_peak=[ceiling, ceiling, None], **kw)
    w0 = base3[0].equalised(AN_EQ).compressed(LOW).ambient(OTHER).normalised(target, peak_limit=math.inf).limited_to(ceiling)
    w1 = base3[1].equalised("voice").ambient("voice").limited_to(ceiling)
    w2 = base3[2].compressed(LOW).normalised(target)
    for clip, w in zip(got, (w0, w1, w2)):
        assert clip.audio_data.tobytes() == w.audio_data.tobytes()
        assert (clip.lufs, clip.gain, clip.dbtp) == (w.lufs, w.gain, w.dbtp)
        assert (clip.eq is None) == (w.eq is None) and (clip.comp is None) == (w.comp is None) and (clip.ambience is None) == (w.ambience is None)
    assert got[0].ambience.peak_out == w0.ambience.peak_out and got[2].ambience is None
