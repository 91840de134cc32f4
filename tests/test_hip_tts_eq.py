"""GPU tests of eq= on the facade: TTS.infer, infer_vc and infer_batched return, for an equaliser, the clip they return without it
through AudioClip.equalised, bit for bit, with the record of the peaks; a text of infer_batched with None comes back exactly as
without the parameter; with loudness= and true_peak= as well the order is EQ, gain, limiter and the clip carries all three records.

Setup: the toy front end and the synthetic 6-layer models exactly as tests/test_hip_tts_loudness.py sets them up (copied): fp32,
greedy, noise_scale=0."""
import asyncio
import math

import numpy as np
import pytest
import torch

from gsv_tts_lite_amd import synth
from gsv_tts_lite_amd.eq import EQ, Band

pytestmark = pytest.mark.gpu

TWO_SEGMENTS = "willow violet. xenon tango yonder?"
THREE = [TWO_SEGMENTS, "pixel delta beta?", "yonder willow!"]
REF = ("spk.wav", "prompt.wav", "prompt text.")
OTHER = EQ([Band("lowshelf", 150.0, gain_db=4.0), Band("peak", 2500.0, q=3.0, gain_db=-6.0), Band("lowpass", 12000.0)])


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


def _check(clip, base, e):
    assert base.eq is None
    want = base.equalised(e)
    assert clip.audio_data.dtype == np.float32 and clip.audio_data.tobytes() == want.audio_data.tobytes()
    assert clip.audio_data.tobytes() != base.audio_data.tobytes()              # the synthetic vocoder is not silent
    assert clip.subtitles == base.subtitles and clip.audio_len_s == base.audio_len_s and clip.orig_text == base.orig_text
    assert clip.eq.equalised and not clip.eq.nonfinite and clip.eq.sections == want.eq.sections > 0
    assert clip.eq.peak_out == np.abs(clip.audio_data).max() and clip.eq.peak_in == np.abs(base.audio_data).max()
    assert clip.lufs is None and clip.dbtp is None


def test_infer_with_an_equaliser(tts):
    base = tts.infer(*REF, TWO_SEGMENTS, top_k=1, noise_scale=0.0, return_subtitles=True)
    rate = tts.samplerate
    clip = tts.infer(*REF, TWO_SEGMENTS, top_k=1, noise_scale=0.0, return_subtitles=True, eq="voice")
    _check(clip, base, EQ.preset("voice", rate))
    _check(tts.infer(*REF, TWO_SEGMENTS, top_k=1, noise_scale=0.0, return_subtitles=True, eq=OTHER), base, OTHER)
    _check(asyncio.run(tts.infer_async(*REF, TWO_SEGMENTS, top_k=1, noise_scale=0.0, return_subtitles=True, eq="voice")), base, "voice")
    same = tts.infer(*REF, TWO_SEGMENTS, top_k=1, noise_scale=0.0, return_subtitles=True, eq=EQ([Band("peak", 300.0)]))
    assert same.audio_data.tobytes() == base.audio_data.tobytes() and same.eq is None      # the identity: today's branch
    for bad in ([Band("peak", 300.0, gain_db=2.0)], "radio", 3.0):
        with pytest.raises(ValueError):
            tts.infer(*REF, TWO_SEGMENTS, top_k=1, eq=bad)


def test_infer_vc_with_an_equaliser(tts):
    base = tts.infer_vc(*REF, noise_scale=0.0)
    _check(tts.infer_vc(*REF, noise_scale=0.0, eq="voice"), base, "voice")


def test_infer_batched_with_an_equaliser_per_text(tts):
    kw = dict(top_k=1, noise_scale=0.0, cut_minlen=8)
    base = tts.infer_batched(*REF, THREE, **kw)
    eqs = ["voice", None, OTHER]
    got = tts.infer_batched(*REF, THREE, eq=eqs, **kw)
    assert len(got) == 3
    for clip, b, e in zip(got, base, eqs):
        if e is None:
            assert clip.audio_data.tobytes() == b.audio_data.tobytes() and clip.eq is None and clip.subtitles == b.subtitles
        else:
            _check(clip, b, e)
    base2 = tts.infer_batched(*REF, THREE[1:], **kw)
    one = asyncio.run(tts.infer_batched_async(*REF, THREE[1:], eq="voice", **kw))      # one value for the call
    for clip, b in zip(one, base2):
        _check(clip, b, "voice")
    with pytest.raises(ValueError):
        tts.infer_batched(*REF, THREE, eq=["voice", None], **kw)                        # a wrong length
    with pytest.raises(ValueError):
        tts.infer_batched(*REF, THREE, eq=[Band("peak", 300.0, gain_db=2.0)] * 3, **kw)   # a bare list of bands
    with pytest.raises(ValueError):
        tts.infer_batched(*REF, THREE, eq="radio", **kw)


def test_all_three_keywords_in_the_references_order(tts):
    target, ceiling = -16.0, -3.0
    base = tts.infer(*REF, TWO_SEGMENTS, top_k=1, noise_scale=0.0)
    want = base.equalised(OTHER).normalised(target, peak_limit=math.inf).limited_to(ceiling)
    clip = tts.infer(*REF, TWO_SEGMENTS, top_k=1, noise_scale=0.0, eq=OTHER, loudness=target, true_peak=ceiling)
    assert clip.audio_data.tobytes() == want.audio_data.tobytes()
    assert clip.eq.peak_out == want.eq.peak_out and clip.eq.sections == 3
    assert (clip.lufs, clip.gain, clip.dbtp, clip.limited) == (want.lufs, want.gain, want.dbtp, want.limited)
    assert math.isfinite(clip.lufs) and clip.dbtp <= ceiling + 1e-3
    kw = dict(top_k=1, noise_scale=0.0, cut_minlen=8)
    base3 = tts.infer_batched(*REF, THREE, **kw)
    got = tts.infer_batched(*REF, THREE, eq=[OTHER, "voice", None], loudness=[target, None, target], true_peak=[ceiling, ceiling, None], **kw)
    w0 = base3[0].equalised(OTHER).normalised(target, peak_limit=math.inf).limited_to(ceiling)
    w1 = base3[1].equalised("voice").limited_to(ceiling)
    w2 = base3[2].normalised(target)
    for clip, w in zip(got, (w0, w1, w2)):
        assert clip.audio_data.tobytes() == w.audio_data.tobytes()
        assert (clip.lufs, clip.gain, clip.dbtp) == (w.lufs, w.gain, w.dbtp) and (clip.eq is None) == (w.eq is None)
    assert got[0].eq.peak_out == w0.eq.peak_out and got[2].eq is None
