"""GPU tests of compress= on the facade: TTS.infer, infer_vc and infer_batched return, for a compressor, the clip they return without
it through AudioClip.compressed, bit for bit, with the record; a text of infer_batched with None comes back exactly as without the
parameter; with eq=, loudness= and true_peak= as well the order is EQ, compressor, gain, limiter -- the reference's -- and the clip
carries all four records.  The thresholds are low enough (-40 dB and below) that the synthetic vocoder's output is compressed.

Setup: the toy front end and the synthetic 6-layer models exactly as tests/test_hip_tts_eq.py sets them up (copied): fp32, greedy,
noise_scale=0."""
import asyncio
import math

import numpy as np
import pytest
import torch

from gsv_tts_lite_amd import synth
from gsv_tts_lite_amd.compressor import Compressor
from gsv_tts_lite_amd.eq import EQ, Band

pytestmark = pytest.mark.gpu

TWO_SEGMENTS = "willow violet. xenon tango yonder?"
THREE = [TWO_SEGMENTS, "pixel delta beta?", "yonder willow!"]
REF = ("spk.wav", "prompt.wav", "prompt text.")
LOW = Compressor(-40.0, 3.5, 1.0, 100.0, 0.0)               # "voice" with a threshold the synthetic vocoder passes
OTHER = Compressor(-50.0, math.inf, 0.1, 20.0, 6.0)
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


def _check(clip, base, c):
    assert base.comp is None
    want = base.compressed(c)
    assert clip.audio_data.dtype == np.float32 and clip.audio_data.tobytes() == want.audio_data.tobytes()
    assert clip.audio_data.tobytes() != base.audio_data.tobytes()              # the synthetic vocoder is not silent
    assert clip.subtitles == base.subtitles and clip.audio_len_s == base.audio_len_s and clip.orig_text == base.orig_text
    assert clip.comp.compressed and not clip.comp.nonfinite and clip.comp.min_gain == want.comp.min_gain < 1
    assert clip.comp.peak_out == np.abs(clip.audio_data).max() and clip.comp.peak_in == np.abs(base.audio_data).max()
    assert clip.lufs is None and clip.dbtp is None and clip.eq is None


def test_infer_with_a_compressor(tts):
    kw = dict(top_k=1, noise_scale=0.0, return_subtitles=True)
    base = tts.infer(*REF, TWO_SEGMENTS, **kw)
    _check(tts.infer(*REF, TWO_SEGMENTS, compress=LOW, **kw), base, LOW)
    _check(tts.infer(*REF, TWO_SEGMENTS, compress=OTHER, **kw), base, OTHER)
    _check(asyncio.run(tts.infer_async(*REF, TWO_SEGMENTS, compress=LOW, **kw)), base, LOW)
    voice = tts.infer(*REF, TWO_SEGMENTS, compress="voice", **kw)               # the preset by name: whatever it does, the same bytes
    assert voice.audio_data.tobytes() == base.compressed("voice").audio_data.tobytes() and voice.comp is not None
    same = tts.infer(*REF, TWO_SEGMENTS, compress=Compressor(ratio=1.0), **kw)
    assert same.audio_data.tobytes() == base.audio_data.tobytes() and same.comp is None    # the identity: today's branch
    for bad in ([LOW], "radio", -18.0):
        with pytest.raises(ValueError):
            tts.infer(*REF, TWO_SEGMENTS, top_k=1, compress=bad)


def test_infer_vc_with_a_compressor(tts):
    base = tts.infer_vc(*REF, noise_scale=0.0)
    _check(tts.infer_vc(*REF, noise_scale=0.0, compress=LOW), base, LOW)
    with pytest.raises(ValueError):
        tts.infer_vc(*REF, noise_scale=0.0, compress="radio")


def test_infer_batched_with_a_compressor_per_text(tts):
    kw = dict(top_k=1, noise_scale=0.0, cut_minlen=8)
    base = tts.infer_batched(*REF, THREE, **kw)
    cs = [LOW, None, OTHER]
    got = tts.infer_batched(*REF, THREE, compress=cs, **kw)
    assert len(got) == 3
    for clip, b, c in zip(got, base, cs):
        if c is None:
            assert clip.audio_data.tobytes() == b.audio_data.tobytes() and clip.comp is None and clip.subtitles == b.subtitles
        else:
            _check(clip, b, c)
    base2 = tts.infer_batched(*REF, THREE[1:], **kw)
    one = asyncio.run(tts.infer_batched_async(*REF, THREE[1:], compress=LOW, **kw))    # one value for the call
    for clip, b in zip(one, base2):
        _check(clip, b, LOW)
    with pytest.raises(ValueError):
        tts.infer_batched(*REF, THREE, compress=[LOW, None], **kw)                      # a wrong length
    with pytest.raises(ValueError):
        tts.infer_batched(*REF, THREE, compress="radio", **kw)
    with pytest.raises(ValueError):
        tts.infer_batched(*REF, THREE, compress=[LOW, 3.0, None], **kw)


def test_all_four_keywords_in_the_references_order(tts):
    target, ceiling = -16.0, -3.0
    base = tts.infer(*REF, TWO_SEGMENTS, top_k=1, noise_scale=0.0)
    want = base.equalised(AN_EQ).compressed(LOW).normalised(target, peak_limit=math.inf).limited_to(ceiling)
    clip = tts.infer(*REF, TWO_SEGMENTS, top_k=1, noise_scale=0.0, eq=AN_EQ, compress=LOW, loudness=target, true_peak=ceiling)
    assert clip.audio_data.tobytes() == want.audio_data.tobytes()
    assert clip.eq.peak_out == want.eq.peak_out == clip.comp.peak_in and clip.eq.sections == 2
    assert clip.comp.compressed and (clip.comp.peak_out, clip.comp.min_gain) == (want.comp.peak_out, want.comp.min_gain)
    assert (clip.lufs, clip.gain, clip.dbtp, clip.limited) == (want.lufs, want.gain, want.dbtp, want.limited)
    assert math.isfinite(clip.lufs) and clip.dbtp <= ceiling + 1e-3
    other_order = base.compressed(LOW).equalised(AN_EQ)                         # the order matters, so the test can tell
    assert other_order.audio_data.tobytes() != base.equalised(AN_EQ).compressed(LOW).audio_data.tobytes()
    kw = dict(top_k=1, noise_scale=0.0, cut_minlen=8)
    base3 = tts.infer_batched(*REF, THREE, **kw)
    got = tts.infer_batched(*REF, THREE, eq=[AN_EQ, "voice", None], compress=[LOW, None, OTHER], loudness=[target, None, target],
                            true_peak=[ceiling, ceiling, None], **kw)
    w0 = base3[0].equalised(AN_EQ).compressed(LOW).normalised(target, peak_limit=math.inf).limited_to(ceiling)
    w1 = base3[1].equalised("voice").limited_to(ceiling)
    w2 = base3[2].compressed(OTHER).normalised(target)
    for clip, w in zip(got, (w0, w1, w2)):
        assert clip.audio_data.tobytes() == w.audio_data.tobytes()
        assert (clip.lufs, clip.gain, clip.dbtp) == (w.lufs, w.gain, w.dbtp)
        assert (clip.eq is None) == (w.eq is None) and (clip.comp is None) == (w.comp is None)
    assert got[0].comp.min_gain == w0.comp.min_gain and got[1].comp is None and got[2].comp.peak_out == w2.comp.peak_out
