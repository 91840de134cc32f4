"""GPU tests of loudness= on the facade: TTS.infer, infer_vc and infer_batched return, for a target in LUFS, the clip they return
without it times ONE fp32 gain, bit for bit; the clip says what was measured (lufs, before the gain) and done (gain, limited), and
measuring it again reads the target.  A text of infer_batched with None comes back exactly as without the parameter.

Setup: the toy front end and the synthetic 6-layer models exactly as tests/test_hip_tts_track.py sets them up (copied): fp32, greedy,
noise_scale=0.  Tolerance: tests/test_loudness_cpu.py (the twin against the fp64 definition, plus the fp32 rounding of the gain and
of every product)."""
import asyncio
import math

import numpy as np
import pytest
import torch

from gsv_tts_lite_amd import synth

pytestmark = pytest.mark.gpu

TWO_SEGMENTS = "willow violet. xenon tango yonder?"
THREE = [TWO_SEGMENTS, "pixel delta beta?", "yonder willow!"]
REF = ("spk.wav", "prompt.wav", "prompt text.")
ROUND_TRIP_TOL = 4 * 1.35e-8 + 20 * math.log10(1 + 2.0 ** -23)       # tests/test_loudness_cpu.py: TOL + one ulp of the gain's effect


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


def _check(clip, base, target):
    assert base.lufs is None and base.gain is None
    assert clip.audio_data.dtype == np.float32 and clip.audio_data.shape == base.audio_data.shape
    assert isinstance(clip.gain, np.float32)
    assert clip.audio_data.tobytes() == np.float32(base.audio_data * clip.gain).tobytes()
    assert clip.subtitles == base.subtitles and clip.audio_len_s == base.audio_len_s and clip.orig_text == base.orig_text
    assert clip.lufs == base.loudness()
    print("base %.3f LUFS -> %.3f, gain %.4f, limited %r, %d samples" % (clip.lufs, clip.loudness(), clip.gain, clip.limited,
                                                                       len(clip.audio_data)))
    assert math.isfinite(clip.lufs) and clip.gain != 1                         # the synthetic vocoder is not silent
    if clip.limited:
        assert np.abs(clip.audio_data).max() <= 1.0 and clip.loudness() < target
    else:
        assert abs(clip.loudness() - target) <= ROUND_TRIP_TOL


def test_infer_with_a_loudness_target(tts):
    base = tts.infer(*REF, TWO_SEGMENTS, top_k=1, noise_scale=0.0, return_subtitles=True)
    for target in (-18.0, -40.0):
        clip = tts.infer(*REF, TWO_SEGMENTS, top_k=1, noise_scale=0.0, return_subtitles=True, loudness=target)
        _check(clip, base, target)
    again = base.normalised(-40.0)
    assert again.audio_data.tobytes() == clip.audio_data.tobytes() and again.lufs == clip.lufs and again.gain == clip.gain
    with pytest.raises(ValueError):
        tts.infer(*REF, TWO_SEGMENTS, top_k=1, loudness=float("nan"))


def test_infer_vc_with_a_loudness_target(tts):
    base = tts.infer_vc(*REF, noise_scale=0.0)
    clip = tts.infer_vc(*REF, noise_scale=0.0, loudness=-40.0)
    _check(clip, base, -40.0)


def test_infer_batched_with_a_target_per_text(tts):
    kw = dict(top_k=1, noise_scale=0.0, cut_minlen=8)
    base = tts.infer_batched(*REF, THREE, **kw)
    targets = [-16.0, None, -23.0]
    got = tts.infer_batched(*REF, THREE, loudness=targets, **kw)
    assert len(got) == 3
    for clip, b, t in zip(got, base, targets):
        if t is None:
            assert clip.audio_data.tobytes() == b.audio_data.tobytes() and clip.lufs is None and clip.gain is None
            assert clip.subtitles == b.subtitles
        else:
            _check(clip, b, t)
    # one value for the call; the async wrapper forwards the keyword
    base2 = tts.infer_batched(*REF, THREE[1:], **kw)
    one = asyncio.run(tts.infer_batched_async(*REF, THREE[1:], loudness=-40.0, **kw))
    for clip, b in zip(one, base2):
        _check(clip, b, -40.0)
    with pytest.raises(ValueError):
        tts.infer_batched(*REF, THREE, loudness=[-16.0, None], **kw)
