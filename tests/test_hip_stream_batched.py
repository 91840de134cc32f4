"""GPU tests of TTS.infer_stream_batched: many texts streamed at once from the continuous-batching slots.  Per text the clips are
the ones TTS.infer_stream yields for that text alone -- the yardstick --, bit for bit for greedy fp32 requests that end with an EOS.

Setup: the toy front end and the synthetic 6-layer models of tests/test_hip_tts.py (copied), gpt_cache [(1, 160), (4, 160)],
top_k=1, noise_scale=0, stream_chunk=8, overlap_len=2.  One thing differs from that file: the GPT's eos_gain is 4.0, not 1.0.  With
1.0 the greedy model never samples an EOS inside a 160-row cache (measured over 40 texts), every request ends at the full cache,
and for such an end the streams are not claimed equal (a slot ends by `host_end`'s rule, a few tokens before `infer_stream`'s last
bucket is full).  With 4.0 the texts below end with an EOS after 26 .. 67 tokens: at least three chunks each, measured on the
solo runs and asserted from them."""
import asyncio

import numpy as np
import pytest
import torch

from gsv_tts_lite_amd import synth

pytestmark = pytest.mark.gpu

TWO_SEGMENTS = "willow violet. xenon tango yonder?"          # cut_minlen 8 cuts it behind the full stop
THREE = [TWO_SEGMENTS, "pixel delta beta?", "yonder willow!"]
SIX = THREE + ["tango xenon orbit?", "river orbit quartz?", "beta yonder?"]
KW = dict(top_k=1, noise_scale=0.0, stream_chunk=8, overlap_len=2, cut_minlen=8, debug=False)
REF = ("spk.wav", "prompt.wav", "prompt text.")


def _toy_frontend(text):
    ids = [1 + (ord(c) * 7) % 690 for c in text if not c.isspace()]
    return ids, {"word": list(text), "ph": [1] * len(text)}, None, text


def _word_frontend(text):
    """words = latin runs or single marks; one phoneme per character (the toy front end's ids); norm_text == text"""
    import re
    words = re.findall(r"[A-Za-z]+|[^\sA-Za-z]", text)
    ids = [1 + (ord(c) * 7) % 690 for w in words for c in w]
    return ids, {"word": words, "ph": [len(w) for w in words]}, None, text


def _make_tts(dtype):
    from gsv_tts import TTS
    tts = TTS(gpt_cache=[(1, 160), (4, 160)], sovits_cache=[50, 55], device="cuda:0", dtype=dtype)
    tts.load_gpt_model("synthetic://gpt?seed=1234&n_layer=6&eos_gain=4.0")
    tts.load_sovits_model("synthetic://sovits?version=v2Pro&seed=1234")
    tts.set_text_frontend(_toy_frontend)
    tts.cache_spk_audio("spk.wav", ge=torch.from_numpy(synth.synth_ge(0, 1024)))
    x, y, _, _ = synth.synth_request(0, 12, 0, 30)
    tts.cache_prompt_audio("prompt.wav", "prompt text.", prompt=torch.from_numpy(y)[None], phones1=x.tolist())
    return tts


@pytest.fixture(scope="module")
def tts():
    assert torch.cuda.is_available()
    return _make_tts("float32")


@pytest.fixture(scope="module")
def solo(tts):
    """the yardstick, computed once: each text's clips through TTS.infer_stream, left unchanged"""
    out = {}
    for t in SIX:
        out[t] = list(tts.infer_stream(*REF, t, **KW))
        n_seg = 2 if t == TWO_SEGMENTS else 1
        assert len(out[t]) >= 3 * n_seg, (t, len(out[t]))           # every segment streams at least three chunks
    return out


def _by_text(pairs, n):
    got = [[] for _ in range(n)]
    for t, clip in pairs:
        got[t].append(clip)
    return got


def _same(got, want, subtitles=False):
    assert len(got) == len(want), (len(got), len(want))
    for g, w in zip(got, want):
        assert g.audio_data.dtype == np.float32 and np.array_equal(g.audio_data, w.audio_data)
        assert g.audio_len_s == w.audio_len_s and g.samplerate == w.samplerate and g.orig_text == w.orig_text
        if subtitles:
            assert g.subtitles == w.subtitles
        else:
            assert g.subtitles == []


def test_three_texts_in_slots_equal_their_solo_streams(tts, solo):
    order = list(tts.infer_stream_batched(*REF, THREE, **KW))
    got = _by_text(order, len(THREE))
    for t, text in enumerate(THREE):
        _same(got[t], solo[text])
    # interleaving: all four requests sit in slots; before the final clip of text 0 every text has yielded a clip
    last0 = max(i for i, (t, _) in enumerate(order) if t == 0)
    assert {t for t, _ in order[:last0]} == {0, 1, 2}
    t2s = next(iter(tts.gpt_models.values())).t2s_model
    assert t2s.last_stats["slots"] == 4 and t2s.last_stats["refills"] == 0


def test_subtitles_equal_the_solo_streams(tts, monkeypatch):
    from gsv_tts_lite_amd import subtitles as sub
    tts.set_text_frontend(_word_frontend)
    try:
        want = [list(tts.infer_stream(*REF, t, return_subtitles=True, **KW)) for t in THREE]
        # in the batched loop the frame -> phoneme path reaches the host rules as pinned host memory (an asynchronous copy behind
        # the chunk's event), never as a device tensor whose read would wait for everything queued on the stream
        paths = []
        real = sub.get_subtitles
        monkeypatch.setattr(sub, "get_subtitles", lambda word2ph, assign, *a, **kw: (paths.append(assign), real(word2ph, assign, *a, **kw))[1])
        got = _by_text(tts.infer_stream_batched(*REF, THREE, return_subtitles=True, **KW), len(THREE))
        monkeypatch.undo()
    finally:
        tts.set_text_frontend(_toy_frontend)
    assert paths and all(not p.is_cuda and p.is_pinned() for p in paths)
    assert any(c.subtitles for w in want for c in w)
    for g, w in zip(got, want):
        _same(g, w, subtitles=True)


def test_six_texts_through_four_slots_equal_their_solo_streams(tts, solo):
    got = _by_text(tts.infer_stream_batched(*REF, SIX, **KW), len(SIX))
    for t, text in enumerate(SIX):
        _same(got[t], solo[text])
    t2s = next(iter(tts.gpt_models.values())).t2s_model
    assert t2s.last_stats["slots"] == 4 and t2s.last_stats["refills"] >= 3      # seven requests, four slots


def test_the_staged_loop_streams_the_same_clips(tts, solo, monkeypatch):
    """GSV_REFILL_AHEAD=0: a finished slot is parked and refilled in place (slot_loop.StagedLoop)"""
    t2s = next(iter(tts.gpt_models.values())).t2s_model
    monkeypatch.setattr(t2s, "refill_ahead", 0)
    got = _by_text(tts.infer_stream_batched(*REF, SIX, **KW), len(SIX))
    for t, text in enumerate(SIX):
        _same(got[t], solo[text])
    assert t2s.last_stats["refills"] >= 3 and "passes" not in t2s.last_stats


def test_a_seeded_text_does_not_depend_on_its_neighbours(tts):
    kw = dict(KW, noise_scale=0.5, seed=[11, 12, 13])
    one = _by_text(tts.infer_stream_batched(*REF, THREE, slots=1, **kw), len(THREE))
    four = _by_text(tts.infer_stream_batched(*REF, THREE, slots=4, **kw), len(THREE))
    for a, b in zip(one, four):
        assert len(a) == len(b) >= 3
        for x, y in zip(a, b):
            assert np.array_equal(x.audio_data, y.audio_data) and x.audio_len_s == y.audio_len_s
    silent = _by_text(tts.infer_stream_batched(*REF, THREE, slots=4, **KW), len(THREE))
    assert not np.array_equal(silent[1][0].audio_data, four[1][0].audio_data)          # the noise is there


def test_bf16_streams_run_and_cover_the_solo_length():
    tts = _make_tts("bfloat16")
    got = _by_text(tts.infer_stream_batched(*REF, THREE, **KW), len(THREE))
    for t, text in enumerate(THREE):
        want = list(tts.infer_stream(*REF, text, **KW))
        assert len(got[t]) >= 2
        assert all(np.isfinite(c.audio_data).all() for c in got[t])
        n_got, n_want = sum(len(c.audio_data) for c in got[t]), sum(len(c.audio_data) for c in want)
        print("bf16 text %d: %d clips, %d samples; solo %d clips, %d samples" % (t, len(got[t]), n_got, len(want), n_want))
        assert abs(n_got - n_want) <= 320 * len(got[t]) + 640, (t, n_got, n_want, len(got[t]))


def test_an_abandoned_stream_leaves_the_engine_usable(tts):
    text = THREE[1]
    want = tts.infer(*REF, text, top_k=1, noise_scale=0.0)
    gen = tts.infer_stream_batched(*REF, THREE, **KW)
    t, clip = next(gen)
    assert 0 <= t < 3 and len(clip.audio_data) > 0
    with pytest.raises(RuntimeError):           # the same thread calling back in between two clips
        tts.infer(*REF, text, top_k=1, noise_scale=0.0)
    gen.close()
    vq = next(iter(tts.sovits_models.values())).vq_model
    assert vq.enc_p.y_overlap is None
    again = tts.infer(*REF, text, top_k=1, noise_scale=0.0)      # its usual audio: the tolerance of tests/test_hip_tts.py for two runs
    assert again.audio_data.shape == want.audio_data.shape
    np.testing.assert_allclose(again.audio_data, want.audio_data, atol=1e-5)


def test_the_async_wrapper_yields_the_same_clips(tts, solo):
    async def go():
        return [item async for item in tts.infer_stream_batched_async(*REF, THREE, **KW)]
    got = _by_text(asyncio.run(go()), len(THREE))
    for t, text in enumerate(THREE):
        _same(got[t], solo[text])


def test_arguments(tts):
    assert list(tts.infer_stream_batched(*REF, [], **KW)) == []                         # no texts: an empty stream
    with pytest.raises(ValueError):
        list(tts.infer_stream_batched(*REF, THREE, **dict(KW, top_k=[1, 1])))           # one value per text, or one
    with pytest.raises(ValueError):
        list(tts.infer_stream_batched(*REF, THREE, slots=3, **KW))                      # no such slot family
    assert len(tts.infer(*REF, THREE[2], top_k=1, noise_scale=0.0).audio_data) > 0      # the lock was released both times
