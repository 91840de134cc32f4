"""GPU checks of WAV files as reference audio: the sample conversion (gsv_wav_to_mono / gsv_wav_to_mono_batch behind
wavio.load_wav / load_wavs) bit for bit against numpy on the integers the test wrote, and the facade reading WAV paths
(cache_spk_audio, cache_prompt_audio, verify_speaker, infer and the list forms) equal to the same calls on the
waveforms those files hold."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wav_writer as ww  # noqa: E402

from gsv_tts_lite_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu
SEED = 1234
PRO = "synthetic://sovits?version=v2Pro&seed=%d" % SEED
V2 = "synthetic://sovits?version=v2&seed=%d" % SEED


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------------------ kernel
@pytest.mark.parametrize("fmt", ww.FORMATS)
@pytest.mark.parametrize("ch", [1, 2])
def test_conversion_is_bit_exact(dev, tmp_path, fmt, ch):
    from gsv_tts_lite_amd.wavio import load_wav
    for n in (1, 255, 256, 257, 10 * 48000):
        x = ww.samples(fmt, n, ch, seed=n)
        got, sr = load_wav(ww.write(tmp_path / ("%d.wav" % n), x, fmt, 48000), dev)
        assert sr == 48000 and got.dtype == torch.float32 and got.device == dev and got.shape == (n,)
        assert torch.equal(got.cpu(), torch.from_numpy(ww.expected(x, fmt))), (fmt, ch, n)


def test_extensible_and_streamed_files_convert_alike(dev, tmp_path):
    from gsv_tts_lite_amd.wavio import load_wav
    x = ww.samples("s24", 1001, 2)
    want = torch.from_numpy(ww.expected(x, "s24"))
    for i, kw in enumerate(({}, {"extensible": True}, {"data_size": 0xFFFFFFFF}, {"before_data": (ww.chunk(b"LIST", b"abc"),)})):
        got, _ = load_wav(ww.write(tmp_path / ("%d.wav" % i), x, "s24", 44100, **kw), dev)
        assert torch.equal(got.cpu(), want), kw


def test_batch_equals_single(dev, tmp_path):
    from gsv_tts_lite_amd import _native as N
    from gsv_tts_lite_amd.wavio import load_wav, load_wavs
    specs = [("u8", 1, 8000, 3), ("s16", 2, 44100, 30000), ("s24", 1, 22050, 257), ("s32", 2, 48000, 1),
             ("f32", 1, 16000, 16000), ("f64", 2, 32000, 4097), ("s16", 1, 24000, 255), ("s24", 2, 96000, 12345)]
    paths = []
    for i, (fmt, ch, rate, n) in enumerate(specs):
        paths.append(ww.write(tmp_path / ("c%d.wav" % i), ww.samples(fmt, n, ch, seed=i), fmt, rate))
    single = [load_wav(p, dev) for p in paths]
    for order in (list(range(len(paths))), [5, 2, 7, 0, 3, 6, 1, 4]):
        got = load_wavs([paths[i] for i in order], dev)
        for j, i in enumerate(order):
            assert got[j][1] == single[i][1] == specs[i][2]
            assert torch.equal(got[j][0], single[i][0]), (order, i)
    # past the per-launch cap: the clips go in chunks of AUX_MAX_CLIPS
    many = [paths[i % len(paths)] for i in range(N.AUX_MAX_CLIPS + 5)]
    for k, (w, sr) in enumerate(load_wavs(many, dev)):
        assert torch.equal(w, single[k % len(paths)][0]), k


def test_abi_refuses_bad_clips(dev):
    from gsv_tts_lite_amd import _native as N
    L = N.lib()
    pcm = torch.zeros(16, dtype=torch.uint8, device=dev)
    out = torch.zeros(16, dtype=torch.float32, device=dev)
    st = N.current_stream_ptr(dev)
    assert L.gsv_wav_to_mono(pcm.data_ptr(), 16, 5, N.PCM_S16, 2, out.data_ptr(), st) == 1      # 20 bytes > 16
    assert b"past" in L.gsv_last_error()
    assert L.gsv_wav_to_mono(pcm.data_ptr(), 16, 2, N.PCM_S16, 3, out.data_ptr(), st) == 1
    assert L.gsv_wav_to_mono(pcm.data_ptr(), 16, 2, 6, 1, out.data_ptr(), st) == 1
    assert L.gsv_wav_to_mono(pcm.data_ptr(), 16, 0, N.PCM_S16, 1, out.data_ptr(), st) == 1
    clips = (N.WavClip * 2)(N.WavClip(0, 4, N.PCM_S16, 1), N.WavClip(10, 2, N.PCM_F32, 1))    # clip 1: bytes 10..18
    assert L.gsv_wav_to_mono_batch(pcm.data_ptr(), 16, clips, 2, out.data_ptr(), st) == 1
    assert b"clip 1" in L.gsv_last_error()
    many = (N.WavClip * (N.AUX_MAX_CLIPS + 1))(*[N.WavClip(0, 1, N.PCM_U8, 1)] * (N.AUX_MAX_CLIPS + 1))
    assert L.gsv_wav_to_mono_batch(pcm.data_ptr(), 16, many, N.AUX_MAX_CLIPS + 1, out.data_ptr(), st) == 1
    assert L.gsv_wav_to_mono_batch(pcm.data_ptr(), 16, clips, 1, out.data_ptr(), st) == 0
    torch.cuda.synchronize(dev)
    assert torch.equal(out.cpu(), torch.zeros(16))


# ------------------------------------------------------------------------------------------------------------ facade
def _toy_frontend(text):
    ids = [1 + (ord(c) * 7) % 690 for c in text if not c.isspace()]
    return ids, {"word": list(text), "ph": [1] * len(text)}, None, text


def _models_dir(path):
    synth.write_hubert_dir(str(path / "chinese-hubert-base"), seed=SEED)
    synth.write_sv_ckpt(str(path / "sv" / "pretrained_eres2netv2w24s4ep4.ckpt"), seed=SEED)
    return str(path)


@pytest.fixture(scope="module")
def tts(dev, tmp_path_factory):
    from gsv_tts import TTS
    t = TTS(gpt_cache=[(1, 128)], sovits_cache=[50, 55], models_dir=_models_dir(tmp_path_factory.mktemp("models")),
            device=str(dev), dtype="bfloat16", always_load_cnhubert=True, always_load_sv=True)
    t.load_sovits_model(PRO, V2)
    t.set_text_frontend(_toy_frontend)
    return t


def _clip(fmt, ch, rate, seconds, i, gain=1.0):
    """a speech-like [n, ch] of format fmt (synth_audio's partials), and its fp32 mono as the device must read it"""
    n = int(rate * seconds)
    w = np.stack([synth.synth_audio(i + c, n) for c in range(ch)], axis=1).astype(np.float64) * gain
    if fmt in ("f32", "f64"):
        x = w.astype(np.float32 if fmt == "f32" else np.float64)
    else:
        bits = {"u8": 8, "s16": 16, "s24": 24, "s32": 32}[fmt]
        x = np.clip(np.round(w * 2.0 ** (bits - 1)), -2.0 ** (bits - 1), 2.0 ** (bits - 1) - 1).astype(np.int64)
        if fmt == "u8":
            x = x + 128
    return x, ww.expected(x, fmt)


# (format, channels, gain): the float files peak above 1, so the peak rule runs after the resample
SPK_FILES = {16000: ("s16", 1, 1.0), 22050: ("f32", 1, 4.0), 32000: ("s24", 1, 1.0), 44100: ("s16", 2, 1.0),
             48000: ("f64", 2, 3.0)}


@pytest.mark.parametrize("model", [PRO, V2])
@pytest.mark.parametrize("rate", sorted(SPK_FILES))
def test_cache_spk_audio_reads_the_file(tts, tmp_path, model, rate):
    fmt, ch, gain = SPK_FILES[rate]
    x, mono = _clip(fmt, ch, rate, 2.0, rate % 97, gain)
    path = ww.write(tmp_path / "spk.wav", x, fmt, rate)
    key = "arr-%d-%s" % (rate, model[-20:])
    tts.cache_spk_audio(path, sovits_model=model)
    tts.cache_spk_audio(key, sovits_model=model, audio=torch.from_numpy(mono), sample_rate=rate)
    a, b = tts.spk_audio_cache[path], tts.spk_audio_cache[key]
    assert torch.equal(a["ge"][model], b["ge"][model])
    if model == PRO:
        assert a["sv_emb"].shape == (1, 20480) and torch.equal(a["sv_emb"], b["sv_emb"])
    else:
        assert "sv_emb" not in a and "sv_emb" not in b
    if rate == 32000:       # at the model rate sample_rate changes nothing
        tts.cache_spk_audio(key + "-none", sovits_model=model, audio=torch.from_numpy(mono))
        assert torch.equal(tts.spk_audio_cache[key + "-none"]["ge"][model], a["ge"][model])


@pytest.mark.parametrize("rate", [16000, 44100])
def test_cache_prompt_audio_reads_the_file(tts, tmp_path, rate):
    text = "prompt text."
    x, mono = _clip("s16", 1 if rate == 16000 else 2, rate, 1.5, 7)
    path = ww.write(tmp_path / "p.wav", x, "s16", rate)
    tts.cache_prompt_audio(path, text, sovits_model=PRO)
    key = "parr-%d" % rate
    tts.cache_prompt_audio(key, text, audio=torch.from_numpy(mono), sample_rate=rate, phones1=_toy_frontend(text)[0],
                           sovits_model=PRO)
    a, b = tts.prompt_audio_cache[path], tts.prompt_audio_cache[key]
    assert a["prompt"].dtype == torch.int64 and a["prompt"].shape[0] == 1 and a["prompt"].shape[1] > 10
    assert torch.equal(a["prompt"], b["prompt"])
    assert a["phones1"] == b["phones1"] == _toy_frontend(text)[0] and a["text"] == text
    assert torch.equal(a["bert1"], b["bert1"])


def test_verify_speaker_reads_files(tts, tmp_path, dev):
    from gsv_tts_lite_amd.sv import resample
    xa, ma = _clip("s16", 1, 32000, 2.0, 21)
    xb, mb = _clip("s16", 2, 48000, 2.0, 23)
    pa, pb = ww.write(tmp_path / "a.wav", xa, "s16", 32000), ww.write(tmp_path / "b.wav", xb, "s16", 48000)
    s = tts.verify_speaker(pa, pb)
    want = tts.verify_speaker(torch.from_numpy(ma), resample(torch.from_numpy(mb).to(dev), 48000, 32000))
    assert isinstance(s, float) and s == want
    assert abs(tts.verify_speaker(pa, pa) - 1.0) <= 1e-6
    assert pa not in tts.spk_audio_cache and pb not in tts.spk_audio_cache


def test_list_forms_equal_single_calls(tts, tmp_path):
    specs = [("s16", 1, 32000), ("s24", 2, 44100), ("f32", 1, 16000)]
    clips = [_clip(fmt, ch, rate, 1.0 + 0.5 * i, 40 + i) for i, (fmt, ch, rate) in enumerate(specs)]
    (tmp_path / "l").mkdir()
    (tmp_path / "s").mkdir()
    lst = [ww.write(tmp_path / "l" / ("%d.wav" % i), x, fmt, rate) for i, ((x, _), (fmt, _, rate)) in enumerate(zip(clips, specs))]
    one = [ww.write(tmp_path / "s" / ("%d.wav" % i), x, fmt, rate) for i, ((x, _), (fmt, _, rate)) in enumerate(zip(clips, specs))]
    # speakers: every key a file, then a file next to a waveform key
    tts.cache_spk_audio(lst, sovits_model=PRO)
    for p, q in zip(lst, one):
        tts.cache_spk_audio(q, sovits_model=PRO)
        assert torch.equal(tts.spk_audio_cache[p]["sv_emb"], tts.spk_audio_cache[q]["sv_emb"]), p
        assert torch.equal(tts.spk_audio_cache[p]["ge"][PRO], tts.spk_audio_cache[q]["ge"][PRO]), p
    mixed = [str(tmp_path / "l" / "mixed.wav"), "mixed-arr"]
    ww.write(mixed[0], clips[1][0], "s24", 44100)
    tts.cache_spk_audio(mixed, sovits_model=V2, audio=[None, torch.from_numpy(clips[2][1])], sample_rate=[None, 16000])
    tts.cache_spk_audio(one[1], sovits_model=V2)
    tts.cache_spk_audio("single-arr", sovits_model=V2, audio=torch.from_numpy(clips[2][1]), sample_rate=16000)
    assert torch.equal(tts.spk_audio_cache[mixed[0]]["ge"][V2], tts.spk_audio_cache[one[1]]["ge"][V2])
    assert torch.equal(tts.spk_audio_cache["mixed-arr"]["ge"][V2], tts.spk_audio_cache["single-arr"]["ge"][V2])
    # prompts: phones1 and bert1 from the text frontend
    texts = ["first prompt.", "second one.", "third!"]
    tts.cache_prompt_audio(lst, texts, sovits_model=PRO)
    for p, q, t in zip(lst, one, texts):
        tts.cache_prompt_audio(q, t, sovits_model=PRO)
        a, b = tts.prompt_audio_cache[p], tts.prompt_audio_cache[q]
        assert torch.equal(a["prompt"], b["prompt"]), p
        assert a["phones1"] == b["phones1"] == _toy_frontend(t)[0] and torch.equal(a["bert1"], b["bert1"])


def test_infer_with_wav_paths(dev, tmp_path):
    """infer / infer_vc on WAV paths against the same runs on the waveforms, cached first under other keys"""
    from gsv_tts import TTS
    tts = TTS(gpt_cache=[(1, 128), (1, 160)], sovits_cache=[50, 55], models_dir=_models_dir(tmp_path), device=str(dev),
              dtype="bfloat16")
    tts.load_gpt_model("synthetic://gpt?seed=1234&n_layer=6&eos_gain=1.0")
    tts.load_sovits_model(PRO)
    tts.set_text_frontend(_toy_frontend)
    xs, ms = _clip("s16", 2, 44100, 2.0, 31)
    xp, mp = _clip("s16", 1, 16000, 1.0, 33)
    spk, prm = ww.write(tmp_path / "spk.wav", xs, "s16", 44100), ww.write(tmp_path / "prompt.wav", xp, "s16", 16000)
    clip = tts.infer(spk, prm, "prompt text.", "Hello there, from a file", top_k=1, noise_scale=0.0)
    assert spk in tts.spk_audio_cache and prm in tts.prompt_audio_cache
    tts.cache_spk_audio("spk-arr", audio=torch.from_numpy(ms), sample_rate=44100)
    tts.cache_prompt_audio("prompt-arr", "prompt text.", audio=torch.from_numpy(mp), phones1=_toy_frontend("prompt text.")[0])
    assert torch.equal(tts.spk_audio_cache[spk]["ge"][PRO], tts.spk_audio_cache["spk-arr"]["ge"][PRO])
    assert torch.equal(tts.prompt_audio_cache[prm]["prompt"], tts.prompt_audio_cache["prompt-arr"]["prompt"])
    again = tts.infer("spk-arr", "prompt-arr", "prompt text.", "Hello there, from a file", top_k=1, noise_scale=0.0)
    assert clip.audio_data.shape == again.audio_data.shape and len(clip.audio_data) > 6400
    np.testing.assert_allclose(clip.audio_data, again.audio_data, atol=1e-5, rtol=0)   # the bound of two identical runs
    vc = tts.infer_vc(spk, prm, "prompt text.", noise_scale=0.0)
    vc2 = tts.infer_vc("spk-arr", "prompt-arr", "prompt text.", noise_scale=0.0)
    np.testing.assert_allclose(vc.audio_data, vc2.audio_data, atol=1e-5, rtol=0)
