"""CPU checks of the list forms of TTS.cache_prompt_audio / cache_spk_audio: mismatched list lengths and empty texts are
refused with a ValueError naming what is wrong before any model is loaded, and a str (or tuple) key still takes the
single-clip path.  No GPU: the model loaders are spies that fail the test if they are reached."""
import numpy as np
import pytest
import torch

from gsv_tts_lite_amd import synth


@pytest.fixture
def tts(tmp_path, monkeypatch):
    import gsv_tts_lite_amd.hubert as hubert
    import gsv_tts_lite_amd.sv as sv
    from gsv_tts import TTS

    def spy(name):
        def load(*a, **k):
            raise AssertionError("%s was called" % name)
        return load

    monkeypatch.setattr(hubert, "load_cnhubert", spy("load_cnhubert"))
    monkeypatch.setattr(sv, "load_sv", spy("load_sv"))
    t = TTS(models_dir=str(tmp_path), device="cpu")
    t.load_sovits_model = spy("load_sovits_model")
    return t


def _w(i, n=16000):
    return torch.from_numpy(synth.synth_audio(i, n))


def test_prompt_list_lengths_and_empty_texts(tts):
    keys = ["a", "b", "c"]
    audio = [_w(0), _w(1), _w(2)]
    with pytest.raises(ValueError, match="prompt_audio_texts has 2 entries for 3 keys"):
        tts.cache_prompt_audio(keys, ["x", "y"], audio=audio, phones1=[1, 2])
    with pytest.raises(ValueError, match=r"prompt_audio_texts\[1\] must not be empty"):
        tts.cache_prompt_audio(keys, ["x", "", "z"], audio=audio, phones1=[1, 2])
    with pytest.raises(ValueError, match="audio has 2 entries for 3 keys"):
        tts.cache_prompt_audio(keys, "x", audio=audio[:2], phones1=[1, 2])
    with pytest.raises(ValueError, match="phones1 has 2 entries for 3 keys"):
        tts.cache_prompt_audio(keys, "x", audio=audio, phones1=[[1], [2]])
    with pytest.raises(ValueError, match="bert1 has 1 entries for 3 keys"):
        tts.cache_prompt_audio(keys, "x", audio=audio, phones1=[1, 2], bert1=[torch.zeros(2, 1024)])
    with pytest.raises(ValueError, match="sample_rate has 2 entries for 3 keys"):
        tts.cache_prompt_audio(keys, "x", audio=audio, phones1=[1, 2], sample_rate=[16000, 16000])
    with pytest.raises(ValueError, match=r"audio\[2\] must be one mono waveform"):
        tts.cache_prompt_audio(keys, "x", audio=audio[:2] + [torch.zeros(2, 100)], phones1=[1, 2])
    assert tts.prompt_audio_cache == {} and tts.cnhubert_model is None


def test_spk_list_lengths(tts):
    keys = ["s1", "s2"]
    with pytest.raises(ValueError, match="audio has 1 entries for 2 keys"):
        tts.cache_spk_audio(keys, audio=[_w(0)])
    with pytest.raises(ValueError, match="sv_emb has 3 entries for 2 keys"):
        tts.cache_spk_audio(keys, audio=[_w(0), _w(1)], sv_emb=[None, None, None])
    with pytest.raises(ValueError, match="ge has 1 entries for 2 keys"):
        tts.cache_spk_audio(keys, ge=[torch.zeros(1, 1024, 1)])
    with pytest.raises(NotImplementedError, match="key 1"):
        tts.cache_spk_audio(keys, audio=[_w(0), None])
    assert tts.spk_audio_cache == {} and tts.sv_model is None


def test_spk_list_of_finished_ge_needs_no_model(tts):
    ges = [torch.from_numpy(synth.synth_ge(i, 1024)) for i in range(3)]
    tts.cache_spk_audio(["s1", "s2", "s3"], ge=ges)
    for i, k in enumerate(["s1", "s2", "s3"]):
        assert torch.equal(tts.spk_audio_cache[k]["ge"][tts.default_sovits_path], ges[i])
        assert "sv_emb" not in tts.spk_audio_cache[k]


def test_str_and_tuple_keys_take_the_single_path(tts, monkeypatch):
    from gsv_tts import TTS

    def no_batch(*a, **k):
        raise AssertionError("a single key went down the batch path")

    monkeypatch.setattr(TTS, "_cache_prompt_batch", no_batch)
    monkeypatch.setattr(TTS, "_cache_spk_batch", no_batch)
    prompt = torch.arange(5, dtype=torch.int64)[None]
    tts.cache_prompt_audio("p.wav", "text.", prompt=prompt, phones1=[1, 2])
    tts.cache_prompt_audio(("p1.wav", "p2.wav"), "text.", prompt=prompt, phones1=[3])
    assert torch.equal(tts.prompt_audio_cache["p.wav"]["prompt"], prompt)
    assert tts.prompt_audio_cache[("p1.wav", "p2.wav")]["phones1"] == [3]
    with pytest.raises(ValueError):
        tts.cache_prompt_audio("q.wav", "", prompt=prompt, phones1=[1])
    ge = torch.from_numpy(synth.synth_ge(0, 1024))
    tts.cache_spk_audio("spk.wav", ge=ge)
    tts.cache_spk_audio(("a.wav", "b.wav"), None, ge)          # positional sovits_model, then ge
    assert torch.equal(tts.spk_audio_cache["spk.wav"]["ge"][tts.default_sovits_path], ge)
    assert np.array_equal(tts.spk_audio_cache[("a.wav", "b.wav")]["ge"][tts.default_sovits_path].numpy(), ge.numpy())
