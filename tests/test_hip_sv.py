"""GPU parity of the speaker-verification path (csrc/sv.h behind gsv_sv_*): resample and fbank against the fp64
restatement tests/sv_ref.py; forward3 against the reference's ERes2NetV2 (tests/golden/sv.npz) and, in full, against the
restatement from T = 1 to 30 s; bit-reproducibility and workspace reuse; TTS.cache_spk_audio / verify_speaker /
cache_prompt_audio(sample_rate=...) through the facade.

Tolerances, from the fp32 restatement's own spread against fp64 (tests/test_sv_cpu.py):
  resample   1e-5 abs (fp32 spread 1.3e-7 on |x| <= 1)
  fbank      2e-3 in the log domain (fp32 spread 5.5e-5; the DFT's fp32 sums leave relative errors in the quiet bins)
  forward3   2e-3 abs on outputs up to ~70 (fp32 spread 1.5e-4), and cosine >= 1 - 1e-7 against the reference"""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sv_ref  # noqa: E402

from gsv_tts_lite_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu
TOL_RS, TOL_FB, TOL = 1e-5, 2e-3, 2e-3
LOG_EPS = math.log(sv_ref.FLT_EPS)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "sv.npz"))


@pytest.fixture(scope="module")
def model(dev, gold):
    from gsv_tts_lite_amd.sv import SVNative
    w = synth.sv_weights(int(gold["seed"]), 64)
    return SVNative(w, dev), w


def _cos(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b)))


@pytest.mark.parametrize("orig,new", [(32000, 16000), (48000, 16000), (16000, 32000), (44100, 16000), (16000, 16000)])
@pytest.mark.parametrize("n", [1, 7, 27, 1001, 48001])
def test_resample(dev, orig, new, n):
    from gsv_tts_lite_amd.sv import resample, resample_length
    x = synth.synth_audio(4, n)
    want = sv_ref.resample(x, orig, new)
    got = resample(torch.from_numpy(x), orig, new, dev).cpu().numpy()
    assert got.shape == want.shape and resample_length(n, orig, new) == want.shape[0]
    assert np.abs(got - want).max() <= TOL_RS


def _signal(kind, n):
    x = synth.synth_audio(5, n).astype(np.float32)
    if kind == "silent_mid":
        x[n // 4: n // 2] = 0.0
    elif kind == "dc_mid":
        x[n // 4: n // 2] = 0.3
    elif kind == "silent":
        x[:] = 0.0
    return x


@pytest.mark.parametrize("kind,n", [("audio", 400), ("audio", 401), ("audio", 559), ("audio", 560), ("audio", 48007),
                                    ("silent_mid", 16000), ("dc_mid", 16000), ("silent", 1200)])
def test_fbank(model, kind, n):
    m, _ = model
    x = _signal(kind, n)
    want = sv_ref.fbank(x)
    got = m.fbank(torch.from_numpy(x)).cpu().numpy()
    assert got.shape == want.shape == (m.frames(n), 80)
    assert np.abs(got - want).max() <= TOL_FB
    floor = want == LOG_EPS
    if kind == "audio":
        assert not floor.any()
    assert (np.abs(got[floor] - LOG_EPS) <= 2e-6).all()     # logf(FLT_EPSILON), within an ulp


@pytest.mark.parametrize("name", ["m64_T1", "m64_T37", "m64_T298", "m64_T998"])
def test_forward3_golden(model, gold, name):
    m, _ = model
    T, step = int(gold[name + "_T"]), int(gold[name + "_step"])
    got = m.forward3(torch.from_numpy(synth.sv_feat(T, T, int(gold["seed"])))).cpu().numpy()[0]
    assert got.shape == (20480,)
    want = gold[name + "_emb"]
    assert np.abs(got[::step] - want).max() <= TOL
    assert _cos(got[::step], want) >= 1 - 1e-7


def test_forward3_golden_m16(dev, gold):
    from gsv_tts_lite_amd.sv import SVNative
    m = SVNative(synth.sv_weights(int(gold["seed"]), 16), dev)
    for name in ("m16_T37", "m16_T298"):
        T = int(gold[name + "_T"])
        got = m.forward3(torch.from_numpy(synth.sv_feat(T, T, int(gold["seed"])))).cpu().numpy()[0]
        assert got.shape == (5120,)
        assert np.abs(got - gold[name + "_emb"]).max() <= TOL, name


@pytest.mark.parametrize("T", [1, 2, 3, 61, 298, 998, 2998])
def test_forward3_vs_restatement(model, T):
    m, w = model
    feat = synth.sv_feat(1000 + T, T)
    want = sv_ref.forward3(w, feat).numpy()
    got = m.forward3(torch.from_numpy(feat)).cpu().numpy()[0]
    assert np.isfinite(got).all()
    assert np.abs(got - want).max() <= TOL
    assert _cos(got, want) >= 1 - 1e-7


def test_embed_vs_restatement(model):
    m, w = model
    x = synth.synth_audio(6, 32000 * 3 + 17)
    want = sv_ref.forward3(w, sv_ref.fbank(sv_ref.resample(x, 32000, 16000)).astype(np.float32)).numpy()
    got = m.embed(torch.from_numpy(x), 32000).cpu().numpy()[0]
    assert np.abs(got - want).max() <= 5 * TOL
    assert _cos(got, want) >= 1 - 1e-6
    with pytest.raises(ValueError):
        m.embed(torch.zeros(797), 32000)             # 399 samples at 16 kHz: 400 is the shortest input
    assert m.frames(799, 32000) == 1


def test_bit_reproducible_and_workspace_reuse(model, dev):
    m, _ = model
    lens = [32000 * 10, 32000, 801, 32000 * 10, 32000]
    first = {}
    for n in lens:
        a = torch.from_numpy(synth.synth_audio(9, n)).to(dev)
        out = m.embed(a, 32000).clone()
        if n in first:
            assert torch.equal(out, first[n]), n
        else:
            first[n] = out
            assert torch.equal(m.embed(a, 32000), out), n


# ------------------------------------------------------------------------------------------------------------ facade
def _tts(tmp_path, dev, with_ckpt=True, seed=1234):
    from gsv_tts import TTS
    if with_ckpt:
        synth.write_sv_ckpt(str(tmp_path / "sv" / "pretrained_eres2netv2w24s4ep4.ckpt"), seed=seed)
    return TTS(gpt_cache=[(1, 128)], sovits_cache=[50, 55], models_dir=str(tmp_path), device=str(dev), dtype="bfloat16")


def test_tts_cache_spk_audio_computes_sv_emb(dev, tmp_path):
    seed = 1234
    tts = _tts(tmp_path, dev, seed=seed)
    pro = "synthetic://sovits?version=v2ProPlus&seed=%d" % seed
    pro2 = "synthetic://sovits?version=v2Pro&seed=%d" % (seed + 1)
    tts.load_sovits_model(pro, pro2)
    wave = synth.synth_audio(11, 32000 * 3)
    tts.cache_spk_audio("spk", sovits_model=pro, audio=torch.from_numpy(wave))
    assert tts.sv_model is None                     # always_load_sv=False: dropped after the call
    entry = tts.spk_audio_cache["spk"]
    w = synth.sv_weights(seed, 64)
    want_sv = sv_ref.forward3(w, sv_ref.fbank(sv_ref.resample(wave, 32000, 16000)).astype(np.float32)).numpy()
    sv = entry["sv_emb"]
    assert tuple(sv.shape) == (1, 20480) and sv.dtype == torch.float32
    assert _cos(sv.cpu().numpy(), want_sv) >= 1 - 1e-6
    vq = tts.sovits_models[pro].vq_model
    audio = torch.from_numpy(wave).to(dev).reshape(1, -1)
    spec = vq.spectrogram(audio)
    want_ge = vq.get_ge(spec, torch.from_numpy(want_sv).to(dev)[None]).float()
    assert torch.allclose(entry["ge"][pro].float(), want_ge, atol=2e-3, rtol=0)
    no_sv = vq.get_ge(spec, None).float()
    assert (entry["ge"][pro].float() - no_sv).abs().max().item() > 1e-2     # the sv term is in
    # a second SoVITS model reuses the cached sv_emb
    tts.always_load_sv = True
    tts.cache_spk_audio("spk", sovits_model=pro2, audio=torch.from_numpy(wave))
    assert tts.sv_model is None                     # not even loaded: the entry's sv_emb was reused
    assert torch.equal(tts.spk_audio_cache["spk"]["sv_emb"], sv)
    vq2 = tts.sovits_models[pro2].vq_model
    assert torch.equal(entry["ge"][pro2], vq2.get_ge(vq2.spectrogram(audio), sv))
    # an explicit sv_emb still wins
    explicit = torch.from_numpy(synth.synth_sv_emb(3)).to(dev)
    tts.cache_spk_audio("spk2", sovits_model=pro, audio=torch.from_numpy(wave), sv_emb=explicit)
    assert torch.equal(tts.spk_audio_cache["spk2"]["ge"][pro], vq.get_ge(spec, explicit))
    # verify_speaker: cache keys and waveforms
    assert abs(tts.verify_speaker("spk", "spk") - 1.0) <= 1e-6
    other = synth.synth_audio(12, 32000 * 2)
    s = tts.verify_speaker("spk", torch.from_numpy(other))
    assert tts.sv_model is not None                 # always_load_sv=True keeps it
    want_o = sv_ref.forward3(w, sv_ref.fbank(sv_ref.resample(other, 32000, 16000)).astype(np.float32)).numpy()
    assert isinstance(s, float) and abs(s - _cos(want_sv, want_o)) <= 1e-4
    with pytest.raises(NotImplementedError, match="decoding"):
        tts.verify_speaker("spk", "no_such_file.wav")


def test_tts_v2_and_missing_checkpoint(dev, tmp_path, caplog):
    seed = 1234
    tts = _tts(tmp_path, dev, with_ckpt=False, seed=seed)
    v2 = "synthetic://sovits?version=v2&seed=%d" % seed
    pro = "synthetic://sovits?version=v2ProPlus&seed=%d" % seed
    tts.load_sovits_model(v2, pro)
    wave = torch.from_numpy(synth.synth_audio(13, 32000 * 2))
    audio = wave.to(dev).reshape(1, -1)
    tts.cache_spk_audio("a", sovits_model=v2, audio=wave)
    vq = tts.sovits_models[v2].vq_model
    assert torch.equal(tts.spk_audio_cache["a"]["ge"][v2], vq.get_ge(vq.spectrogram(audio), None))
    assert "sv_emb" not in tts.spk_audio_cache["a"] and tts.sv_model is None
    with caplog.at_level("WARNING", logger="gsv_tts_lite_amd"):
        tts.cache_spk_audio("b", sovits_model=pro, audio=wave)
    assert sum("ERes2NetV2 checkpoint" in r.getMessage() for r in caplog.records) == 1
    vqp = tts.sovits_models[pro].vq_model
    assert torch.equal(tts.spk_audio_cache["b"]["ge"][pro], vqp.get_ge(vqp.spectrogram(audio), None))


def test_tts_prompt_audio_sample_rate(dev, gold, tmp_path):
    """cache_prompt_audio(audio at 32 kHz, sample_rate=32000) gives the codes of the 16 kHz waveform the restatement
    resamples, wherever the code margin is clear"""
    from gsv_tts import TTS
    synth.write_hubert_dir(str(tmp_path / "chinese-hubert-base"), seed=1234)
    tts = TTS(gpt_cache=[(1, 128)], sovits_cache=[50, 55], models_dir=str(tmp_path), device=str(dev), dtype="bfloat16")
    tts.load_sovits_model("synthetic://sovits?version=v2Pro&seed=1234")
    x32 = synth.synth_audio(14, 32000 * 3)
    x16 = sv_ref.resample(x32, 32000, 16000).astype(np.float32)
    tts.cache_prompt_audio("p32", "text.", audio=torch.from_numpy(x32), sample_rate=32000, phones1=[1, 2, 3])
    tts.cache_prompt_audio("p16", "text.", audio=torch.from_numpy(x16), phones1=[1, 2, 3])
    a = tts.prompt_audio_cache["p32"]["prompt"][0].cpu().numpy()
    b = tts.prompt_audio_cache["p16"]["prompt"][0].cpu().numpy()
    m = next(iter(tts.sovits_models.values())).vq_model
    ssl16 = tts._cnhubert_ssl(torch.from_numpy(x16))
    _, margin = m._ref_audio().extract_latent(ssl16, return_margin=True)
    ok = margin.reshape(-1).cpu().numpy() > 1e-2
    assert a.shape == b.shape and ok.mean() > 0.9
    assert np.array_equal(a[ok], b[ok])
